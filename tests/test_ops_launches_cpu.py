"""Characterisation of clipa_amd/ops.py without a GPU: which C entry points every wrapper calls, with which scalars and which
pointers, what it allocates, what it returns, what the profiler records and what it raises.

CPU tensors flow through the real wrappers: `torch.Tensor.is_cuda` reads True, `lib.call` / `lib.query` are recorders (a query
answers 4096 bytes and writes 1 through a byref argument), `ops._stream` gives a null stream, HIP events are dummies.  Per call the
trace holds the entry point, every int and float as passed, and per pointer `null`, `"<caller tensor>+<byte offset>"` or `"fresh"`
(memory ops.py allocated; `"fresh+<byte offset>"` when it points into such an allocation); ctypes arrays are lists.  Per case it also holds dtype / shape / stride of what came back (and which
caller tensor it aliases), the sorted list of torch.empty / zeros / ones / empty_like allocations, and the message of an error.
The profile section is profile_stop()'s keys with launches / work / bytes after a detail=True bracket around the same cases.

tests/golden/ops_launch_trace.json is the trace of the ops.py of the commit named in it - the parent of the host-layer refactor -
and is never regenerated from later code: the refactor has to reproduce it.  It was written from a worktree of that commit:

    git worktree add <dir> <commit> && cp tests/test_ops_launches_cpu.py <dir>/tests/
    (cd <dir> && python -m tests.test_ops_launches_cpu --write <repo>/tests/golden/ops_launch_trace.json)
"""
import contextlib
import ctypes
import json
import os
import subprocess
import sys
from unittest import mock

import pytest
import torch

from clipa_amd import lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ops_launch_trace.json")
bf16, f32, u8, i32, i64 = torch.bfloat16, torch.float32, torch.uint8, torch.int32, torch.int64
WS_BYTES = 4096


# ---- the recorder ----------------------------------------------------------------------------------------------------------
class _Event:
    def __init__(self, *a, **k):
        pass

    def record(self, *a):
        pass

    def synchronize(self):
        pass

    def query(self):
        return True

    def elapsed_time(self, other):
        return 0.0


class _Recorder:
    def __init__(self):
        self.begin({})

    def begin(self, named):
        self.named, self.calls, self.allocs, self.live = named, [], [], []

    def label(self, addr):
        if addr is None:
            return None
        for name, t in self.named.items():
            lo = t.data_ptr()
            hi = t.untyped_storage().data_ptr() + t.untyped_storage().nbytes()
            if lo <= addr < hi:
                return f"{name}+{addr - lo}"
        for t in self.live:      # the allocations ops.py made for this case, kept alive so that no address is reused
            if t.data_ptr() < addr < t.data_ptr() + t.numel() * t.element_size():
                return f"fresh+{addr - t.data_ptr()}"
        return "fresh"

    def arg(self, a):
        if a is None:
            return None
        if isinstance(a, ctypes.c_void_p):
            return self.label(a.value)
        if isinstance(a, ctypes.Array):
            return [self.label(v) if a._type_ is ctypes.c_void_p else v for v in a]
        if isinstance(a, (bool, int, float)):
            return a
        if type(a).__name__ == "CArgObject":      # ctypes.byref(c_int64): the query's second result
            a._obj.value = 1
            return "byref"
        raise TypeError(f"unexpected argument {a!r}")

    def call(self, name, *args):
        self.calls.append([name] + [self.arg(a) for a in args])

    def query(self, name, *args):
        self.call(name, *args)
        return WS_BYTES

    def describe(self, r):
        if r is None:
            return None
        if isinstance(r, (tuple, list)):
            return [self.describe(x) for x in r]
        d = {"dtype": str(r.dtype), "shape": list(r.shape), "stride": list(r.stride())}
        where = self.label(r.data_ptr())
        if where != "fresh":
            d["is"] = where
        return d


def _alloc_spy(rec, fn):
    def wrapped(*a, **k):
        k.pop("pin_memory", None)
        t = fn(*a, **k)
        rec.allocs.append(f"{t.dtype}{list(t.shape)}")
        rec.live.append(t)
        return t
    return wrapped


@contextlib.contextmanager
def _host_only(rec):
    with contextlib.ExitStack() as st:
        st.enter_context(mock.patch.object(torch.Tensor, "is_cuda", True))
        st.enter_context(mock.patch.object(lib, "call", rec.call))
        st.enter_context(mock.patch.object(lib, "query", rec.query))
        st.enter_context(mock.patch.object(ops, "_stream", lambda: None))
        st.enter_context(mock.patch.object(torch.cuda, "Event", _Event))
        st.enter_context(mock.patch.object(torch.cuda, "synchronize", lambda *a: None))
        st.enter_context(mock.patch.object(torch.Tensor, "pin_memory", lambda self, *a, **k: self))
        for name in ("empty", "zeros", "ones", "empty_like", "zeros_like"):
            st.enter_context(mock.patch.object(torch, name, _alloc_spy(rec, getattr(torch, name))))
        yield


# ---- the cases: name -> (named caller tensors, function of them) ------------------------------------------------------------
def _z(*shape, dtype=bf16):
    return torch.zeros(shape, dtype=dtype)


def _gemm_nt_cases():
    E = ops
    for M, N, K in ((256, 256, 256), (256, 256, 128), (200, 136, 72), (1, 256, 256)):
        def T():
            t = {"a": _z(M, K), "b": _z(N, K), "bias": _z(N, dtype=f32), "aux": _z(M, N), "aux8": _z(M, N, dtype=u8)}
            t["a_s"] = _z(M, K + 8)[:, :K]
            t["aux_s"] = _z(M, N + 8)[:, :N]
            t["aux8_s"] = _z(M, N + 16, dtype=u8)[:, :N]
            t["out_s"] = _z(M, 2 * N)[:, N:]
            return t
        V = {
            "plain": lambda t: ops.gemm_nt(t["a"], t["b"]),
            "bias": lambda t: ops.gemm_nt(t["a"], t["b"], t["bias"]),
            "alpha": lambda t: ops.gemm_nt(t["a"], t["b"], alpha=0.5),
            "f32": lambda t: ops.gemm_nt(t["a"], t["b"], t["bias"], out_f32=True),
            "act": lambda t: ops.gemm_nt(t["a"], t["b"], t["bias"], epi=E.EPI_ACT, act=E.ACT_QUICK_GELU),
            "act_pre": lambda t: ops.gemm_nt(t["a"], t["b"], t["bias"], epi=E.EPI_ACT, want_pre=True),
            "act_pre8": lambda t: ops.gemm_nt(t["a"], t["b"], t["bias"], epi=E.EPI_ACT, want_pre="e4m3"),
            "act_pre8_f32": lambda t: ops.gemm_nt(t["a"], t["b"], epi=E.EPI_ACT, want_pre="e4m3", out_f32=True),
            "add": lambda t: ops.gemm_nt(t["a"], t["b"], t["bias"], epi=E.EPI_ADD, aux=t["aux"]),
            "dact": lambda t: ops.gemm_nt(t["a"], t["b"], epi=E.EPI_DACT, act=E.ACT_GELU_TANH, aux=t["aux"]),
            "dact8": lambda t: ops.gemm_nt(t["a"], t["b"], epi=E.EPI_DACT, aux=t["aux8"]),
            "dact8_act": lambda t: ops.gemm_nt(t["a"], t["b"], epi=E.EPI_DACT, aux=t["aux8"], want_act=True),
            "strided": lambda t: ops.gemm_nt(t["a_s"], t["b"], epi=E.EPI_ADD, aux=t["aux_s"]),
            "strided_dact8": lambda t: ops.gemm_nt(t["a_s"], t["b"], epi=E.EPI_DACT, aux=t["aux8_s"]),
            "out_slice": lambda t: ops.gemm_nt(t["a"], t["b"], t["bias"], out=t["out_s"]),
            "out_slice_pre": lambda t: ops.gemm_nt(t["a"], t["b"], epi=E.EPI_ACT, want_pre=True, out=t["out_s"]),
            "out_slice_dact8_act": lambda t: ops.gemm_nt(t["a"], t["b"], epi=E.EPI_DACT, aux=t["aux8"], want_act=True, out=t["out_s"]),
            "err_want_act": lambda t: ops.gemm_nt(t["a"], t["b"], epi=E.EPI_DACT, aux=t["aux"], want_act=True),
            "err_aux8_epi": lambda t: ops.gemm_nt(t["a"], t["b"], epi=E.EPI_ADD, aux=t["aux8"]),
            "err_pre8_out_slice": lambda t: ops.gemm_nt(t["a"], t["b"], epi=E.EPI_ACT, want_pre="e4m3", out=t["out_s"]),
            "err_k": lambda t: ops.gemm_nt(t["a"], t["b"][:, :K - 8]),
        }
        for v, fn in V.items():
            yield f"gemm_nt/{M}x{N}x{K}/{v}", T, fn


def _gemm_f8_cases():
    E = ops
    for M, N, K in ((256, 256, 512), (256, 256, 256), (300, 264, 144)):
        def T():
            return {"a8": _z(M, K, dtype=u8), "b8": _z(N, K, dtype=u8), "sa": _z(M, dtype=f32), "sb": _z(N, dtype=f32),
                    "bias": _z(N, dtype=f32), "aux": _z(M, N), "aux8": _z(M, N, dtype=u8), "os": _z(M, dtype=f32),
                    "t": _z(1, dtype=f32), "a8_s": _z(M, K + 16, dtype=u8)[:, :K], "aux8_s": _z(M, N + 16, dtype=u8)[:, :N]}
        for fb in (E.FMT_E4M3, E.FMT_E5M2):
            def g(t, *a, fb=fb, **k):
                return ops.gemm_nt_f8(t["a8"], t["sa"], t["b8"], t["sb"], *a, fmt_b=fb, **k)
            V = {
                "plain": lambda t, g=g: g(t),
                "no_sa": lambda t, fb=fb: ops.gemm_nt_f8(t["a8"], None, t["b8"], t["sb"], t["bias"], fmt_b=fb, fmt_a=E.FMT_E5M2),
                "bias_alpha": lambda t, g=g: g(t, t["bias"], alpha=0.25),
                "act": lambda t, g=g: g(t, t["bias"], epi=E.EPI_ACT, act=E.ACT_QUICK_GELU),
                "act_pre": lambda t, g=g: g(t, t["bias"], epi=E.EPI_ACT, want_pre=True),
                "act_pre8": lambda t, g=g: g(t, t["bias"], epi=E.EPI_ACT, want_pre="e4m3"),
                "add": lambda t, g=g: g(t, t["bias"], epi=E.EPI_ADD, aux=t["aux"]),
                "add_pre8": lambda t, g=g: g(t, epi=E.EPI_ADD, aux=t["aux"], want_pre="e4m3"),
                "dact": lambda t, g=g: g(t, epi=E.EPI_DACT, aux=t["aux"]),
                "dact8": lambda t, g=g: g(t, epi=E.EPI_DACT, act=E.ACT_GELU_TANH, aux=t["aux8"]),
                "strided_dact8": lambda t, fb=fb: ops.gemm_nt_f8(t["a8_s"], t["sa"], t["b8"], t["sb"], epi=E.EPI_DACT, aux=t["aux8_s"], fmt_b=fb),
                "q_plain": lambda t, g=g: g(t, t["bias"], out_scale=t["os"]),
                "q_act": lambda t, g=g: g(t, t["bias"], epi=E.EPI_ACT, out_scale=t["os"]),
                "q_act_pre": lambda t, g=g: g(t, t["bias"], epi=E.EPI_ACT, want_pre=True, out_scale=t["os"]),
                "q_act_pre8": lambda t, g=g: g(t, t["bias"], epi=E.EPI_ACT, want_pre="e4m3", out_scale=t["os"]),
                "q_act_colsum": lambda t, g=g: g(t, epi=E.EPI_ACT, out_scale=t["os"], want_colsum=True),
                "q_dact8_colsum": lambda t, g=g: g(t, epi=E.EPI_DACT, aux=t["aux8"], out_scale=t["os"], want_colsum=True),
                "q_dact8": lambda t, g=g: g(t, epi=E.EPI_DACT, aux=t["aux8_s"], out_scale=t["os"]),
                "q_dact8_bias": lambda t, g=g: g(t, t["bias"], epi=E.EPI_DACT, aux=t["aux8"], out_scale=t["os"], want_colsum=True),
                "q_dact16": lambda t, g=g: g(t, epi=E.EPI_DACT, aux=t["aux"], out_scale=t["os"]),
                "err_sa_len": lambda t, fb=fb: ops.gemm_nt_f8(t["a8"], t["sb"][:7], t["b8"], t["sb"], fmt_b=fb),
                "err_q_sb_len": lambda t, fb=fb: ops.gemm_nt_f8(t["a8"], t["sa"], t["b8"], t["sa"][:9], epi=E.EPI_ACT, out_scale=t["os"], fmt_b=fb),
                "err_q_os_len": lambda t, g=g: g(t, epi=E.EPI_ACT, out_scale=t["sb"][:5]),
                "err_k": lambda t, fb=fb: ops.gemm_nt_f8(t["a8"], t["sa"], t["aux8_s"][:N, :K - 8], t["sb"], fmt_b=fb),
                "err_aux8_epi": lambda t, g=g: g(t, epi=E.EPI_ADD, aux=t["aux8"]),
            }
            for v, fn in V.items():
                yield f"gemm_nt_f8/{M}x{N}x{K}/fmt_b{fb}/{v}", T, fn
        yield (f"gemm_nt_f8_emit/{M}x{N}x{K}/sa", T,
               lambda t: ops.gemm_nt_f8_emit(t["a8"], t["sa"], t["b8"], t["sb"], t["aux8"], t["t"], act=E.ACT_GELU_TANH))
        yield (f"gemm_nt_f8_emit/{M}x{N}x{K}/strided_no_sb", T,
               lambda t: ops.gemm_nt_f8_emit(t["a8_s"], t["sa"], t["b8"], None, t["aux8_s"], t["t"], fmt_a=E.FMT_E5M2))
        yield (f"gemm_nt_f8_emit/{M}x{N}x{K}/err_shape", T,
               lambda t: ops.gemm_nt_f8_emit(t["a8"], t["sa"], t["b8"], t["sb"][:3], t["aux8"], t["t"]))
    # without sa the emit form has no row scales to quantise with: the GEMM runs, then the quantiser trips over the None
    M, N, K = 256, 256, 512
    yield ("gemm_nt_f8_emit/256x256x512/no_sa",
           lambda: {"a8": _z(M, K, dtype=u8), "b8": _z(N, K, dtype=u8), "sb": _z(N, dtype=f32), "aux8": _z(M, N, dtype=u8), "t": _z(1, dtype=f32)},
           lambda t: ops.gemm_nt_f8_emit(t["a8"], None, t["b8"], t["sb"], t["aux8"], t["t"]))


def _varlen():
    return ops.VarLen(torch.tensor([3, 40, 33, 1]), 48, "cpu")


def _vl_named(vl):
    d = {"vl.seq_start": vl.seq_start, "vl.seq_len": vl.seq_len}
    for k, (_, ids, _) in enumerate(vl.classes):
        d[f"vl.ids{k}"] = ids
    return d


def _other_cases():
    E = ops
    R, D = 24, 64

    def case(name, T, fn):
        return name, T, fn

    x2 = lambda: {"x": _z(R, D), "x_s": _z(R, D + 8)[:, :D]}
    yield case("quantize_rows/plain", x2, lambda t: ops.quantize_rows(t["x"]))
    yield case("quantize_rows/colsum_strided_e5m2", x2, lambda t: ops.quantize_rows(t["x_s"], E.FMT_E5M2, want_colsum=True))
    yield case("quantize_rows/colsum_rownorm", x2, lambda t: ops.quantize_rows(t["x"], want_colsum=True, want_rownorm=True))
    yield case("quantize_rows/err_rownorm", x2, lambda t: ops.quantize_rows(t["x"], want_rownorm=True))

    def ln():
        return {"x": _z(2, 12, D), "x32": _z(2, 12, D, dtype=f32), "gamma": _z(D, dtype=f32), "beta": _z(D, dtype=f32),
                "dy": _z(2, 12, D), "dy32": _z(2, 12, D, dtype=f32), "dres": _z(2, 12, D), "dres32": _z(2, 12, D, dtype=f32),
                "rs": _z(R, dtype=f32), "t": _z(1, dtype=f32)}
    yield case("layernorm_fwd/f32", ln, lambda t: ops.layernorm_fwd(t["x32"], t["gamma"], t["beta"]))
    yield case("layernorm_fwd/bf16", ln, lambda t: ops.layernorm_fwd(t["x"], t["gamma"], t["beta"], eps=1e-6))
    yield case("layernorm_fwd/f32_to_bf16", ln, lambda t: ops.layernorm_fwd(t["x32"], t["gamma"], t["beta"], out_dtype=bf16))
    yield case("layernorm_fwd_q8/plain", ln, lambda t: ops.layernorm_fwd_q8(t["x"], t["gamma"], t["beta"]))
    yield case("layernorm_fwd_q8/bf16", ln, lambda t: ops.layernorm_fwd_q8(t["x"], t["gamma"], t["beta"], want_bf16=True))
    yield case("layernorm_fwd_q8/rownorm", ln, lambda t: ops.layernorm_fwd_q8(t["x"], t["gamma"], t["beta"], want_rownorm=True))
    yield case("layernorm_fwd_q8/bf16_rownorm", ln, lambda t: ops.layernorm_fwd_q8(t["x"], t["gamma"], t["beta"], 1e-6, True, True))
    yield case("layernorm_fwd_q8s/plain", ln, lambda t: ops.layernorm_fwd_q8s(t["x"], t["gamma"], t["beta"], t["rs"], t["t"]))
    yield case("layernorm_fwd_q8s/err_rows", ln, lambda t: ops.layernorm_fwd_q8s(t["x"], t["gamma"], t["beta"], t["rs"][:5], t["t"]))
    for dres in (False, True):
        s = "_dres" if dres else ""
        yield case(f"layernorm_bwd/plain{s}", ln,
                   lambda t, dres=dres: ops.layernorm_bwd(t["x"], t["gamma"], t["dy"], t["dres"] if dres else None))
        yield case(f"layernorm_bwd/plain_f32{s}", ln,
                   lambda t, dres=dres: ops.layernorm_bwd(t["x32"], t["gamma"], t["dy32"], t["dres32"] if dres else None, eps=1e-6))
        yield case(f"layernorm_bwd/mixed{s}", ln,
                   lambda t, dres=dres: ops.layernorm_bwd(t["x32"], t["gamma"], t["dy"], t["dres32"] if dres else None, beta=t["beta"]))
        yield case(f"layernorm_bwd/beta{s}", ln,
                   lambda t, dres=dres: ops.layernorm_bwd(t["x"], t["gamma"], t["dy"], t["dres"] if dres else None, beta=t["beta"]))
        yield case(f"layernorm_bwd/q8{s}", ln,
                   lambda t, dres=dres: ops.layernorm_bwd(t["x"], t["gamma"], t["dy"], t["dres"] if dres else None, q8_fmt=E.FMT_E5M2))
        yield case(f"layernorm_bwd/q8_rownorm{s}", ln,
                   lambda t, dres=dres: ops.layernorm_bwd(t["x"], t["gamma"], t["dy"], t["dres"] if dres else None, q8_fmt=E.FMT_E4M3,
                                                          want_rownorm=True))
        yield case(f"layernorm_bwd/q8_beta_rownorm{s}", ln,
                   lambda t, dres=dres: ops.layernorm_bwd(t["x"], t["gamma"], t["dy"], t["dres"] if dres else None, beta=t["beta"],
                                                          q8_fmt=E.FMT_E4M3, want_rownorm=True))
    yield case("layernorm_bwd/err_dres_dtype", ln, lambda t: ops.layernorm_bwd(t["x"], t["gamma"], t["dy"], t["dres32"]))
    yield case("layernorm_bwd/err_q8_f32", ln, lambda t: ops.layernorm_bwd(t["x32"], t["gamma"], t["dy"], q8_fmt=E.FMT_E4M3))

    B, L, H, dh = 2, 5, 2, 64

    def att():
        return {"qkv": _z(B * L, 3 * H * dh), "out": _z(B * L, H * dh), "dout": _z(B * L, H * dh),
                "stats": _z(B * H * L, 2, dtype=f32), "qkv_s": _z(B * L, 3 * H * dh + 64)[:, :3 * H * dh]}
    yield case("attention_fwd/plain", att, lambda t: ops.attention_fwd(t["qkv"], B, L, H, False))
    yield case("attention_fwd/causal_stats_strided", att, lambda t: ops.attention_fwd(t["qkv_s"], B, L, H, True, want_stats=True))
    yield case("attention_bwd/plain", att, lambda t: ops.attention_bwd(t["qkv"], t["out"], t["dout"], t["stats"], B, L, H, False))
    yield case("attention_bwd/causal", att, lambda t: ops.attention_bwd(t["qkv"], t["out"], t["dout"], t["stats"], B, L, H, True))

    def attv():
        vl = _varlen()
        d = {"qkv": _z(vl.rows, 3 * H * dh), "out": _z(vl.rows, H * dh), "dout": _z(vl.rows, H * dh),
             "stats": _z(vl.rows * H, 2, dtype=f32), "_vl": vl}
        d.update(_vl_named(vl))
        return d
    yield case("attention_fwd_varlen/plain", attv, lambda t: ops.attention_fwd_varlen(t["qkv"], t["_vl"], H, True))
    yield case("attention_fwd_varlen/stats", attv, lambda t: ops.attention_fwd_varlen(t["qkv"], t["_vl"], H, False, want_stats=True))
    yield case("attention_bwd_varlen/plain", attv,
               lambda t: ops.attention_bwd_varlen(t["qkv"], t["out"], t["dout"], t["stats"], t["_vl"], H, True))

    def img():
        return {"nchw": _z(2, 3, 32, 32, dtype=u8), "nhwc": _z(2, 3, 32, 32, dtype=f32).contiguous(memory_format=torch.channels_last),
                "bf": _z(2, 3, 32, 32), "odd": _z(2, 3, 32, 64, dtype=f32)[:, :, :, ::2]}
    yield case("patchify/nchw_u8_norm", img, lambda t: ops.patchify(t["nchw"], 16, 768, (0.5, 0.4, 0.3), (0.2, 0.25, 0.3)))
    yield case("patchify/nhwc_f32", img, lambda t: ops.patchify(t["nhwc"], 16, 768))
    yield case("patchify/nhwc_f32_norm", img, lambda t: ops.patchify(t["nhwc"], 8, 192, (0.5, 0.5, 0.5), (0.25, 0.25, 0.25)))
    yield case("patchify/bf16", img, lambda t: ops.patchify(t["bf"], 16, 768))
    yield case("patchify/noncontiguous", img, lambda t: ops.patchify(t["odd"], 16, 768))
    yield case("patchify/err_dtype", img, lambda t: ops.patchify(t["nchw"].to(torch.int16), 16, 768))

    def aug():
        return {"src": _z(3, 40, 48, 3, dtype=u8), "boxes": _z(3, 4, dtype=i32), "gray": _z(3, dtype=u8), "img": _z(3, 16, 16, 3, dtype=u8),
                "apply": _z(3, dtype=u8), "order": _z(3, 4, dtype=i32), "factors": _z(3, 4, dtype=f32)}
    yield case("resized_crop_u8/plain", aug, lambda t: ops.resized_crop_u8(t["src"], t["boxes"], 16))
    yield case("resized_crop_u8/gray", aug, lambda t: ops.resized_crop_u8(t["src"], t["boxes"], 24, t["gray"]))
    yield case("color_jitter_u8_/full", aug, lambda t: ops.color_jitter_u8_(t["img"], t["apply"], t["order"], t["factors"], t["gray"]))
    yield case("color_jitter_u8_/gray_only", aug, lambda t: ops.color_jitter_u8_(t["img"], gray_flags=t["gray"]))

    def tok():
        return {"patch": _z(2 * 4, D), "cls": _z(D, dtype=f32), "pos": _z(5, D, dtype=f32), "dtok": _z(2 * 5, D),
                "ids": torch.arange(2 * 7).reshape(2, 7), "table": _z(50, D, dtype=f32), "table16": _z(50, D), "tpos": _z(7, D, dtype=f32),
                "dx": _z(2 * 7, D)}
    yield case("assemble_tokens/plain", tok, lambda t: ops.assemble_tokens(t["patch"], t["cls"], t["pos"], 2, 5))
    yield case("assemble_tokens_bwd/pos", tok, lambda t: ops.assemble_tokens_bwd(t["dtok"], 2, 5))
    yield case("assemble_tokens_bwd/no_pos", tok, lambda t: ops.assemble_tokens_bwd(t["dtok"], 2, 5, need_pos=False))
    yield case("embed_tokens/f32", tok, lambda t: ops.embed_tokens(t["ids"], t["table"], t["tpos"]))
    yield case("embed_tokens/bf16", tok, lambda t: ops.embed_tokens(t["ids"], t["table16"], t["tpos"]))
    yield case("embed_tokens_bwd/both", tok, lambda t: ops.embed_tokens_bwd(t["ids"], t["dx"], 50))
    yield case("embed_tokens_bwd/table_only", tok, lambda t: ops.embed_tokens_bwd(t["ids"], t["dx"], 50, need_pos=False))
    yield case("embed_tokens_bwd/pos_only", tok, lambda t: ops.embed_tokens_bwd(t["ids"], t["dx"], 50, need_table=False))
    yield case("argmax_tokens/plain", tok, lambda t: ops.argmax_tokens(t["ids"]))

    def pool():
        return {"x": _z(2 * 5, D), "idx": _z(2, dtype=i32), "dout": _z(2, D, dtype=f32), "rows": torch.arange(0, 10, 2), "dy": _z(5, D)}
    yield case("pool_fwd/first", pool, lambda t: ops.pool_fwd(t["x"], 2, 5, E.POOL_FIRST))
    yield case("pool_fwd/index", pool, lambda t: ops.pool_fwd(t["x"], 2, 5, E.POOL_INDEX, t["idx"]))
    yield case("pool_bwd/mean_patch", pool, lambda t: ops.pool_bwd(t["dout"], 2, 5, E.POOL_MEAN_PATCH))
    yield case("pool_bwd/index", pool, lambda t: ops.pool_bwd(t["dout"], 2, 5, E.POOL_INDEX, t["idx"]))
    yield case("gather_rows/plain", pool, lambda t: ops.gather_rows(t["x"], t["rows"]))
    yield case("scatter_rows/plain", pool, lambda t: ops.scatter_rows(t["dy"], t["rows"], 10))

    def misc():
        return {"x32": _z(6, 10, dtype=f32), "x": _z(6, 16), "x_s": _z(6, 24)[:, :16], "x8": _z(6, 16, dtype=u8), "inv": _z(6, dtype=f32),
                "rs": _z(6, dtype=f32), "t": _z(1, dtype=f32), "w": _z(1, dtype=f32), "out0": _z(1, dtype=f32)[0]}
    yield case("l2norm_fwd/plain", misc, lambda t: ops.l2norm_fwd(t["x32"]))
    yield case("l2norm_fwd/bf16", misc, lambda t: ops.l2norm_fwd(t["x32"], eps=1e-6, want_bf16=True))
    yield case("l2norm_bwd/plain", misc, lambda t: ops.l2norm_bwd(t["x32"], t["inv"], t["x32"]))
    yield case("colsum/plain", misc, lambda t: ops.colsum(t["x"]))
    yield case("colsum/strided", misc, lambda t: ops.colsum(t["x_s"]))
    yield case("cast_e4m3/plain", misc, lambda t: ops.cast_e4m3(t["x"]))
    yield case("e4m3_to_bf16/plain", misc, lambda t: ops.e4m3_to_bf16(t["x8"]))
    yield case("to_bf16/f32", misc, lambda t: ops.to_bf16(t["x32"]))
    yield case("to_bf16/bf16", misc, lambda t: ops.to_bf16(t["x"]))
    yield case("to_bf16/err", misc, lambda t: ops.to_bf16(t["x8"]))
    yield case("to_f32/bf16", misc, lambda t: ops.to_f32(t["x"]))
    yield case("to_f32/f32", misc, lambda t: ops.to_f32(t["x32"]))
    yield case("transpose_bf16/f32", misc, lambda t: ops.transpose_bf16(t["x32"]))
    yield case("transpose_bf16/bf16_strided", misc, lambda t: ops.transpose_bf16(t["x_s"]))
    yield case("activation_fwd/bf16", misc, lambda t: ops.activation_fwd(t["x"], E.ACT_GELU_TANH))
    yield case("activation_fwd/u8", misc, lambda t: ops.activation_fwd(t["x8"], E.ACT_QUICK_GELU))
    yield case("scale_quantize_rows/bf16", misc, lambda t: ops.scale_quantize_rows(t["x_s"], t["rs"], t["t"]))
    yield case("scale_quantize_rows/u8_act", misc, lambda t: ops.scale_quantize_rows(t["x8"], t["rs"], t["t"], act=E.ACT_GELU_ERF))
    yield case("scale_quantize_rows/err_rows", misc, lambda t: ops.scale_quantize_rows(t["x"], t["rs"][:4], t["t"]))
    yield case("row_bound/plain", misc, lambda t: ops.row_bound(t["rs"], t["w"]))
    yield case("row_bound/bmax", misc, lambda t: ops.row_bound(t["rs"], t["w"], t["t"], factor=1.5))
    yield case("rownorm_max/strided", misc, lambda t: ops.rownorm_max(t["x_s"]))
    yield case("absmax/plain", misc, lambda t: ops.absmax(t["rs"]))
    yield case("rowscale_max/one", misc, lambda t: ops.rowscale_max(t["rs"]))
    yield case("rowscale_max/two", misc, lambda t: ops.rowscale_max(t["rs"], t["inv"]))
    yield case("rowscale_max/err", misc, lambda t: ops.rowscale_max(t["rs"], t["inv"][:3]))
    yield case("sum_scale/new", misc, lambda t: ops.sum_scale(t["x32"], 0.5))
    yield case("sum_scale/accumulate", misc, lambda t: ops.sum_scale(t["x32"], 2.0, out=t["out0"], accumulate=True))

    def tn():
        return {"p": _z(40, 24), "q": _z(40, 16), "p_s": _z(40, 32)[:, :24], "p8": _z(40, 32, dtype=u8), "q8": _z(40, 16, dtype=u8),
                "t": _z(1, dtype=f32), "q_bad": _z(39, 16)}
    yield case("gemm_tn/plain", tn, lambda t: ops.gemm_tn(t["p"], t["q"]))
    yield case("gemm_tn/bf16_colsum_strided", tn, lambda t: ops.gemm_tn(t["p_s"], t["q"], bf16, want_colsum=True))
    yield case("gemm_tn/err_m", tn, lambda t: ops.gemm_tn(t["p"], t["q_bad"]))
    yield case("gemm_tn/err_dtype", tn, lambda t: ops.gemm_tn(t["p"], t["q"], torch.float16))
    yield case("gemm_tn_f8/plain", tn, lambda t: ops.gemm_tn_f8(t["p8"], t["q8"]))
    yield case("gemm_tn_f8/t_alpha_e5m2_bf16", tn, lambda t: ops.gemm_tn_f8(t["p8"], t["q8"], t["t"], 0.5, E.FMT_E5M2, bf16))
    yield case("gemm_tn_f8/err_dtype", tn, lambda t: ops.gemm_tn_f8(t["p8"], t["q8"], out_dtype=torch.float16))

    def sim():
        return {"rows": _z(12, 32), "cols": _z(20, 32), "rows_t": _z(12, 48), "cols_t": _z(20, 48), "cols_s": _z(20, 40)[:, :32],
                "s": _z(1, dtype=f32), "u": _z(1, dtype=f32), "lse_s": _z(12, dtype=f32), "lse_t": _z(12, dtype=f32),
                "g_c": _z(1, dtype=f32), "g_d": _z(1, dtype=f32)}
    yield case("simce/grad", sim, lambda t: ops.simce(t["rows"], t["cols"], 19, 3, 0.125, t["s"]))
    yield case("simce/no_grad_no_scale", sim, lambda t: ops.simce(t["rows"], t["cols_s"], 20, 0, 1.0, want_grad=False))
    yield case("simce/err_cover", sim, lambda t: ops.simce(t["rows"], t["cols"], 21, 0, 1.0))
    yield case("simce_distill/plain", sim, lambda t: ops.simce_distill(t["rows"], t["cols_s"], t["rows_t"], t["cols_t"], 19, 3))
    yield case("simce_distill/scales", sim,
               lambda t: ops.simce_distill(t["rows"], t["cols"], t["rows_t"], t["cols_t"], 20, 0, t["s"], t["u"]))
    yield case("simce_distill/err_rows", sim, lambda t: ops.simce_distill(t["rows"], t["cols"], t["rows_t"][:5], t["cols_t"], 20, 0))
    yield case("simce_distill_bwd/plain", sim,
               lambda t: ops.simce_distill_bwd(t["rows"], t["cols"], t["rows_t"], t["cols_t"], 19, 3, 0.5, t["lse_s"], t["lse_t"]))
    yield case("simce_distill_bwd/all", sim,
               lambda t: ops.simce_distill_bwd(t["rows"], t["cols_s"], t["rows_t"], t["cols_t"], 20, 0, 1.0, t["lse_s"], t["lse_t"],
                                               t["s"], t["u"], t["g_c"], t["g_d"]))

    def ret():
        return {"img6": _z(5, 6, dtype=f32), "txt6": _z(5, 6, dtype=f32), "img8": _z(5, 8, dtype=f32), "txt8": _z(5, 8, dtype=f32),
                "s": _z(1, dtype=f32)[0], "mtxt": _z(9, 8, dtype=f32), "mtxt6": _z(9, 6, dtype=f32),
                "c_sorted": torch.tensor([0, 0, 1, 1, 1, 2, 3, 4, 4]), "c_unsorted": torch.tensor([4, 0, 1, 3, 1, 2, 1, 0, 4], dtype=i32)}
    yield case("retrieval_ranks/pad", ret, lambda t: ops.retrieval_ranks(t["img6"], t["txt6"]))
    yield case("retrieval_ranks/aligned_scale", ret, lambda t: ops.retrieval_ranks(t["img8"], t["txt8"], t["s"]))
    yield case("retrieval_ranks/err_shape", ret, lambda t: ops.retrieval_ranks(t["img8"], t["txt6"]))
    yield case("retrieval_ranks_multi/sorted", ret, lambda t: ops.retrieval_ranks_multi(t["img8"], t["mtxt"], t["c_sorted"], t["s"]))
    yield case("retrieval_ranks_multi/unsorted", ret, lambda t: ops.retrieval_ranks_multi(t["img8"], t["mtxt"], t["c_unsorted"]))
    yield case("retrieval_ranks_multi/sorted_pad", ret, lambda t: ops.retrieval_ranks_multi(t["img6"], t["mtxt6"], t["c_sorted"]))
    yield case("retrieval_ranks_multi/err_range", ret, lambda t: ops.retrieval_ranks_multi(t["img8"][:4], t["mtxt"], t["c_sorted"]))
    yield case("retrieval_ranks_multi/err_float", ret, lambda t: ops.retrieval_ranks_multi(t["img8"], t["mtxt"], t["c_sorted"].float()))

    def opt():
        d = {}
        for k, n in enumerate((5000, 17, 4096)):
            d[f"p{k}"], d[f"g{k}"], d[f"m{k}"], d[f"v{k}"] = _z(n), _z(n), _z(n, dtype=f32), _z(n, dtype=f32)
        d["g32"] = _z(9000, dtype=f32)
        d["coef"] = _z(1, dtype=f32)
        d["buf"] = _z(3, dtype=f32)
        d["pieces"] = _z(4 * 10, dtype=f32)
        d["pieces16"] = _z(4 * 10)
        d["shard"] = _z(10)
        return d
    hyper = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.2, step=7)
    L3 = lambda t, c: [t[f"{c}{k}"] for k in range(3)]
    yield case("adamw_/plain", opt, lambda t: ops.adamw_(t["p0"], t["g0"], t["m0"], t["v0"], grad_scale=0.5, **hyper))
    yield case("adamw_/err_moments", opt, lambda t: ops.adamw_(t["p0"], t["g0"], t["m1"], t["v0"], **hyper))
    yield case("adamw_multi_/plain", opt, lambda t: ops.adamw_multi_(L3(t, "p"), L3(t, "g"), L3(t, "m"), L3(t, "v"), **hyper))
    yield case("adamw_multi_/coef_clamp", opt,
               lambda t: ops.adamw_multi_(L3(t, "p"), L3(t, "g"), L3(t, "m"), L3(t, "v"), grad_scale=2.0, grad_scale_dev=t["coef"],
                                          clamp_index=1, clamp=(0.0, 4.6), **hyper))
    yield case("adamw_multi_/empty", opt, lambda t: ops.adamw_multi_([], [], [], [], **hyper))
    yield case("adamw_multi_/err_mixed", opt,
               lambda t: ops.adamw_multi_([t["p0"], t["m1"]], [t["g0"], t["g1"]], [t["m0"], t["m1"]], [t["v0"], t["v1"]], **hyper))
    yield case("grad_sqnorm/mixed", opt, lambda t: ops.grad_sqnorm([t["g0"], t["g32"], t["g1"], t["m2"]]))
    yield case("grad_sqnorm/bf16_buf", opt, lambda t: ops.grad_sqnorm([t["g1"]], t["buf"]))
    yield case("grad_sqnorm/err", opt, lambda t: ops.grad_sqnorm([t["g0"], t["g32"][::2]]))
    yield case("clip_coef/plain", opt, lambda t: ops.clip_coef(t["buf"], 1.0))
    yield case("grad_clip_coef/plain", opt, lambda t: ops.grad_clip_coef([t["g0"], t["g32"]], 2.0))
    yield case("reduce_shards/f32", opt, lambda t: ops.reduce_shards(t["pieces"], 4))
    yield case("reduce_shards/bf16_out_scale", opt, lambda t: ops.reduce_shards(t["pieces16"], 4, out=t["shard"], scale=1.0))
    yield case("reduce_shards/f32_to_bf16", opt, lambda t: ops.reduce_shards(t["pieces"], 4, out_dtype=bf16))
    yield case("reduce_shards/err", opt, lambda t: ops.reduce_shards(t["pieces"], 3))


def _cases():
    yield from _gemm_nt_cases()
    yield from _gemm_f8_cases()
    yield from _other_cases()


def record(profile):
    """-> ({case: {"calls", "allocs", "returns" | "error"}}, profile_stop()'s summary when `profile`)."""
    rec, out, prof = _Recorder(), {}, None
    with _host_only(rec):
        if profile:
            ops.profile_start(detail=True)
        for name, make, fn in _cases():
            named = make()
            rec.begin({k: v for k, v in named.items() if torch.is_tensor(v)})
            entry = {}
            try:
                entry["returns"] = rec.describe(fn(named))
            except (RuntimeError, AttributeError) as e:
                entry["error"] = f"{type(e).__name__}: {e}"
            entry["calls"], entry["allocs"] = rec.calls, sorted(rec.allocs)
            assert name not in out, name
            out[name] = entry
        ops.check_token_ids(wait=True)
        if profile:
            prof = {k: {f: v[f] for f in ("launches", "work", "bytes")} for k, v in ops.profile_stop().items()}
    return out, prof


def _canon(x):
    """Through JSON text, so that 1, 1.0 and true stay three different things."""
    return json.dumps(x, sort_keys=True)


@pytest.fixture(scope="module")
def golden_trace():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def traced():
    plain, _ = record(profile=False)
    again, prof = record(profile=True)
    return plain, again, prof


def _case_names():
    if not os.path.exists(GOLDEN):      # only while --write creates it
        return []
    with open(GOLDEN) as f:
        return sorted(json.load(f)["cases"])


def test_the_cases_are_the_golden_file_s(golden_trace, traced):
    assert sorted(traced[0]) == sorted(golden_trace["cases"])
    assert len(golden_trace["commit"]) == 40


@pytest.mark.parametrize("name", _case_names())
def test_launch_trace(name, golden_trace, traced):
    """Calls, allocations, returned tensors and error text of one case equal the golden trace, with and without the profiler."""
    want = golden_trace["cases"][name]
    for got in (traced[0][name], traced[1][name]):
        for field in ("error", "calls", "allocs", "returns"):
            assert _canon(got.get(field)) == _canon(want.get(field)), (name, field)


def test_profiler_records(golden_trace, traced):
    got, want = traced[2], golden_trace["profile"]
    assert sorted(got) == sorted(want)
    for key in want:
        assert _canon(got[key]) == _canon(want[key]), key


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--write":
        sys.exit("usage: python -m tests.test_ops_launches_cpu --write <path>   (from a worktree of the commit to pin)")
    commit = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    cases, prof = record(profile=True)
    plain, _ = record(profile=False)
    assert _canon(plain) == _canon(cases)
    with open(sys.argv[2], "w") as f:
        f.write('{"commit": "%s",\n "cases": {\n' % commit)
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in cases.items()))
        f.write('\n },\n "profile": {\n')
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in sorted(prof.items())))
        f.write("\n }\n}\n")
    print(f"{len(cases)} cases, {sum(len(c['calls']) for c in cases.values())} calls, {len(prof)} profiler keys -> {sys.argv[2]}")
