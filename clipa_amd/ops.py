"""Tensor-level wrappers over the C ABI: argument checking, output / workspace allocation with torch,
current-stream plumbing.  No arithmetic happens here - every op below is one or two HIP launches.
"""
import ctypes
import math
import threading

import torch

from . import lib

EPI_NONE, EPI_ACT, EPI_ADD, EPI_DACT = 0, 1, 2, 3
EPI_ACT_PRE8, EPI_DACT8 = 4, 5      # include/clipa_hip.h: e4m3 pre-activation copy / e4m3 second operand (whole-tile shapes)
ACT_GELU_ERF, ACT_GELU_TANH, ACT_QUICK_GELU = 0, 1, 2
DT_U8, DT_BF16, DT_F32 = 0, 1, 2
POOL_FIRST, POOL_LAST, POOL_INDEX, POOL_MEAN_ALL, POOL_MEAN_PATCH = 0, 1, 2, 3, 4
FMT_E4M3, FMT_E5M2 = 0, 1

bf16 = torch.bfloat16
f32 = torch.float32
u8 = torch.uint8

# ---- optional per-launch timing (bench.py roofline): HIP events on the launch stream ------------
_PROF = None
_DETAIL = False      # profile_start(detail=True): additionally key the records by shape ("gemm_nt|M,N,K,epi")

# Out-of-range token ids: nn.Embedding raises; the kernels count them into a device int32 instead of clamping silently.
# The count is fetched without stalling the stream (pinned buffer + event) and checked at the next embedding call or by
# `check_token_ids()`: a bad id surfaces as a RuntimeError at most one step late.
_OOB_PENDING = []
_OOB_LOCK = threading.Lock()      # appended to from the autograd thread (embed_tokens_bwd), drained from the main thread


def profile_start(detail=False):
    global _PROF, _DETAIL
    _PROF = {}
    _DETAIL = bool(detail)


def profile_stop():
    """-> {kernel: {"launches", "ms", "work"}}; work = algorithmic FLOPs (GEMM/attention) of the launches."""
    global _PROF
    prof, _PROF = _PROF, None
    if not prof:
        return {}
    torch.cuda.synchronize()
    out = {}
    for name, recs in prof.items():
        out[name] = {"launches": len(recs), "ms": sum(r[0].elapsed_time(r[1]) for r in recs),
                     "work": float(sum(r[2] for r in recs)), "bytes": float(sum(r[3] for r in recs))}
    return out


class _Timed:
    __slots__ = ("name", "work", "nbytes", "a", "tag")

    def __init__(self, name, work, nbytes=0.0, tag=None):
        self.name, self.work, self.nbytes, self.tag = name, work, nbytes, tag

    def __enter__(self):
        if _PROF is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if _PROF is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            _PROF.setdefault(self.name, []).append((self.a, b, self.work, self.nbytes))
            if self.name == "gemm_nt" and self.tag is not None:       # the family split by epilogue ("gemm_nt#epi3,aux8+act")
                _PROF.setdefault("gemm_nt#" + self.tag[self.tag.index("epi"):], []).append((self.a, b, self.work, self.nbytes))
            if _DETAIL and self.tag is not None:
                _PROF.setdefault(f"{self.name}|{self.tag}", []).append((self.a, b, self.work, self.nbytes))
        return False


# ---- helpers ---------------------------------------------------------------------------------------
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _chk(t, dtype, name, dims=None):
    if not t.is_cuda:
        raise RuntimeError(f"clipa_amd.ops: {name} must live on the GPU (no CPU fallback); got {t.device}")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"clipa_amd.ops: {name} must be {dtype}, got {t.dtype}")
    if dims is not None and t.dim() != dims:
        raise RuntimeError(f"clipa_amd.ops: {name} must be {dims}-D, got shape {tuple(t.shape)}")
    if t.dim() > 0 and t.stride(-1) != 1 and t.shape[-1] != 1:
        raise RuntimeError(f"clipa_amd.ops: {name} must be contiguous in its last dim")


def _chk_out_dtype(dtype, name):
    """The kernels store f32, or bf16 when told so: any other dtype would be allocated and then overrun by the f32 store."""
    if dtype not in (f32, bf16):
        raise RuntimeError(f"clipa_amd.ops.{name}: out_dtype must be torch.float32 or torch.bfloat16, got {dtype}")


def _rowmajor(t):
    """Accept [rows, cols] views with unit column stride; return (tensor, ld)."""
    if t.stride(-1) != 1:
        t = t.contiguous()
    return t, t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _workspace(name, *dims, device, dtype=f32, floor=4):
    """The scratch buffer of a kernel, sized by the library's own query `name(*dims)`: -> (buffer, its size in bytes as the kernel
    wants it passed).  floor: the smallest allocation in bytes (a query may answer 0; a null pointer would be an argument error)."""
    wsb = lib.query(name, *dims)
    return torch.empty(max(wsb, floor) // dtype.itemsize, device=device, dtype=dtype), wsb


def _qkv_ptrs(t, D):
    """The q | k | v column blocks of a bf16 [rows, 3D] matrix (or of its gradient) as three pointers."""
    base = t.data_ptr()
    return ctypes.c_void_p(base), ctypes.c_void_p(base + 2 * D), ctypes.c_void_p(base + 4 * D)


def _aligned_rows(x):
    """[N, E] f32 -> (row-major tensor, row stride) with 16-byte aligned rows, as the retrieval kernels load them: a matrix that
    is not becomes an [N, E] view of a fresh [N, E rounded up to 4] buffer."""
    x, ld = _rowmajor(x)
    if ld % 4 or x.data_ptr() % 16:
        n, e = x.shape
        buf = torch.empty((n, (e + 3) // 4 * 4), device=x.device, dtype=x.dtype)
        buf[:, :e] = x
        x, ld = buf[:, :e], buf.shape[1]
    return x, ld


def _aligned16(t):
    """A [rows, E] bf16 operand of the similarity-loss kernels -> (tensor, ld).  Their global -> LDS loads move 16 bytes per lane:
    next to ld % 8 == 0 (checked on the C side) the first element has to be 16-byte aligned, which a column slice at an offset
    that is no multiple of 8 (buf[:, 4:76]) is not.  Such a view is copied, as _aligned_rows does for the eval kernels."""
    t, ld = _rowmajor(t)
    if t.data_ptr() % 16:
        t = t.contiguous()
        if t.data_ptr() % 16:      # dense already, at an odd offset of its buffer
            t = t.clone()
        ld = t.shape[1]
    return t, ld


def _scalar1(scale):
    """An optional f32 device scalar as the contiguous [1] tensor the kernels read."""
    if scale is None:
        return None
    _chk(scale, f32, "scale")
    return scale.reshape(1).contiguous()


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _numel_array(tensors):
    return (ctypes.c_int64 * len(tensors))(*[t.numel() for t in tensors])


# ---- NT GEMMs: one planning step, one launch path ----------------------------------------------------
def _whole_tiles(M, N, K, f8=False):
    """Shapes the four-wave GEMM kernels take (gemm_nta.hip: nta_eligible; f8=True: gemm_f8a.hip: f8a_eligible, whose K tile is
    twice as deep): the fused e4m3 epilogues exist only there."""
    kt = 256 if f8 else 128
    return M % 256 == 0 and N % 256 == 0 and K % kt == 0 and K >= 2 * kt


def _plan_nt(M, N, K, *, f8, epi, want_pre, aux8, want_act=False, out_f32=False, dense_out=True, fmt_b=FMT_E4M3, sa=True,
             bias=False, out_scale=False, want_colsum=False, emit=False):
    """How an NT GEMM request is served: -> (entry point, epilogue code, unfused steps).  Every extra of a request (an e4m3
    pre-activation copy, an e4m3 second operand, its activation, a quantised output, the emitted weight-gradient operand) is
    written by the GEMM's own epilogue where a kernel for it exists - whole-tile shapes, e4m3 weights - and is otherwise one
    more launch before or after a plainer GEMM, named in `unfused`: "decode_aux" (e4m3_to_bf16 before), "cast_pre" (cast_e4m3
    of the bf16 pre-activation), "act" (activation_fwd of the operand), "quantize" (scale_quantize_rows [+ colsum] of the bf16
    output), "emit" (scale_quantize_rows of the operand)."""
    whole = _whole_tiles(M, N, K, f8) and fmt_b == FMT_E4M3
    entry, unfused = "clipa_gemm_nt_f8" if f8 else "clipa_gemm_nt", []
    if emit:
        if whole and sa:
            entry = "clipa_gemm_nt_f8_emit"
        else:
            unfused.append("emit")
    if out_scale:
        if whole and ((epi == EPI_ACT and not want_colsum) or (epi == EPI_DACT and aux8 and not bias)):
            entry = "clipa_gemm_nt_f8q"
        else:
            unfused.append("quantize")
    if want_act and not (whole and dense_out):
        unfused.append("act")
    if want_pre == "e4m3" and not (epi == EPI_ACT and not out_f32 and whole):
        unfused.append("cast_pre")
    if aux8 and not whole:
        unfused.append("decode_aux")
    code = EPI_DACT8 if aux8 and whole else EPI_ACT_PRE8 if want_pre == "e4m3" and "cast_pre" not in unfused else epi
    return entry, code, unfused


def _gemm_nt(who, a, b, bias=None, *, sa=None, sb=None, epi=EPI_NONE, act=ACT_GELU_ERF, aux=None, alpha=1.0, out_f32=False,
             want_pre=False, out=None, want_act=False, fmt_a=FMT_E4M3, fmt_b=FMT_E4M3, out_scale=None, want_colsum=False, emit=None):
    """The launch path of gemm_nt (who = "gemm_nt": bf16 operands) and of gemm_nt_f8 / gemm_nt_f8_emit ("gemm_nt_f8": fp8 bytes
    with row scales sa, sb; emit = the tensor scale t).  -> (C, pre-activation or activation | None, column sums | None, emitted
    operand | None), fused or not as _plan_nt says."""
    f8 = who == "gemm_nt_f8"
    aux8 = aux is not None and aux.dtype == u8
    if aux8 and epi != EPI_DACT:
        raise RuntimeError(f"{who}: an e4m3 (uint8) second operand goes with EPI_DACT only")
    _chk(a, u8 if f8 else bf16, "a8" if f8 else "a", 2)
    _chk(b, u8 if f8 else bf16, "b8" if f8 else "b", 2)
    a, lda = _rowmajor(a)
    b, ldb = _rowmajor(b)
    M, K = a.shape
    N, Kb = b.shape
    entry, code, unfused = _plan_nt(M, N, K, f8=f8, epi=epi, want_pre=want_pre, aux8=aux8, want_act=want_act, out_f32=out_f32,
                                    dense_out=out is None or out.stride(0) == N, fmt_b=fmt_b, sa=sa is not None,
                                    bias=bias is not None, out_scale=out_scale is not None, want_colsum=want_colsum,
                                    emit=emit is not None)
    fused_emit, fused_q = entry == "clipa_gemm_nt_f8_emit", entry == "clipa_gemm_nt_f8q"
    if "cast_pre" in unfused:
        out_f32 = False      # GEMM + cast has always answered in bf16, whatever out_f32 asked for
    if fused_emit:
        _chk(emit, f32, "t")
        if Kb != K or tuple(aux.shape) != (M, N) or sa.numel() != M or (sb is not None and sb.numel() != N):
            raise RuntimeError("gemm_nt_f8_emit: shape mismatch")
    operand = aux
    if "decode_aux" in unfused:
        aux = e4m3_to_bf16(aux)
    if K != Kb:
        raise RuntimeError(f"{who}: K mismatch {K} vs {Kb}")
    if fused_q:
        _chk(out_scale, f32, "out_scale", 1)
        if out_scale.numel() != M:
            raise RuntimeError(f"gemm_nt_f8: out_scale has {out_scale.numel()} entries for {M} rows")
    for name, t, n in (("sa", sa, M), ("sb", sb, N)):
        if t is not None:
            _chk(t, f32, name, 1)
            if t.numel() != n or not t.is_contiguous():
                raise RuntimeError(f"{who}: {name} must be a contiguous f32 vector of {n} elements")
    if bias is not None:
        _chk(bias, f32, "bias", 1)
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=u8 if fused_q else f32 if out_f32 else bf16)
    ldc = out.stride(0) if M > 1 else N
    pre8, fused_act = code == EPI_ACT_PRE8, want_act and "act" not in unfused
    pre = torch.empty((M, N), device=a.device, dtype=u8 if pre8 else bf16) if (want_pre or fused_act) else None
    if pre8 and ldc != N:
        raise RuntimeError(f"{who}: want_pre='e4m3' needs a dense output (the copy shares its row stride)")
    ldaux = 0
    if aux is not None:
        _chk(aux, u8 if code == EPI_DACT8 else bf16, "aux", 2)
        aux, ldaux = _rowmajor(aux)
    part = torch.empty((M // 128, N), device=a.device, dtype=f32) if fused_q and epi == EPI_DACT else None
    x8 = torch.empty((M, N), device=a.device, dtype=u8) if fused_emit else None
    nbytes = (1.0 if f8 else 2.0) * (M * K + N * K) + out.element_size() * M * N + \
        (float(aux.element_size()) * M * N if aux is not None else 0) + ((1.0 if pre8 else 2.0) * M * N if want_pre else 0)
    if fused_act:
        nbytes += 2.0 * M * N
    if fused_emit:
        nbytes += 1.0 * M * N
    tag_epi = "1+pre8" if pre8 else "3,aux8" if code == EPI_DACT8 else f"{epi}{'+pre' if want_pre else ''}"
    tag_epi += "+act" if fused_act else "+emit" if fused_emit else ""
    dims = (M, N, K, lda, ldb, ldc, ldaux)
    with _Timed(who, 2.0 * M * N * K, nbytes, f"{M},{N},{K},epi{tag_epi}{',f32' if out_f32 else ''}{',q8' if fused_q else ''}"):
        if not f8:
            lib.call(entry, _p(a), _p(b), _p(out), _p(pre), _p(bias), _p(aux), *dims, float(alpha), code, act,
                     1 if out_f32 else 0, _stream())
        elif fused_emit:
            lib.call(entry, _p(a), _p(b), _p(sa), _p(sb), _p(out), _p(x8), _p(aux), _p(emit), *dims, act, int(fmt_a), _stream())
        elif fused_q:
            lib.call(entry, _p(a), _p(b), _p(sa), _p(sb), _p(out), _p(pre), _p(bias), _p(aux), _p(out_scale.contiguous()), _p(part),
                     *dims, float(alpha), code, act, int(fmt_a), _stream())
        else:
            lib.call(entry, _p(a), _p(b), _p(sa), _p(sb), _p(out), _p(pre), _p(bias), _p(aux), *dims, float(alpha), code, act,
                     int(fmt_a), int(fmt_b), _stream())
    cs = None
    if "cast_pre" in unfused:
        pre = cast_e4m3(pre)
    if "act" in unfused:
        pre = activation_fwd(operand, act)
    if "quantize" in unfused:
        dense = out
        out = scale_quantize_rows(dense, out_scale, torch.ones(1, device=out.device, dtype=f32))
        if want_colsum:
            cs = colsum(dense)
    elif fused_q and want_colsum:
        cs = torch.empty(N, device=a.device, dtype=f32)
        lib.call("clipa_reduce_partial_rows", _p(part), _p(cs), M // 128, N, _stream())
    if "emit" in unfused:
        x8 = scale_quantize_rows(operand, sa, emit, act=act)
    return out, pre, cs, x8


def gemm_nt(a, b, bias=None, *, epi=EPI_NONE, act=ACT_GELU_ERF, aux=None, alpha=1.0, out_f32=False,
            want_pre=False, out=None, want_act=False):
    """C[M,N] = epi(alpha * a[M,K] @ b[N,K]^T + bias). a, b bf16; bias f32 [N].
    want_pre: True -> also the bf16 pre-activation; "e4m3" -> it as saturating e4m3 bytes (uint8 [M,N], the "light8" keep tier:
    fused into the epilogue on whole-tile shapes, GEMM + cast otherwise).  aux of EPI_DACT may be such a uint8 tensor;
    want_act (with it): -> (C, act(aux) as bf16 [M,N]) - what activation_fwd(aux, act) returns, written by the epilogue that
    reads the bytes anyway on whole-tile shapes (by activation_fwd otherwise)."""
    if want_act and not (epi == EPI_DACT and aux is not None and aux.dtype == u8 and not want_pre and not out_f32):
        raise RuntimeError("gemm_nt: want_act goes with EPI_DACT on an e4m3 (uint8) second operand")
    out, pre, _, _ = _gemm_nt("gemm_nt", a, b, bias, epi=epi, act=act, aux=aux, alpha=alpha, out_f32=out_f32, want_pre=want_pre,
                              out=out, want_act=want_act)
    return (out, pre) if (want_pre or want_act) else out


def gemm_nt_f8(a8, sa, b8, sb, bias=None, *, epi=EPI_NONE, act=ACT_GELU_ERF, aux=None, alpha=1.0, want_pre=False,
               fmt_a=FMT_E4M3, fmt_b=FMT_E4M3, out_scale=None, want_colsum=False):
    """C[M,N] bf16 = epi(alpha * sa[m] * sb[n] * a8[M,K] @ b8[N,K]^T + bias); a8, b8 uint8 tensors of fp8 bytes.
    want_pre: True -> also the bf16 pre-activation; "e4m3" -> it as saturating e4m3 bytes (uint8 [M,N]: fused into the epilogue on
    whole-tile shapes, GEMM + cast otherwise).  aux of EPI_DACT may be such a uint8 tensor.
    out_scale (f32 [M]; round 6): the output leaves as e4m3 bytes, row m = the bf16 result times out_scale[m] (the operand of the
    next GEMM with de-quantisation scale 1 / out_scale: row_bound) - written by the epilogue itself for EPI_ACT and for EPI_DACT
    from an e4m3 operand on whole-tile shapes, GEMM + scaled quantiser otherwise; want_colsum (EPI_DACT): also the column sums of
    the unscaled outputs (f32 [N]).  -> q8 [, pre] [, colsum]."""
    out, pre, cs, _ = _gemm_nt("gemm_nt_f8", a8, b8, bias, sa=sa, sb=sb, epi=epi, act=act, aux=aux, alpha=alpha, want_pre=want_pre,
                               fmt_a=fmt_a, fmt_b=fmt_b, out_scale=out_scale, want_colsum=want_colsum)
    res = [out] + ([pre] if want_pre else []) + ([cs] if want_colsum and out_scale is not None else [])
    return res[0] if len(res) == 1 else tuple(res)


def gemm_nt_f8_emit(a8, sa, b8, sb, aux8, t, *, act=ACT_GELU_ERF, fmt_a=FMT_E4M3):
    """EPI_DACT from the kept e4m3 pre-activation that also emits the activation operand of the same layer's fp8 weight gradient:
    -> (C bf16 [M,N] = gemm_nt_f8(a8, sa, b8, sb, epi=EPI_DACT, aux=aux8), X8 uint8 [M,N] = scale_quantize_rows(aux8, sa, t, act=act)),
    X8 written by the GEMM's epilogue on whole-tile shapes (clipa_gemm_nt_f8_emit), by the two separate launches otherwise."""
    out, _, _, x8 = _gemm_nt("gemm_nt_f8", a8, b8, None, sa=sa, sb=sb, epi=EPI_DACT, act=act, aux=aux8, fmt_a=fmt_a, emit=t)
    return out, x8


def cast_e4m3(x):
    """bf16 -> saturating OCP e4m3 bytes (uint8, same shape): the unfused form of gemm_nt(..., want_pre="e4m3")."""
    _chk(x, bf16, "x")
    x = x.contiguous()
    out = torch.empty(x.shape, device=x.device, dtype=u8)
    with _Timed("cast_e4m3", 0.0, 3.0 * x.numel()):
        lib.call("clipa_cast_bf16_to_e4m3", _p(x), _p(out), x.numel(), _stream())
    return out


def e4m3_to_bf16(x8):
    """e4m3 bytes (uint8) -> bf16 (exact)."""
    _chk(x8, u8, "x8")
    x8 = x8.contiguous()
    out = torch.empty(x8.shape, device=x8.device, dtype=bf16)
    with _Timed("cast_e4m3", 0.0, 3.0 * x8.numel()):
        lib.call("clipa_cast_e4m3_to_bf16", _p(x8), _p(out), x8.numel(), _stream())
    return out


def quantize_rows(x, fmt=FMT_E4M3, want_colsum=False, want_rownorm=False):
    """Row-scaled fp8 operand of a bf16 matrix: -> (q uint8 [M,K] holding OCP e4m3 / e5m2 bytes, dq f32 [M]) with
    x[r,:] ~ dq[r] * fp8(q[r,:]).  want_colsum: also sum_r x[r,:] (f32 [K]; the bias gradient when x is a layer's dY);
    want_rownorm (with want_colsum): also ||x[r,:]||_2 (f32 [M]: the row bound of the product this gradient feeds, row_bound)."""
    if want_rownorm and not want_colsum:
        raise RuntimeError("clipa_amd.ops.quantize_rows: want_rownorm needs want_colsum")
    _chk(x, bf16, "x", 2)
    x, ld = _rowmajor(x)
    M, K = x.shape
    q = torch.empty((M, K), device=x.device, dtype=u8)
    dq = torch.empty(M, device=x.device, dtype=f32)
    if want_colsum:
        cs = torch.empty(K, device=x.device, dtype=f32)
        rn = torch.empty(M, device=x.device, dtype=f32) if want_rownorm else None
        ws, wsb = _workspace("clipa_quantize_rows_colsum_workspace", M, K, device=x.device)
        with _Timed("quantize_rows", 0.0, 3.0 * M * K, f"{M},{K},+colsum"):
            lib.call("clipa_quantize_rows_colsum", _p(x), _p(q), _p(dq), _p(cs), _p(rn), M, K, ld, K, int(fmt), _p(ws), wsb, _stream())
        return (q, dq, cs, rn) if want_rownorm else (q, dq, cs)
    with _Timed("quantize_rows", 0.0, 3.0 * M * K, f"{M},{K}"):
        lib.call("clipa_quantize_rows", _p(x), _p(q), _p(dq), M, K, ld, K, int(fmt), _stream())
    return q, dq


def layernorm_fwd_q8(x, gamma, beta, eps=1e-5, want_bf16=False, want_rownorm=False):
    """LayerNorm of bf16 rows emitting the e4m3 operand of the next GEMM: -> (y bf16 | None, q uint8, dq f32 [rows]) (+ the rows'
    L2 norms, f32 [rows], with want_rownorm)."""
    _chk(x, bf16, "x")
    _chk(gamma, f32, "gamma", 1)
    _chk(beta, f32, "beta", 1)
    x = x.contiguous()
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty(x.shape, device=x.device, dtype=bf16) if want_bf16 else None
    q = torch.empty(x.shape, device=x.device, dtype=u8)
    dq = torch.empty(rows, device=x.device, dtype=f32)
    rn = torch.empty(rows, device=x.device, dtype=f32) if want_rownorm else None
    with _Timed("ln_fwd_q8", 0.0, float(rows) * D * (3 + (2 if want_bf16 else 0)), f"{rows},{D}"):
        lib.call("clipa_layernorm_fwd_q8n", _p(x), _p(gamma), _p(beta), _p(y), _p(q), _p(dq), _p(rn), rows, D, float(eps), _stream())
    return (y, q, dq, rn) if want_rownorm else (y, q, dq)


def row_bound(rownorm, wnorm, bmax=None, factor=1.13):
    """Predicted row scales of a GEMM output: bound[m] = factor * rownorm[m] * wnorm[0] + bmax[0] >= every |output| of row m
    (Cauchy-Schwarz; factor 1.13 covers the e4m3 rounding of both operands) -> (scale = bound / 448, inv = 448 / bound), f32 [M]."""
    _chk(rownorm, f32, "rownorm", 1)
    _chk(wnorm, f32, "wnorm", 1)
    if bmax is not None:
        _chk(bmax, f32, "bmax", 1)
    M = rownorm.numel()
    scale = torch.empty(M, device=rownorm.device, dtype=f32)
    inv = torch.empty(M, device=rownorm.device, dtype=f32)
    lib.call("clipa_row_bound", _p(rownorm.contiguous()), _p(wnorm), _p(bmax), float(factor), _p(scale), _p(inv), M, _stream())
    return scale, inv


def rownorm_max(w):
    """f32 device scalar [1] = max_r ||w[r,:]||_2 of a bf16 matrix (a weight operand: once per optimizer step)."""
    _chk(w, bf16, "w", 2)
    w, ld = _rowmajor(w)
    out = torch.empty(1, device=w.device, dtype=f32)
    lib.call("clipa_rownorm_max", _p(w), w.shape[0], w.shape[1], ld, _p(out), _stream())
    return out


def absmax(v):
    """f32 device scalar [1] = max |v[i]| of an f32 vector (a bias)."""
    _chk(v, f32, "v", 1)
    out = torch.empty(1, device=v.device, dtype=f32)
    lib.call("clipa_absmax_f32", _p(v.contiguous()), v.numel(), _p(out), _stream())
    return out


def rowscale_max(a, b=None):
    """f32 device scalar [1] = max_m a[m] * b[m] (b None = 1): the tensor scale t of an fp8 weight-gradient operand."""
    _chk(a, f32, "a", 1)
    a = a.contiguous()
    if b is not None:
        _chk(b, f32, "b", 1)
        b = b.contiguous()
        if b.numel() != a.numel():
            raise RuntimeError(f"rowscale_max: {a.numel()} vs {b.numel()} rows")
    out = torch.empty(1, device=a.device, dtype=f32)
    lib.call("clipa_rowscale_max", _p(a), _p(b), a.numel(), _p(out), _stream())
    return out


def scale_quantize_rows(x, rowscale, t, act=-1):
    """q[m,:] = e4m3(act(x[m,:]) * rowscale[m] / t[0]) - the activation operand of an fp8 weight gradient (act -1 = none).
    x bf16, or uint8 e4m3 bytes (the kept pre-activation of the "h8" tier)."""
    in8 = x.dtype == u8
    _chk(x, u8 if in8 else bf16, "x", 2)
    _chk(rowscale, f32, "rowscale", 1)
    _chk(t, f32, "t", 1)
    x, ld = _rowmajor(x)
    M, K = x.shape
    if rowscale.numel() != M:
        raise RuntimeError(f"scale_quantize_rows: {rowscale.numel()} row scales for {M} rows")
    q = torch.empty((M, K), device=x.device, dtype=u8)
    with _Timed("scale_quantize_rows", 0.0, (2.0 if in8 else 3.0) * M * K, f"{M},{K},act{act}{',in8' if in8 else ''}"):
        lib.call("clipa_scale_quantize_rows_e4m3" if in8 else "clipa_scale_quantize_rows", _p(x), _p(rowscale.contiguous()), _p(t),
                 _p(q), M, K, ld, K, int(act), _stream())
    return q


def layernorm_fwd_q8s(x, gamma, beta, rowscale, t, eps=1e-5):
    """q[m,:] = e4m3(LayerNorm(x)[m,:] * rowscale[m] / t[0]): the LayerNorm output as the activation operand of an fp8 weight gradient."""
    _chk(x, bf16, "x")
    _chk(gamma, f32, "gamma", 1)
    _chk(beta, f32, "beta", 1)
    _chk(rowscale, f32, "rowscale", 1)
    _chk(t, f32, "t", 1)
    x = x.contiguous()
    D = x.shape[-1]
    rows = x.numel() // D
    if rowscale.numel() != rows:
        raise RuntimeError(f"layernorm_fwd_q8s: {rowscale.numel()} row scales for {rows} rows")
    q = torch.empty(x.shape, device=x.device, dtype=u8)
    with _Timed("ln_fwd_q8", 0.0, 3.0 * rows * D, f"{rows},{D},s"):
        lib.call("clipa_layernorm_fwd_q8s", _p(x), _p(gamma), _p(beta), _p(rowscale.contiguous()), _p(t), _p(q), rows, D, float(eps), _stream())
    return q


def gemm_tn_f8(p8, q8, t=None, alpha=1.0, fmt_p=FMT_E4M3, out_dtype=f32):
    """out[R,C] = alpha * t[0] * p8[M,R]^T @ q8[M,C]; p8 (fmt_p: e4m3 / e5m2), q8 (e4m3) uint8 tensors of fp8 bytes, t an
    optional f32 device scalar."""
    _chk_out_dtype(out_dtype, "gemm_tn_f8")
    _chk(p8, u8, "p8", 2)
    _chk(q8, u8, "q8", 2)
    p8, ldp = _rowmajor(p8)
    q8, ldq = _rowmajor(q8)
    M, R = p8.shape
    M2, C = q8.shape
    if M != M2:
        raise RuntimeError(f"gemm_tn_f8: M mismatch {M} vs {M2}")
    if t is not None:
        _chk(t, f32, "t", 1)
    ws, wsb = _workspace("clipa_gemm_tn_f8_workspace", M, R, C, device=p8.device)
    out = torch.empty((R, C), device=p8.device, dtype=out_dtype)
    with _Timed("gemm_tn_f8", 2.0 * M * R * C, 1.0 * M * (R + C) + out.element_size() * R * C, f"{M},{R},{C}"):
        lib.call("clipa_gemm_tn_f8", _p(p8), _p(q8), _p(out), M, R, C, ldp, ldq, float(alpha), _p(t), int(fmt_p),
                 1 if out_dtype == bf16 else 0, _p(ws), wsb, _stream())
    return out


def gemm_tn(p, q, out_dtype=f32, want_colsum=False):
    """out[R,C] = p[M,R]^T @ q[M,C]; p, q bf16.  want_colsum: also return sum_m p[m,:] (f32 [R])."""
    _chk_out_dtype(out_dtype, "gemm_tn")
    _chk(p, bf16, "p", 2)
    _chk(q, bf16, "q", 2)
    p, ldp = _rowmajor(p)
    q, ldq = _rowmajor(q)
    M, R = p.shape
    M2, C = q.shape
    if M != M2:
        raise RuntimeError(f"gemm_tn: M mismatch {M} vs {M2}")
    ws, wsb = _workspace("clipa_gemm_tn_workspace", M, R, C, ctypes.byref(ctypes.c_int64(0)), device=p.device)
    out = torch.empty((R, C), device=p.device, dtype=out_dtype)
    cs = torch.empty(R, device=p.device, dtype=f32) if want_colsum else None
    with _Timed("gemm_tn", 2.0 * M * R * C, 2.0 * M * (R + C) + out.element_size() * R * C, f"{M},{R},{C}"):
        lib.call("clipa_gemm_tn", _p(p), _p(q), _p(out), _p(cs), M, R, C, ldp, ldq, 1 if out_dtype == bf16 else 0, _p(ws),
                 wsb, _stream())
    return (out, cs) if want_colsum else out


def layernorm_fwd(x, gamma, beta, eps=1e-5, out_dtype=None):
    _chk(gamma, f32, "gamma", 1)
    _chk(beta, f32, "beta", 1)
    x = x.contiguous()
    D = x.shape[-1]
    rows = x.numel() // D
    out_dtype = out_dtype or x.dtype
    y = torch.empty(x.shape, device=x.device, dtype=out_dtype)
    with _Timed("ln_fwd", 0.0, float(rows) * D * (x.element_size() + y.element_size()), f"{rows},{D}"):
        lib.call("clipa_layernorm_fwd", _p(x), _p(gamma), _p(beta), _p(y), rows, D, float(eps),
                 int(x.dtype == f32), int(out_dtype == f32), _stream())
    return y


def layernorm_bwd(x, gamma, dy, dres=None, eps=1e-5, beta=None, q8_fmt=None, want_rownorm=False):
    """Returns dx (dtype of x, + dres if given), dgamma, dbeta (f32) - and, when `beta` is given, y = LayerNorm(x) (dtype of
    dy) as a fourth value: bit for bit what layernorm_fwd returns, written by the pass that has the rows in registers anyway.
    q8_fmt (FMT_E4M3 / FMT_E5M2; bf16 tensors): a last value (q, dq, colsum[, rownorm]) = quantize_rows(dx, q8_fmt, want_colsum=True
    [, want_rownorm=True]) - the fp8 operand of the linear layer this gradient reaches next, from the same pass."""
    x = x.contiguous()
    dy = dy.contiguous()
    if dres is not None:
        dres = dres.contiguous()
    D = x.shape[-1]
    rows = x.numel() // D
    q8 = q8_fmt is not None
    if q8:
        _chk(x, bf16, "x")
        _chk(dy, bf16, "dy")
        if dres is not None:
            _chk(dres, bf16, "dres")
    ws, wsb = _workspace("clipa_layernorm_bwd_q8_workspace" if q8 else "clipa_layernorm_bwd_workspace", rows, D, device=x.device)
    dx = torch.empty_like(x)
    dgamma = torch.empty(D, device=x.device, dtype=f32)
    dbeta = torch.empty(D, device=x.device, dtype=f32)
    if not q8 and dres is not None and dres.dtype != x.dtype:
        raise RuntimeError("layernorm_bwd: dres dtype must match x")
    y = None
    if beta is not None:
        _chk(beta, f32, "beta", 1)
        y = torch.empty(x.shape, device=x.device, dtype=dy.dtype)
    res = (dx, dgamma, dbeta) if y is None else (dx, dgamma, dbeta, y)
    if q8:
        q = torch.empty((rows, D), device=x.device, dtype=u8)
        dq = torch.empty(rows, device=x.device, dtype=f32)
        cs = torch.empty(D, device=x.device, dtype=f32)
        rn = torch.empty(rows, device=x.device, dtype=f32) if want_rownorm else None
        nbytes = float(rows) * D * (7 + (2 if dres is not None else 0) + (2 if y is not None else 0))
        with _Timed("ln_bwd", 0.0, nbytes, f"{rows},{D},+q8{',+y' if y is not None else ''}"):
            lib.call("clipa_layernorm_bwd_q8", _p(x), _p(gamma), _p(beta), _p(dy), _p(dres), _p(dx), _p(y), _p(q), _p(dq), _p(cs), _p(rn),
                     _p(dgamma), _p(dbeta), rows, D, float(eps), int(q8_fmt), _p(ws), wsb, _stream())
        return res + ((q, dq, cs, rn) if want_rownorm else (q, dq, cs),)
    nbytes = float(rows) * D * (2 * x.element_size() + dy.element_size() + (x.element_size() if dres is not None else 0))
    tail = (rows, D, float(eps), int(x.dtype == f32), int(dy.dtype == f32), _p(ws), wsb, _stream())
    if y is not None:
        with _Timed("ln_bwd", 0.0, nbytes + float(rows) * D * y.element_size(), f"{rows},{D},+y"):
            lib.call("clipa_layernorm_bwd_y", _p(x), _p(gamma), _p(beta), _p(dy), _p(dres), _p(dx), _p(y), _p(dgamma), _p(dbeta), *tail)
    else:
        with _Timed("ln_bwd", 0.0, nbytes, f"{rows},{D}"):
            lib.call("clipa_layernorm_bwd", _p(x), _p(gamma), _p(dy), _p(dres), _p(dx), _p(dgamma), _p(dbeta), *tail)
    return res


def _attention(name, qkv, H, causal, pairs, tag):
    """What the four attention wrappers share: -> (D, head dim, softmax scale, the launch's profiler record).  pairs = the
    (query, key) pairs of one head: 4 FLOPs per pair and head-dim element forward, 10 backward, half of them under a causal mask."""
    _chk(qkv, bf16, "qkv", 2)
    D = qkv.shape[1] // 3
    dh = D // H
    work = (4.0 if name == "attention_fwd" else 10.0) * H * pairs * dh * (0.5 if causal else 1.0)
    return D, dh, 1.0 / math.sqrt(dh), _Timed(name, work, 0.0, f"{tag},dh{dh}")


def attention_fwd(qkv, B, L, H, causal, want_stats=False):
    """qkv [B*L, 3*H*64] bf16 (q | k | v column blocks) -> out [B*L, H*64] bf16 (+ softmax statistics
    f32 [B*H*L, 2] for the backward when want_stats)."""
    D, dh, sm_scale, timed = _attention("attention_fwd", qkv, H, causal, B * L * L, f"B{B},H{H},L{L}")
    out = torch.empty((B * L, D), device=qkv.device, dtype=bf16)
    stats = torch.empty((B * H * L, 2), device=qkv.device, dtype=f32) if want_stats else None
    with timed:
        lib.call("clipa_attention_fwd", *_qkv_ptrs(qkv, D), _p(out), _p(stats), B, H, L, dh, qkv.stride(0), D, sm_scale, int(causal),
                 _stream())
    return (out, stats) if want_stats else out


def attention_bwd(qkv, out, dout, stats, B, L, H, causal):
    D, dh, sm_scale, timed = _attention("attention_bwd", qkv, H, causal, B * L * L, f"B{B},H{H},L{L}")
    _chk(stats, f32, "stats", 2)
    _chk(out, bf16, "out", 2)
    _chk(dout, bf16, "dout", 2)
    dout = dout.contiguous()
    dqkv = torch.empty_like(qkv)
    with timed:
        lib.call("clipa_attention_bwd", *_qkv_ptrs(qkv, D), _p(out), _p(dout), _p(stats), *_qkv_ptrs(dqkv, D), B, H, L, dh,
                 qkv.stride(0), D, dqkv.stride(0), sm_scale, int(causal), _stream())
    return dqkv


class VarLen:
    """Packed variable-length sequences (the text tower on the tokens up to each caption's EOT): host-built index structure.
    lens: int64 CPU tensor [B] (>= 1 each).  Sequence b occupies rows [start[b], start[b] + lens[b]) of a [rows, D] token matrix
    whose row count is padded to a multiple of 256 (whole GEMM tiles; the pad rows are zero and belong to no sequence)."""

    def __init__(self, lens, ctx, device):
        lens = lens.to(torch.int64).cpu()
        self.B, self.ctx = int(lens.numel()), int(ctx)
        start = torch.cumsum(lens, 0) - lens
        self.T = int(lens.sum())
        self.rows = max(256, (self.T + 255) // 256 * 256)
        self.lens_host = lens
        put = (lambda t: t.pin_memory().to(device, non_blocking=True)) if torch.device(device).type == "cuda" else (lambda t: t)
        self.seq_start = put(start.to(torch.int32))
        self.seq_len = put(lens.to(torch.int32))
        # packed row -> row of the padded [B * ctx, D] matrix (-1 = pad row: gathers zeros, receives no gradient)
        src = torch.repeat_interleave(torch.arange(self.B) * self.ctx - start, lens) + torch.arange(self.T)
        self.src_rows = put(torch.cat([src, torch.full((self.rows - self.T,), -1, dtype=torch.int64)]))
        self.last_rows = put(start + lens - 1)                     # the EOT token of every sequence, in packed rows
        tiles = (lens + 31) // 32
        self.classes = []                                          # (32-row tiles, int32 device ids, count)
        for k in sorted(set(tiles.tolist())):
            ids = torch.nonzero(tiles == k).flatten().to(torch.int32)
            self.classes.append((int(k), put(ids), int(ids.numel())))
        self.sum_len2 = float((lens.double() ** 2).sum())          # attention work: sum of len^2


def attention_fwd_varlen(qkv, vl, H, causal, want_stats=False):
    """attention_fwd on packed sequences: qkv [vl.rows, 3D] -> out [vl.rows, D] (pad rows zero) (+ statistics [vl.rows * H, 2])."""
    D, dh, sm_scale, timed = _attention("attention_fwd", qkv, H, causal, vl.sum_len2, f"varlen{vl.B},H{H},T{vl.T}")
    out = torch.zeros((vl.rows, D), device=qkv.device, dtype=bf16)
    stats = torch.empty((vl.rows * H, 2), device=qkv.device, dtype=f32)
    with timed:
        for tiles, ids, n in vl.classes:
            lib.call("clipa_attention_fwd_varlen", *_qkv_ptrs(qkv, D), _p(out), _p(stats), _p(vl.seq_start), _p(vl.seq_len), _p(ids),
                     n, tiles, H, dh, qkv.stride(0), D, sm_scale, int(causal), _stream())
    return (out, stats) if want_stats else out


def attention_bwd_varlen(qkv, out, dout, stats, vl, H, causal):
    D, dh, sm_scale, timed = _attention("attention_bwd", qkv, H, causal, vl.sum_len2, f"varlen{vl.B},H{H},T{vl.T}")
    _chk(stats, f32, "stats", 2)
    dout = dout.contiguous()
    dqkv = torch.zeros_like(qkv)                                   # pad rows belong to no sequence: their gradient is zero
    with timed:
        for tiles, ids, n in vl.classes:
            lib.call("clipa_attention_bwd_varlen", *_qkv_ptrs(qkv, D), _p(out), _p(dout), _p(stats), *_qkv_ptrs(dqkv, D),
                     _p(vl.seq_start), _p(vl.seq_len), _p(ids), n, tiles, H, dh, qkv.stride(0), D, dqkv.stride(0), sm_scale,
                     int(causal), _stream())
    return dqkv


def _patch_source(img, mean, std, who):
    """The image operand of patchify / patchify_ln: -> (tensor in NCHW or channels_last memory, B, S, dtype code, nhwc,
    normalize, mean[3], std[3] as C arrays)."""
    if not img.is_cuda:
        raise RuntimeError(f"{who}: image must be on the GPU")
    B, C, S, S2 = img.shape
    if C != 3 or S != S2:
        raise RuntimeError(f"{who}: expected [B,3,S,S], got {tuple(img.shape)}")
    if img.is_contiguous():
        nhwc = 0
    elif img.is_contiguous(memory_format=torch.channels_last):
        nhwc = 1
    else:
        img, nhwc = img.contiguous(), 0
    dt = {torch.uint8: DT_U8, bf16: DT_BF16, f32: DT_F32}.get(img.dtype)
    if dt is None:
        raise RuntimeError(f"{who}: unsupported image dtype {img.dtype}")
    normalize = mean is not None
    m3 = (ctypes.c_float * 3)(*([float(v) for v in mean] if normalize else [0, 0, 0]))
    s3 = (ctypes.c_float * 3)(*([float(v) for v in std] if normalize else [1, 1, 1]))
    return img, B, S, dt, nhwc, int(normalize), m3, s3


def patchify(img, P, Kp, mean=None, std=None):
    """img [B,3,S,S] (NCHW or channels_last memory), u8 / bf16 / f32 -> bf16 [B*(S//P)^2, Kp]."""
    img, B, S, dt, nhwc, normalize, m3, s3 = _patch_source(img, mean, std, "patchify")
    g = S // P
    out = torch.empty((B * g * g, Kp), device=img.device, dtype=bf16)
    with _Timed("patchify", 0.0, float(img.numel()) * img.element_size() + 2.0 * out.numel(), f"{B},{S},{P}"):
        lib.call("clipa_patchify", _p(img), _p(out), B, S, P, Kp, dt, nhwc, normalize, m3, s3, _stream())
    return out


def _chk_patch_geometry(P, Kp, who):
    if P <= 0 or Kp % 8 != 0 or Kp < 3 * P * P or Kp > 3072:
        raise RuntimeError(f"clipa_amd.ops.{who}: bad geometry P={P} Kp={Kp} (Kp % 8 == 0, 3*P*P <= Kp <= 3072)")


def patchify_ln(img, P, Kp, mean=None, std=None, eps=1e-5):
    """patchify followed by the LayerNorm of dual PatchNorm WITHOUT its affine (transformer.py:483-488): img as for patchify ->
    bf16 [B*(S//P)^2, Kp] = (x - mean) * rstd per patch row over its 3*P*P elements (fp32 statistics), (ph,pw,c) order, pad
    columns zero.  A constant patch gives exact zeros."""
    _chk_patch_geometry(P, Kp, "patchify_ln")
    img, B, S, dt, nhwc, normalize, m3, s3 = _patch_source(img, mean, std, "patchify_ln")
    g = S // P
    if g <= 0:
        raise RuntimeError(f"clipa_amd.ops.patchify_ln: image size {S} below the patch size {P}")
    out = torch.empty((B * g * g, Kp), device=img.device, dtype=bf16)
    with _Timed("patchify_ln", 0.0, float(img.numel()) * img.element_size() + 2.0 * out.numel(), f"{B},{S},{P}"):
        lib.call("clipa_patchify_ln", _p(img), _p(out), B, S, P, Kp, dt, nhwc, normalize, m3, s3, float(eps), _stream())
    return out


def _chk_patchnorm(w, gamma, beta, P, who):
    if w.dtype not in (f32, bf16):
        raise RuntimeError(f"clipa_amd.ops.{who}: w must be torch.float32 or torch.bfloat16, got {w.dtype}")
    _chk(w, None, "w", 2)
    K = 3 * P * P
    if w.shape[1] != K:
        raise RuntimeError(f"clipa_amd.ops.{who}: w has {w.shape[1]} columns for 3*P*P = {K}")
    for name, t in (("gamma", gamma), ("beta", beta)):
        _chk(t, f32, name, 1)
        if t.shape[0] != K:
            raise RuntimeError(f"clipa_amd.ops.{who}: {name} has {t.shape[0]} entries for 3*P*P = {K}")


def patchnorm_fold(w, b, gamma, beta, P, Kp):
    """Dual PatchNorm's LayerNorm affine folded into the Linear behind it (transformer.py:368-369,487-488): w [N,K] f32/bf16 and
    b f32 [N] of conv1, gamma / beta f32 [K] of patchnorm_pre_ln, K = 3*P*P in (c,p1,p2) order -> (bf16 [N,Kp] = bf16(w * gamma)
    with the columns in (ph,pw,c) order and zero padding, f32 [N] = b + w @ beta); fp32, one rounding, fixed order."""
    _chk_patch_geometry(P, Kp, "patchnorm_fold")
    _chk_patchnorm(w, gamma, beta, P, "patchnorm_fold")
    _chk(b, f32, "b", 1)
    N = w.shape[0]
    if b.shape[0] != N:
        raise RuntimeError(f"clipa_amd.ops.patchnorm_fold: b has {b.shape[0]} entries for {N} rows of w")
    w, b, gamma, beta = w.contiguous(), b.contiguous(), gamma.contiguous(), beta.contiguous()
    wf = torch.empty((N, Kp), device=w.device, dtype=bf16)
    bfold = torch.empty(N, device=w.device, dtype=f32)
    with _Timed("patchnorm_fold", 2.0 * N * w.shape[1], float(N) * (w.shape[1] * w.element_size() + 2 * Kp)):
        lib.call("clipa_patchnorm_fold", _p(w), int(w.dtype == f32), _p(b), _p(gamma), _p(beta), _p(wf), _p(bfold), N, P, Kp,
                 _stream())
    return wf, bfold


def patchnorm_unfold(g, s, w, gamma, beta, P, out_dtype=f32, want=(True, True, True)):
    """The parameters' gradients of a stem that ran with folded PatchNorm: g f32 [N,Kp] = dPE^T xhat ((ph,pw,c) columns) and
    s f32 [N] = colsum(dPE) -> (dw [N,K] in out_dtype = gamma * g + beta * s[:,None], dgamma f32 [K] = sum_n w * g, dbeta f32 [K]
    = sum_n w * s[:,None]), all in the parameters' (c,p1,p2) order; fp32, fixed order over n.  want: which of the three to
    compute (None in place of the others).  The gradient of conv1.bias is s."""
    _chk_out_dtype(out_dtype, "patchnorm_unfold")
    _chk_patchnorm(w, gamma, beta, P, "patchnorm_unfold")
    _chk(g, f32, "g", 2)
    N, K = w.shape
    Kp = g.shape[1]
    _chk_patch_geometry(P, Kp, "patchnorm_unfold")
    if g.shape[0] != N:
        raise RuntimeError(f"clipa_amd.ops.patchnorm_unfold: g {tuple(g.shape)} vs w {tuple(w.shape)}")
    _chk(s, f32, "s", 1)
    if s.shape[0] != N:
        raise RuntimeError(f"clipa_amd.ops.patchnorm_unfold: s has {s.shape[0]} entries for {N} rows of w")
    want_w, want_g, want_b = (bool(v) for v in want)
    g, s, w, gamma, beta = g.contiguous(), s.contiguous(), w.contiguous(), gamma.contiguous(), beta.contiguous()
    dw = torch.empty((N, K), device=w.device, dtype=out_dtype) if want_w else None
    dg = torch.empty(K, device=w.device, dtype=f32) if want_g else None
    db = torch.empty(K, device=w.device, dtype=f32) if want_b else None
    with _Timed("patchnorm_unfold", 4.0 * N * K if want_g or want_b else 0.0,
                float(N) * K * (4 + (w.element_size() if want_g or want_b else 0) + (dw.element_size() if want_w else 0))):
        lib.call("clipa_patchnorm_unfold", _p(g), _p(s), _p(w), int(w.dtype == f32), _p(gamma), _p(beta), _p(dw),
                 int(out_dtype == f32), _p(dg), _p(db), N, P, Kp, _stream())
    return dw, dg, db


def resized_crop_u8(src, boxes, size, gray_flags=None):
    """Device-side RandomResizedCrop (+ Grayscale of the flagged samples), bit-exact with Pillow's bicubic resize of the
    cropped image: src uint8 [B,Hs,Ws,3] (NHWC), boxes int32 [B,4] = (top, left, height, width) -> uint8 [B,size,size,3].
    Samples whose box leaves the image (or shrinks more than 11x) come back as zeros and raise at the next check."""
    _chk(src, u8, "src", 4)
    _chk(boxes, torch.int32, "boxes", 2)
    if src.shape[3] != 3 or not src.is_contiguous():
        raise RuntimeError(f"resized_crop_u8: src must be a contiguous uint8 [B,H,W,3] tensor, got {tuple(src.shape)}")
    B, Hs, Ws, _ = src.shape
    if tuple(boxes.shape) != (B, 4) or not boxes.is_contiguous():
        raise RuntimeError(f"resized_crop_u8: boxes must be contiguous int32 [{B},4]")
    if gray_flags is not None:
        _chk(gray_flags, u8, "gray_flags", 1)
        if gray_flags.numel() != B:
            raise RuntimeError("resized_crop_u8: gray_flags must have one byte per sample")
    check_token_ids()                                   # surfaces an earlier launch's rejected samples
    out = torch.empty((B, size, size, 3), device=src.device, dtype=u8)
    ws, wsb = _workspace("clipa_resized_crop_workspace", B, Hs, size, device=src.device, dtype=u8, floor=0)
    err = _oob_counter(src.device)
    with _Timed("resized_crop", 0.0, 3.0 * B * (Hs * Ws + Hs * size * 2 + size * size)):
        lib.call("clipa_resized_crop_u8", _p(src), _p(boxes), _p(gray_flags), _p(out), B, Hs, Ws, size, _p(ws), wsb, _p(err),
                 _stream())
    _oob_submit(err, "resized_crop_u8", "samples rejected (crop box outside the image or a down-scale above 11x)")
    return out


RAGGED_MAX_SIDE, RAGGED_MAX_DOWN, RAGGED_MAX_SIZE = 16384, 64, 4096      # csrc/resample_ragged.hip: RR_MAX_SIDE, RR_MAX_DOWN
_RAGGED_FILTERS = {"bicubic": (0, 2.0), "bilinear": (1, 1.0)}             # name -> (filter id of the C entry, Pillow's support)


def _ragged_refuse(bad, what):
    """ValueError naming the first sample of the bool [B] mask `bad`."""
    if bool(bad.any()):
        i = int(bad.to(torch.uint8).argmax())
        raise ValueError(f"resample_ragged_u8: sample {i}: {what}")


def ragged_layout(offsets, sizes, geometry, size, interpolation="bicubic", packed_bytes=None, validate=True):
    """Host side of clipa_resample_ragged_u8: the per-sample descriptors with each sample's own storage, from the size table.
    offsets int64 [B], sizes int32 [B,2] = (H, W), geometry int32 [B,8] = (box top, left, height, width, out_h, out_w, oy, ox),
    all on the CPU -> (desc int64 [B,16], max_rows, tmp_bytes, coef_ints, moved bytes).  What the entry refuses is refused
    here, with the sample's index: a side above 16384 or a down-scale above 64x always; with validate, also a descriptor the
    device would reject (image outside the packed buffer, box outside the image, window outside the resized image)."""
    if interpolation not in _RAGGED_FILTERS:
        raise ValueError(f"resample_ragged_u8: interpolation must be 'bicubic' or 'bilinear', got {interpolation!r}")
    S = int(size)
    if not 1 <= S <= RAGGED_MAX_SIZE:
        raise ValueError(f"resample_ragged_u8: size must be in 1..{RAGGED_MAX_SIZE}, got {size}")
    off, hw, g = offsets.to(torch.int64), sizes.to(torch.int64), geometry.to(torch.int64)
    B = off.numel()
    if tuple(hw.shape) != (B, 2) or tuple(g.shape) != (B, 8):
        raise ValueError(f"resample_ragged_u8: sizes must be [{B},2] and geometry [{B},8], got {tuple(hw.shape)} and {tuple(g.shape)}")
    H, W = hw[:, 0], hw[:, 1]
    top, left, bh, bw, oh, ow, oy, ox = g.unbind(1)
    sides = torch.stack([H, W, bh, bw, oh, ow], 1)
    _ragged_refuse(((sides < 1) | (sides > RAGGED_MAX_SIDE)).any(1), f"image, box and resized sides must be in 1..{RAGGED_MAX_SIDE}")
    _ragged_refuse((bh > oh * RAGGED_MAX_DOWN) | (bw > ow * RAGGED_MAX_DOWN), f"down-scale above {RAGGED_MAX_DOWN}x")
    if validate:
        bad = off < 0
        if packed_bytes is not None:
            bad |= off + H * W * 3 > int(packed_bytes)
        _ragged_refuse(bad, "image outside the packed buffer")
        _ragged_refuse((top < 0) | (left < 0) | (top + bh > H) | (left + bw > W), "crop box outside the image")
        _ragged_refuse((oy < 0) | (ox < 0) | (oy + S > oh) | (ox + S > ow), f"the {S} x {S} window lies outside the resized image")
    support = _RAGGED_FILTERS[interpolation][1]

    def taps(n_in, n_out):          # Resample.c precompute_coeffs: ksize, in the same double operations
        scale = n_in.double() / n_out.double()
        sup = support * scale.clamp(min=1.0)
        return scale, sup, torch.ceil(sup).long() * 2 + 1

    _, _, kh = taps(bw, ow)
    scale, sup, kv = taps(bh, oh)
    # the box rows that the window's vertical taps read: xmin of its first row .. xmax of its last (C casts truncate)
    first = ((oy.double() + 0.5) * scale - sup + 0.5).long().clamp(min=0)
    last = torch.minimum((((oy + S - 1).double() + 0.5) * scale + sup + 0.5).long(), bh)
    rows = torch.minimum((last - first).clamp(min=1), bh)
    tmp = (rows * S * 3 + 15) // 16 * 16
    coef = S * (kh + kv)
    tmp_off, coef_off = torch.cumsum(tmp, 0) - tmp, torch.cumsum(coef, 0) - coef
    desc = torch.stack([off, H, W, top, left, bh, bw, oh, ow, oy, ox, tmp_off, coef_off, kh, kv, rows], 1).contiguous()
    nbytes = 3.0 * float((rows * (bw + 2 * S)).sum() + B * S * S)
    return desc, int(rows.max()) if B else 1, int(tmp.sum()), int(coef.sum()), nbytes


def resample_ragged_u8(images, geometry, size, interpolation="bicubic", gray_flags=None, validate=True):
    """Device-side resize of a batch of images of DIFFERENT sizes (+ Grayscale of the flagged samples), bit-exact with Pillow:
    out[b] = resize(crop(image b, box b), (out_h, out_w), interpolation)[oy : oy + size, ox : ox + size] -> uint8 [B,size,size,3].
    images: a clipa_amd.data.RaggedImages on the device; geometry int32 [B,8] = (box top, left, height, width, out_h, out_w,
    oy, ox) on the CPU - data.eval_geometry for the inference transform, a sampled box with (size, size, 0, 0) for
    RandomResizedCrop.  A side above 16384, a down-scale above 64x or (validate) a descriptor that leaves its image raise a
    ValueError that names the sample; validate=False leaves the latter to the device, where such samples come back as zeros and
    raise at the next check."""
    data = images.data
    _chk(data, u8, "images.data", 1)
    if not data.is_contiguous():
        raise RuntimeError("resample_ragged_u8: images.data must be a contiguous 1-D uint8 tensor")
    offsets, sizes = images.host_tables()
    B = offsets.numel()
    geometry = torch.as_tensor(geometry).cpu()
    if gray_flags is not None:
        _chk(gray_flags, u8, "gray_flags", 1)
        if gray_flags.numel() != B:
            raise RuntimeError("resample_ragged_u8: gray_flags must have one byte per sample")
    if B > 65535:
        raise ValueError(f"resample_ragged_u8: at most 65535 samples per call, got {B}")
    desc, max_rows, tmp_bytes, coef_ints, nbytes = ragged_layout(offsets, sizes, geometry, size, interpolation, data.numel(), validate)
    size = int(size)
    check_token_ids()                                   # surfaces an earlier launch's rejected samples
    out = torch.empty((B, size, size, 3), device=data.device, dtype=u8)
    if B == 0:
        return out
    desc = desc.pin_memory().to(data.device, non_blocking=True)
    ws, wsb = _workspace("clipa_resample_ragged_workspace", B, size, tmp_bytes, coef_ints, device=data.device, dtype=u8, floor=0)
    err = _oob_counter(data.device)
    with _Timed("resample_ragged", 0.0, nbytes):
        lib.call("clipa_resample_ragged_u8", _p(data), data.numel(), _p(desc), _p(gray_flags), _p(out), B, size,
                 _RAGGED_FILTERS[interpolation][0], max_rows, tmp_bytes, coef_ints, _p(ws), wsb, _p(err), _stream())
    _oob_submit(err, "resample_ragged_u8", "samples rejected (image, crop box or window outside its bounds, or a down-scale above 64x)")
    return out


def color_jitter_u8_(img, apply=None, order=None, factors=None, gray_flags=None):
    """In place on uint8 [B,S,S,3]: torchvision ColorJitter with per-sample op order (int32 [B,4] over 0 brightness, 1 contrast,
    2 saturation, 3 hue) and factors (f32 [B,4], indexed by op) for the samples with apply[b] != 0, then Grayscale(3) of the
    samples flagged in gray_flags - bit-exact with the Pillow code paths.  order=None: grayscale only."""
    _chk(img, u8, "img", 4)
    if img.shape[3] != 3 or img.shape[1] != img.shape[2] or not img.is_contiguous():
        raise RuntimeError(f"color_jitter_u8_: img must be a contiguous uint8 [B,S,S,3] tensor, got {tuple(img.shape)}")
    B, S = img.shape[0], img.shape[1]
    if order is not None:
        _chk(order, torch.int32, "order", 2)
        _chk(factors, f32, "factors", 2)
        if tuple(order.shape) != (B, 4) or tuple(factors.shape) != (B, 4) or not order.is_contiguous() or not factors.is_contiguous():
            raise RuntimeError("color_jitter_u8_: order int32 [B,4] and factors f32 [B,4], contiguous")
    for name, t in (("apply", apply), ("gray_flags", gray_flags)):
        if t is not None:
            _chk(t, u8, name, 1)
            if t.numel() != B:
                raise RuntimeError(f"color_jitter_u8_: {name} must have one byte per sample")
    ws = torch.empty(B, device=img.device, dtype=torch.int64)
    lib.call("clipa_color_jitter_u8", _p(img), _p(apply), _p(order), _p(factors), _p(gray_flags), B, S, _p(ws), B * 8, _stream())
    return img


def mixcut_u8(img, lam=None, box=None):
    """Batch Mixup or CutMix in place on uint8 [B,3,S,S] in NCHW or channels_last memory (what DeviceAugment returns): sample b
    is mixed with its mirror B-1-b (clipa_jax/transforms/mixup.py:141-201).  Exactly one of
      lam f32 [B]                      mixup: out_b = lam_b x_b + (1 - lam_b) x_{B-1-b}, the fp32 byte arithmetic of csrc/mixcut.hip
      box int32 [B,4] = (y0,y1,x0,x1)  cutmix: out_b = x_{B-1-b} inside the half-open box, x_b outside
    on the device.  lam outside [0, 1] or NaN, a box outside the image or with y0 > y1 or x0 > x1: that pair is left as it was and
    the call raises at the next check (check_token_ids, as for the other device-validated descriptors).  -> img."""
    if (lam is None) == (box is None):
        raise RuntimeError("clipa_amd.ops.mixcut_u8: give lam (mixup) or box (cutmix), not both")
    if not img.is_cuda:
        raise RuntimeError(f"clipa_amd.ops.mixcut_u8: img must live on the GPU (no CPU fallback); got {img.device}")
    if img.dtype != u8 or img.dim() != 4 or img.shape[1] != 3 or img.shape[2] != img.shape[3]:
        raise RuntimeError(f"clipa_amd.ops.mixcut_u8: expected uint8 [B,3,S,S], got {img.dtype} {tuple(img.shape)}")
    B, S = img.shape[0], img.shape[2]
    if img.is_contiguous():
        nhwc = 0
    elif img.is_contiguous(memory_format=torch.channels_last):
        nhwc = 1
    else:
        raise RuntimeError("clipa_amd.ops.mixcut_u8: img must be dense in NCHW or channels_last memory (the operation is in place)")
    if lam is not None:
        _chk(lam, f32, "lam", 1)
        if lam.numel() != B:
            raise RuntimeError(f"clipa_amd.ops.mixcut_u8: lam must be f32 [{B}], got {tuple(lam.shape)}")
        lam = lam.contiguous()
    else:
        _chk(box, torch.int32, "box", 2)
        if tuple(box.shape) != (B, 4):
            raise RuntimeError(f"clipa_amd.ops.mixcut_u8: box must be int32 [{B},4], got {tuple(box.shape)}")
        box = box.contiguous()
    if B == 0:
        return img
    check_token_ids()                                   # surfaces an earlier launch's rejected samples
    err = _oob_counter(img.device)
    with _Timed("mixcut", 0.0, 4.0 * (B // 2) * 3 * S * S):
        lib.call("clipa_mixcut_u8", _p(img), _p(lam), _p(box), B, S, nhwc, 0 if lam is not None else 1, _p(err), _stream())
    _oob_submit(err, "mixcut_u8", "samples rejected (lam outside [0, 1], or a box outside the image or with y0 > y1 / x0 > x1)")
    return img


SOFTCE_MAX_CLASSES = 32768      # csrc/softce.hip: SCE_MAX_C


def soft_target_ce(logits, ya, yb=None, lam=None, smoothing=0.0, gscale=None, _max_workgroups=0):
    """Soft-target cross-entropy rows in one pass (clipa_jax/losses/common.py:104-109 on the labels of transforms/mixup.py:203-211):
    logits f32 [B, C] (a [B, C] view of a wider buffer is read in place: its other columns are never touched), ya int32 [B],
    optional yb int32 [B] with lam f32 [B]; t_c = (1 - smoothing) (lam [c = ya] + (1 - lam) [c = yb]) + smoothing / C.
    -> (loss f32 [B], lse f32 [B], dlogits): dlogits = gscale (softmax - t) as the bf16 [B, C] view of a [B, C rounded up to 8]
    buffer whose other columns are zero, or None when gscale is None.  Fixed summation order: the same bits for every grid.
    Labels outside [0, C) or lam outside [0, 1] raise at the next check (check_token_ids); such rows come back NaN."""
    _chk(logits, f32, "logits", 2)
    _chk(ya, torch.int32, "ya", 1)
    B, C = logits.shape
    if not 2 <= C <= SOFTCE_MAX_CLASSES:
        raise RuntimeError(f"clipa_amd.ops.soft_target_ce: C = {C} classes; the kernel takes 2 to {SOFTCE_MAX_CLASSES}")
    if (yb is None) != (lam is None):
        raise RuntimeError("clipa_amd.ops.soft_target_ce: yb and lam come together")
    vecs = [("ya", ya)]
    if yb is not None:
        _chk(yb, torch.int32, "yb", 1)
        _chk(lam, f32, "lam", 1)
        vecs += [("yb", yb), ("lam", lam)]
    if any(t.numel() != B for _, t in vecs):
        raise RuntimeError(f"clipa_amd.ops.soft_target_ce: {', '.join(n for n, _ in vecs)} must have B = {B} entries")
    if not 0.0 <= float(smoothing) <= 1.0:
        raise RuntimeError(f"clipa_amd.ops.soft_target_ce: smoothing = {smoothing} outside [0, 1]")
    ya, yb, lam = (None if t is None else t.contiguous() for t in (ya, yb, lam))
    ya, yb, lam = (t.clone() if t is not None and t.data_ptr() % 16 else t for t in (ya, yb, lam))
    logits, ld = _aligned_rows(logits)
    loss = torch.empty(B, device=logits.device, dtype=f32)
    lse = torch.empty(B, device=logits.device, dtype=f32)
    ldd = (C + 7) // 8 * 8
    dl = torch.empty((B, ldd), device=logits.device, dtype=bf16) if gscale is not None else None
    if B == 0:
        return loss, lse, (dl[:, :C] if dl is not None else None)
    check_token_ids()
    err = _oob_counter(logits.device)
    with _Timed("softce", 0.0, 4.0 * B * C + (2.0 * B * ldd if dl is not None else 0.0), f"{B},{C}"):
        lib.call("clipa_softce", _p(logits), B, C, ld, _p(ya), _p(yb), _p(lam), float(smoothing),
                 float(gscale) if gscale is not None else 0.0, _p(loss), _p(lse), _p(dl), ldd, int(_max_workgroups), _p(err),
                 _stream())
    _oob_submit(err, "soft_target_ce", "rows rejected (a label outside [0, C), or lam outside [0, 1] or NaN)")
    return loss, lse, (dl[:, :C] if dl is not None else None)


def assemble_tokens(patch, cls, pos, B, L):
    D = patch.shape[1]
    tok = torch.empty((B * L, D), device=patch.device, dtype=bf16)
    lib.call("clipa_assemble_tokens", _p(patch), _p(cls), _p(pos), _p(tok), B, L, D, _stream())
    return tok


def assemble_tokens_bwd(dtok, B, L, need_pos=True):
    D = dtok.shape[1]
    dtok = dtok.contiguous()
    dpatch = torch.empty((B * (L - 1), D), device=dtok.device, dtype=bf16)
    dcls = torch.empty(D, device=dtok.device, dtype=f32)
    dpos = torch.empty((L, D), device=dtok.device, dtype=f32) if need_pos else None
    ws, wsb = _workspace("clipa_assemble_tokens_bwd_workspace", B, L, D, device=dtok.device)
    lib.call("clipa_assemble_tokens_bwd", _p(dtok), _p(dpatch), _p(dcls), _p(dpos), B, L, D, _p(ws), wsb, _stream())
    return dpatch, dcls, dpos


def _oob_counter(device):
    return torch.zeros(1, device=device, dtype=torch.int32)


def _oob_submit(counter, what, msg="token ids outside [0, vocab) (nn.Embedding would raise)"):
    host = torch.empty(1, dtype=torch.int32, pin_memory=True)
    host.copy_(counter, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    with _OOB_LOCK:
        _OOB_PENDING.append((host, ev, (what, msg), counter))


def check_token_ids(wait=False):
    """Raise if an earlier embedding forward / backward met token ids outside the table (wait=True: block on all)."""
    with _OOB_LOCK:
        pending = list(_OOB_PENDING)
        _OOB_PENDING.clear()
    keep, bad = [], None
    for host, ev, what, counter in pending:
        if wait:
            ev.synchronize()
        if ev.query():
            if int(host[0]) != 0 and bad is None:
                bad = f"clipa_amd.ops.{what[0]}: {int(host[0])} {what[1]}"
        else:
            keep.append((host, ev, what, counter))
    if bad is not None:
        raise RuntimeError(bad)      # everything submitted so far is dropped with it
    if keep:
        with _OOB_LOCK:
            _OOB_PENDING[:0] = keep


def embed_tokens(ids, table, pos):
    _chk(ids, torch.int64, "ids", 2)
    _chk(pos, f32, "pos", 2)
    check_token_ids()
    ids = ids.contiguous()
    B, T = ids.shape
    V, D = table.shape
    out = torch.empty((B * T, D), device=ids.device, dtype=bf16)
    oob = _oob_counter(ids.device)
    lib.call("clipa_embed_tokens", _p(ids), _p(table.contiguous()), int(table.dtype == bf16), _p(pos.contiguous()), _p(out),
             B, T, D, V, _p(oob), _stream())
    _oob_submit(oob, "embed_tokens")
    return out


def embed_tokens_bwd(ids, dx, vocab, need_table=True, need_pos=True):
    ids = ids.contiguous()
    B, T = ids.shape
    D = dx.shape[1]
    dx = dx.contiguous()
    dtable = torch.empty((vocab, D), device=dx.device, dtype=f32) if need_table else None
    dpos = torch.empty((T, D), device=dx.device, dtype=f32) if need_pos else None
    oob = _oob_counter(ids.device)
    ws, wsb = _workspace("clipa_embed_tokens_bwd_workspace", B, T, D, vocab, int(need_table), int(need_pos), device=dx.device,
                         dtype=torch.int64, floor=8)
    lib.call("clipa_embed_tokens_bwd", _p(ids), _p(dx), _p(dtable), _p(dpos), B, T, D, vocab, _p(oob), _p(ws), wsb, _stream())
    _oob_submit(oob, "embed_tokens_bwd")
    return dtable, dpos


def argmax_tokens(ids):
    ids = ids.contiguous()
    B, T = ids.shape
    out = torch.empty(B, device=ids.device, dtype=torch.int32)
    lib.call("clipa_argmax_tokens", _p(ids), _p(out), B, T, _stream())
    return out


def pool_fwd(x, B, L, mode, idx=None):
    D = x.shape[-1]
    out = torch.empty((B, D), device=x.device, dtype=f32)
    lib.call("clipa_pool_fwd", _p(x), _p(idx), _p(out), B, L, D, mode, _stream())
    return out


def pool_bwd(dout, B, L, mode, idx=None):
    D = dout.shape[-1]
    dx = torch.empty((B * L, D), device=dout.device, dtype=bf16)
    lib.call("clipa_pool_bwd", _p(dout.contiguous()), _p(idx), _p(dx), B, L, D, mode, _stream())
    return dx


def _chk_mappool(who, x, u, B, L, H):
    _chk(x, bf16, "x", 2)
    _chk(u, bf16, "u", 2)
    D = x.shape[1]
    if not 1 <= H <= 16 or D % 64 or not 64 <= D <= 2048 or L < 1:
        raise RuntimeError(f"clipa_amd.ops.{who}: unsupported shape H={H}, D={D}, L={L} (1 <= H <= 16, D a multiple of 64 up to "
                           f"2048, L >= 1)")
    if x.shape[0] != B * L or tuple(u.shape) != (H, D):
        raise RuntimeError(f"clipa_amd.ops.{who}: x {tuple(x.shape)} / u {tuple(u.shape)} do not match B={B}, L={L}, H={H}")
    u = u.contiguous()
    x, ldx = _aligned16(x)
    if ldx % 8:      # a row stride the 16-byte loads cannot take: copied, like a misaligned base
        x, ldx = x.contiguous(), D
    return x, ldx, u if u.data_ptr() % 16 == 0 else u.clone(), D


def mappool_fwd(x, u, B, L, H, _max_workgroups=0):
    """Folded multihead attention pooling (clipa_jax/models/vit.py:187-207; csrc/mappool.hip): x bf16 [B*L, D] (a row-strided or
    misaligned view is copied), u bf16 [H, D] -> (z f32 [B,H,D] = sum_l softmax_l(x u_h^T) x, stats f32 [B,H,2] = (max, sum))."""
    x, ldx, u, D = _chk_mappool("mappool_fwd", x, u, B, L, H)
    z = torch.empty((B, H, D), device=x.device, dtype=f32)
    stats = torch.empty((B, H, 2), device=x.device, dtype=f32)
    with _Timed("mappool_fwd", 4.0 * B * L * H * D, 2.0 * B * L * D + 4.0 * B * H * D, f"{B},{L},{D},{H}"):
        lib.call("clipa_mappool_fwd", _p(x), _p(u), _p(z), _p(stats), B, L, D, H, ldx, int(_max_workgroups), _stream())
    return z, stats


def mappool_bwd(x, u, z, stats, dz, B, L, H, _max_workgroups=0):
    """-> (dx bf16 [B*L, D], du f32 [H, D]) of mappool_fwd; du is summed over per-workgroup partials in a fixed order."""
    x, ldx, u, D = _chk_mappool("mappool_bwd", x, u, B, L, H)
    for name, t, shape in (("z", z, (B, H, D)), ("stats", stats, (B, H, 2)), ("dz", dz, (B, H, D))):
        _chk(t, f32, name, 3)
        if tuple(t.shape) != shape:
            raise RuntimeError(f"clipa_amd.ops.mappool_bwd: {name} {tuple(t.shape)} is not {shape}")
    z, stats, dz = z.contiguous(), stats.contiguous(), dz.contiguous()
    dx = torch.empty((B * L, D), device=x.device, dtype=bf16)
    du = torch.empty((H, D), device=x.device, dtype=f32)
    ws, wsb = _workspace("clipa_mappool_bwd_workspace", B, H, D, int(_max_workgroups), device=x.device, floor=16)
    with _Timed("mappool_bwd", 10.0 * B * L * H * D, 4.0 * B * L * D + 8.0 * B * H * D, f"{B},{L},{D},{H}"):
        lib.call("clipa_mappool_bwd", _p(x), _p(u), _p(z), _p(stats), _p(dz), _p(dx), _p(du), B, L, D, H, ldx, D,
                 int(_max_workgroups), _p(ws), wsb, _stream())
    return dx, du


def gather_rows(x, rows):
    """out[r] = x[rows[r]]: bf16 [n_src, D], int64 device row list -> bf16 [len(rows), D] (PatchDropout's token selection)."""
    _chk(x, bf16, "x", 2)
    _chk(rows, torch.int64, "rows", 1)
    x = x.contiguous()
    out = torch.empty((rows.numel(), x.shape[1]), device=x.device, dtype=bf16)
    with _Timed("gather_rows", 0.0, 4.0 * out.numel()):
        lib.call("clipa_gather_rows", _p(x), _p(rows), _p(out), rows.numel(), x.shape[0], x.shape[1], _stream())
    return out


def scatter_rows(dy, rows, n_dst):
    """dx [n_dst, D] = 0; dx[rows[r]] = dy[r] (distinct rows): the backward of gather_rows."""
    _chk(dy, bf16, "dy", 2)
    _chk(rows, torch.int64, "rows", 1)
    dy = dy.contiguous()
    dx = torch.empty((n_dst, dy.shape[1]), device=dy.device, dtype=bf16)
    with _Timed("scatter_rows", 0.0, 2.0 * (dx.numel() + 2 * dy.numel())):
        lib.call("clipa_scatter_rows", _p(dy), _p(rows), _p(dx), dy.shape[0], n_dst, dy.shape[1], _stream())
    return dx


def l2norm_fwd(x, eps=1e-12, want_bf16=False):
    x = x.contiguous()
    rows, E = x.shape
    y = torch.empty_like(x)
    ybf = torch.empty((rows, E), device=x.device, dtype=bf16) if want_bf16 else None
    inv = torch.empty(rows, device=x.device, dtype=f32)
    lib.call("clipa_l2norm_fwd", _p(x), _p(y), _p(ybf), _p(inv), rows, E, float(eps), _stream())
    return y, ybf, inv


def l2norm_bwd(y, inv, dy):
    rows, E = y.shape
    dx = torch.empty_like(y)
    lib.call("clipa_l2norm_bwd", _p(y), _p(inv), _p(dy.contiguous()), _p(dx), rows, E, _stream())
    return dx


def colsum(dy):
    _chk(dy, bf16, "dy", 2)
    dy, ld = _rowmajor(dy)
    M, N = dy.shape
    ws, wsb = _workspace("clipa_colsum_workspace", M, N, device=dy.device)
    out = torch.empty(N, device=dy.device, dtype=f32)
    lib.call("clipa_colsum", _p(dy), _p(out), M, N, ld, _p(ws), wsb, _stream())
    return out


def to_bf16(t):
    """Flat cast f32/bf16 -> new bf16 tensor (weights are re-cast once per optimizer step)."""
    t = t.contiguous()
    if t.dtype not in (f32, bf16):
        raise RuntimeError(f"to_bf16: unsupported dtype {t.dtype}")
    out = torch.empty(t.shape, device=t.device, dtype=bf16)
    lib.call("clipa_cast_to_bf16", _p(t), int(t.dtype == f32), _p(out), t.numel(), _stream())
    return out


def to_f32(t):
    t = t.contiguous()
    if t.dtype == f32:
        return t
    out = torch.empty(t.shape, device=t.device, dtype=f32)
    lib.call("clipa_cast_bf16_to_f32", _p(t), _p(out), t.numel(), _stream())
    return out


def transpose_bf16(t):
    """[R,C] f32/bf16 -> [C,R] bf16 (used for W^T operands)."""
    t, ldi = _rowmajor(t)
    R, C = t.shape
    out = torch.empty((C, R), device=t.device, dtype=bf16)
    lib.call("clipa_transpose_to_bf16", _p(t), int(t.dtype == f32), _p(out), R, C, ldi, R, _stream())
    return out


def _chk_layerscale(w, gamma, b, who):
    if w.dtype not in (f32, bf16):
        raise RuntimeError(f"clipa_amd.ops.{who}: w must be torch.float32 or torch.bfloat16, got {w.dtype}")
    _chk(w, None, "w", 2)
    _chk(gamma, f32, "gamma", 1)
    N = w.shape[0]
    if gamma.shape[0] != N:
        raise RuntimeError(f"clipa_amd.ops.{who}: gamma has {gamma.shape[0]} entries for {N} rows of w")
    _chk(b, f32, "b", 1)
    if b.shape[0] != N:
        raise RuntimeError(f"clipa_amd.ops.{who}: b has {b.shape[0]} entries for {N} rows of w")


def layerscale_fold(w, gamma, b):
    """LayerScale folded into the layer it scales (transformer.py:43-50,248-249): w [N,K] f32/bf16, gamma / b f32 [N] ->
    (bf16 [N,K] = bf16(gamma[:,None] * w), f32 [N] = gamma * b); fp32 product, one rounding."""
    _chk_layerscale(w, gamma, b, "layerscale_fold")
    w, gamma, b = w.contiguous(), gamma.contiguous(), b.contiguous()
    N, K = w.shape
    wf = torch.empty((N, K), device=w.device, dtype=bf16)
    bf = torch.empty(N, device=w.device, dtype=f32)
    with _Timed("layerscale_fold", 0.0, float(N) * K * (w.element_size() + 2)):
        lib.call("clipa_layerscale_fold", _p(w), int(w.dtype == f32), _p(gamma), _p(b), _p(wf), _p(bf), N, K, _stream())
    return wf, bf


def layerscale_unfold(dwf, w, gamma, dbf, b, out_dtype=f32, want=(True, True, True)):
    """The parameters' gradients of a layer that ran with folded LayerScale: dwf f32 [N,K] and dbf f32 [N] are the folded layer's
    weight and bias gradients -> (dw [N,K] in out_dtype = gamma[:,None] * dwf, db f32 = gamma * dbf, dgamma f32 [N] =
    sum_k dwf * w + dbf * b; fp32, fixed order).  want: which of the three to compute (None in place of the others)."""
    _chk_out_dtype(out_dtype, "layerscale_unfold")
    _chk_layerscale(w, gamma, b, "layerscale_unfold")
    _chk(dwf, f32, "dwf", 2)
    if dwf.shape != w.shape:
        raise RuntimeError(f"clipa_amd.ops.layerscale_unfold: dwf {tuple(dwf.shape)} vs w {tuple(w.shape)}")
    _chk(dbf, f32, "dbf", 1)
    if dbf.shape[0] != w.shape[0]:
        raise RuntimeError(f"clipa_amd.ops.layerscale_unfold: dbf has {dbf.shape[0]} entries for {w.shape[0]} rows of w")
    want_w, want_b, want_g = (bool(v) for v in want)
    dwf, w, gamma, dbf, b = dwf.contiguous(), w.contiguous(), gamma.contiguous(), dbf.contiguous(), b.contiguous()
    N, K = w.shape
    dw = torch.empty((N, K), device=w.device, dtype=out_dtype) if want_w else None
    db = torch.empty(N, device=w.device, dtype=f32) if want_b else None
    dg = torch.empty(N, device=w.device, dtype=f32) if want_g else None
    with _Timed("layerscale_unfold", 2.0 * N * K if want_g else 0.0,
                float(N) * K * (4 + (w.element_size() if want_g else 0) + (dw.element_size() if want_w else 0))):
        lib.call("clipa_layerscale_unfold", _p(dwf), _p(w), int(w.dtype == f32), _p(gamma), _p(dbf), _p(b), _p(dw),
                 int(out_dtype == f32), _p(db), _p(dg), N, K, _stream())
    return dw, db, dg


def activation_fwd(x, act):
    """bf16 act(x) (gelu erf / tanh / quick); x bf16, or e4m3 bytes (uint8: the "light8" keep tier's pre-activation)."""
    if x.dtype == u8:
        x = x.contiguous()
        out = torch.empty(x.shape, device=x.device, dtype=bf16)
        with _Timed("activation_fwd", 0.0, 3.0 * x.numel()):
            lib.call("clipa_activation_fwd_e4m3", _p(x), _p(out), x.numel(), act, _stream())
        return out
    _chk(x, bf16, "x")
    x = x.contiguous()
    out = torch.empty_like(x)
    with _Timed("activation_fwd", 0.0, 4.0 * x.numel()):
        lib.call("clipa_activation_fwd", _p(x), _p(out), x.numel(), act, _stream())
    return out


def simce(rows, cols, n_valid, label0, gscale, scale=None, want_grad=True):
    """Fused similarity + cross-entropy (InfoNCE): logits = s * rows @ cols[:n_valid]^T, labels label0 + row; s =
    scale[0] read on the device (None = 1).  rows [R,E], cols [>= n_valid, E] bf16, row-major views with ld % 8 == 0 (a view
    whose first element is not 16-byte aligned is copied).  Returns loss_rows f32 [R], the bf16
    d loss / d (rows @ cols^T) [R, n8] (n8 = n_valid rounded up to 8, pad columns zero) | None, and the per-row
    d loss / d s.  The fp32 logits never exist in HBM (the backward re-runs the similarity GEMM)."""
    _chk(rows, bf16, "rows", 2)
    _chk(cols, bf16, "cols", 2)
    rows, lda = _aligned16(rows)
    cols, ldb = _aligned16(cols)
    R, E = rows.shape
    if cols.shape[1] != E or cols.shape[0] < n_valid:
        raise RuntimeError(f"simce: cols {tuple(cols.shape)} does not cover {n_valid} x {E}")
    if scale is not None:
        _chk(scale, f32, "scale")
    n8 = (n_valid + 7) // 8 * 8
    ws, wsb = _workspace("clipa_simce_workspace", R, n_valid, device=rows.device)
    lse = torch.empty(R, device=rows.device, dtype=f32)
    loss_rows = torch.empty(R, device=rows.device, dtype=f32)
    with _Timed("simce", 2.0 * R * n_valid * E * (2 if want_grad else 1)):
        lib.call("clipa_simce_fwd", _p(rows), _p(cols), R, n_valid, E, lda, ldb, _p(scale), label0, _p(lse), _p(loss_rows), _p(ws),
                 wsb, _stream())
        if not want_grad:
            return loss_rows, None, None
        dl = torch.empty((R, n8), device=rows.device, dtype=bf16)
        dscale_rows = torch.empty(R, device=rows.device, dtype=f32)
        lib.call("clipa_simce_bwd", _p(rows), _p(cols), R, n_valid, E, lda, ldb, _p(scale), label0, float(gscale), _p(lse), _p(dl),
                 n8, _p(dscale_rows), _p(ws), wsb, _stream())
    return loss_rows, dl, dscale_rows


def simsig(rows, cols, n_valid, label0, gscale, scale, bias, want_grad=True):
    """Fused similarity + pairwise sigmoid loss (SigLIP): l = s * rows @ cols[:n_valid]^T + b, y = +1 at column label0 + row
    and -1 elsewhere; s = scale[0], b = bias[0], f32 DEVICE scalars.  rows [R,E], cols [>= n_valid, E] bf16.  One pass over the
    GEMM returns loss_rows f32 [R] = sum_n softplus(-y l) (not scaled by gscale) and, with gg = gscale * d loss / d l, the bf16
    d loss / d (rows @ cols^T) = gg * s [R, n8] (n8 = n_valid rounded up to 8, pad columns zero) | None, the per-row
    d loss / d s | None and d loss / d b | None.  The fp32 logits never exist in HBM."""
    _chk(rows, bf16, "rows", 2)
    _chk(cols, bf16, "cols", 2)
    _chk(scale, f32, "scale")
    _chk(bias, f32, "bias")
    rows, lda = _aligned16(rows)
    cols, ldb = _aligned16(cols)
    R, E = rows.shape
    if cols.shape[1] != E or cols.shape[0] < n_valid:
        raise RuntimeError(f"simsig: cols {tuple(cols.shape)} does not cover {n_valid} x {E}")
    if scale.numel() != 1 or bias.numel() != 1:
        raise RuntimeError(f"simsig: scale and bias are scalars, got {tuple(scale.shape)} and {tuple(bias.shape)}")
    n8 = (n_valid + 7) // 8 * 8
    dev = rows.device
    ws, wsb = _workspace("clipa_simsig_workspace", R, n_valid, device=dev)
    loss_rows = torch.empty(R, device=dev, dtype=f32)
    dl = torch.empty((R, n8), device=dev, dtype=bf16) if want_grad else None
    dscale_rows = torch.empty(R, device=dev, dtype=f32) if want_grad else None
    dbias_rows = torch.empty(R, device=dev, dtype=f32) if want_grad else None
    with _Timed("simsig", 2.0 * R * n_valid * E):
        lib.call("clipa_simsig", _p(rows), _p(cols), R, n_valid, E, lda, ldb, _p(scale), _p(bias), label0, float(gscale),
                 _p(loss_rows), _p(dl), n8, _p(dscale_rows), _p(dbias_rows), _p(ws), wsb, _stream())
    return loss_rows, dl, dscale_rows, dbias_rows


def _distill_operands(rows_s, cols_s, rows_t, cols_t, n_valid, scale_s, scale_t, extra=()):
    for t, name in ((rows_s, "rows_s"), (cols_s, "cols_s"), (rows_t, "rows_t"), (cols_t, "cols_t")):
        _chk(t, bf16, name, 2)
    rows_s, ldas = _aligned16(rows_s)
    cols_s, ldbs = _aligned16(cols_s)
    rows_t, ldat = _aligned16(rows_t)
    cols_t, ldbt = _aligned16(cols_t)
    R, Es = rows_s.shape
    Et = rows_t.shape[1]
    if rows_t.shape[0] != R:
        raise RuntimeError(f"simce_distill: teacher rows {tuple(rows_t.shape)} vs student rows {tuple(rows_s.shape)}")
    if cols_s.shape[1] != Es or cols_s.shape[0] < n_valid:
        raise RuntimeError(f"simce_distill: cols_s {tuple(cols_s.shape)} does not cover {n_valid} x {Es}")
    if cols_t.shape[1] != Et or cols_t.shape[0] < n_valid:
        raise RuntimeError(f"simce_distill: cols_t {tuple(cols_t.shape)} does not cover {n_valid} x {Et}")
    for t, name in ((scale_s, "scale_s"), (scale_t, "scale_t")) + tuple(extra):
        if t is not None:
            _chk(t, f32, name)
    return (rows_s, cols_s, rows_t, cols_t), (R, Es, Et, ldas, ldbs, ldat, ldbt)


def simce_distill(rows_s, cols_s, rows_t, cols_t, n_valid, label0, scale_s=None, scale_t=None):
    """Forward of the fused similarity + cross-entropy + distillation loss (one direction of DistillClipLoss): student
    logits z = s * rows_s @ cols_s[:n_valid]^T, teacher logits y = u * rows_t @ cols_t[:n_valid]^T, labels label0 + row.
    rows_* [R, E_*], cols_* [>= n_valid, E_*] bf16 (E_s and E_t may differ); s, u f32 DEVICE scalars (None = 1).
    Returns f32 [R] ce_rows = lse(z) - z[label], dist_rows = -sum softmax(y) log_softmax(z), lse_s and lse_t (the last
    two feed simce_distill_bwd).  Neither logit matrix exists in HBM."""
    ops4, (R, Es, Et, ldas, ldbs, ldat, ldbt) = _distill_operands(rows_s, cols_s, rows_t, cols_t, n_valid, scale_s, scale_t)
    dev = ops4[0].device
    ws, wsb = _workspace("clipa_simce_distill_workspace", R, n_valid, device=dev)
    lse_s, lse_t, ce_rows, dist_rows = (torch.empty(R, device=dev, dtype=f32) for _ in range(4))
    with _Timed("simce_distill", 2.0 * R * n_valid * (Es + Et)):
        lib.call("clipa_simce_distill_fwd", *(_p(t) for t in ops4), R, n_valid, Es, Et, ldas, ldbs, ldat, ldbt, _p(scale_s),
                 _p(scale_t), label0, _p(lse_s), _p(lse_t), _p(ce_rows), _p(dist_rows), _p(ws), wsb, _stream())
    return ce_rows, dist_rows, lse_s, lse_t


def simce_distill_bwd(rows_s, cols_s, rows_t, cols_t, n_valid, label0, gscale, lse_s, lse_t, scale_s=None, scale_t=None,
                      g_c=None, g_d=None):
    """Backward of simce_distill: re-runs both similarity GEMMs and returns the bf16
    d loss / d (rows_s @ cols_s^T) = s * gscale * (g_c (p^s - onehot) + g_d (p^s - p^t))  [R, n8] (n8 = n_valid rounded
    up to 8, pad columns zero) and the per-row d loss / d s f32 [R].  g_c, g_d: upstream gradients of the two losses as
    f32 DEVICE scalars (None = 1) - no host sync.  The teacher gets no gradient."""
    ops4, (R, Es, Et, ldas, ldbs, ldat, ldbt) = _distill_operands(rows_s, cols_s, rows_t, cols_t, n_valid, scale_s, scale_t,
                                                                  ((lse_s, "lse_s"), (lse_t, "lse_t"), (g_c, "g_c"),
                                                                   (g_d, "g_d")))
    dev = ops4[0].device
    n8 = (n_valid + 7) // 8 * 8
    ws, wsb = _workspace("clipa_simce_distill_workspace", R, n_valid, device=dev)
    dl = torch.empty((R, n8), device=dev, dtype=bf16)
    dscale_rows = torch.empty(R, device=dev, dtype=f32)
    with _Timed("simce_distill_bwd", 2.0 * R * n_valid * (Es + Et)):
        lib.call("clipa_simce_distill_bwd", *(_p(t) for t in ops4), R, n_valid, Es, Et, ldas, ldbs, ldat, ldbt, _p(scale_s),
                 _p(scale_t), label0, float(gscale), _p(g_c), _p(g_d), _p(lse_s.contiguous()), _p(lse_t.contiguous()),
                 _p(dl), n8, _p(dscale_rows), _p(ws), wsb, _stream())
    return dl, dscale_rows


def retrieval_ranks(img, txt, scale=None):
    """Retrieval ranks of the positives of get_clip_metrics (train.py:432-449) without the [N, N] logits: img, txt
    f32 [N, E] (row i of each a matched pair), v = s * img @ txt^T in fp32 with s = scale[0] read on the device (None = 1).
    Returns int32 [N] (i2t_gt, i2t_eq, t2i_gt, t2i_eq): per image row i the number of other texts j with v_ij > v_ii /
    v_ij == v_ii, per text column j the number of other images i with v_ij > v_jj / == v_jj.  The reference's 0-based
    rank from an unstable argsort lies in [gt, gt + eq]; gt (ties broken in the positive's favour) is the engine's rank."""
    _chk(img, f32, "img", 2)
    _chk(txt, f32, "txt", 2)
    if img.shape != txt.shape:
        raise RuntimeError(f"retrieval_ranks: img {tuple(img.shape)} and txt {tuple(txt.shape)} must be the same [N, E]")
    img, lda = _aligned_rows(img)
    txt, ldb = _aligned_rows(txt)
    N, E = img.shape
    scale = _scalar1(scale)
    dev = img.device
    ws, wsb = _workspace("clipa_retrieval_ranks_workspace", N, device=dev, floor=16)
    out = torch.empty((4, (N + 3) // 4 * 4), device=dev, dtype=torch.int32)       # rows 16-byte aligned
    with _Timed("retrieval_ranks", 2.0 * N * N * E):
        lib.call("clipa_retrieval_ranks", _p(img), _p(txt), N, E, lda, ldb, _p(scale), *(_p(out[k]) for k in range(4)), _p(ws),
                 wsb, _stream())
    return tuple(out[k, :N] for k in range(4))


def retrieval_ranks_multi(img, txt, txt2img, scale=None):
    """Multi-caption retrieval ranks (image_text_retrieval.py of the reference's evaluators) without the [Ni, Nt]
    similarities: img f32 [Ni, E], txt f32 [Nt, E], txt2img integer [Nt] on the device (text t describes image c(t) in
    [0, Ni)), v = s * img @ txt^T in fp32 with s = scale[0] read on the device (None = 1).  Returns int32 (i2t_gt, i2t_eq)
    [Ni] and (t2i_gt, t2i_eq) [Nt] in the caller's text order: per image i the number of texts that beat / tie (not its
    own) its best caption's score m_i, per text t the number of images that beat / tie (other than c(t)) v_{c(t), t}.
    A captionless image has m_i = -inf, so i2t_gt = Nt.  Ties resolve in the positive's favour (gt), as retrieval_ranks.
    The kernel is fastest with the captions of an image adjacent; other orders are stable-sorted by image here (a
    temporary permuted copy of txt) and the per-text results scattered back, so the result does not depend on the order."""
    _chk(img, f32, "img", 2)
    _chk(txt, f32, "txt", 2)
    if not torch.is_tensor(txt2img) or not txt2img.is_cuda or txt2img.dim() != 1 or txt2img.dtype.is_floating_point \
            or txt2img.dtype.is_complex or txt2img.dtype == torch.bool:
        raise RuntimeError("retrieval_ranks_multi: txt2img must be a 1-D integer GPU tensor")
    if img.shape[1] != txt.shape[1] or txt2img.shape[0] != txt.shape[0]:
        raise RuntimeError(f"retrieval_ranks_multi: img {tuple(img.shape)}, txt {tuple(txt.shape)} and txt2img "
                           f"{tuple(txt2img.shape)} must be [Ni, E], [Nt, E] and [Nt]")
    Ni, Nt = img.shape[0], txt.shape[0]
    if Ni < 1 or Nt < 1:
        raise RuntimeError(f"retrieval_ranks_multi: needs at least one image and one text (Ni = {Ni}, Nt = {Nt})")
    c = txt2img.to(torch.int64)
    lo, hi, unsorted = torch.stack([c.min(), c.max(), (c[1:] < c[:-1]).sum()]).tolist()      # one host sync
    if lo < 0 or hi >= Ni:
        raise RuntimeError(f"retrieval_ranks_multi: txt2img values must lie in [0, {Ni}); got [{lo}, {hi}]")
    order = None
    if unsorted:
        order = torch.argsort(c, stable=True)
        txt, c = txt.index_select(0, order), c[order]
    c = c.to(torch.int32)                                  # a fresh, 16-byte aligned buffer
    img, lda = _aligned_rows(img)
    txt, ldb = _aligned_rows(txt)
    E = img.shape[1]
    scale = _scalar1(scale)
    dev = img.device
    ws, wsb = _workspace("clipa_retrieval_ranks_multi_workspace", Ni, Nt, device=dev, floor=16)
    oi = torch.empty((2, (Ni + 3) // 4 * 4), device=dev, dtype=torch.int32)       # rows 16-byte aligned
    ot = torch.empty((2, (Nt + 3) // 4 * 4), device=dev, dtype=torch.int32)
    with _Timed("retrieval_ranks_multi", 2.0 * Ni * Nt * E):
        lib.call("clipa_retrieval_ranks_multi", _p(img), _p(txt), _p(c), Ni, Nt, E, lda, ldb, _p(scale), _p(oi[0]),
                 _p(oi[1]), _p(ot[0]), _p(ot[1]), _p(ws), wsb, _stream())
    t2i_gt, t2i_eq = ot[0, :Nt], ot[1, :Nt]
    if order is not None:
        t2i_gt, t2i_eq = (torch.empty_like(t).index_copy_(0, order, t) for t in (t2i_gt, t2i_eq))
    return oi[0, :Ni], oi[1, :Ni], t2i_gt, t2i_eq


def _fewshot_rows(x, index, who, validate=True):
    """x [Ntot, D] f32 and an optional row list -> (x with a 16-byte aligned base, ldx, int32 list | None, rows taken).  A
    misaligned x is copied into a dense buffer (whose row stride is then D, whatever the view's was).  validate: check the
    list's values here (one host sync); a caller that built the list on the host from valid rows passes an int32 tensor and
    validate=False.  The kernels never dereference a bad value either (its row reads NaN)."""
    _chk(x, f32, "x", 2)
    x, ldx = _rowmajor(x)
    if x.data_ptr() % 16:
        x = x.clone(memory_format=torch.contiguous_format)
        ldx = x.shape[1]
    if index is None:
        return x, ldx, None, x.shape[0]
    if not torch.is_tensor(index) or not index.is_cuda or index.dim() != 1 or index.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f"{who}: index must be a 1-D int32 / int64 GPU tensor")
    if validate and index.numel():
        lo, hi = torch.stack([index.min(), index.max()]).tolist()
        if lo < 0 or hi >= x.shape[0]:
            raise RuntimeError(f"{who}: index values must lie in [0, {x.shape[0]}); got [{lo}, {hi}]")
    return x, ldx, index.to(torch.int32).contiguous(), index.numel()


def _vec16(t, n, name):
    _chk(t, f32, name, 1)
    if t.shape[0] != n:
        raise RuntimeError(f"clipa_amd.ops: {name} must hold {n} values, got {t.shape[0]}")
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def fewshot_moments(x, index=None, validate=True):
    """Whitening statistics of the few-shot probe (fewshot_lsr.py:39-40) over rows `index` (int GPU tensor; None = all) of
    x f32 [Ntot, D]: -> (mean [D], std [D]), std = sqrt(mean((x - mean)^2)) + 1e-5, two passes, a fixed summation order.
    validate=False skips the range check of `index` (and its host sync) for a list the caller knows to be valid."""
    x, ldx, index, N = _fewshot_rows(x, index, "fewshot_moments", validate)
    D = x.shape[1]
    if N < 1:
        raise RuntimeError("fewshot_moments: needs at least one row")
    out = torch.empty((2, (D + 3) // 4 * 4), device=x.device, dtype=f32)       # rows 16-byte aligned
    with _Timed("fewshot_moments", 0.0, 8.0 * N * D):
        lib.call("clipa_fewshot_moments", _p(x), _p(index), N, x.shape[0], D, ldx, _p(out[0]), _p(out[1]), _stream())
    return out[0, :D], out[1, :D]


def fewshot_whiten(x, mean, std, index=None, transpose=False, validate=True):
    """z = (x[index] - mean) / std with the constant 100.0 column appended (fewshot_lsr.py:41-44, 95-96): -> Z, the [N, D + 1]
    view of a [N, D + 1 rounded up to 4] buffer whose other columns are 0; with transpose=True -> (Z, Zt), Zt the [D + 1, N]
    view of a [D + 1, N rounded up to 4] buffer padded the same way.  validate: as fewshot_moments."""
    x, ldx, index, N = _fewshot_rows(x, index, "fewshot_whiten", validate)
    D = x.shape[1]
    mean, std = _vec16(mean, D, "mean"), _vec16(std, D, "std")
    dim = D + 1
    zb = torch.empty((N, (dim + 3) // 4 * 4), device=x.device, dtype=f32)
    tb = torch.empty((dim, (N + 3) // 4 * 4), device=x.device, dtype=f32) if transpose else None
    with _Timed("fewshot_whiten", 0.0, 4.0 * N * D * (3 if transpose else 2)):
        lib.call("clipa_fewshot_whiten", _p(x), _p(index), N, x.shape[0], D, ldx, _p(mean), _p(std), _p(zb), zb.shape[1], _p(tb),
                 tb.shape[1] if transpose else 0, _stream())
    return (zb[:, :dim], tb[:, :N]) if transpose else zb[:, :dim]


def fewshot_gram(a):
    """S = a @ a^T for a f32 [M, E] in the fp32 arithmetic of the retrieval kernels (one ascending-k chain per entry); only the
    upper 128 x 128 tiles are computed, their mirror images written: S == S^T bit for bit.  -> f32 [M, M]."""
    _chk(a, f32, "a", 2)
    a, lda = _aligned_rows(a)
    M, E = a.shape
    if E < 1:
        raise RuntimeError("fewshot_gram: a has no columns")
    S = torch.empty((M, M), device=a.device, dtype=f32)
    with _Timed("fewshot_gram", 1.0 * M * M * E):
        lib.call("clipa_fewshot_gram", _p(a), M, E, lda, _p(S), M, _stream())
    return S


def fewshot_class_sums(z, offsets):
    """z^T y of the few-shot probe (fewshot_lsr.py:47, 74) for y = +1 at the label and -1 elsewhere, without y: z f32 [N, dim]
    with its rows sorted by class, offsets the C + 1 segment bounds (host sequence or tensor: 0 = offsets[0] <= ... <=
    offsets[C] = N).  -> R f32 [dim, C], R[d, c] = 2 * (sum of class c's rows) - (sum of all rows)."""
    _chk(z, f32, "z", 2)
    z, ldz = _aligned_rows(z)
    N, dim = z.shape
    off = [int(v) for v in (offsets.reshape(-1).tolist() if torch.is_tensor(offsets) else offsets)]
    if len(off) < 2 or off[0] != 0 or off[-1] != N or any(b < a for a, b in zip(off, off[1:])):
        raise RuntimeError(f"fewshot_class_sums: offsets must rise from 0 to N = {N} over at least one class; got "
                           f"{off[:4]}...{off[-2:]}")
    C = len(off) - 1
    offs = torch.tensor(off, dtype=torch.int32).to(z.device)
    R = torch.empty((dim, C), device=z.device, dtype=f32)
    with _Timed("fewshot_class_sums", 0.0, 4.0 * (N * dim + 3 * dim * C)):
        lib.call("clipa_fewshot_class_sums", _p(z), _p(offs), N, dim, C, ldz, _p(R), C, _stream())
    return R


def fewshot_predict(z, w):
    """argmax over classes of z @ w^T (fewshot_lsr.py:107) without the [Nt, C] logits: z f32 [Nt, dim] whitened test rows,
    w f32 [C, dim] class-major weights.  -> (pred int32 [Nt], best f32 [Nt]): the lowest class index among a row's maxima and
    that logit."""
    _chk(z, f32, "z", 2)
    _chk(w, f32, "w", 2)
    if z.shape[1] != w.shape[1] or w.shape[0] < 1 or w.shape[1] < 1:
        raise RuntimeError(f"fewshot_predict: z {tuple(z.shape)} and w {tuple(w.shape)} must be [Nt, dim] and [C >= 1, dim >= 1]")
    z, ldz = _aligned_rows(z)
    w, ldw = _aligned_rows(w)
    Nt, dim = z.shape
    C = w.shape[0]
    out_p = torch.empty((Nt + 3) // 4 * 4, device=z.device, dtype=torch.int32)
    out_b = torch.empty((Nt + 3) // 4 * 4, device=z.device, dtype=f32)
    with _Timed("fewshot_predict", 2.0 * Nt * C * dim):
        lib.call("clipa_fewshot_predict", _p(z), _p(w), Nt, C, dim, ldz, ldw, _p(out_p), _p(out_b), _stream())
    return out_p[:Nt], out_b[:Nt]


LOGREG_MAX_N = 1 << 21      # csrc/logreg.hip: a 128-class block of the [C, N] logits stays below 1 GiB


def logreg_prepare(x):
    """The operands of the logistic-regression probe (csrc/logreg.hip), once per fit: x f32 [N, D] -> (xp, xt), xp the
    [N, D + 1] view of a [N, D + 1 rounded up to 4] buffer holding [x, 1] and zeros, xt the [D + 1, N] view of its transpose in
    a [D + 1, N rounded up to 4] buffer padded the same way."""
    x, ldx, _, N = _fewshot_rows(x, None, "logreg_prepare")
    D = x.shape[1]
    if N < 1 or N >= LOGREG_MAX_N:
        raise RuntimeError(f"logreg_prepare: N = {N} rows must lie in [1, 2^21 = {LOGREG_MAX_N}) (features that do not fit one "
                           f"problem are not supported)")
    dim = D + 1
    pb = torch.empty((N, (dim + 3) // 4 * 4), device=x.device, dtype=f32)
    tb = torch.empty((dim, (N + 3) // 4 * 4), device=x.device, dtype=f32)
    with _Timed("logreg_prepare", 0.0, 12.0 * N * dim):
        lib.call("clipa_logreg_prepare", _p(x), N, D, ldx, _p(pb), pb.shape[1], _p(tb), tb.shape[1], _stream())
    return pb[:, :dim], tb[:, :N]


def _logreg_view(t, name, rows=None, cols=None):
    """A matrix the logreg kernels take as it is: f32 [rows, cols], unit column stride, 16-byte aligned rows."""
    _chk(t, f32, name, 2)
    ld = t.stride(0) if t.shape[0] > 1 else (t.shape[1] + 3) // 4 * 4
    if t.stride(1) != 1 or ld % 4 or t.data_ptr() % 16 or ld < t.shape[1]:
        raise RuntimeError(f"clipa_amd.ops: {name} must have unit column stride and 16-byte aligned rows (as logreg_prepare / "
                           f"logreg_logits return it); got strides {tuple(t.stride())}")
    if (rows is not None and t.shape[0] != rows) or (cols is not None and t.shape[1] != cols):
        raise RuntimeError(f"clipa_amd.ops: {name} must be [{rows}, {cols}], got {tuple(t.shape)}")
    return ld


def logreg_logits(theta, xp, out=None):
    """theta f32 [C, dim] (class-major, the last column the bias), xp [N, dim] of logreg_prepare -> (zt, lse, pred, best):
    zt the [C, N] view of a [C, N rounded up to 4] buffer (`out`: such a view to write into, from an earlier call), zt[c, n] =
    theta_c . xp_n; lse f32 [N] = log sum_c exp zt[c, n]; pred int32 [N] / best f32 [N]: the lowest class among a sample's
    maxima and that logit, as fewshot_predict(xp, theta) gives them bit for bit."""
    _chk(theta, f32, "theta", 2)
    if theta.shape[0] < 1 or theta.shape[1] < 1 or xp.dim() != 2 or theta.shape[1] != xp.shape[1]:
        raise RuntimeError(f"logreg_logits: theta {tuple(theta.shape)} and xp {tuple(xp.shape)} must be [C >= 1, dim] and [N, dim]")
    theta, ldt = _aligned_rows(theta)
    C, dim = theta.shape
    N = xp.shape[0]
    ld = _logreg_view(xp, "xp")
    if N < 1 or N >= LOGREG_MAX_N:
        raise RuntimeError(f"logreg_logits: N = {N} rows must lie in [1, 2^21 = {LOGREG_MAX_N})")
    zt = torch.empty((C, (N + 3) // 4 * 4), device=xp.device, dtype=f32)[:, :N] if out is None else out
    ldz = _logreg_view(zt, "out", C, N)
    vec = torch.empty((3, (N + 3) // 4 * 4), device=xp.device, dtype=f32)
    pred = vec[1].view(torch.int32)
    with _Timed("logreg_logits", 2.0 * N * C * dim, 4.0 * (N * C + N * dim + C * dim)):
        lib.call("clipa_logreg_logits", _p(theta), _p(xp), C, N, dim, ldt, ld, _p(zt), ldz, _p(vec[0]), _p(pred), _p(vec[2]),
                 _stream())
    return zt, vec[0, :N], pred[:N], vec[2, :N]


def logreg_residual(zt, lse, y, overwrite=True):
    """ce[n] = lse[n] - zt[y_n, n]; with overwrite, then in place zt[c, n] <- exp(zt[c, n] - lse[n]) - [c == y_n].  zt, lse of
    logreg_logits; y int32 GPU tensor [N] with values in [0, C) (a value outside gives ce = NaN).  -> ce f32 [N]."""
    C, N = zt.shape
    ldz = _logreg_view(zt, "zt")
    if not torch.is_tensor(y) or not y.is_cuda or y.dtype != torch.int32 or tuple(y.shape) != (N,):
        raise RuntimeError(f"logreg_residual: y must be an int32 GPU tensor of {N} labels")
    lse, y = _vec16(lse, N, "lse"), (y.contiguous() if y.data_ptr() % 16 == 0 and y.is_contiguous() else y.clone())
    ce = torch.empty((N + 3) // 4 * 4, device=zt.device, dtype=f32)
    with _Timed("logreg_residual", 0.0, (8.0 if overwrite else 0.0) * N * C + 16.0 * N):
        lib.call("clipa_logreg_residual", _p(zt), _p(lse), _p(y), C, N, ldz, _p(ce), 1 if overwrite else 0, _stream())
    return ce[:N]


def logreg_grad(gt, xt, _slice=0, _max_workgroups=0):
    """dtheta[c, d] = sum_n gt[c, n] * xt[d, n]: gt f32 [C, N] (the residual), xt [dim, N] of logreg_prepare -> f32 [C, dim].
    n runs in slices of 4096 samples, each an ascending-n fp32 chain, the slices added in ascending order: bit-identical
    whatever the launch.  _slice / _max_workgroups: tests only - another slice length (another, equally fixed, summation
    order) and a cap on the grid (no effect on any bit)."""
    C, N = gt.shape
    ldz = _logreg_view(gt, "gt")
    ldn = _logreg_view(xt, "xt", None, N)
    dim = xt.shape[0]
    out = torch.empty((C, (dim + 3) // 4 * 4), device=gt.device, dtype=f32)
    ws, wsb = _workspace("clipa_logreg_grad_workspace", C, dim, N, int(_slice), device=gt.device, floor=16)
    with _Timed("logreg_grad", 2.0 * N * C * dim, 4.0 * (N * C + N * dim + C * dim)):
        lib.call("clipa_logreg_grad", _p(gt), _p(xt), C, dim, N, ldz, ldn, _p(out), out.shape[1], int(_slice),
                 int(_max_workgroups), _p(ws), wsb, _stream())
    return out[:, :dim]


def zeroshot_class_mean(emb, offsets, eps=0.0):
    """The prompt-ensemble classifier of zero-shot classification (zero_shot.py:37-38; _average_embeddings of
    discriminative_classifier.py:165-170): emb f32 [N, E] with its rows sorted by class, offsets the C + 1 segment bounds (host
    sequence or tensor: 0 = offsets[0] < ... < offsets[C] = N).  -> W, the [C, E] view of a [C, E rounded up to 4] buffer whose
    other columns are 0: W_c = m_c / (eps + ||m_c||), m_c the mean of class c's rows, in the fixed order of csrc/zeroshot.hip.
    An empty class raises ("Classes without embeddings")."""
    _chk(emb, f32, "emb", 2)
    emb, lde = _rowmajor(emb)
    if emb.data_ptr() % 16:
        emb = emb.clone(memory_format=torch.contiguous_format)
        lde = emb.shape[1]
    N, E = emb.shape
    off = [int(v) for v in (offsets.reshape(-1).tolist() if torch.is_tensor(offsets) else offsets)]
    if len(off) < 1 or off[0] != 0 or off[-1] != N or any(b < a for a, b in zip(off, off[1:])):
        raise RuntimeError(f"zeroshot_class_mean: offsets must rise from 0 to N = {N}; got {off[:4]}...{off[-2:]}")
    empty = [c for c, (a, b) in enumerate(zip(off, off[1:])) if a == b]
    if empty:
        raise RuntimeError(f"zeroshot_class_mean: Classes without embeddings: {empty[:8]}{'...' if len(empty) > 8 else ''}")
    if not float(eps) >= 0.0:
        raise RuntimeError(f"zeroshot_class_mean: eps = {eps} must be >= 0")
    C = len(off) - 1
    ldw = (E + 3) // 4 * 4
    W = torch.empty((C, ldw), device=emb.device, dtype=f32)
    if C:
        offs = torch.tensor(off, dtype=torch.int32).to(emb.device)
        with _Timed("zeroshot_class_mean", 0.0, 4.0 * (N * E + 3 * C * E)):
            lib.call("clipa_zeroshot_class_mean", _p(emb), _p(offs), N, C, E, lde, float(eps), _p(W), ldw, _stream())
    return W[:, :E]


def zeroshot_ranks(feat, w, labels):
    """Rank of every image's best label among the classes, without the [B, C] logits (zero_shot.py:47-50, 77-80;
    discriminative_classifier.py:303-309): feat f32 [B, E], w f32 [C, E] (class-major classifier), labels int32 [B, Lmax] on the
    device, 1 <= Lmax <= 32, -1 = no label, other values in [0, C) (the caller's to check: a value outside names no class).
    v = feat @ w^T in fp32, no scale.  -> int32 [B] (gt, eq, pred): the classes that beat / tie (not themselves labels) the
    image's best label, and the lowest class index among the row's maxima.  A row without labels: gt = C, eq = 0."""
    _chk(feat, f32, "feat", 2)
    _chk(w, f32, "w", 2)
    _chk(labels, torch.int32, "labels", 2)
    B, E = feat.shape
    C, Lmax = w.shape[0], labels.shape[1]
    if w.shape[1] != E or labels.shape[0] != B:
        raise RuntimeError(f"zeroshot_ranks: feat {tuple(feat.shape)}, w {tuple(w.shape)} and labels {tuple(labels.shape)} must be "
                           f"[B, E], [C, E] and [B, Lmax]")
    if not 1 <= Lmax <= 32:
        raise RuntimeError(f"zeroshot_ranks: Lmax = {Lmax} labels per image; the kernel takes 1 to 32")
    out = torch.empty((3, (B + 3) // 4 * 4), device=feat.device, dtype=torch.int32)       # rows 16-byte aligned
    if B == 0:
        return tuple(out[k, :0] for k in range(3))
    if C < 1 or E < 1:
        raise RuntimeError(f"zeroshot_ranks: C = {C} classes of E = {E} columns: nothing to rank {B} rows against")
    feat, lda = _aligned_rows(feat)
    w, ldw = _aligned_rows(w)
    labels = labels.contiguous()
    if labels.data_ptr() % 16:
        labels = labels.clone()
    with _Timed("zeroshot_ranks", 4.0 * B * C * E):
        lib.call("clipa_zeroshot_ranks", _p(feat), _p(w), _p(labels), B, C, E, Lmax, lda, ldw, *(_p(out[k]) for k in range(3)),
                 _stream())
    return tuple(out[k, :B] for k in range(3))


def topk_similarity(q, g, k, scale=None, index_base=0, carry=None, splits=0):
    """The k best gallery rows of every query without the [Nq, Ng] similarities (zero_shot.py:47-50 `output.topk`;
    image_text_retrieval.py:77-82): q f32 [Nq, E], g f32 [Ng, E], v = s * q @ g^T in fp32 with s = scale[0] read on the device
    (None = 1).  -> (values f32 [Nq, k], indices int64 [Nq, k]), best first under the strict order of csrc/topk.hip: the larger
    value first, equal values (IEEE ==) by the lower index, a NaN before every number; index = index_base + gallery row; with
    fewer than k entries the tail is (-inf, -1).  carry = (values, indices) of earlier calls over other shards of the gallery
    (same k): the result is the first k of both.  splits: column splits of the launch, 0 = the entry point's choice; every value
    in [1, gallery tiles of 128] gives the same output."""
    _chk(q, f32, "q", 2)
    _chk(g, f32, "g", 2)
    Nq, E = q.shape
    Ng = g.shape[0]
    k, index_base, splits = int(k), int(index_base), int(splits)
    if g.shape[1] != E:
        raise RuntimeError(f"topk_similarity: q {tuple(q.shape)} and g {tuple(g.shape)} must be [Nq, E] and [Ng, E]")
    if not 1 <= k <= 32:
        raise RuntimeError(f"topk_similarity: k = {k}; the kernel takes 1 to 32")
    cv = ci = None
    if carry is not None:
        cv, ci = carry
        _chk(cv, f32, "carry values", 2)
        _chk(ci, torch.int64, "carry indices", 2)
        if tuple(cv.shape) != (Nq, k) or tuple(ci.shape) != (Nq, k):
            raise RuntimeError(f"topk_similarity: carry {tuple(cv.shape)}, {tuple(ci.shape)} must both be [Nq, k] = [{Nq}, {k}]")
        cv, ci = cv.contiguous(), ci.contiguous()
        if cv.data_ptr() % 16:
            cv = cv.clone()
        if ci.data_ptr() % 16:
            ci = ci.clone()
    out_v = torch.empty((Nq, k), device=q.device, dtype=f32)
    out_i = torch.empty((Nq, k), device=q.device, dtype=torch.int64)
    if Nq == 0:
        return out_v, out_i
    q, ldq = _aligned_rows(q)
    g, ldg = _aligned_rows(g)
    scale = _scalar1(scale)
    ws, wsb = _workspace("clipa_topk_workspace", Nq, Ng, k, splits, device=q.device, floor=16)
    with _Timed("topk_similarity", 2.0 * Nq * Ng * E):
        lib.call("clipa_topk", _p(q), _p(g), Nq, Ng, E, ldq, ldg, _p(scale), k, index_base, splits, _p(cv), _p(ci), _p(out_v),
                 _p(out_i), _p(ws), wsb, _stream())
    return out_v, out_i


def sum_scale(x, scale, out=None, accumulate=False):
    x = x.contiguous()
    if out is None:
        out = torch.empty((), device=x.device, dtype=f32)
    lib.call("clipa_sum_scale", _p(x), _p(out), x.numel(), float(scale), int(accumulate), _stream())
    return out


def _chk_moments(p, m, v):
    for name, t in (("exp_avg", m), ("exp_avg_sq", v)):
        if t.dtype != f32 or not t.is_contiguous() or t.numel() != p.numel() or not t.is_cuda:
            raise RuntimeError(f"adamw: {name} must be a contiguous f32 GPU tensor with the parameter's numel (got {t.dtype}, "
                               f"{t.numel()} vs {p.numel()}) - the kernel reads and writes it as float*")


def adamw_(param, grad, exp_avg, exp_avg_sq, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    _chk_moments(param, exp_avg, exp_avg_sq)
    lib.call("clipa_adamw", _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), int(param.dtype == f32),
             int(grad.dtype == f32), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step),
             float(grad_scale), _stream())


def adamw_multi_(params, grads, exp_avgs, exp_avg_sqs, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0,
                 grad_scale_dev=None, clamp_index=-1, clamp=(0.0, 0.0)):
    """One AdamW update over a list of tensors that share dtypes, hyper-parameters and step count.  grad_scale_dev: f32
    device scalar multiplied into every gradient (clip coefficient); clamp_index: list position of the tensor that is
    clamped to `clamp` after its update."""
    n = len(params)
    if n == 0:
        return
    pf32, gf32 = params[0].dtype == f32, grads[0].dtype == f32
    for t, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs):
        if (t.dtype == f32) != pf32 or (g.dtype == f32) != gf32 or not t.is_cuda:
            raise RuntimeError("adamw_multi_: mixed dtypes in one call / tensors must live on the GPU")
        if t.dtype not in (f32, bf16) or g.dtype not in (f32, bf16) or g.numel() != t.numel() or not t.is_contiguous() \
                or not g.is_contiguous():
            raise RuntimeError("adamw_multi_: parameters / gradients must be contiguous f32 or bf16 tensors of equal numel")
        _chk_moments(t, m, v)
    if grad_scale_dev is not None:
        _chk(grad_scale_dev, f32, "grad_scale_dev")
    lib.call("clipa_adamw_multi", _ptr_array(params), _ptr_array(grads), _ptr_array(exp_avgs), _ptr_array(exp_avg_sqs),
             _numel_array(params), n, int(pf32), int(gf32), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
             int(step), float(grad_scale), _p(grad_scale_dev), int(clamp_index), float(clamp[0]), float(clamp[1]), _stream())


def grad_sqnorm(grads, buf=None):
    """buf[0] += sum of squares of the listed gradients (device f32 [3] = [sum of squares, norm, coef]; created zeroed)."""
    dev = grads[0].device
    if buf is None:
        buf = torch.zeros(3, device=dev, dtype=f32)
    for is32 in (True, False):
        sel = [g for g in grads if (g.dtype == f32) == is32]
        if not sel:
            continue
        for g in sel:
            if g.dtype not in (f32, bf16) or not g.is_contiguous() or not g.is_cuda:
                raise RuntimeError("grad_sqnorm: gradients must be contiguous f32 / bf16 GPU tensors")
        nblk = sum((g.numel() + 4095) // 4096 for g in sel)            # one partial per 4096-element block, summed in a fixed order
        part = torch.empty(max(nblk, 1), device=dev, dtype=f32)
        lib.call("clipa_grad_sqnorm_multi", _ptr_array(sel), _numel_array(sel), len(sel), int(is32), _p(buf), _p(part), nblk, _stream())
    return buf


def clip_coef(buf, max_norm):
    """buf[0] = sum of squares -> (total_norm, coef) device scalars (views of buf), coef = clamp(max_norm / (norm + 1e-6), max=1):
    1 below the threshold, 0 for an infinite norm, NaN for a NaN norm (torch.nn.utils.clip_grad_norm_)."""
    lib.call("clipa_clip_coef", _p(buf), float(max_norm), ctypes.c_void_p(buf.data_ptr() + 4), ctypes.c_void_p(buf.data_ptr() + 8),
             _stream())
    return buf[1], buf[2]


def grad_clip_coef(grads, max_norm):
    """clip_grad_norm_ on the device: -> (total_norm, coef) f32 device scalars, coef = clamp(max_norm / (norm + 1e-6), max=1)
    (NaN when any gradient element is NaN)."""
    return clip_coef(grad_sqnorm(grads), max_norm)


def reduce_shards(pieces, world, out=None, scale=None, out_dtype=None):
    """out[i] = scale * sum_w pieces[w*n + i] (scale defaults to 1/world): the local sum of a one-hop reduce-scatter."""
    if pieces.dtype not in (f32, bf16) or not pieces.is_contiguous() or not pieces.is_cuda:
        raise RuntimeError("reduce_shards: pieces must be a contiguous f32 / bf16 GPU tensor")
    n = pieces.numel() // world
    if n * world != pieces.numel():
        raise RuntimeError("reduce_shards: numel must be a multiple of world")
    if out is None:
        out = torch.empty(n, device=pieces.device, dtype=out_dtype or pieces.dtype)
    lib.call("clipa_reduce_shards", _p(pieces), _p(out), n, int(world), int(pieces.dtype == f32), int(out.dtype == f32),
             float(1.0 / world if scale is None else scale), _stream())
    return out
