"""Characterisation of clipa_amd/engine.py without a GPU: which `ops.*` calls one training step issues, on which operands, in
which order at token level, and how many bytes of op results are alive while it does so.

The real engine, model and loss run with `ops` swapped for a recording wrapper around the torch stand-ins of tests/cpu_ops.py
(plus the LayerScale and attention-pooling stand-ins), the way tests/test_engine_cpu.py swaps them; per configuration one
forward + loss + backward of a tiny fixture.  Per call the trace holds the op's name, every argument bound to the stand-in's
signature (so a default and the same value spelled out are one thing; 1, 1.0 and True stay three), and per tensor operand and
result its dtype, shape and an IDENTITY.  The identity is structural, never a digest of values (CPU BLAS results differ between
hosts):
    p:<name>              a parameter or buffer of the model         in:<name>    the model's input
    <digest>.<position>   result <position> of the recorded call with that digest; the digest is taken over the call's name,
                          arguments and operand identities, so it does not depend on when the call ran - a tensor that the
                          backward rebuilds with the launch the forward used IS the forward's tensor
    t:<dtype><shape>      anything else: memory torch allocated in engine code or computed outside `ops`
with "@offset,shape,stride" appended where the operand is another view of that storage than the one first seen.

Against tests/golden/engine_call_trace.json, per configuration:
  (a) the multiset of calls is equal: no launch added, dropped or given another operand;
  (b) the subsequence of TOKEN-LEVEL calls - those that read or write a tensor with as many rows as the token matrix a tower's
      blocks receive (after patch dropout / unpadding) - is identical in order; no parameter dimension of a fixture equals such
      a row count, so the split is unambiguous;
  (c) in a second run that holds only weak references to the tensors the ops return, the bytes of still-alive op results at
      every token-level call are not higher than the golden's, nor is their maximum: a helper's frame that keeps an [M, 4D]
      tensor alive longer than before shows here.  That run measures a model's second step, so the weight cache's operand
      copies - which outlive every step - are not counted as a step's transients.

The golden is the trace of the engine.py of the commit named in it - the parent of the engine's "one copy of each half-block"
refactor - and is never regenerated from later code: the refactor has to reproduce it.  It was written from a worktree of that
commit with only this file copied in:

    git worktree add <dir> <commit> && cp tests/test_engine_trace_cpu.py <dir>/tests/
    (cd <dir> && python -m tests.test_engine_trace_cpu --write <repo>/tests/golden/engine_call_trace.json)

To keep the file small it holds, per call, the op and a digest of the whole description (arguments, operand identities, result
dtypes and shapes), not the description: a failure prints the current code's calls in full and names the golden's by op + digest.
"""
import collections
import contextlib
import hashlib
import inspect
import json
import os
import subprocess
import sys
import types
import weakref

import pytest
import torch

import clipa_amd
from clipa_amd import engine, loss as loss_mod, model as model_mod, optim as optim_mod, zero as zero_mod

from . import cpu_ops, layerscale_cpu_ops, mappool_cases, mappool_cpu_ops
from . import layerscale_cases
from .conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_call_trace.json")
_SWAPPED = (engine, loss_mod, model_mod, optim_mod, zero_mod)
BATCH = 7
_DT = {torch.bfloat16: "bf16", torch.float32: "f32", torch.uint8: "u8", torch.int32: "i32", torch.int64: "i64",
       torch.float64: "f64", torch.bool: "b8"}


def _standins():
    """Every stand-in under one namespace: tests/cpu_ops, the LayerScale ops, the attention-pooling ops (and its gemm_nt, which
    honours `out=`)."""
    ns = {}
    for mod in (cpu_ops, layerscale_cpu_ops, mappool_cpu_ops):
        ns.update({k: v for k, v in vars(mod).items() if not k.startswith("_") and k != "swap_in"})
    return ns


def _view(t):
    return f"{t.storage_offset()},{list(t.shape)},{list(t.stride())}"


def _shape(t):
    return f"{_DT.get(t.dtype, str(t.dtype))}{list(t.shape)}"


class Recorder:
    """strong=True: the identity run - every tensor an op returned is kept alive, so no address is reused and a storage address
    names one tensor.  strong=False: the live-byte run - weak references only, no identities."""

    def __init__(self, named, strong):
        self.strong, self.depth = strong, 0
        self.calls = []            # identity run: the description of every call
        self.shapes = []           # both runs: per call, the set of leading dimensions of its tensor operands and results
        self.live = []             # live-byte run: bytes of alive op results when the call was made
        self.store = {}            # storage address -> (identity, view first seen, the tensor: kept alive)
        self.results = []          # weak references to the tensors the ops returned
        for name, t in named.items():
            if t.numel():
                self.store.setdefault(t.untyped_storage().data_ptr(), (name, _view(t), t))

    # ---- identities -------------------------------------------------------------------------------------------------------
    def ident(self, t):
        ent = self.store.get(t.untyped_storage().data_ptr()) if t.numel() else None
        if ent is None:
            whole = t.is_contiguous() and t.numel() * t.element_size() == t.untyped_storage().nbytes()
            return "t:" + _shape(t) + ("" if whole else "@" + _view(t))
        return ent[0] + ("" if ent[1] == _view(t) else "@" + _view(t))

    def arg(self, a):
        if torch.is_tensor(a):
            return f"{self.ident(a)}|{_shape(a)}"
        if a is None or isinstance(a, (bool, int, float, str)):
            return a
        if isinstance(a, torch.dtype):
            return str(a)
        if isinstance(a, (tuple, list)):
            return [self.arg(v) for v in a]
        if type(a).__name__ == "VarLen":
            return f"VarLen(B={a.B},ctx={a.ctx},T={a.T},rows={a.rows})"
        raise TypeError(f"unexpected argument {a!r}")

    def _tensors(self, x, path=""):
        if torch.is_tensor(x):
            yield path, x
        elif isinstance(x, (tuple, list)):
            for i, v in enumerate(x):
                yield from self._tensors(v, f"{path}.{i}" if path else str(i))
        elif type(x).__name__ == "VarLen":
            pass
        elif isinstance(x, dict):
            for k, v in x.items():
                yield from self._tensors(v, k)

    # ---- the wrapper ------------------------------------------------------------------------------------------------------
    def wrap(self, name, fn):
        sig = inspect.signature(getattr(cpu_ops, name, fn))      # (the attention-pooling gemm_nt forwards **kw to cpu_ops')

        def wrapped(*args, **kw):
            if self.depth:
                return fn(*args, **kw)
            bound = sig.bind(*args, **kw)
            bound.apply_defaults()
            rows = {t.shape[0] for _, t in self._tensors(dict(bound.arguments)) if t.ndim}
            if self.strong:
                desc = {"op": name, "args": {k: self.arg(v) for k, v in bound.arguments.items()}}
                cid = hashlib.sha1(json.dumps(desc, sort_keys=True).encode()).hexdigest()[:12]
            else:
                self.live.append(self.live_bytes())
            del bound
            self.depth += 1
            try:
                r = fn(*args, **kw)
            finally:
                self.depth -= 1
            outs = list(self._tensors(r))
            rows |= {t.shape[0] for _, t in outs if t.ndim}
            self.shapes.append((name, rows))
            if self.strong:
                desc["out"] = []
                for pos, t in outs:
                    known = self.store.get(t.untyped_storage().data_ptr()) if t.numel() else None
                    if known is None and t.numel():
                        self.store[t.untyped_storage().data_ptr()] = (f"{cid}.{pos}", _view(t), t)
                    desc["out"].append(_shape(t) + ("" if known is None else "=" + self.ident(t)))
                self.calls.append(desc)
            else:
                self.results.extend(weakref.ref(t) for _, t in outs)
            return r
        return wrapped

    def live_bytes(self):
        seen, alive = {}, []
        for ref in self.results:
            t = ref()
            if t is not None:
                alive.append(ref)
                seen[t.untyped_storage().data_ptr()] = t.untyped_storage().nbytes()
            del t
        self.results = alive
        return sum(seen.values())


@contextlib.contextmanager
def _recording(rec, token_rows):
    ns = types.SimpleNamespace(**{k: rec.wrap(k, v) if inspect.isfunction(v) else v for k, v in _standins().items()})
    real = [mod.ops for mod in _SWAPPED]
    run = model_mod.Transformer.run

    def spy(self, x, *a, **k):
        token_rows.add(int(x.shape[0]))
        return run(self, x, *a, **k)
    for mod in _SWAPPED:
        mod.ops = ns
    model_mod.Transformer.run = spy
    try:
        yield
    finally:
        model_mod.Transformer.run = run
        for mod, ops in zip(_SWAPPED, real):
            mod.ops = ops


# ---- the configurations: name -> () -> (model, images, texts, seed | None) ----------------------------------------------------
def _golden_model(case, precision="fp32", recompute=True, grad_fmt="e4m3", predict=False, visual=None, text=None, counts=None,
                  unlocked=None, unpad=False, seed=None, load=load_golden):
    def make():
        g = load(case)
        m = clipa_amd.CLIP(**g.cfg, output_dict=True)
        m.load_state_dict(g.sd, strict=True)
        if precision in ("bf16", "fp8"):
            clipa_amd.convert_weights_to_lp(m, torch.bfloat16)
        m.set_grad_checkpointing(recompute)
        for t, knobs in ((m.visual.transformer, visual), (m.transformer, text)):
            if precision == "fp8":
                t.fp8, t.fp8_grad_format, t.fp8_predicted_scales = True, grad_fmt, predict
            for k, v in (knobs or {}).items():
                setattr(t, k, v)
            if counts:
                t.keep_counts = dict(t.keep_counts, **counts)
        if unlocked is not None:
            m.lock_image_tower(unlocked_groups=unlocked)
        m.unpad_text = unpad
        # the first BATCH samples of the fixture: with all 8 the text towers' 8 * 16 = 128 (8 * 8 = 64) token rows would equal a width
        return m, g.images_u8[:BATCH], g.texts[:BATCH], (g.drop_seed if seed == "drop" else seed)
    return make


def _map_model():
    m, images, texts = mappool_cases.toy_model()
    clipa_amd.convert_weights_to_lp(m, torch.bfloat16)
    m.set_grad_checkpointing(True)
    return m, images, texts, None


G, LS = _golden_model, layerscale_cases.load
CONFIGS = {
    "cls_erf/bf16/recompute": G("cls_erf", "bf16"),
    "cls_erf/bf16/keep_all": G("cls_erf", "bf16", recompute=False),
    "cls_erf/bf16/light+light8|light8+medium": G("cls_erf", "bf16", visual=dict(keep_blocks=1, light8_blocks=1),
                                                 text=dict(light8_blocks=1, medium_blocks=1)),
    "cls_erf/bf16/light+medium": G("cls_erf", "bf16", visual=dict(keep_blocks=1, medium_blocks=1),
                                   text=dict(keep_blocks=1, medium_blocks=1)),
    "cls_erf/bf16/keep_qkv1_a1": G("cls_erf", "bf16", counts={"qkv": 1, "a": 1}),
    "cls_erf/bf16/keep_h8_1_x1_1": G("cls_erf", "bf16", counts={"h8": 1, "x1": 1}),
    # (a count of 1 reaches the towers' last blocks only - LastBlockFn, whose x1 / pre-activation are B rows; 2: a ResBlockFn too)
    "cls_erf/bf16/keep_h8_2_x1_2": G("cls_erf", "bf16", counts={"h8": 2, "x1": 2}),
    "cls_erf/bf16/keep_h_2_qkv_2": G("cls_erf", "bf16", counts={"h": 2, "qkv": 2}),
    "cls_erf/bf16/keep_a_2": G("cls_erf", "bf16", counts={"a": 2}),
    "cls_erf/fp32": G("cls_erf"),
    "cls_erf/fp8/recompute": G("cls_erf", "fp8"),
    "cls_erf/fp8/keep_all": G("cls_erf", "fp8", recompute=False),
    "cls_erf/fp8/keep_h8_1": G("cls_erf", "fp8", counts={"h8": 1}),
    "cls_erf/fp8/keep_h8_2": G("cls_erf", "fp8", counts={"h8": 2}),
    "cls_erf/fp8/keep_a_2_x1_2": G("cls_erf", "fp8", counts={"a": 2, "x1": 2}),
    "cls_erf/fp8/predict_keep_h8_2": G("cls_erf", "fp8", predict=True, counts={"h8": 2}),
    "cls_erf/fp8/e5m2_keep_h8_2": G("cls_erf", "fp8", grad_fmt="e5m2", counts={"h8": 2}),
    "cls_erf/fp8/light+medium": G("cls_erf", "fp8", visual=dict(keep_blocks=1, medium_blocks=1),
                                  text=dict(keep_blocks=1, medium_blocks=1)),
    "cls_erf/fp8/predict": G("cls_erf", "fp8", predict=True),
    "cls_erf/fp8/predict_keep_h8_1": G("cls_erf", "fp8", predict=True, counts={"h8": 1}),
    "cls_erf/fp8/predict_e5m2": G("cls_erf", "fp8", predict=True, grad_fmt="e5m2"),
    "cls_erf/bf16/image_tower_locked": G("cls_erf", "bf16", unlocked=0),
    "cls_erf/bf16/image_tower_locked_but_2_groups": G("cls_erf", "bf16", unlocked=2),
    "cls_erf/fp8/image_tower_locked_but_2_groups": G("cls_erf", "fp8", unlocked=2),
    "gap_sincos_tanh/bf16": G("gap_sincos_tanh", "bf16"),
    "gap_sincos_tanh/bf16/light8+medium": G("gap_sincos_tanh", "bf16", visual=dict(light8_blocks=1, medium_blocks=1),
                                            text=dict(light8_blocks=1, medium_blocks=1)),
    "gap_sincos_tanh/fp8": G("gap_sincos_tanh", "fp8"),
    "layerscale_cls_erf/bf16": G("layerscale_cls_erf", "bf16", load=LS),
    "layerscale_cls_erf/fp8": G("layerscale_cls_erf", "fp8", load=LS),
    "patchdrop_gap/fp32": G("patchdrop_gap", visual=dict(medium_blocks=1), seed="drop"),
    "cls_erf/fp32/unpad_text": G("cls_erf", text=dict(medium_blocks=1), unpad=True),
    "cls_erf/fp8/unpad_text": G("cls_erf", "fp8", unpad=True),
    "map_toy/bf16": _map_model,
}


def _step(m, images, texts, seed):
    if seed is not None:
        torch.manual_seed(seed)
    out = m(images, texts)
    clipa_amd.ClipLoss()(**out, output_dict=True)["contrastive_loss"].backward()


def record(name):
    """-> dict(token_rows, weight_dims, calls: [(description, token-level?)], live: bytes alive at each token-level call)."""
    # the identity run: the model's first step, which also fills the weight cache (operand copies, folds: part of the multiset)
    m, images, texts, seed = CONFIGS[name]()
    assert m.training
    named = {"p:" + k: v for k, v in list(m.named_parameters()) + list(m.named_buffers())}
    named.update({"in:images": images, "in:texts": texts})
    ident, token_rows = Recorder(named, True), set()
    with _recording(ident, token_rows):
        _step(m, images, texts, seed)
    dims = {int(d) for p in m.parameters() for d in p.shape}
    token = [bool(rows & token_rows) for _, rows in ident.shapes]
    # the live-byte run: the SECOND step of a fresh model - the steady state, in which the cached operands exist before the step
    # and are nobody's transient (when in the first step a cache entry is built is not a property of the step)
    m, images, texts, seed = CONFIGS[name]()
    with _recording(Recorder({}, False), set()):
        _step(m, images, texts, seed)
    m.zero_grad(set_to_none=True)
    weak, rows2 = Recorder({}, False), set()
    with _recording(weak, rows2):
        _step(m, images, texts, seed)
    steady = [(n, bool(rows & rows2), b) for (n, rows), b in zip(weak.shapes, weak.live)]
    assert token_rows == rows2, name
    assert [n for n, tok, _ in steady if tok] == [n for (n, _), tok in zip(ident.shapes, token) if tok], name
    return {"token_rows": sorted(token_rows), "weight_dims": sorted(dims), "calls": list(zip(ident.calls, token)),
            "live": [b for _, tok, b in steady if tok]}


def _key(desc):
    return desc["op"] + ":" + hashlib.sha1(json.dumps(desc, sort_keys=True).encode()).hexdigest()[:10]


@pytest.fixture(scope="module")
def golden_trace():
    with open(GOLDEN) as f:
        g = json.load(f)
    for c in g["configs"].values():      # a call is written "<index into ops>:<digest>", with a * behind it when at token level
        c["trace"] = [(g["ops"][int(e.split(":")[0])] + ":" + e.split(":")[1].rstrip("*"), e.endswith("*")) for e in c["trace"].split()]
    return g


def test_the_configurations_are_the_golden_file_s(golden_trace):
    assert sorted(CONFIGS) == sorted(golden_trace["configs"])
    assert len(golden_trace["commit"]) == 40


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_engine_call_trace(name, golden_trace):
    """A failure prints the head's calls in full; of the golden's it has the op and the digest (the full description is what the
    same run at the golden's commit prints)."""
    want = golden_trace["configs"][name]
    got = record(name)
    assert got["token_rows"] == want["token_rows"]
    assert not set(got["token_rows"]) & set(got["weight_dims"]), "a parameter dimension equals a token row count"
    got_keys = [_key(d) for d, _ in got["calls"]]
    describe = {k: d for k, (d, _) in zip(got_keys, got["calls"])}
    # (a) the multiset of calls
    extra = collections.Counter(got_keys) - collections.Counter(k for k, _ in want["trace"])
    missing = collections.Counter(k for k, _ in want["trace"]) - collections.Counter(got_keys)
    assert not extra and not missing, (
        f"{name}: calls the golden step does not make:\n" + "\n".join(f"  {n} x {json.dumps(describe[k])}" for k, n in extra.items())
        + "\ncalls of the golden step that are missing:\n" + "\n".join(f"  {n} x {k}" for k, n in missing.items()))
    # (b) the order of the token-level calls
    got_tok = [k for k, (_, tok) in zip(got_keys, got["calls"]) if tok]
    want_tok = [k for k, tok in want["trace"] if tok]
    for i, (a, b) in enumerate(zip(got_tok, want_tok)):
        assert a == b, f"{name}: token-level call {i} is\n  {json.dumps(describe[a])}\nthe golden step makes {b}"
    assert len(got_tok) == len(want_tok)
    # (c) live bytes of op results at every token-level call
    assert len(got["live"]) == len(want["live"])
    for i, (a, b) in enumerate(zip(got["live"], want["live"])):
        assert a <= b, f"{name}: {a} bytes of op results alive at token-level call {i} ({json.dumps(describe[got_tok[i]])}), golden {b}"
    assert max(got["live"]) <= max(want["live"])


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--write":
        sys.exit("usage: python -m tests.test_engine_trace_cpu --write <path>   (from a worktree of the commit to pin)")
    commit = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    ops_seen, configs = [], {}
    for name in CONFIGS:
        r, again = record(name), record(name)
        assert json.dumps(r, sort_keys=True) == json.dumps(again, sort_keys=True), f"{name}: two runs differ"
        assert not set(r["token_rows"]) & set(r["weight_dims"]), name
        trace = []
        for desc, tok in r["calls"]:
            if desc["op"] not in ops_seen:
                ops_seen.append(desc["op"])
            trace.append(f"{ops_seen.index(desc['op'])}:{_key(desc).split(':')[1]}{'*' if tok else ''}")
        configs[name] = {"token_rows": r["token_rows"], "trace": " ".join(trace), "live": r["live"]}
        print(f"{name}: {len(trace)} calls, {len(r['live'])} at token level, peak {max(r['live'])} live bytes")
    with open(sys.argv[2], "w") as f:
        f.write('{"commit": "%s",\n "ops": %s,\n "configs": {\n' % (commit, json.dumps(ops_seen)))
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in configs.items()))
        f.write("\n }\n}\n")
    print(f"{len(configs)} configurations -> {sys.argv[2]}")
