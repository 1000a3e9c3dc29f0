"""TEST INFRASTRUCTURE shared by tests/test_layerscale_gpu.py (the kernels and the engine on the device) and
tests/test_layerscale_cpu.py (the torch stand-ins of tests/layerscale_cpu_ops.py): one case table for the two LayerScale ops
and the helpers of the model tests (fixtures with their stored gammas, the oracle reference with the scale folded in).

Kernel cases.  layerscale_unfold is a row reduction, so its inputs are chosen such that every product and every partial sum
is exact in fp32 and ANY summation order gives the same bits: dW' and db' are integers in [-8, 8], W, gamma and b signed powers
of two (2^-3 .. 2^3), K <= 4096 - a partial sum is a multiple of 2^-3 below 4096 * 8 * 8 = 2^18, 21 significant bits.  The
comparison is torch.equal.  layerscale_fold is one fp32 product and one rounding per element: random operands, compared
exactly against (gamma.float()[:, None] * W.float()).bfloat16().
Shapes (N, K): (64, 64) plain; (3, 8) fewer rows than the four waves of a workgroup; (130, 200) a row tail (130 = 32 * 4 + 2) and
a column count that is not a multiple of the 512 elements a wave takes per pass; (128, 2048) four passes of a wave over a row;
(64, 72) one vector chunk past a pass of eight lanes; (5, 77) K % 8 != 0: rows that are not 16-byte aligned take the scalar
path; `misaligned`: K % 8 == 0 but every base pointer is off the 16-byte grid (the scalar path again)."""
import numpy as np
import torch

from oracle import clip_oracle as O

from .conftest import load_golden

bf16, f32 = torch.bfloat16, torch.float32
SHAPES = [(64, 64), (3, 8), (130, 200), (128, 2048), (64, 72), (5, 77)]
ALL = (True, True, True)


def names(cases):
    return [c["name"] for c in cases]


def _dt(d):
    return "bf16" if d == bf16 else "f32"


def _case(N, K, w, dw=f32, want=ALL, misaligned=False):
    tag = f"{N}x{K}-w_{_dt(w)}-dw_{_dt(dw)}"
    if want != ALL:
        tag += "-want_" + "".join("wbg"[i] for i in range(3) if want[i]) + ("none" if not any(want) else "")
    tag += "-misaligned" if misaligned else ""
    return dict(name=tag, N=N, K=K, w=w, dw=dw, want=want, misaligned=misaligned)


UNFOLD = [_case(N, K, w, dw) for N, K in SHAPES for w in (bf16, f32) for dw in (bf16, f32)]
UNFOLD += [_case(130, 200, bf16, bf16, want=wt) for wt in ((False, True, True), (True, False, True), (True, True, False),
                                                           (False, False, True), (True, False, False), (False, False, False))]
UNFOLD += [_case(16, 64, bf16, bf16, misaligned=True), _case(16, 64, f32, f32, misaligned=True)]
FOLD = [_case(N, K, w) for N, K in SHAPES for w in (bf16, f32)]
FOLD += [_case(16, 64, bf16, misaligned=True), _case(16, 64, f32, misaligned=True)]


def _place(t, dev, misaligned):
    """t on `dev`; misaligned: as a contiguous view one element into a larger buffer (base address off the 16-byte grid)."""
    t = t.to(dev)
    if not misaligned:
        return t
    buf = torch.empty(t.numel() + 1, device=dev, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def _pow2(rng, shape, emax):
    return np.ldexp(np.where(rng.randint(0, 2, size=shape) == 1, 1.0, -1.0), rng.randint(-emax, emax + 1, size=shape))


def check_unfold(ops, dev, c):
    N, K = c["N"], c["K"]
    rng = np.random.RandomState(1000 + 7 * N + K)
    dwf = rng.randint(-8, 9, size=(N, K)).astype(np.float64)
    w, gamma, b = _pow2(rng, (N, K), 3), _pow2(rng, (N,), 2), _pow2(rng, (N,), 3)
    dbf = rng.randint(-8, 9, size=(N,)).astype(np.float64)
    ref_dw = torch.from_numpy(gamma[:, None] * dwf).to(c["dw"])
    ref_db = torch.from_numpy(gamma * dbf).to(f32)
    ref_dg = torch.from_numpy((dwf * w).sum(1) + dbf * b).to(f32)
    T = lambda a, dt=f32: _place(torch.from_numpy(a).to(dt), dev, c["misaligned"])
    wt = T(w, c["w"])
    assert torch.equal(wt.double().cpu(), torch.from_numpy(w))                  # the operands are exact in their storage types
    dw, db, dg = ops.layerscale_unfold(T(dwf), wt, T(gamma), T(dbf), T(b), out_dtype=c["dw"], want=c["want"])
    want_w, want_b, want_g = c["want"]
    for got, ref, wanted, what in ((dw, ref_dw, want_w, "dw"), (db, ref_db, want_b, "db"), (dg, ref_dg, want_g, "dgamma")):
        if not wanted:
            assert got is None, what
            continue
        assert got.dtype == ref.dtype and got.shape == ref.shape, what
        assert torch.equal(got.cpu(), ref), (c["name"], what, float((got.cpu().double() - ref.double()).abs().max()))


def check_fold(ops, dev, c):
    N, K = c["N"], c["K"]
    gen = torch.Generator().manual_seed(2000 + 7 * N + K)
    w = torch.randn(N, K, generator=gen).to(c["w"])
    gamma = torch.randn(N, generator=gen) * 1.5
    b = torch.randn(N, generator=gen)
    wf, bfold = ops.layerscale_fold(_place(w, dev, c["misaligned"]), _place(gamma, dev, c["misaligned"]),
                                    _place(b, dev, c["misaligned"]))
    assert wf.dtype == bf16 and wf.shape == (N, K)
    assert torch.equal(wf.cpu(), (gamma.float()[:, None] * w.float()).bfloat16()), c["name"]
    assert bfold.dtype == f32 and torch.equal(bfold.cpu(), gamma * b), c["name"]


def check_argument_checks(ops, dev):
    """The wrappers' own checks (they run before any launch)."""
    import pytest
    w, g, b = torch.zeros(4, 8, device=dev), torch.ones(4, device=dev), torch.ones(4, device=dev)
    with pytest.raises(RuntimeError, match="gamma has 3 entries"):
        ops.layerscale_fold(w, g[:3], b)
    with pytest.raises(RuntimeError, match="b has 5 entries"):
        ops.layerscale_fold(w, g, torch.ones(5, device=dev))
    with pytest.raises(RuntimeError, match="w must be"):
        ops.layerscale_fold(w.half(), g, b)
    with pytest.raises(RuntimeError, match="dbf has 3 entries"):
        ops.layerscale_unfold(w, w, g, g[:3], b)
    with pytest.raises(RuntimeError, match="dwf"):
        ops.layerscale_unfold(w[:, :4], w, g, g, b)
    with pytest.raises(RuntimeError, match="out_dtype"):
        ops.layerscale_unfold(w, w, g, g, b, out_dtype=torch.float16)


# ---- model fixtures ---------------------------------------------------------------------------------------------------------
MODEL_CASES = ["layerscale_cls_erf", "layerscale_gap_sincos_tanh"]
_LS = {"ls_1.gamma": ("attn.out_proj.weight", "attn.out_proj.bias"), "ls_2.gamma": ("mlp.c_proj.weight", "mlp.c_proj.bias")}


def load(name):
    """The fixture with the gammas the reference ran with (tools/make_layerscale_golden.py stores them) in its state dict."""
    g = load_golden(name)
    g.gammas = {str(k): g.t(f"gamma_{i}") for i, k in enumerate(g.z["gamma_names"])}
    assert g.gammas and all(k in g.sd and g.sd[k].shape == v.shape for k, v in g.gammas.items())
    g.sd.update({k: v.clone() for k, v in g.gammas.items()})
    return g


def fold_state(sd):
    """A state dict with LayerScale -> the one of the same network without it: W' = diag(gamma) W, b' = gamma * b, as torch
    expressions (autograd carries a gradient of the result back to W, b and gamma)."""
    out = {k: v for k, v in sd.items() if not k.endswith(".gamma")}
    for k, gamma in sd.items():
        if k.endswith(".gamma"):
            for tail, (wn, bn) in _LS.items():
                if k.endswith(tail):
                    pre = k[:-len(tail)]
                    out[pre + wn] = gamma[:, None] * sd[pre + wn]
                    out[pre + bn] = gamma * sd[pre + bn]
    return out


class FoldingOracle:
    """oracle.clip_oracle with LayerScale: the oracle restates the block without it (transformer.py:238-250 at
    ls_init_value=None), so clip_forward runs on fold_state(sd) - x + gamma * (a W^T + b) == x + a (diag(gamma) W)^T + gamma * b.
    Every other name is the oracle's own.  The reference for the fold itself is the REAL reference: the fixtures' features,
    loss and gradient digests."""

    def __getattr__(self, name):
        return getattr(O, name)

    @staticmethod
    def clip_forward(sd, cfg, image, text, emulate_bf16=False, patch_keep=None):
        return O.clip_forward(fold_state(sd), cfg, image, text, emulate_bf16, patch_keep)


def oracle_grads(g, sd=None):
    """fp32 loss and every parameter gradient (the gammas included) of the fixture's step; sd: other weights (bf16-rounded)."""
    leaves = {k: v.clone().requires_grad_(k not in g.frozen) for k, v in (sd or g.sd).items()}
    i, t, s = FoldingOracle.clip_forward(leaves, g.ocfg, O.normalize_images(g.images_u8), g.texts)
    loss, _ = O.clip_loss(i, t, s)
    loss.backward()
    return float(loss), {k: v.grad for k, v in leaves.items() if v.grad is not None}, i.detach(), t.detach()


def dgamma_error(got, ref):
    """Worst relative L2 error of a gamma gradient: max over the gammas of |got - ref| / |ref|."""
    worst = (0.0, None)
    for k, r in ref.items():
        if k.endswith(".gamma"):
            a, b = got[k].double().cpu().reshape(-1), r.double().reshape(-1)
            worst = max(worst, (float((a - b).norm() / b.norm()), k))
    assert worst[1] is not None
    return worst
