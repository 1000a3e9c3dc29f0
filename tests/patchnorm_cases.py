"""TEST INFRASTRUCTURE shared by tests/test_patchnorm_gpu.py (the kernels and the engine on the device) and
tests/test_patchnorm_cpu.py (the torch stand-ins of tests/patchnorm_cpu_ops.py): the case tables of the three dual-PatchNorm ops
(input_patchnorm, open_clip/transformer.py:362-371,483-489) and the helpers of the model tests - the fixtures of
tools/make_patchnorm_golden.py with their stored stem tensors, and PatchNormOracle, oracle.clip_oracle with the PatchNorm stem
restated in torch in front of it.

patchify_ln cases.  P in {8, 14, 16, 32}: K = 192 (24 of a wave's 64 lanes), 588 (no multiple of 8: the last chunk is ragged
against Kp = 592), 768 and 3072 (6 chunks per lane).  Per P an image size that is a multiple of P and one that is not (the
pixels beyond g * P must never be read); B = 2 - 3, g = 2 - 3.  Layouts / dtypes: u8 channels_last (the 8-byte fast path where
3 P and 3 S are multiples of 8: P = 8 / S = 24, P = 16, P = 32; the generic channels_last path at P = 8 / S = 20 and P = 14), u8
NCHW, bf16, f32.  Normalisation: none, the OpenAI mean / std (per-channel: a constant raw patch is NOT constant behind it) and
mean = 0.5 / std = 0.25 for every channel (constant stays constant).  Inputs are position-coded - element (c, ph, pw) of patch n
holds ((c P P + ph P + pw) (3 + 2 n) + 11 n) mod 251, f32 images the un-reduced code plus n / 4 - so an element-order error
moves every value; one patch per case is constant and must come out as exact zeros (none / equal-channel normalisation).

fold / unfold cases.  Inputs whose products and partial sums are exact in fp32 (as tests/glue_cases.py does): W, gamma, beta
signed powers of two, G, s and the fold's beta small integers - any summation order gives the same bits and the comparison is
torch.equal.  N in {128, 130} (130: a row tail of the 4-row / 16-row workgroups), K in {588, 768}, W fp32 and bf16, every
nullable output null in turn.  The pad columns of G hold 99: they must not be read into anything."""
import numpy as np
import torch

from oracle import clip_oracle as O

from . import patchnorm_cpu_ops as S
from .conftest import load_golden

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
OPENAI = ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))
NORMS = {"raw": (None, None), "openai": OPENAI, "eq": ((0.5, 0.5, 0.5), (0.25, 0.25, 0.25))}
# (P, S, B): g = S // P
GEOMETRY = [(8, 24, 3), (8, 20, 2), (14, 42, 2), (14, 33, 3), (16, 48, 2), (16, 40, 3), (32, 64, 2), (32, 72, 3)]
LAYOUTS = ["u8_nhwc", "u8_nchw", "bf16", "f32"]
PATCHIFY = [dict(name=f"P{P}-S{S_}-B{B}-{lay}-{norm}", P=P, S=S_, B=B, layout=lay, norm=norm)
            for P, S_, B in GEOMETRY for lay in LAYOUTS for norm in NORMS]


def names(cases):
    return [c["name"] for c in cases]


def patchify_input(c):
    """-> (image tensor of the case's dtype and memory format, the same values as float64 NCHW, (b, py, px) of the constant
    patch).  Pixels beyond g * P hold 255 / 8192: reading one would show."""
    P, S_, B = c["P"], c["S"], c["B"]
    g = S_ // P
    n = torch.arange(B * g * g).view(B, 1, g, 1, g, 1)
    code = (torch.arange(3).view(1, 3, 1, 1, 1, 1) * P * P + torch.arange(P).view(1, 1, 1, P, 1, 1) * P
            + torch.arange(P).view(1, 1, 1, 1, 1, P)) * (3 + 2 * n) + 11 * n
    u8 = c["layout"].startswith("u8")
    img = torch.full((B, 3, S_, S_), 255.0 if u8 else 8192.0, dtype=f64)
    body = (code % 251).to(f64) if c["layout"] != "f32" else code.to(f64) + n.to(f64) / 4
    img[:, :, :g * P, :g * P] = body.reshape(B, 3, g * P, g * P)
    const = (B - 1, g - 1, 1)
    img[const[0], :, const[1] * P:(const[1] + 1) * P, const[2] * P:(const[2] + 1) * P] = 77.0
    t = img.to({"u8_nhwc": torch.uint8, "u8_nchw": torch.uint8, "bf16": bf16, "f32": f32}[c["layout"]])
    assert torch.equal(t.to(f64), img)                      # the values are exact in the case's storage type
    if c["layout"] == "u8_nhwc":
        t = t.contiguous(memory_format=torch.channels_last)
    return t, img, const


def patchify_reference(c, img64, eps=1e-5):
    """-> (float64 xhat [rows, K], the error of the fp32 stand-in of the same statistics against it: max |stand-in - ref|)."""
    mean, std = NORMS[c["norm"]]
    ref = S.xhat(S.patches_f32(img64, c["P"], mean, std), eps)
    standin = S.xhat(S.patches_f32(img64.to(f32), c["P"], mean, std), eps)
    return ref, float((standin.to(f64) - ref).abs().max())


def check_patchify_ln(ops, dev, c, kappa):
    """|got - ref| <= 2^-7 |ref| + kappa elementwise (bf16 rounds to 2^-9 relative; kappa: the caller's absolute term), pad
    columns zero, the constant patch exact zeros where the normalisation keeps it constant."""
    P, K = c["P"], 3 * c["P"] ** 2
    Kp = (K + 7) // 8 * 8
    t, img64, (cb, cy, cx) = patchify_input(c)
    ref, _ = patchify_reference(c, img64)
    mean, std = NORMS[c["norm"]]
    got = ops.patchify_ln(t.to(dev), P, Kp, mean, std)
    assert got.dtype == bf16 and tuple(got.shape) == (ref.shape[0], Kp)
    got = got.cpu().to(f64)
    assert torch.isfinite(got).all()
    assert torch.equal(got[:, K:], torch.zeros_like(got[:, K:])), "pad columns"
    err = (got[:, :K] - ref).abs()
    bound = 2.0 ** -7 * ref.abs() + kappa
    assert (err <= bound).all(), (c["name"], float((err - bound).max()), float(err.max()))
    g = c["S"] // P
    row = (cb * g + cy) * g + cx
    if c["norm"] != "openai":
        assert torch.equal(got[row], torch.zeros_like(got[row])), "constant patch"
        assert float(ref[row].abs().max()) == 0.0
    else:
        assert float(ref[row].abs().max()) > 0.1
    return float(err.max())


def _pow2(rng, shape, emax):
    return np.ldexp(np.where(rng.randint(0, 2, size=shape) == 1, 1.0, -1.0), rng.randint(-emax, emax + 1, size=shape))


ALL = (True, True, True)
_FU = [(N, P, w) for N in (128, 130) for P in (14, 16) for w in (f32, bf16)]
FOLD = [dict(name=f"N{N}-K{3 * P * P}-w_{'f32' if w == f32 else 'bf16'}", N=N, P=P, w=w) for N, P, w in _FU]
UNFOLD = [dict(FOLD[i], want=ALL) for i in range(len(FOLD))]
UNFOLD += [dict(name=f"N130-K588-w_bf16-want_{''.join('wgb'[i] for i in range(3) if wt[i]) or 'none'}", N=130, P=14, w=bf16, want=wt)
           for wt in ((False, True, True), (True, False, True), (True, True, False), (True, False, False), (False, False, False))]


def _perm(P):
    return S._perm(P).numpy()


def check_fold(ops, dev, c):
    N, P, K = c["N"], c["P"], 3 * c["P"] ** 2
    Kp = (K + 7) // 8 * 8
    rng = np.random.RandomState(3000 + 7 * N + K)
    w, gamma = _pow2(rng, (N, K), 3), _pow2(rng, (K,), 2)
    beta, b = rng.randint(-8, 9, size=(K,)).astype(np.float64), _pow2(rng, (N,), 3)
    T = lambda a, dt=f32: torch.from_numpy(a).to(dt).to(dev)
    wf, bfold = ops.patchnorm_fold(T(w, c["w"]), T(b), T(gamma), T(beta), P, Kp)
    ref_w = np.zeros((N, Kp))
    ref_w[:, :K] = (w * gamma)[:, _perm(P)]
    assert wf.dtype == bf16 and tuple(wf.shape) == (N, Kp) and bfold.dtype == f32 and tuple(bfold.shape) == (N,)
    assert torch.equal(wf.cpu(), torch.from_numpy(ref_w).to(bf16)), c["name"]
    assert torch.equal(wf.cpu().double(), torch.from_numpy(ref_w))                      # (the reference itself is exact in bf16)
    assert torch.equal(bfold.cpu().double(), torch.from_numpy(b + w @ beta)), c["name"]


def unfold_inputs(c, dev):
    N, P, K = c["N"], c["P"], 3 * c["P"] ** 2
    Kp = (K + 7) // 8 * 8
    rng = np.random.RandomState(4000 + 7 * N + K)
    g = np.full((N, Kp), 99.0)
    g[:, :K] = rng.randint(-8, 9, size=(N, K))
    s = rng.randint(-8, 9, size=(N,)).astype(np.float64)
    w, gamma, beta = _pow2(rng, (N, K), 3), _pow2(rng, (K,), 2), _pow2(rng, (K,), 2)
    T = lambda a, dt=f32: torch.from_numpy(a).to(dt).to(dev)
    return (g, s, w, gamma, beta), (T(g), T(s), T(w, c["w"]), T(gamma), T(beta))


def check_unfold(ops, dev, c):
    P, K = c["P"], 3 * c["P"] ** 2
    (g, s, w, gamma, beta), dev_in = unfold_inputs(c, dev)
    inv = np.empty(K, dtype=np.int64)
    inv[_perm(P)] = np.arange(K)
    gk = g[:, :K][:, inv]
    refs = (torch.from_numpy(gamma * gk + beta * s[:, None]).to(c["w"]), torch.from_numpy((w * gk).sum(0)).to(f32),
            torch.from_numpy((w * s[:, None]).sum(0)).to(f32))
    got = ops.patchnorm_unfold(*dev_in, P, out_dtype=c["w"], want=c["want"])
    for out, ref, wanted, what in zip(got, refs, c["want"], ("dw", "dgamma", "dbeta")):
        if not wanted:
            assert out is None, what
            continue
        assert out.dtype == ref.dtype and out.shape == ref.shape, what
        assert torch.equal(out.cpu(), ref), (c["name"], what, float((out.cpu().double() - ref.double()).abs().max()))


def check_argument_checks(ops, dev):
    """The wrappers' own checks (they run before any launch)."""
    import pytest
    K = 192
    w, b = torch.zeros(4, K, device=dev), torch.zeros(4, device=dev)
    ga, be = torch.ones(K, device=dev), torch.zeros(K, device=dev)
    img = torch.zeros(1, 3, 16, 16, device=dev)
    with pytest.raises(RuntimeError, match="bad geometry"):
        ops.patchify_ln(img, 8, 196)                       # Kp % 8 != 0
    with pytest.raises(RuntimeError, match="bad geometry"):
        ops.patchify_ln(img, 8, 184)                       # Kp < 3 P P
    with pytest.raises(RuntimeError, match="bad geometry"):
        ops.patchify_ln(torch.zeros(1, 3, 40, 40, device=dev), 40, 4800)      # beyond the 3072 elements a wave holds
    with pytest.raises(RuntimeError, match=r"expected \[B,3,S,S\]"):
        ops.patchify_ln(img[:, :2], 8, 192)
    with pytest.raises(RuntimeError, match="unsupported image dtype"):
        ops.patchify_ln(img.to(torch.int16), 8, 192)
    with pytest.raises(RuntimeError, match="below the patch size"):
        ops.patchify_ln(img, 32, 3072)
    with pytest.raises(RuntimeError, match="bad geometry"):
        ops.patchnorm_fold(w, b, ga, be, 8, 196)
    with pytest.raises(RuntimeError, match="w has 192 columns"):
        ops.patchnorm_fold(w, b, ga, be, 16, 768)
    with pytest.raises(RuntimeError, match="gamma has 191 entries"):
        ops.patchnorm_fold(w, b, ga[:191], be, 8, 192)
    with pytest.raises(RuntimeError, match="b has 3 entries"):
        ops.patchnorm_fold(w, b[:3], ga, be, 8, 192)
    with pytest.raises(RuntimeError, match="w must be"):
        ops.patchnorm_fold(w.half(), b, ga, be, 8, 192)
    with pytest.raises(RuntimeError, match="s has 3 entries"):
        ops.patchnorm_unfold(w, b[:3], w, ga, be, 8)
    with pytest.raises(RuntimeError, match="bad geometry"):
        ops.patchnorm_unfold(w[:, :188], b, w, ga, be, 8)
    with pytest.raises(RuntimeError, match="g .* vs w"):
        ops.patchnorm_unfold(w[:3], b, w, ga, be, 8)
    with pytest.raises(RuntimeError, match="out_dtype"):
        ops.patchnorm_unfold(w, b, w, ga, be, 8, out_dtype=torch.float16)


# ---- model fixtures ---------------------------------------------------------------------------------------------------------
MODEL_CASES = ["patchnorm_cls_erf", "patchnorm_p14_gap"]
PN_W, PN_B = "visual.patchnorm_pre_ln.weight", "visual.patchnorm_pre_ln.bias"
CONV_W, CONV_B = "visual.conv1.weight", "visual.conv1.bias"


def load(name):
    """The fixture with the stem tensors the reference ran with (tools/make_patchnorm_golden.py stores them) in its state dict;
    .stem_grads: the reference's full gradients of the stem's parameters."""
    g = load_golden(name)
    g.stem = {str(k): g.t(f"stem_{i}") for i, k in enumerate(g.z["stem_names"])}
    assert sorted(g.stem) == sorted((PN_W, PN_B, CONV_B)) and all(g.sd[k].shape == v.shape for k, v in g.stem.items())
    g.sd.update({k: v.clone() for k, v in g.stem.items()})
    g.stem_grads = {str(k): g.t(f"stem_grad_{i}") for i, k in enumerate(g.z["stem_grad_names"])}
    return g


def stem_as_conv(sd, cfg, image, folded=False):
    """A PatchNorm state dict and a normalised image batch -> (state dict, image) of the SAME network with a plain convolution
    stem, as torch expressions (autograd carries the gradients back to gamma, beta, W and b): the patches are normalised in
    torch and put back in image layout, conv1.weight is the Linear's matrix reshaped to [D,3,P,P] ((c,p1,p2) is the
    convolution's own element order) and the Linear's bias rides on the patch rows of the positional embedding.  folded: the
    engine's split instead - the image holds xhat without the affine, the weight W diag(gamma), the bias b + W beta - so that
    the bf16 emulation of the oracle rounds what the engine rounds."""
    P = cfg["vision"]["patch_size"]
    B, _, S_, _ = image.shape
    g = S_ // P
    K = 3 * P * P
    x = image[:, :, :g * P, :g * P].reshape(B, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, K)
    w, b, gamma, beta = sd[CONV_W].to(x.dtype), sd[CONV_B].to(x.dtype), sd[PN_W].to(x.dtype), sd[PN_B].to(x.dtype)
    if folded:
        h = torch.nn.functional.layer_norm(x, (K,), None, None, 1e-5)
        w, b = w * gamma, b + w @ beta
    else:
        h = torch.nn.functional.layer_norm(x, (K,), gamma, beta, 1e-5)
    out = {k: v for k, v in sd.items() if k not in (PN_W, PN_B, CONV_W, CONV_B)}
    out[CONV_W] = w.reshape(-1, 3, P, P)
    pos = sd["visual.positional_embedding"]
    out["visual.positional_embedding"] = torch.cat([pos[:1], pos[1:] + b.to(pos.dtype)])
    return out, h.reshape(B, g, g, 3, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, g * P, g * P)


class PatchNormOracle:
    """oracle.clip_oracle with dual PatchNorm: clip_forward runs on stem_as_conv(sd, image).  Every other name is the oracle's
    own.  The reference for the restatement itself is the REAL reference: the fixtures' features, loss, gradient digests and
    full stem gradients (tests/test_patchnorm_cpu.py)."""

    def __getattr__(self, name):
        return getattr(O, name)

    @staticmethod
    def clip_forward(sd, cfg, image, text, emulate_bf16=False, patch_keep=None):
        sd2, image2 = stem_as_conv(sd, cfg, image, folded=emulate_bf16)
        return O.clip_forward(sd2, cfg, image2, text, emulate_bf16, patch_keep)


def oracle_grads(g, sd=None, patch_keep=None):
    """fp32 loss and every parameter gradient of the fixture's step; sd: other weights (bf16-rounded)."""
    leaves = {k: v.clone().requires_grad_(k not in g.frozen) for k, v in (sd or g.sd).items()}
    i, t, s = PatchNormOracle.clip_forward(leaves, g.ocfg, O.normalize_images(g.images_u8), g.texts, patch_keep=patch_keep)
    loss, _ = O.clip_loss(i, t, s)
    loss.backward()
    return float(loss), {k: v.grad for k, v in leaves.items() if v.grad is not None}, i.detach(), t.detach()


def affine_grad_error(got, ref):
    """Relative L2 errors |got - ref| / |ref| of the gradients of patchnorm_pre_ln.weight and .bias -> (dgamma, dbeta)."""
    rel = lambda k: float((got[k].double().cpu().reshape(-1) - ref[k].double().reshape(-1)).norm() / ref[k].double().norm())
    return rel(PN_W), rel(PN_B)
