"""TEST INFRASTRUCTURE: tests/cpu_ops plus torch-CPU stand-ins for the three dual-PatchNorm ops (clipa_amd.ops.patchify_ln /
patchnorm_fold / patchnorm_unfold), same signatures, statistics and rounding points.  Swapped in for `ops` the way
tests/layerscale_cpu_ops.py is, so the PatchNorm stem of the engine (folded operands, the multi-tensor weight cache, the unfold
after the weight-gradient product) runs without a GPU.  Never imported by the product."""
import torch

from .cpu_ops import *  # noqa: F401,F403  (every stand-in of tests/cpu_ops under the same name)
from .cpu_ops import bf16, f32


def patches_f32(img, P, mean=None, std=None):
    """[B,3,S,S] -> f32 [B*g*g, 3*P*P] in the engine's (ph,pw,c) order with the kernel's normalisation arithmetic
    (x * (1/255) - mean) * (1/std) in fp32; float64 images stay float64 (the exact reference of the GPU test)."""
    B, _, S, _ = img.shape
    g = S // P
    dt = torch.float64 if img.dtype == torch.float64 else f32
    x = img.to(dt)
    if mean is not None:
        m = torch.tensor(mean, dtype=dt).view(1, 3, 1, 1)
        if dt == f32:
            x = (x * (1.0 / 255.0) - m) * (1.0 / torch.tensor(std, dtype=f32)).view(1, 3, 1, 1)      # (the scalar becomes f32)
        else:
            x = (x / 255.0 - m) / torch.tensor(std, dtype=dt).view(1, 3, 1, 1)
    return x[:, :, :g * P, :g * P].reshape(B, 3, g, P, g, P).permute(0, 2, 4, 3, 5, 1).reshape(B * g * g, 3 * P * P)


def xhat(pt, eps=1e-5):
    """The kernel's statistics in the dtype of pt [rows, K]: on the row minus its first element, mean first, then the centred
    sum of squares; -> (x - mean) * rstd, not yet rounded."""
    K = pt.shape[1]
    y = pt - pt[:, :1]
    d = y - (y.sum(1, keepdim=True) / K)
    return d * torch.rsqrt((d * d).sum(1, keepdim=True) / K + eps)


def patchify_ln(img, P, Kp, mean=None, std=None, eps=1e-5):
    pt = patches_f32(img, P, mean, std)
    return torch.nn.functional.pad(xhat(pt, eps), (0, Kp - pt.shape[1])).to(bf16)


def _perm(P):
    """perm[j] = the (c,p1,p2) column of the parameters that sits at column j of the engine's (ph,pw,c) order."""
    j = torch.arange(3 * P * P)
    return (j % 3) * (P * P) + j // 3


def patchnorm_fold(w, b, gamma, beta, P, Kp):
    """fp32 product, one rounding to bf16; b' = b + W beta in fp32 (the kernel's arithmetic up to the order of the sum)."""
    wf = (w.float() * gamma.float())[:, _perm(P)]
    return torch.nn.functional.pad(wf, (0, Kp - wf.shape[1])).to(bf16), b.float() + w.float() @ beta.float()


def patchnorm_unfold(g, s, w, gamma, beta, P, out_dtype=f32, want=(True, True, True)):
    want_w, want_g, want_b = (bool(v) for v in want)
    K = 3 * P * P
    inv = torch.empty(K, dtype=torch.int64)
    inv[_perm(P)] = torch.arange(K)
    gk = g.float()[:, :K][:, inv]                                     # g in the parameters' column order
    dw = (gamma.float() * gk + beta.float() * s.float()[:, None]).to(out_dtype) if want_w else None
    dg = (w.float() * gk).sum(0) if want_g else None
    db = (w.float() * s.float()[:, None]).sum(0) if want_b else None
    return dw, dg, db


def swap_in():
    """Point the engine, model, loss and optimizer modules at these stand-ins; -> the function that puts the real ops back."""
    import sys
    from clipa_amd import engine, loss as loss_mod, model as model_mod, optim as optim_mod, zero as zero_mod, ops as real_ops
    me = sys.modules[__name__]
    mods = (engine, loss_mod, model_mod, optim_mod, zero_mod)
    for mod in mods:
        mod.ops = me

    def restore():
        for mod in mods:
            mod.ops = real_ops
    return restore
