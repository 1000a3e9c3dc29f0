"""TEST INFRASTRUCTURE: tests/cpu_ops plus torch-CPU stand-ins for the two attention-pooling ops (clipa_amd.ops.mappool_fwd /
mappool_bwd; csrc/mappool.hip), same signatures and rounding points: chunks of CHUNK rows with an online softmax, the
probabilities rounded to bf16 relative to the running maximum, the sum taken over the unrounded values; in backward dz, P and dS
rounded to bf16, p = exp(s - max) / sum from the saved statistics, dU as per-workgroup partials (workgroup w owns the samples
w, w + G, ...) summed in index order.  Swapped in for `ops` exactly like tests/layerscale_cpu_ops.py, so the engine's MAP-head
path (the fold, the per-head V projection, the gradient wiring) runs without a GPU.  `mutant=` builds deliberately wrong
variants for tests/test_mappool_cpu.py (the comparison must refuse them).  Never imported by the product."""
import torch

from . import cpu_ops as _base
from .cpu_ops import *  # noqa: F401,F403  (every stand-in of tests/cpu_ops under the same name)
from .cpu_ops import bf16, f32

CHUNK = 32                 # csrc/mappool.hip: MP_CH
DEFAULT_WORKGROUPS = 768   # csrc/mappool.hip: MP_DEFAULT_WG


def gemm_nt(a, b, bias=None, *, out=None, **kw):
    """tests/cpu_ops.gemm_nt that also honours `out=` (a strided view the result is written into), as the kernel does."""
    r = _base.gemm_nt(a, b, bias, **kw)
    if out is None:
        return r
    out.copy_(r)
    return out


def _chk(who, x, u, B, L, H):
    D = x.shape[1]
    if not 1 <= H <= 16 or D % 64 or not 64 <= D <= 2048 or L < 1:
        raise RuntimeError(f"clipa_amd.ops.{who}: unsupported shape H={H}, D={D}, L={L} (1 <= H <= 16, D a multiple of 64 up to "
                           f"2048, L >= 1)")
    if x.dtype != bf16 or u.dtype != bf16 or x.shape[0] != B * L or tuple(u.shape) != (H, D):
        raise RuntimeError(f"clipa_amd.ops.{who}: x {tuple(x.shape)} / u {tuple(u.shape)} do not match B={B}, L={L}, H={H}")
    return D


def _r(t):
    return t.to(bf16).float()


def mappool_fwd(x, u, B, L, H, _max_workgroups=0, mutant=None):
    D = _chk("mappool_fwd", x, u, B, L, H)
    xf, uf = x.float().reshape(B, L, D), u.float()
    if mutant == "neighbour_head":
        uf = uf.roll(1, 0)
    m = torch.full((B, H), -3.0e38)
    ssum = torch.zeros(B, H)
    acc = torch.zeros(B, H, D)
    for l0 in range(0, L, CHUNK):
        xc = xf[:, l0:l0 + CHUNK]
        s = xc @ uf.T                                                   # [B, c, H]
        if mutant == "drop_last_row" and xc.shape[1] == CHUNK:
            s[:, CHUNK - 1] = -3.0e38
        mnew = torch.maximum(m, s.amax(1))
        scale = torch.exp(m - mnew)
        e = torch.exp(s - mnew[:, None])
        if mutant == "no_rescale":
            scale = torch.ones_like(scale)
        ssum = ssum * scale + e.sum(1)
        acc = acc * scale[..., None] + torch.einsum("blh,bld->bhd", _r(e), xc)
        m = mnew
    return acc / ssum[..., None], torch.stack([m, ssum], dim=-1)


def mappool_bwd(x, u, z, stats, dz, B, L, H, _max_workgroups=0, mutant=None):
    D = _chk("mappool_bwd", x, u, B, L, H)
    xf, uf, dzb = x.float().reshape(B, L, D), u.float(), _r(dz)
    delta = (z * dz).sum(-1)                                            # [B, H]
    if mutant == "no_delta":
        delta = torch.zeros_like(delta)
    s = xf @ uf.T
    dp = torch.einsum("bld,bhd->blh", xf, dzb)
    p = torch.exp(s - stats[:, None, :, 0]) * (1.0 / stats[:, None, :, 1])
    pb, dsb = _r(p), _r(p * (dp - delta[:, None]))
    hx = H - 1 if mutant == "heads_minus_one" else H
    dx = (torch.einsum("blh,bhd->bld", pb[..., :hx], dzb[:, :hx]) + torch.einsum("blh,hd->bld", dsb[..., :hx], uf[:hx])).to(bf16)
    G = min(B, _max_workgroups if _max_workgroups > 0 else DEFAULT_WORKGROUPS)
    du = torch.zeros(H, D)
    for w in range(G):
        part = torch.zeros(H, D)
        for k, b in enumerate(range(w, B, G)):
            if mutant == "skip_second_sample" and k == 1:
                continue
            part = part + torch.einsum("lh,ld->hd", dsb[b], xf[b])
        du = du + part
    return dx.reshape(B * L, D), du


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
