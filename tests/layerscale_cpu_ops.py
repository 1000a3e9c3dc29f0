"""TEST INFRASTRUCTURE: tests/cpu_ops plus torch-CPU stand-ins for the two LayerScale ops (clipa_amd.ops.layerscale_fold /
layerscale_unfold), same signatures and rounding points.  Swapped in for `ops` the way tests/test_dist_engine_cpu.py swaps
tests/cpu_ops in, so the LayerScale engine path (folded operands, the multi-tensor weight cache, the unfold after the weight
gradients) runs without a GPU.  Never imported by the product."""
import torch

from .cpu_ops import *  # noqa: F401,F403  (every stand-in of tests/cpu_ops under the same name)
from .cpu_ops import bf16, f32


def layerscale_fold(w, gamma, b):
    """fp32 product, one rounding to bf16 (the kernel's arithmetic)."""
    return (gamma.float()[:, None] * w.float()).to(bf16), gamma.float() * b.float()


def layerscale_unfold(dwf, w, gamma, dbf, b, out_dtype=f32, want=(True, True, True)):
    want_w, want_b, want_g = (bool(v) for v in want)
    g = gamma.float()
    dw = (g[:, None] * dwf.float()).to(out_dtype) if want_w else None
    db = g * dbf.float() if want_b else None
    dg = (dwf.float() * w.float()).sum(1) + dbf.float() * b.float() if want_g else None
    return dw, db, dg


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
