"""tests/cpu_ops plus torch / numpy stand-ins of the fine-tuning kernels (csrc/mixcut.hip, csrc/softce.hip), swapped in for
clipa_amd.ops the way tests/patchnorm_cpu_ops.py is, so that clipa_amd.finetune - the head Function, the loss Function, the
evaluator - runs without a GPU.  Never imported by the product."""
import torch

from .cpu_ops import *  # noqa: F401,F403  (every stand-in of tests/cpu_ops under the same name)
from .cpu_ops import bf16, f32
from . import finetune_cases as C

SOFTCE_MAX_CLASSES = 32768


def check_token_ids(wait=False):
    """The stand-ins raise at once; nothing is ever pending."""


def mixcut_u8(img, lam=None, box=None):
    """The kernel's contract in torch float32 ops (an implementation of its own, not tests/finetune_cases.mixcut_reference): in
    place on a dense NCHW / channels_last uint8 batch; a pair with a bad descriptor is left alone and the call raises."""
    if (lam is None) == (box is None):
        raise RuntimeError("mixcut_u8: give lam (mixup) or box (cutmix), not both")
    if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[1] != 3 or img.shape[2] != img.shape[3]:
        raise RuntimeError("mixcut_u8: expected uint8 [B,3,S,S]")
    if not (img.is_contiguous() or img.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError("mixcut_u8: img must be dense")
    B, S = img.shape[0], img.shape[2]
    if lam is not None:
        ok = (lam >= 0) & (lam <= 1)
    else:
        y0, y1, x0, x1 = box.long().unbind(1)
        ok = (y0 >= 0) & (y0 <= y1) & (y1 <= S) & (x0 >= 0) & (x0 <= x1) & (x1 <= S)
    ok = ok & ok.flip(0)
    src = img.clone()
    for b in range(B):
        q = B - 1 - b
        if not bool(ok[b]) or q == b:
            continue
        if lam is not None:
            a, o = src[b].to(f32), src[q].to(f32)
            t = lam[b].to(f32) * (a - o)
            img[b] = ((t + o) + 0.5).to(torch.int32).to(torch.uint8)
        else:
            img[b, :, int(y0[b]):int(y1[b]), int(x0[b]):int(x1[b])] = src[q, :, int(y0[b]):int(y1[b]), int(x0[b]):int(x1[b])]
    if not bool(ok.all()):
        raise RuntimeError(f"clipa_amd.ops.mixcut_u8: {int((~ok).sum())} samples rejected")
    return img


def soft_target_ce(logits, ya, yb=None, lam=None, smoothing=0.0, gscale=None, _max_workgroups=0, _bug=None):
    """tests/finetune_cases.softce_sweeps (numpy float32, the kernel's order) behind the wrapper's contract: logits may be a
    [B, C] view of a wider buffer; -> (loss, lse, bf16 [B, C] view of a zero-padded [B, C8] buffer | None)."""
    if logits.dtype != f32 or logits.dim() != 2:
        raise RuntimeError("soft_target_ce: logits must be f32 [B, C]")
    B, Cn = logits.shape
    if not 2 <= Cn <= SOFTCE_MAX_CLASSES:
        raise RuntimeError(f"soft_target_ce: C = {Cn} classes; the kernel takes 2 to {SOFTCE_MAX_CLASSES}")
    if (yb is None) != (lam is None):
        raise RuntimeError("soft_target_ce: yb and lam come together")
    if not 0.0 <= float(smoothing) <= 1.0:
        raise RuntimeError("soft_target_ce: smoothing outside [0, 1]")
    bad = (ya < 0) | (ya >= Cn)
    if yb is not None:
        bad = bad | (yb < 0) | (yb >= Cn) | ~((lam >= 0) & (lam <= 1))
    if bool(bad.any()):
        raise RuntimeError(f"clipa_amd.ops.soft_target_ce: {int(bad.sum())} rows rejected")
    ld = logits.stride(0) if logits.stride(1) == 1 and logits.stride(0) >= Cn else Cn
    wide = logits.detach().as_strided((B, ld), (ld, 1)) if ld > Cn and _bug in ("pad_lse", "smooth_ld") else logits.detach()
    g = 0.0 if gscale is None else float(gscale)
    loss, lse, dl = C.softce_sweeps(wide.numpy(), Cn, ya.numpy(), None if yb is None else yb.numpy(),
                                    None if lam is None else lam.numpy(), smoothing, g, bug=_bug)
    loss, lse = torch.from_numpy(loss), torch.from_numpy(lse)
    if gscale is None:
        return loss, lse, None
    full = torch.zeros((B, (Cn + 7) // 8 * 8), dtype=bf16)
    full[:, :Cn] = torch.from_numpy(dl).to(bf16)
    return loss, lse, full[:, :Cn]


def zeroshot_ranks(feat, w, labels):
    """ops.zeroshot_ranks in torch fp32: -> int32 (gt, eq, pred)."""
    v = feat.float() @ w.float().T
    B, Cn = v.shape
    lab = labels.long()
    has = (lab >= 0) & (lab < Cn)                      # a value outside [0, C) names no class
    safe = lab.clamp(0, Cn - 1)
    tv = torch.where(has, v.gather(1, safe), torch.full_like(lab, float("-inf"), dtype=f32)).max(1).values
    is_label = torch.zeros(B, Cn, dtype=torch.bool)
    is_label.scatter_(1, safe, has)
    gt = (v > tv[:, None]).sum(1)
    eq = ((v == tv[:, None]) & ~is_label).sum(1)
    gt = torch.where(has.any(1), gt, torch.full_like(gt, Cn))
    return gt.to(torch.int32), eq.to(torch.int32), v.argmax(1).to(torch.int32)


def swap_in():
    """Point the engine, model, optimizer and fine-tuning modules at these stand-ins; -> the function that puts the real ops back."""
    import sys
    from clipa_amd import engine, finetune, model as model_mod, optim as optim_mod, zero_shot, ops as real_ops
    me = sys.modules[__name__]
    mods = (engine, finetune, model_mod, optim_mod, zero_shot)
    for mod in mods:
        mod.ops = me

    def restore():
        for mod in mods:
            mod.ops = real_ops
    return restore
