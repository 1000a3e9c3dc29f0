"""CPU tests of the SigLIP surface: create_loss's `siglip` branch, the optional `logit_bias` / `init_logit_scale` of CLIP, the
C-ABI declarations of the fused kernel, the no-host-fallback rule, and - under 2- and 3-rank gloo groups - the multi-rank glue
of SigLipLoss (bf16 text all-gather, label offset B * rank, pad to 8, the reduce-scatter backward) against a fp64 restatement
of upstream's value.  The HIP kernels cannot run here, so - in the worker processes only - `clipa_amd.loss.ops` is replaced
by torch-CPU stand-ins; the product never takes that route."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

import clipa_amd
from clipa_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, E = 5, 16                    # W * B (10, 15) is no multiple of 8: the pad path runs
S, BIAS = 10.0, -10.0


class _Args:
    local_loss, gather_with_grad, rank, world_size, horovod, distill, model = True, False, 2, 4, False, False, "ViT-B-16"
    siglip = True


def test_create_loss_siglip_returns_siglip_loss_with_reference_arguments():
    loss = clipa_amd.create_loss(_Args)
    assert type(loss) is clipa_amd.SigLipLoss
    assert (loss.rank, loss.world_size, loss.use_horovod, loss.cache_labels, loss.bidir) == (2, 4, False, False, True)
    # a model handed to create_loss is not bound: nothing is gathered early
    model = types.SimpleNamespace(_gather_partner=None)
    assert type(clipa_amd.create_loss(_Args, model)) is clipa_amd.SigLipLoss and model._gather_partner is None


def test_create_loss_other_branches_unchanged():
    class Plain(_Args):
        siglip = False
    assert type(clipa_amd.create_loss(Plain)) is clipa_amd.ClipLoss

    class NoAttr:
        local_loss, gather_with_grad, rank, world_size, horovod, distill, model = True, True, 3, 8, False, False, "ViT-L-16"
    assert type(clipa_amd.create_loss(NoAttr)) is clipa_amd.ClipLoss

    class Distill(_Args):
        distill = True
    assert type(clipa_amd.create_loss(Distill)) is clipa_amd.DistillClipLoss      # distill is decided first, as upstream

    class Coca(_Args):
        model = "coca_ViT-B-32"
    with pytest.raises(NotImplementedError, match="CoCa"):
        clipa_amd.create_loss(Coca)


def test_siglip_loss_constructor_contract():
    with pytest.raises(NotImplementedError, match="horovod"):
        clipa_amd.SigLipLoss(use_horovod=True)
    loss = clipa_amd.SigLipLoss(cache_labels=True, rank=1, world_size=2, bidir=False)
    assert (loss.cache_labels, loss.rank, loss.world_size, loss.bidir, loss.group) == (True, 1, 2, False, None)


def test_default_clip_has_no_logit_bias_and_the_same_state_dict():
    m = clipa_amd.create_model("ViT-S-16", force_image_size=112)
    assert m.logit_bias is None
    keys = set(m.state_dict())
    assert "logit_bias" not in keys and "logit_scale" in keys
    assert "logit_bias" not in dict(m.named_parameters())
    assert abs(float(m.logit_scale.detach()) - math.log(1 / 0.07)) < 1e-6


def test_clip_with_logit_bias():
    plain = set(clipa_amd.create_model("ViT-S-16", force_image_size=112).state_dict())
    m = clipa_amd.create_model("ViT-S-16", force_image_size=112, init_logit_bias=-10, init_logit_scale=math.log(10),
                               precision="bf16")
    assert isinstance(m.logit_bias, torch.nn.Parameter) and m.logit_bias.dim() == 0 and m.logit_scale.dim() == 0
    assert abs(float(m.logit_bias.detach()) + 10.0) < 1e-6 and abs(float(m.logit_scale.detach()) - math.log(10)) < 1e-6
    assert m.logit_bias.dtype == torch.float32 and m.logit_scale.dtype == torch.float32       # convert_weights_to_lp leaves them
    assert set(m.state_dict()) == plain | {"logit_bias"}
    m2, _, _ = clipa_amd.create_model_and_transforms("ViT-S-16", force_image_size=112, init_logit_bias=-3.0)
    assert abs(float(m2.logit_bias.detach()) + 3.0) < 1e-6 and abs(float(m2.logit_scale.detach()) - math.log(1 / 0.07)) < 1e-6


def test_model_config_may_carry_the_siglip_keys():
    cfg = clipa_amd.get_model_config("ViT-S-16")
    cfg["init_logit_bias"], cfg["init_logit_scale"] = -10.0, math.log(10)
    cfg["vision_cfg"]["image_size"] = 112
    m = clipa_amd.CLIP(**cfg)                           # what create_model does with a config that carries the keys
    assert abs(float(m.logit_bias.detach()) + 10.0) < 1e-6 and abs(float(m.logit_scale.detach()) - math.log(10)) < 1e-6


def test_header_declares_the_simsig_entry_points():
    header = open(os.path.join(ROOT, "include", "clipa_hip.h")).read()
    declared = set(re.findall(r"\b(clipa_[a-z0-9_]+)\s*\(", header))
    assert {"clipa_simsig_workspace", "clipa_simsig"} <= declared
    assert {"clipa_simsig_workspace", "clipa_simsig"} <= set(lib.SIGNATURES)
    assert "losses/common.py:25-32" in header
    h = lib.load()
    assert h.clipa_simsig_workspace(300, 517) == 3 * 300 * 3 * 4              # [tilesN][R][3] floats
    args = lambda E=16, lda=16, label0=0, ldd=8: (None, None, 8, 8, E, lda, 16, None, None, label0, 1.0, None, None, ldd,
                                                  None, None, None, 0, None)
    assert h.clipa_simsig(*args(E=12)) < 0 and "multiples of 8" in lib.last_error()
    assert h.clipa_simsig(*args(lda=12)) < 0 and "multiples of 8" in lib.last_error()
    assert h.clipa_simsig(*args(label0=1)) < 0 and "outside [0, 8)" in lib.last_error()
    assert h.clipa_simsig(None, None, 0, 8, 12, 16, 16, None, None, 0, 1.0, None, None, 8, None, None, None, 0, None) == 0


def test_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="GPU"):
        clipa_amd.SigLipLoss()(torch.randn(8, 16), torch.randn(8, 16), torch.tensor(10.0), torch.tensor(-10.0))
    from clipa_amd import ops
    x = torch.zeros(8, 16, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.simsig(x, x, 8, 0, 1.0, torch.ones(1), torch.zeros(1))


# ---- multi-rank glue under gloo ---------------------------------------------------------------------------------------
def _cpu_ops():
    """Stand-ins with the signatures clipa_amd.loss uses (test infrastructure); simsig is the fp32 torch restatement of the
    kernel's contract."""
    bf16, f32 = torch.bfloat16, torch.float32
    o = types.SimpleNamespace()
    o.to_bf16 = lambda t: t.to(bf16)
    o.transpose_bf16 = lambda t: t.to(bf16).T.contiguous()
    o.gemm_nt = lambda a, b, alpha=1.0, out_f32=True: (a.float() @ b.float().T) * alpha
    o.gemm_tn = lambda p, q, dt=f32: (p.float().T @ q.float()).to(dt)

    def simsig(rows, cols, n_valid, label0, gscale, scale, bias, want_grad=True):
        R = rows.shape[0]
        n8 = (n_valid + 7) // 8 * 8
        s, b = float(scale.reshape(-1)[0]), float(bias.reshape(-1)[0])
        raw = rows.float() @ cols[:n_valid].float().T
        y = -torch.ones(R, n_valid)
        y[torch.arange(R), torch.arange(R) + label0] = 1.0
        t = y * (s * raw + b)
        loss_rows = F.softplus(-t).sum(1)
        if not want_grad:
            return loss_rows, None, None, None
        gg = gscale * (-y) * torch.sigmoid(-t)
        dl = torch.zeros((R, n8), dtype=bf16)
        dl[:, :n_valid] = (gg * s).to(bf16)
        return loss_rows, dl, (gg * raw).sum(1), gg.sum(1)

    def sum_scale(x, scale, out=None, accumulate=False):
        v = x.sum() * scale
        if out is None:
            return v.reshape(())
        out.copy_(out + v if accumulate else v)
        return out

    o.simsig, o.sum_scale = simsig, sum_scale
    return o


def _features(world):
    g = torch.Generator().manual_seed(1234 + world)
    img = F.normalize(torch.randn(world * B, E, generator=g), dim=-1)
    txt = F.normalize(torch.randn(world * B, E, generator=g), dim=-1)
    return img, txt


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    sys.path.insert(0, ROOT)
    import clipa_amd.loss as L
    L.ops = _cpu_ops()
    img, txt = _features(world)
    i = img[rank * B:(rank + 1) * B].clone().requires_grad_(True)
    t = txt[rank * B:(rank + 1) * B].clone().requires_grad_(True)
    s = torch.tensor(S, requires_grad=True)
    b = torch.tensor(BIAS, requires_grad=True)
    fn = L.SigLipLoss(rank=rank, world_size=world)
    loss = fn(i, t, s, b, output_dict=True)["contrastive_loss"]
    with torch.no_grad():
        value_no_grad = float(fn(i, t, s, b))
    loss.backward()
    q.put((rank, (float(loss), value_no_grad, i.grad.numpy(), t.grad.numpy(), float(s.grad), float(b.grad))))
    dist.barrier()
    dist.destroy_process_group()


def _restatement(img, txt, world):
    """fp64, from the bf16-rounded operands the op receives: every rank's upstream value
    -logsigmoid(labels * (s * I @ T.T + b)).sum() / B, and the gradients of the SUM over ranks of those values (what the
    reduce-scatter of the text gradient implements)."""
    I = img.to(torch.bfloat16).double().requires_grad_(True)
    T = txt.to(torch.bfloat16).double().requires_grad_(True)
    s = torch.tensor(S, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(BIAS, dtype=torch.float64, requires_grad=True)
    losses, dsb = [], []
    for r in range(world):
        labels = -torch.ones(B, world * B, dtype=torch.float64)
        labels[torch.arange(B), torch.arange(B) + r * B] = 1.0
        loss = -F.logsigmoid(labels * (s * I[r * B:(r + 1) * B] @ T.T + b)).sum() / B
        losses.append(loss)
        dsb.append(tuple(float(g) for g in torch.autograd.grad(loss, (s, b), retain_graph=True)))   # d_scale, d_bias are rank-local
    gi, gt = torch.autograd.grad(sum(losses), (I, T))
    return [float(l) for l in losses], gi.numpy(), gt.numpy(), dsb


@pytest.mark.parametrize("world,port", [(2, 29791), (3, 29793)])
def test_sigliploss_gloo_ranks_match_restatement(world, port):
    """Tolerances: those of tests/test_dist_cpu.py (bf16 features / bf16 dlogits in the engine's data path)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    img, txt = _features(world)
    losses, gi, gt, dsb = _restatement(img, txt, world)
    for rank in range(world):
        loss, value_no_grad, d_i, d_t, d_s, d_b = got[rank]
        assert abs(loss - losses[rank]) < 2e-2 * abs(losses[rank]), (rank, loss, losses[rank])
        assert value_no_grad == loss
        for a, ref in ((d_i, gi[rank * B:(rank + 1) * B]), (d_t, gt[rank * B:(rank + 1) * B])):
            a, ref = a.reshape(-1).astype(np.float64), ref.reshape(-1)
            cos = float(a @ ref / (np.linalg.norm(a) * np.linalg.norm(ref)))
            assert cos > 0.999, (rank, cos)
            assert abs(np.linalg.norm(a) / np.linalg.norm(ref) - 1) < 2e-2, rank
        for a, ref in ((d_s, dsb[rank][0]), (d_b, dsb[rank][1])):
            assert abs(a - ref) < 3e-2 * abs(ref) + 1e-4, (rank, a, ref)
