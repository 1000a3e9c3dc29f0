"""GPU tests of the SigLIP objective: the fused kernel (`ops.simsig`, csrc/simsig.hip) at every shape that reaches another
code path and at the logit magnitudes where a naive log(1 + exp) overflows, `SigLipLoss` at one rank and at two ranks sharing
the GPU over gloo, and a model built with `logit_bias`.  Reference for every comparison: the fp64 torch restatement
-F.logsigmoid(labels * (s * I @ T.T + b)).sum() / B with autograd, computed on the CPU from the SAME bf16-rounded operands
the kernel receives.  Inputs come from a seeded CPU generator."""
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

import clipa_amd
from clipa_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
bf16, f64 = torch.bfloat16, torch.float64

# the project's own bounds for the same GEMM + fp32 epilogue + bf16 store (test_fused_similarity_cross_entropy)
LOSS_TOL = dict(rtol=1e-4, atol=2e-4)
DL_TOL = dict(rtol=2.0 ** -7, atol=1e-6)
SCALAR_TOL = dict(rtol=2e-3, atol=2e-5)


def _unit(n, e, gen):
    return F.normalize(torch.randn(n, e, generator=gen), dim=-1)


def _labels(R, N, label0):
    y = -torch.ones(R, N, dtype=f64)
    y[torch.arange(R), torch.arange(R) + label0] = 1.0
    return y


def _reference(rows_b, cols_b, N, label0, gscale, s, b):
    """fp64 from the bf16 operands: loss_rows, d (gscale * loss) / d raw, and its per-row d / d s and d / d b."""
    R = rows_b.shape[0]
    raw = (rows_b.double() @ cols_b[:N].double().T).requires_grad_(True)
    sv = torch.full((R, 1), s, dtype=f64, requires_grad=True)          # one copy per row: per-row scalar gradients
    bv = torch.full((R, 1), b, dtype=f64, requires_grad=True)
    loss_rows = -F.logsigmoid(_labels(R, N, label0) * (sv * raw + bv)).sum(1)
    draw, ds, db = torch.autograd.grad(gscale * loss_rows.sum(), (raw, sv, bv))
    return loss_rows.detach(), draw, ds.reshape(-1), db.reshape(-1)


def _check_simsig(rows, cols, N, label0, s, b):
    R = rows.shape[0]
    gscale = 1.0 / R
    rows_b, cols_b = rows.to(bf16), cols.to(bf16)
    sd, bd = torch.tensor([s], device=DEV), torch.tensor([b], device=DEV)
    loss_rows, dl, dsr, dbr = ops.simsig(rows_b.to(DEV), cols_b.to(DEV), N, label0, gscale, sd, bd)
    fwd_only = ops.simsig(rows_b.to(DEV), cols_b.to(DEV), N, label0, gscale, sd, bd, want_grad=False)
    torch.cuda.synchronize()
    n8 = (N + 7) // 8 * 8
    assert dl.shape == (R, n8) and dl.dtype == bf16
    for t in (loss_rows, dl, dsr, dbr):
        assert bool(torch.isfinite(t.float()).all())
    ref_loss, ref_draw, ref_ds, ref_db = _reference(rows_b, cols_b, N, label0, gscale, s, b)
    torch.testing.assert_close(loss_rows.cpu().double(), ref_loss, **LOSS_TOL)
    torch.testing.assert_close(dl[:, :N].cpu().double(), ref_draw, **DL_TOL)
    assert not bool(dl[:, N:].float().any()), "pad columns of dl must be exactly zero"
    torch.testing.assert_close(dsr.cpu().double(), ref_ds, **SCALAR_TOL)
    torch.testing.assert_close(dbr.cpu().double(), ref_db, **SCALAR_TOL)
    assert fwd_only[1] is None and fwd_only[2] is None and fwd_only[3] is None
    assert torch.equal(fwd_only[0], loss_rows), "the forward-only variant must return bit-identical loss rows"


@pytest.mark.parametrize("R,N,E,label0,s,b", [
    (8, 8, 64, 0, 10.0, -10.0),             # one partial tile
    (4, 4, 32, 0, 10.0, -10.0),             # K below one BK step
    (16, 61, 72, 45, 10.0, -10.0),          # N no multiple of 8 (pad columns), K tail, label0 + R == N
    (300, 517, 136, 100, 10.0, -10.0),      # 2 tile rows x 3 tile columns, ragged edges, the diagonal crosses both tile borders
    (512, 512, 512, 0, 14.3, -3.0),         # whole tiles only
])
def test_simsig_kernel_matches_fp64(R, N, E, label0, s, b):
    gen = torch.Generator().manual_seed(100 + R + N + E)
    rows = _unit(R, E, gen)
    cols = _unit((N + 7) // 8 * 8, E, gen)            # the rows past N hold data: the kernel must not read them into the loss
    with torch.no_grad():
        # correlate the matched pairs, so that positives and negatives sit at different logits
        cols[label0:label0 + R] = F.normalize(cols[label0:label0 + R] + rows, dim=-1)
    _check_simsig(rows, cols, N, label0, s, b)


def test_simsig_is_stable_at_large_logits():
    """s = 100, b = -10: a positive at l = -110 (its row is the exact negative of its label column) and a negative at
    l = +90 (the row copies a non-label column) - softplus of 110 and 90, where log(1 + exp(.)) overflows fp32."""
    R = N = 16
    gen = torch.Generator().manual_seed(7)
    cols = _unit(N, 64, gen).to(bf16).float()
    rows = _unit(R, 64, gen)
    rows[0:4] = -cols[0:4]                              # positives at l = -100 |c|^2 - 10
    rows[4:8] = cols[9:13]                              # negatives (label columns are 4..7) at l = +100 |c|^2 - 10
    _check_simsig(rows, cols, N, 0, 100.0, -10.0)
    raw = rows.to(bf16).double() @ cols.double().T
    assert float((100 * raw[0, 0] - 10)) < -105 and float(100 * raw[4, 9] - 10) > 85


def _loss_reference(img, txt, s, b, rank=0, world=1):
    """fp64 restatement of every rank's upstream value from the bf16-rounded features; returns the value of `rank` and the
    gradients of the SUM over ranks (the reduce-scatter backward) for the features, of `rank`'s own value for s and b."""
    Bl = img.shape[0] // world
    I = img.to(bf16).double().requires_grad_(True)
    T = txt.to(bf16).double().requires_grad_(True)
    sv = torch.tensor(s, dtype=f64, requires_grad=True)
    bv = torch.tensor(b, dtype=f64, requires_grad=True)
    losses = [-F.logsigmoid(_labels(Bl, world * Bl, r * Bl) * (sv * I[r * Bl:(r + 1) * Bl] @ T.T + bv)).sum() / Bl
              for r in range(world)]
    ds, db = torch.autograd.grad(losses[rank], (sv, bv), retain_graph=True)
    gi, gt = torch.autograd.grad(sum(losses), (I, T))
    return float(losses[rank].detach()), gi[rank * Bl:(rank + 1) * Bl], gt[rank * Bl:(rank + 1) * Bl], float(ds), float(db)


def _assert_loss_and_grads(got, ref, factor=1.0):
    loss, gi, gt, gs, gb = got
    rl, ri, rt, rs, rb = ref
    assert abs(loss - rl) <= 1e-4 * abs(rl) + 2e-4, (loss, rl)
    # feature gradients: a GEMM over the bf16 dl (2^-9 relative per element) with fp32 accumulation
    for a, r in ((gi, ri), (gt, rt)):
        r = r * factor
        assert float((a.double() - r).norm()) <= 2.0 ** -7 * float(r.norm()), float((a.double() - r).norm() / r.norm())
    assert abs(gs - factor * rs) <= 2e-3 * abs(factor * rs) + 2e-5, (gs, factor * rs)
    assert abs(gb - factor * rb) <= 2e-3 * abs(factor * rb) + 2e-5, (gb, factor * rb)


def _run_loss(fn, img, txt, s, b, factor=1.0):
    i = img.detach().clone().to(DEV).requires_grad_(True)
    t = txt.detach().clone().to(DEV).requires_grad_(True)
    sp = torch.nn.Parameter(torch.tensor(s, device=DEV))
    bp = torch.nn.Parameter(torch.tensor(b, device=DEV))
    loss = fn(i, t, sp, bp)
    (factor * loss).backward()
    torch.cuda.synchronize()
    assert sp.grad.shape == () and bp.grad.shape == ()
    return (float(loss.detach()), i.grad.cpu(), t.grad.cpu(), float(sp.grad), float(bp.grad)), (i, t, sp, bp)


def test_sigliploss_single_rank_matches_fp64():
    gen = torch.Generator().manual_seed(11)
    img, txt = _unit(12, 64, gen), _unit(12, 64, gen)
    txt = F.normalize(txt + img, dim=-1)
    fn = clipa_amd.SigLipLoss()
    ref = _loss_reference(img, txt, 10.0, -10.0)
    got, (i, t, sp, bp) = _run_loss(fn, img, txt, 10.0, -10.0)
    _assert_loss_and_grads(got, ref)
    out = fn(i, t, sp, bp, output_dict=True)
    assert set(out) == {"contrastive_loss"} and float(out["contrastive_loss"].detach()) == got[0]
    with torch.no_grad():
        value = fn(i, t, sp, bp)
    assert not value.requires_grad and float(value) == got[0]
    got3, _ = _run_loss(fn, img, txt, 10.0, -10.0, factor=3.0)         # a non-unit upstream gradient scales all four
    assert got3[0] == got[0]
    _assert_loss_and_grads(got3, ref, factor=3.0)


def test_model_with_logit_bias_trains_through_sigliploss():
    from oracle import clip_oracle as O
    torch.manual_seed(0)
    model = clipa_amd.create_model("ViT-S-16", force_image_size=112, init_logit_scale=math.log(10), init_logit_bias=-10.0,
                                   precision="bf16", device="cuda", output_dict=True)
    img, txt = O.synthetic_batch(8, 112, 77, 49408, seed=3)
    out = model(img.to(DEV), txt.to(DEV))
    assert set(out) == {"image_features", "text_features", "logit_scale", "logit_bias"}
    assert out["logit_bias"] is model.logit_bias
    loss = clipa_amd.SigLipLoss()(**out)
    loss.backward()
    torch.cuda.synchronize()
    s = float(model.logit_scale.detach().exp())
    rl, _, _, rs, rb = _loss_reference(out["image_features"].detach().float().cpu(), out["text_features"].detach().float().cpu(),
                                       s, float(model.logit_bias))
    assert abs(float(loss) - rl) <= 1e-4 * abs(rl) + 2e-4
    assert abs(float(model.logit_bias.grad) - rb) <= 2e-3 * abs(rb) + 2e-5, (float(model.logit_bias.grad), rb)
    rs = rs * s                                          # d / d logit_scale = d / d s * exp(logit_scale)
    assert abs(float(model.logit_scale.grad) - rs) <= 2e-3 * abs(rs) + 2e-5, (float(model.logit_scale.grad), rs)
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad.float()).all()), n


# ---- two ranks sharing the one GPU over gloo --------------------------------------------------------------------------
B2, E2 = 6, 64


def _features2():
    gen = torch.Generator().manual_seed(21)
    img, txt = _unit(2 * B2, E2, gen), _unit(2 * B2, E2, gen)
    return img, F.normalize(txt + img, dim=-1)


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    sys.path.insert(0, ROOT)
    import clipa_amd
    img, txt = _features2()
    fn = clipa_amd.SigLipLoss(rank=rank, world_size=world)
    got, _ = _run_loss(fn, img[rank * B2:(rank + 1) * B2], txt[rank * B2:(rank + 1) * B2], 10.0, -10.0)
    q.put((rank, (got[0], got[1].numpy(), got[2].numpy(), got[3], got[4])))      # numpy: pickled by value
    dist.barrier()
    dist.destroy_process_group()


def _get(q, procs, limit=300):
    """Queue read that gives up as soon as a worker has died (a crashed rank must not stall the suite)."""
    import queue
    import time
    t0 = time.time()
    while True:
        try:
            return q.get(timeout=2)
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs) or time.time() - t0 > limit:
                for p in procs:
                    if p.is_alive():
                        p.terminate()
                raise AssertionError("a worker rank died or timed out: " + str([p.exitcode for p in procs]))


def test_sigliploss_two_ranks_hip_kernels_match_fp64():
    """B = 6 per rank: 12 gathered texts, padded to 16 for the GEMMs; rank 1's positives start at column 6."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, 29795, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(_get(q, procs) for _ in range(world))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    img, txt = _features2()
    for rank in range(world):
        loss, gi, gt, gs, gb = got[rank]
        _assert_loss_and_grads((loss, torch.from_numpy(gi), torch.from_numpy(gt), gs, gb),
                               _loss_reference(img, txt, 10.0, -10.0, rank, world))
