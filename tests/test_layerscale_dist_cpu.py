"""The 2-rank gloo paths of tests/test_dist_engine_cpu.py and tests/test_zero_cpu.py with a LayerScale config
(tests/golden/layerscale_cls_erf.npz: gammas in both towers), `ops` swapped for the stand-ins of tests/layerscale_cpu_ops.py in
the worker processes: DistributedDataParallel's hooks fire for the two extra gradients of every block and its averaged
gradient is the global-batch gradient, and ShardedAdamW - which sees nothing but a longer parameter list - ends every rank
with the weights of a global-batch AdamW run, the gammas included."""
import math
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from . import layerscale_cases as C
from . import layerscale_cpu_ops

CASE = "layerscale_cls_erf"
HP = dict(lr=2e-3, betas=(0.9, 0.95), eps=1e-6)


def _model(g):
    import clipa_amd
    m = clipa_amd.CLIP(**g.cfg, output_dict=True)
    m.load_state_dict(g.sd, strict=True)
    m.set_grad_checkpointing(True)
    m.visual.transformer.keep_blocks, m.visual.transformer.medium_blocks = 0, 1      # mixed activation tiers
    return m


def _init(rank, world, port):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    layerscale_cpu_ops.swap_in()
    g = C.load(CASE)
    B = g.images_u8.shape[0] // world
    return g, g.images_u8[rank * B:(rank + 1) * B], g.texts[rank * B:(rank + 1) * B]


def _ddp_worker(rank, world, port, q):
    import clipa_amd
    g, img, txt = _init(rank, world, port)
    m = _model(g)
    ddp = torch.nn.parallel.DistributedDataParallel(m, static_graph=True)
    loss_fn = clipa_amd.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True, rank=rank, world_size=world).bind(ddp)
    losses = []
    for _ in range(3):
        ddp.zero_grad(set_to_none=True)
        loss = loss_fn(**ddp(img, txt), output_dict=True)["contrastive_loss"]
        loss.backward()
        losses.append(float(loss.detach()))
    q.put((rank, losses, {n: p.grad.detach().float().numpy() for n, p in m.named_parameters() if p.grad is not None}))
    dist.barrier()
    dist.destroy_process_group()


def _zero_worker(rank, world, port, q):
    import clipa_amd
    from clipa_amd.zero import ShardedAdamW
    g, img, txt = _init(rank, world, port)
    m = _model(g)
    opt = ShardedAdamW([p for p in m.parameters() if p.requires_grad], weight_decay=0.0, bucket_bytes=64 << 10,
                       clamp=(m.logit_scale, 0.0, math.log(100)), **HP)
    loss_fn = clipa_amd.ClipLoss(local_loss=True, gather_with_grad=True, cache_labels=True, rank=rank, world_size=world).bind(m)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = loss_fn(**m(img, txt), output_dict=True)["contrastive_loss"]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    q.put((rank, losses, {n: p.detach().float().numpy().copy() for n, p in m.named_parameters()}))
    dist.barrier()
    dist.destroy_process_group()


def _spawn(target, world, port):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        item = q.get(timeout=300)
        got[item[0]] = item[1:]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return got


def test_two_rank_ddp_step_equals_global_batch_step():
    import clipa_amd
    got = _spawn(_ddp_worker, 2, 29791)
    restore = layerscale_cpu_ops.swap_in()
    try:
        g = C.load(CASE)
        m = _model(g)
        loss = clipa_amd.ClipLoss()(**m(g.images_u8, g.texts), output_dict=True)["contrastive_loss"]
        loss.backward()
        ref = {n: p.grad.detach().float().numpy() for n, p in m.named_parameters() if p.grad is not None}
    finally:
        restore()
    mean_local = 0.5 * (got[0][0][0] + got[1][0][0])
    assert abs(mean_local - float(loss)) <= 2e-3 * abs(float(loss)), (mean_local, float(loss))
    assert max(abs(got[0][0][0] - l) for l in got[0][0][1:]) < 1e-6
    assert set(got[0][1]) == set(ref) and all(k in ref for k in g.gammas)
    for n, gref in ref.items():
        a, b = got[0][1][n], got[1][1][n]
        assert np.array_equal(a, b), f"ranks disagree on {n} after the all-reduce"
        cos = float((a * gref).sum() / (np.linalg.norm(a) * np.linalg.norm(gref) + 1e-30))
        rel = float(np.linalg.norm(a) / (np.linalg.norm(gref) + 1e-30))
        assert cos >= 0.995 and 0.97 <= rel <= 1.03, (n, cos, rel)


def test_two_rank_sharded_adamw_equals_global_batch_adamw():
    import clipa_amd
    got = _spawn(_zero_worker, 2, 29793)
    restore = layerscale_cpu_ops.swap_in()
    try:
        from clipa_amd.optim import AdamW
        g = C.load(CASE)
        m = _model(g)
        opt = AdamW([p for p in m.parameters() if p.requires_grad], weight_decay=0.0, clamp=(m.logit_scale, 0.0, math.log(100)), **HP)
        ref_losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = clipa_amd.ClipLoss()(**m(g.images_u8, g.texts), output_dict=True)["contrastive_loss"]
            loss.backward()
            opt.step()
            ref_losses.append(float(loss.detach()))
        ref = {n: p.detach().float().numpy() for n, p in m.named_parameters()}
    finally:
        restore()
    for n in ref:
        assert np.array_equal(got[0][1][n], got[1][1][n]), n            # every rank ends with the same weights
    mean_losses = [0.5 * (a + b) for a, b in zip(got[0][0], got[1][0])]
    for a, b in zip(mean_losses, ref_losses):                           # the 2-rank run follows the global-batch run
        assert abs(a - b) < 5e-3 * abs(b) + 1e-3, (mean_losses, ref_losses)
    assert ref_losses[-1] < ref_losses[0] and mean_losses[-1] < mean_losses[0]
    # AdamW normalises the step: a sign flip of a ~0 gradient moves a weight by 2 * lr per step (tests/test_zero_cpu.py's bound)
    for n, r in ref.items():
        assert float(np.abs(got[0][1][n] - r).max()) < 1.5e-2, n
    for n, v in g.gammas.items():                                       # the gammas moved, on every rank alike, as the global run moved them
        assert float(np.abs(ref[n] - v.numpy()).max()) > 1e-3, n
        assert float(np.abs(got[0][1][n] - ref[n]).max()) < 1.5e-2, n
