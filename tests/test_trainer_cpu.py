"""The reference's trainer loop drives the engine.

The loop of `training.train.train_one_epoch` (clipa_torch/training/train.py:158-314), as oracle/trainer_harness.py restates it,
runs on the engine with the torch-CPU stand-in ops: `--precision amp_bf16` with a REAL active autocast context (the CPU
flavour of train.py:160's `get_autocast`, since `torch.cuda.amp.autocast` switches itself off without CUDA),
`--to-float-on-device`, clip_grad_norm_, AdamW groups by name, accum_freq 1 and 2.  Compared with
tests/golden/train_loop_ref.npz = the reference's own trainer driving the reference's own CLIP (fp32).  The restated loop -
also the one tests/test_trainer_gpu.py runs - is held operation for operation to the trace of the reference's own
train_one_epoch driving the engine (tests/golden/train_loop_trace.npz, oracle/make_live_golden.py).
"""
import os

import numpy as np
import pytest
import torch

import clipa_amd
from clipa_amd import engine, loss as loss_mod, model as model_mod, optim as optim_mod
from oracle import clip_oracle as O
from oracle import trainer_harness as H
from oracle.make_golden import CASES

from . import cpu_ops
from .conftest import GOLDEN

Z = np.load(os.path.join(GOLDEN, "train_loop_ref.npz"))
TRACES = np.load(os.path.join(GOLDEN, "train_loop_trace.npz"))


@pytest.fixture(autouse=True)
def _swap_ops(monkeypatch):
    for mod in (engine, loss_mod, model_mod, optim_mod):
        monkeypatch.setattr(mod, "ops", cpu_ops)
    yield
    H.unload()


def _cpu_autocast():
    return torch.autocast("cpu", dtype=torch.bfloat16)


def _engine_and_data(accum, nsteps):
    spec = CASES["cls_erf"]
    cfg, B, S, seed = spec["cfg"], spec["B"], spec["S"], spec["seed"]
    m = clipa_amd.CLIP(**cfg, output_dict=True)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd0 = O.make_state_dict(shapes, seed)
    m.load_state_dict(sd0, strict=True)
    m.visual.image_mean, m.visual.image_std = H.IMAGE_MEAN, H.IMAGE_STD
    tc = cfg["text_cfg"]
    batches = H.synthetic_batches(nsteps * accum, B, S, tc["context_length"], tc["vocab_size"], seed + 100)
    return m, sd0, batches, H.make_args("cpu", batch_size=B, accum_freq=accum)


def _run_loop(accum, nsteps, trace=None):
    """One epoch of the restated train_one_epoch on the engine; with `trace`, under that H.LoopTrace."""
    m, sd0, batches, args = _engine_and_data(accum, nsteps)
    opt = H.make_optimizer(m)
    sched = H.make_scheduler(opt)
    loss = H.LossRecorder(clipa_amd.ClipLoss(local_loss=False, gather_with_grad=False, cache_labels=True, rank=0, world_size=1))
    if trace is None:
        H.restated_train_one_epoch(m, batches, loss, opt, sched, args, _cpu_autocast)
    else:
        traced_loss, traced_sched = trace.attach(m, loss, opt, sched)
        with trace.patched():
            H.restated_train_one_epoch(m, batches, traced_loss, opt, traced_sched, args, _cpu_autocast)
    return m, sd0, loss.values


@pytest.mark.parametrize("tag,accum,nsteps", [("a1", 1, 3), ("a2", 2, 2)])
def test_reference_train_one_epoch_drives_the_engine(tag, accum, nsteps):
    m, sd0, losses = _run_loop(accum, nsteps)
    ref = Z[f"{tag}_losses"]
    assert len(losses) == len(ref)
    for a, b in zip(losses, ref):
        assert abs(a - b) < 2e-2 * b, (losses, ref)
    sd1 = m.state_dict()
    assert abs(float(sd1["logit_scale"]) - float(Z[f"{tag}_w::logit_scale"])) < 2e-3
    names = [str(n) for n in Z[f"{tag}_names"]]
    for n, dn in zip(names, Z[f"{tag}_delta_norms"]):
        d = float((sd1[n].double() - sd0[n].double()).norm())
        assert abs(d - dn) <= 0.25 * dn + 1e-6, (n, d, dn)                      # same update size (Adam: ~lr per element)
    for k in Z["keep"]:
        k = str(k)
        if k == "logit_scale" or f"{tag}_w::{k}" not in Z:
            continue
        da = (sd1[k].double() - sd0[k].double()).reshape(-1)
        db = (torch.from_numpy(Z[f"{tag}_w::{k}"]).double() - sd0[k].double()).reshape(-1)
        cos = float(torch.dot(da, db) / (da.norm() * db.norm()))
        assert cos > 0.98, (k, cos)         # the update DIRECTION (Adam's first steps are ~ lr * sign(g): bf16 flips small entries)


@pytest.mark.parametrize("accum,nsteps", [(1, 2), (2, 1)])
def test_restated_loop_equals_reference_loop(accum, nsteps):
    """The loop tests/test_trainer_gpu.py runs on the GPU box is the reference's, operation for operation: model.train,
    scheduler, zero_grad, forward (on the same normalised images and tokens), loss, backward, clip_grad_norm_, step and clamp
    in the same order under the same grad / autocast state as the reference's train_one_epoch driving the engine."""
    trace = H.LoopTrace()
    _run_loop(accum, nsteps, trace)
    assert trace.events == [str(e) for e in TRACES[f"trace_a{accum}_n{nsteps}"]]
