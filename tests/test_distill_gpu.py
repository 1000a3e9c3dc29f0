"""GPU tests of knowledge distillation on the engine: the fused kernel pair (csrc/simce_distill.hip) against fp64 maths,
DistillClipLoss against the REAL reference's golden vectors (tests/golden/distill_loss.npz, tools/make_distill_golden.py)
at W = 1 and under a 2-rank group, a student + teacher CLIP pair end to end against a CPU fp32 restatement, and the
contrastive half against ClipLoss."""
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from .loss_cases import DL_RTOL, KAPPA_FLOOR, kappa_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "distill_loss.npz")
DEV = torch.device("cuda", 0)
pytestmark = pytest.mark.gpu


def _feats(n, e, seed, base=None, noise=1.5):
    g = torch.Generator().manual_seed(seed)
    b = torch.randn(n, e, generator=g) if base is None else base
    x = b + noise * torch.randn(n, e, generator=g)
    return (x / x.norm(dim=-1, keepdim=True)).to(torch.bfloat16), b


def _cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float(a @ b / (a.norm() * b.norm()))


def _fp64_direction(As, Bs, At, Bt, N, label0, s, u, gs, gc, gd):
    """fp64 restatement of one direction, computed in row chunks on the device (no [R, N] fp32 logits needed anyway)."""
    R = As.shape[0]
    out = {k: [] for k in ("lse_s", "lse_t", "ce", "dist", "dl", "mag", "ds", "ds_abs")}
    Bs64, Bt64 = Bs[:N].double(), Bt[:N].double()
    for r0 in range(0, R, 512):
        r1 = min(R, r0 + 512)
        raw = As[r0:r1].double() @ Bs64.T
        z = s * raw
        y = u * (At[r0:r1].double() @ Bt64.T)
        ls, lt = torch.logsumexp(z, 1), torch.logsumexp(y, 1)
        ps, pt = torch.exp(z - ls[:, None]), torch.exp(y - lt[:, None])
        lab = torch.arange(r0, r1, device=As.device) + label0
        oh = F.one_hot(lab, N).double()
        gl = gs * (gc * (ps - oh) + gd * (ps - pt))
        out["lse_s"].append(ls)
        out["lse_t"].append(lt)
        out["ce"].append(ls - z.gather(1, lab[:, None])[:, 0])
        out["dist"].append(ls - (pt * z).sum(1))
        out["dl"].append(s * gl)
        out["mag"].append(s * gs * (gc * (ps + oh) + gd * (ps + pt)))     # the terms whose difference dl is (loss_cases.py)
        out["ds"].append((gl * raw).sum(1))
        out["ds_abs"].append((gl * raw).abs().sum(1))        # the scale of the cancelling sum, for its tolerance
    return {k: torch.cat(v) for k, v in out.items()}


# (R, N) -> the kappa of tests/loss_cases.py's element-wise dl comparison that the fp32 stand-in (tests/cpu_ops) needs on
# these inputs against fp64; the kernel is held to kappa_rule of it (4 x, floored at 2^-20).  The teacher logits reach
# |y| ~ 20 here (u = 100 on raw similarities ~ 0.15), for which 2^-22 |y| predicts 4.8e-6.
DISTILL_KAPPA_FP32 = {(64, 64): 0.0, (100, 100): 0.0, (64, 100): 0.0, (257, 257): 0.0, (1000, 1000): 2.33e-6,
                      (4096, 4096 * 8): 2.21e-6}


@pytest.mark.parametrize("R,N", list(DISTILL_KAPPA_FP32))
def test_simce_distill_kernel_matches_fp64(R, N):
    """dl is compared element by element, |got - ref| <= 2^-7 |ref| + kappa mag: a bound relative to max |dl| (the diagonal
    term) lets an off-diagonal entry, about 1 / N of it, be wrong by 100 %."""
    from clipa_amd import ops
    Es, Et = 512, 768
    label0 = N - R if N != R else 0
    cols_s, base_s = _feats(N, Es, 1)
    cols_t, base_t = _feats(N, Et, 2, noise=2.5)
    rows_s = _feats(R, Es, 3, base=base_s[label0:label0 + R])[0]
    rows_t = _feats(R, Et, 4, base=base_t[label0:label0 + R], noise=2.5)[0]
    n8 = (N + 7) // 8 * 8
    pad = lambda x: torch.cat([x, torch.zeros(n8 - N, x.shape[1], dtype=x.dtype)]) if n8 > N else x   # noqa: E731
    cols_s, cols_t = pad(cols_s).to(DEV), pad(cols_t).to(DEV)
    rows_s, rows_t = rows_s.to(DEV), rows_t.to(DEV)
    s_val, u_val, gc_val, gd_val = 1 / 0.07, 100.0, 0.7, 1.3
    s, u = torch.tensor([s_val], device=DEV), torch.tensor([u_val], device=DEV)
    gc, gd = torch.tensor([gc_val], device=DEV), torch.tensor([gd_val], device=DEV)
    gs = 0.5 / R
    ce, dist_rows, lse_s, lse_t = ops.simce_distill(rows_s, cols_s, rows_t, cols_t, N, label0, s, u)
    dl, ds = ops.simce_distill_bwd(rows_s, cols_s, rows_t, cols_t, N, label0, gs, lse_s, lse_t, s, u, gc, gd)
    torch.cuda.synchronize()
    want = _fp64_direction(rows_s, cols_s, rows_t, cols_t, N, label0, s_val, u_val, gs, gc_val, gd_val)
    for name, got in (("lse_s", lse_s), ("lse_t", lse_t), ("ce", ce), ("dist", dist_rows)):
        err = (got.double() - want[name]).abs().max().item()
        assert err < 2e-3 * max(1.0, want[name].abs().max().item()), (name, err)
    assert dl.shape == (R, n8)
    if n8 > N:
        assert (dl[:, N:] == 0).all(), "pad columns of dl must be zero"
    kappa = kappa_rule(DISTILL_KAPPA_FP32[(R, N)])
    assert kappa >= KAPPA_FLOOR
    ratio = (dl[:, :N].double() - want["dl"]).abs() / (DL_RTOL * want["dl"].abs() + kappa * want["mag"])
    print(f"[distill kernel {R}x{N}] dl: worst error / tolerance {ratio.max().item():.3g}")
    assert ratio.max().item() <= 1.0, (ratio.max().item(), divmod(int(ratio.argmax()), N))
    err_ds = (ds.double() - want["ds"]).abs().max().item()
    assert err_ds < 1e-4 * want["ds_abs"].max().item() + 1e-7, err_ds
    # deterministic: a second call is bitwise equal
    ce2, dist2, lse_s2, lse_t2 = ops.simce_distill(rows_s, cols_s, rows_t, cols_t, N, label0, s, u)
    dl2, ds2 = ops.simce_distill_bwd(rows_s, cols_s, rows_t, cols_t, N, label0, gs, lse_s2, lse_t2, s, u, gc, gd)
    for a, b in ((ce, ce2), (dist_rows, dist2), (lse_s, lse_s2), (lse_t, lse_t2), (dl, dl2), (ds, ds2)):
        assert torch.equal(a, b)


def _golden():
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from tools import make_distill_golden as G
    return G, np.load(GOLDEN)


def _check_against_golden(got, z, prefix):
    G = _golden()[0]
    lc, ld, gi, gt, gs = got
    for val, key in ((lc, "closs"), (ld, "dloss")):
        ref = float(z[f"{prefix}_{key}"])
        assert abs(val - ref) < 2e-2 * abs(ref), (prefix, key, val, ref)
    for a, key in ((gi, "gi"), (gt, "gt")):
        b, idx, ref_norm = G.grad(z, f"{prefix}_{key}")
        a = a.reshape(-1).astype(np.float64)
        full_norm = np.linalg.norm(a)
        if idx is not None:
            a = a[idx]
        b = b.astype(np.float64)
        cos = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
        assert cos > 0.999, (prefix, key, cos)
        assert abs(full_norm / ref_norm - 1) < 2e-2, (prefix, key)
    ref_gs = float(z[f"{prefix}_gs"])
    assert abs(gs - ref_gs) < 3e-2 * abs(ref_gs) + 1e-4, (prefix, gs, ref_gs)


def _run_loss(fn, img, txt, dimg, dtxt, s_val, u_val, dev):
    i = torch.from_numpy(img).to(dev).requires_grad_(True)
    t = torch.from_numpy(txt).to(dev).requires_grad_(True)
    s = torch.tensor(s_val, device=dev, requires_grad=True)
    with torch.no_grad():
        di, dt, u = torch.from_numpy(dimg).to(dev), torch.from_numpy(dtxt).to(dev), torch.tensor(u_val, device=dev)
    out = fn(i, t, s, di, dt, u, output_dict=True)
    (out["contrastive_loss"] + out["distill_loss"]).backward()
    torch.cuda.synchronize()
    return (float(out["contrastive_loss"].detach()), float(out["distill_loss"].detach()), i.grad.cpu().numpy(), t.grad.cpu().numpy(),
            float(s.grad))


@pytest.mark.parametrize("R", [64, 100])
def test_distill_clip_loss_single_rank_matches_reference_golden(R):
    import clipa_amd
    G, z = _golden()
    p = f"w1_r{R}"
    img, txt, dimg, dtxt = G.features(R, int(z[f"{p}_es"]), int(z[f"{p}_et"]), seed=int(z[f"{p}_seed"]))
    got = _run_loss(clipa_amd.DistillClipLoss(), img, txt, dimg, dtxt, float(z["scale_s"]), float(z["scale_t"]), DEV)
    _check_against_golden(got, z, p)
    # the tuple form of the call contract
    fn = clipa_amd.DistillClipLoss()
    i, t = torch.from_numpy(img).to(DEV), torch.from_numpy(txt).to(DEV)
    di, dt = torch.from_numpy(dimg).to(DEV), torch.from_numpy(dtxt).to(DEV)
    c, d = fn(i, t, torch.tensor(float(z["scale_s"]), device=DEV), di, dt, torch.tensor(float(z["scale_t"]), device=DEV))
    assert abs(float(c) - float(z[f"{p}_closs"])) < 2e-2 * float(z[f"{p}_closs"])
    assert abs(float(d) - float(z[f"{p}_dloss"])) < 2e-2 * float(z[f"{p}_dloss"])


def _get(q, procs, limit=300):
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


def _variant_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import clipa_amd
    G, z = _golden()
    B = int(z["w2_B"])
    sl = slice(rank * B, (rank + 1) * B)
    img, txt, dimg, dtxt = G.features(world * B, int(z["w2_es"]), int(z["w2_et"]), seed=int(z["w2_seed"]))
    res = {}
    for local_loss in (True, False):
        for gwg in (True, False):
            fn = clipa_amd.DistillClipLoss(local_loss=local_loss, gather_with_grad=gwg, cache_labels=True, rank=rank,
                                           world_size=world)
            res[f"{int(local_loss)}{int(gwg)}"] = _run_loss(fn, img[sl], txt[sl], dimg[sl], dtxt[sl],
                                                            float(z["scale_s"]), float(z["scale_t"]), dev)
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def test_distill_clip_loss_variants_two_ranks_match_reference_golden():
    """All four local_loss x gather_with_grad variants under a 2-rank group (teacher features ride the student text
    all-gather) against the REAL reference's DistillClipLoss under a 2-rank gloo group."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_variant_worker, args=(r, world, 29787, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(_get(q, procs) for _ in range(world))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    z = _golden()[1]
    for rank in range(world):
        for key, vals in got[rank].items():
            _check_against_golden(vals, z, f"w2_{key}_r{rank}")


# ---- end to end: a training student and an eval() teacher of another architecture in one process ----------------------
STUDENT = {"embed_dim": 64,
           "vision_cfg": {"image_size": 64, "layers": 2, "width": 128, "patch_size": 16},
           "text_cfg": {"context_length": 16, "vocab_size": 512, "width": 128, "heads": 2, "layers": 2}}
TEACHER = {"embed_dim": 96,
           "vision_cfg": {"image_size": 64, "layers": 3, "width": 192, "patch_size": 16},
           "text_cfg": {"context_length": 16, "vocab_size": 512, "width": 192, "heads": 3, "layers": 2}}


def _ref_distill(i, t, s, di, dt, u):
    """CPU fp32 restatement of DistillClipLoss at W = 1 (loss.py:202-238)."""
    labels = torch.arange(i.shape[0])
    zi, zt = s * i @ t.T, s * t @ i.T
    yi, yt = u * di @ dt.T, u * dt @ di.T
    c = (F.cross_entropy(zi, labels) + F.cross_entropy(zt, labels)) / 2
    h = lambda y, z: -(y.softmax(1) * z.log_softmax(1)).sum(1).mean(0)   # noqa: E731
    return c, (h(yi, zi) + h(yt, zt)) / 2


@pytest.mark.parametrize("student_prec,teacher_prec", [("bf16", "fp8"), ("fp8", "bf16")])
def test_student_and_teacher_end_to_end_match_cpu_restatement(tmp_path, student_prec, teacher_prec):
    import clipa_amd
    from oracle import clip_oracle as O
    for name, cfg in (("distill-student", STUDENT), ("distill-teacher", TEACHER)):
        path = os.path.join(str(tmp_path), name + ".json")
        json.dump(cfg, open(path, "w"))
        clipa_amd.add_model_config(path)
    torch.manual_seed(0)
    student, _, _ = clipa_amd.create_model_and_transforms("distill-student", precision=student_prec, device=DEV,
                                                          output_dict=True)
    teacher, _, _ = clipa_amd.create_model_and_transforms("distill-teacher", precision=teacher_prec, device=DEV,
                                                          output_dict=True)
    student.set_grad_checkpointing(True)
    teacher.eval()
    s_sd = {k: v.detach().float().cpu().clone() for k, v in student.state_dict().items()}
    t_sd = {k: v.detach().float().cpu().clone() for k, v in teacher.state_dict().items()}
    loss_fn = clipa_amd.create_loss(type("A", (), dict(local_loss=False, gather_with_grad=False, rank=0, world_size=1,
                                                         horovod=False, distill=True, model="distill-student")))
    images, texts = O.synthetic_batch(16, 64, 16, 512, seed=7)
    # two steps: the teacher's no-grad forward sits between the student's forward and backward, as in train.py:206-213
    for step in range(2):
        student.zero_grad(set_to_none=True)
        out = student(images.to(DEV), texts.to(DEV))
        with torch.no_grad():
            dist_out = teacher(images.to(DEV), texts.to(DEV))
        dist_out = {"dist_" + k: v for k, v in dist_out.items()}
        losses = loss_fn(**out, **dist_out, output_dict=True)
        total = sum(losses.values())
        total.backward()
        torch.cuda.synchronize()
    assert all(p.grad is None for p in teacher.parameters()), "the teacher must not receive gradients"
    # CPU fp32 restatement: oracle student + oracle teacher + the reference loss maths
    ref_s = {k: v.clone().requires_grad_(True) for k, v in s_sd.items()}
    i, t, s = O.clip_forward(ref_s, O.oracle_cfg(STUDENT), O.normalize_images(images), texts)
    with torch.no_grad():
        di, dt, u = O.clip_forward(t_sd, O.oracle_cfg(TEACHER), O.normalize_images(images), texts)
    feat_tol = 6e-2 if "fp8" in (student_prec, teacher_prec) else 2e-2
    assert (dist_out["dist_image_features"].float().cpu() - di).abs().max() < feat_tol
    assert (dist_out["dist_text_features"].float().cpu() - dt).abs().max() < feat_tol
    rc, rd = _ref_distill(i, t, s, di, dt, u)
    (rc + rd).backward()
    loss_tol = 0.05 if "fp8" in (student_prec, teacher_prec) else 2e-2
    assert abs(float(losses["contrastive_loss"]) - float(rc)) < loss_tol * float(rc)
    assert abs(float(losses["distill_loss"]) - float(rd)) < loss_tol * float(rd)
    cos_min = 0.95 if student_prec == "fp8" else 0.99
    worst = 1.0
    for k, p in student.named_parameters():
        assert p.grad is not None, k
        a, b = p.grad.double().cpu().reshape(-1), ref_s[k].grad.double().reshape(-1)
        assert torch.isfinite(a).all(), k
        if float(b.norm()) < 1e-7:
            continue
        c = _cos(a, b)
        worst = min(worst, c)
        assert c > cos_min, (k, c)
    print(f"[distill e2e student {student_prec} teacher {teacher_prec}] worst gradient cosine {worst:.5f}")


def test_contrastive_half_equals_clip_loss():
    """DistillClipLoss's contrastive_loss is ClipLoss's on the same student features; with g_d = 0 its feature and scale
    gradients are ClipLoss's."""
    import clipa_amd
    R, Es, Et = 300, 256, 384
    img, base = _feats(R, Es, 11)
    txt = _feats(R, Es, 12, base=base)[0]
    dimg, bt = _feats(R, Et, 13, noise=2.5)
    dtxt = _feats(R, Et, 14, base=bt, noise=2.5)[0]
    grads = []
    for which in ("clip", "distill"):
        i = img.float().to(DEV).requires_grad_(True)
        t = txt.float().to(DEV).requires_grad_(True)
        s = torch.tensor(1 / 0.07, device=DEV, requires_grad=True)
        if which == "clip":
            c = clipa_amd.ClipLoss()(i, t, s)
        else:
            c, _ = clipa_amd.DistillClipLoss()(i, t, s, dimg.float().to(DEV), dtxt.float().to(DEV),
                                               torch.tensor(100.0, device=DEV))
        grads.append((float(c),) + torch.autograd.grad(c, (i, t, s)))
    (lc, gi_c, gt_c, gs_c), (ld, gi_d, gt_d, gs_d) = grads
    assert abs(lc - ld) < 1e-4 * abs(lc) + 1e-6, (lc, ld)
    for a, b in ((gi_c, gi_d), (gt_c, gt_d)):
        assert _cos(a, b) > 0.9999
        assert abs(float(a.norm() / b.norm()) - 1) < 1e-3
    assert abs(float(gs_c) - float(gs_d)) < 1e-3 * abs(float(gs_c)) + 1e-6
