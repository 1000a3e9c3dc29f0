"""Case tables and references of the fine-tuning kernels (csrc/mixcut.hip, csrc/softce.hip), shared by tests/test_finetune_cpu.py
(the stand-ins of tests/finetune_cpu_ops.py) and tests/test_finetune_gpu.py (the kernels).  The references are restatements
written from the maths of clipa_jax/transforms/mixup.py and clipa_jax/losses/common.py: numpy float32 for the image mixing (bit
for bit), torch fp64 for the loss.

softce bounds: row losses and lse |got - ref| <= KAPPA max(1, |ref|); dlogits |got - ref| <= 2^-7 |ref| + KAPPA_G g.  bf16 rounds
to 2^-9 relative, which the first term covers; KAPPA and KAPPA_G are twice the worst error that the fp32 restatement of the
kernel's sweeps (softce_sweeps below: the same lane order, the same butterfly) shows against fp64 over the whole table, computed
on the CPU by kappas() and never taken from the kernel; tests/test_finetune_cpu.py checks the stated constants against it.  The
absolute term matters where softmax - t cancels: the label column of a confident row (p -> 1 with t = 1), the "confident" rows of
the table."""
import numpy as np
import pytest
import torch

KAPPA = 6.1e-7          # kappas() gives 6.083e-7
KAPPA_G = 1.9e-7        # kappas() gives 1.827e-7

LAMS = (0.0, 1.0, 0.5, 1.0 / 3.0, 1.0 - 2.0 ** -20)


def names(cases):
    return ["-".join(f"{k}{v}" for k, v in c.items()) for c in cases]


# ---- mixcut ----------------------------------------------------------------------------------------------------------------
def boxes(S):
    """(y0, y1, x0, x1): empty, the whole image, one clipped at each border, a 1 x 1 box in two corners."""
    return ((3, 3, 5, 9), (0, S, 0, S), (0, 4, 2, 9), (S - 3, S, 1, 7), (2, 8, 0, 5), (3, 9, S - 4, S), (0, 1, 0, 1),
            (S - 1, S, S - 1, S))


def _mixcut_table():
    out = []
    for layout in ("nchw", "nhwc"):
        for S in (16, 18):                      # 768 and 972 bytes per image: 972 = 60 * 16 + 12, the 16-byte path has a tail
            for B, mix_rots, cut_rots in ((1, (0,), (0,)), (2, (0, 2, 4), (0, 2, 4, 6)), (5, (0,), (0, 4))):
                out += [dict(mode="mixup", B=B, S=S, layout=layout, rot=r) for r in mix_rots]
                out += [dict(mode="cutmix", B=B, S=S, layout=layout, rot=r) for r in cut_rots]
    return out


MIXCUT = _mixcut_table()


def position_coded(B, S):
    """uint8 [B,3,S,S]: the value is a function of (b, y, x, c) mod 251, different in every neighbour."""
    b, c, y, x = np.meshgrid(np.arange(B), np.arange(3), np.arange(S), np.arange(S), indexing="ij")
    return ((b * 89 + y * 37 + x * 11 + c * 101 + y * x) % 251).astype(np.uint8)


def mixcut_operands(case):
    """-> (images uint8 [B,3,S,S] numpy, lam f32 [B] | None, box int32 [B,4] | None), different per sample."""
    B, S, rot = case["B"], case["S"], case["rot"]
    img = position_coded(B, S)
    if case["mode"] == "mixup":
        return img, np.array([LAMS[(b + rot) % len(LAMS)] for b in range(B)], dtype=np.float32), None
    bx = boxes(S)
    return img, None, np.array([bx[(b + rot) % len(bx)] for b in range(B)], dtype=np.int32)


def mixcut_reference(img, lam=None, box=None):
    """The numpy restatement.  mixup: d = a - b', t = lam d, v = t + b', out = uint8(int(v + 0.5)), every step in float32."""
    other = img[::-1]
    if lam is not None:
        a, b = img.astype(np.float32), other.astype(np.float32)
        l = lam.astype(np.float32).reshape(-1, 1, 1, 1)
        d = a - b
        t = l * d
        v = t + b
        assert d.dtype == t.dtype == v.dtype == np.float32
        return (v + np.float32(0.5)).astype(np.int32).astype(np.uint8)
    out = img.copy()
    for i, (y0, y1, x0, x1) in enumerate(box):
        out[i, :, y0:y1, x0:x1] = other[i, :, y0:y1, x0:x1]
    return out


def _to_layout(img, layout, dev):
    t = torch.from_numpy(img.copy()).to(dev)                 # a copy: the operation is in place
    return t.contiguous(memory_format=torch.channels_last) if layout == "nhwc" else t


def check_mixcut(ops, dev, case):
    img, lam, box = mixcut_operands(case)
    ref = mixcut_reference(img, lam, box)
    t = _to_layout(img, case["layout"], dev)
    kw = dict(lam=torch.from_numpy(lam).to(dev)) if lam is not None else dict(box=torch.from_numpy(box).to(dev))
    out = ops.mixcut_u8(t, **kw)
    ops.check_token_ids(wait=True)
    assert out is t                                                     # in place
    got = out.cpu().numpy()
    assert got.shape == ref.shape and np.array_equal(got, ref), f"{int((got != ref).sum())} bytes differ"
    if case["B"] % 2:
        assert np.array_equal(got[case["B"] // 2], img[case["B"] // 2])    # the middle sample: bit for bit
    if case["B"] > 1 and case["mode"] == "mixup":
        assert not np.array_equal(got, img)


def check_mixcut_refuses(ops, dev):
    """Bad lam / bad box raise, and the batch is not altered for such a pair; other pairs of the same launch are served."""
    S = 16
    img = position_coded(4, S)
    for layout in ("nchw", "nhwc"):
        for bad in (-0.25, 1.5, float("nan")):
            t = _to_layout(img, layout, dev)
            lam = torch.tensor([0.5, bad, 0.25, 0.5]).to(dev)
            with pytest.raises(RuntimeError, match="mixcut_u8"):
                ops.mixcut_u8(t, lam=lam)
                ops.check_token_ids(wait=True)
            got = t.cpu().numpy()
            good = mixcut_reference(img, np.array([0.5, 0.5, 0.5, 0.5], dtype=np.float32))
            assert np.array_equal(got[[1, 2]], img[[1, 2]]) and np.array_equal(got[[0, 3]], good[[0, 3]])
        for bad in ((0, S + 1, 0, 4), (-1, 4, 0, 4), (5, 4, 0, 4), (0, 4, 9, 8), (0, 4, 0, S + 1)):
            t = _to_layout(img, layout, dev)
            box = torch.tensor([[0, 4, 0, 4], [2, 6, 2, 6], bad, [1, 3, 1, 3]], dtype=torch.int32).to(dev)
            with pytest.raises(RuntimeError, match="mixcut_u8"):
                ops.mixcut_u8(t, box=box)
                ops.check_token_ids(wait=True)
            got = t.cpu().numpy()
            good = mixcut_reference(img, None, np.array([[0, 4, 0, 4], [0, 0, 0, 0], [0, 0, 0, 0], [1, 3, 1, 3]], dtype=np.int32))
            assert np.array_equal(got, good)
    ops.check_token_ids(wait=True)                                     # nothing is left pending


# ---- softce ----------------------------------------------------------------------------------------------------------------
def _softce_table():
    out = []
    # C: around the wave (63, 64, 65), the register variants' limits (1024 / 1025 and 4096: csrc/softce.hip) and the re-read path
    # (4099); 1001 with ld = 1008 is the padded classifier head of ImageNet with a background class
    for C, ld in ((2, 8), (63, 68), (64, 68), (65, 72), (1000, 1004), (1001, 1008), (1025, 1032), (4096, 4100), (4099, 4104)):
        for B in (1, 5):
            for eps in (0.0, 0.1):
                for targets in ("mix", "hard"):
                    out.append(dict(C=C, ld=ld, B=B, eps=eps, targets=targets, rows="mixed"))
    for C, ld in ((2, 8), (65, 72), (1000, 1004)):
        out.append(dict(C=C, ld=ld, B=5, eps=0.0, targets="hard", rows="confident"))
    return out


SOFTCE = _softce_table()


def softce_operands(case):
    """-> (buffer f32 [B, ld] with NaN in every pad column, ya, yb | None, lam | None) as CPU tensors.  Rows of a B = 5 case:
    0 equal logits, 1 |z| up to 100, 2 the label column holds the row maximum, 3 it holds the minimum, 4 ya == yb.
    "confident" rows: the label's logit leads the others by 10 ... 18, so softmax - t cancels to a few ulp of 1."""
    C, ld, B = case["C"], case["ld"], case["B"]
    rng = np.random.RandomState(C * 7 + B)
    z = (rng.standard_normal((B, C)) * 5.0).astype(np.float32)
    ya = rng.randint(0, C, size=B).astype(np.int32)
    yb = rng.randint(0, C, size=B).astype(np.int32)
    lam = np.array([0.3, 0.0, 1.0, 0.3, 0.3][:B], dtype=np.float32)
    if case["rows"] == "confident":
        z = rng.standard_normal((B, C)).astype(np.float32)
        for r in range(B):
            z[r, ya[r]] = np.float32(10.0 + 2.0 * r) + z[r].max()
    elif B == 1:
        z[0] = rng.uniform(-100.0, 100.0, size=C).astype(np.float32)
    else:
        z[0] = np.float32(3.25)
        z[1] = rng.uniform(-100.0, 100.0, size=C).astype(np.float32)
        ya[2], ya[3] = int(z[2].argmax()), int(z[3].argmin())
        yb[4] = ya[4]
    buf = np.full((B, ld), np.nan, dtype=np.float32)
    buf[:, :C] = z
    t = lambda a: torch.from_numpy(a)
    if case["targets"] == "hard":
        return t(buf), t(ya), None, None
    return t(buf), t(ya), t(yb), t(lam)


def softce_reference(z, ya, yb, lam, eps, g):
    """torch fp64: -> (loss [B], lse [B], dlogits [B, C]) of t_c = (1 - eps) (lam [c=ya] + (1 - lam) [c=yb]) + eps / C."""
    z = z.double()
    B, C = z.shape
    lam = torch.ones(B, dtype=torch.float64) if lam is None else lam.double()
    yb = ya if yb is None else yb
    t = torch.zeros(B, C, dtype=torch.float64)
    rows = torch.arange(B)
    t[rows, ya.long()] += lam
    t[rows, yb.long()] += 1.0 - lam
    t = (1.0 - float(np.float32(eps))) * t + float(np.float32(eps)) / C
    lse = torch.logsumexp(z, dim=1)
    return lse - (t * z).sum(1), lse, g * (torch.softmax(z, dim=1) - t)


def softce_sweeps(buf, C, ya, yb, lam, eps, g, bug=None):
    """The fp32 restatement of the kernel's sweeps in numpy float32, in the kernel's order: lane l of 64 owns the 4-column chunks
    l + 64 j and adds its elements in ascending column order, then the xor butterfly (offsets 32 ... 1); loss = log s - sum_c t_c
    (z_c - m).  buf f32 [B, ld]; -> (loss, lse, dlogits f32 [B, C] not yet rounded to bf16).  bug: one of the four wrong kernels
    the comparison has to refuse - "smooth_ld", "swap", "once", "pad_lse"."""
    f = np.float32
    buf = np.asarray(buf, dtype=f)
    B, ld = buf.shape
    W = ld if bug == "pad_lse" else C                    # the columns that enter the sums
    z = buf[:, :W]
    n_it = (W + 255) // 256
    zp = np.zeros((B, n_it * 256), dtype=f)
    zp[:, :W] = z
    valid = np.zeros((B, n_it * 256), dtype=bool)
    valid[:, :W] = True
    zp, valid = zp.reshape(B, n_it, 64, 4), valid.reshape(B, n_it, 64, 4)
    m = z.max(axis=1) if not np.isnan(z).any() else np.full(B, np.nan, dtype=f)
    with np.errstate(under="ignore", invalid="ignore"):
        d = (zp - m[:, None, None, None]).astype(f)
        e = np.where(valid, np.exp(d).astype(f), f(0))
        d = np.where(valid, d, f(0))
        s, q = np.zeros((B, 64), dtype=f), np.zeros((B, 64), dtype=f)
        for j in range(n_it):
            for i in range(4):
                s = s + e[:, j, :, i]
                q = q + d[:, j, :, i]
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
            q = q + q[:, lanes ^ o]
        s, q = s[:, 0], q[:, 0]
        ya = np.asarray(ya, dtype=np.int64)
        yb = ya if yb is None else np.asarray(yb, dtype=np.int64)
        lam = np.ones(B, dtype=f) if lam is None else np.asarray(lam, dtype=f)
        eps = f(eps)
        base = eps / f(ld if bug == "smooth_ld" else C)
        wa, wb = (f(1) - eps) * lam, (f(1) - eps) * (f(1) - lam)
        if bug == "swap":
            wa, wb = wb, wa
        if bug == "once":
            wb = np.where(ya == yb, f(0), wb)
        rows = np.arange(B)
        logs = np.log(s).astype(f)
        tz = wa * (z[rows, ya] - m) + wb * (z[rows, yb] - m) + base * q
        loss, lse = logs - tz, m + logs
        inv = f(1) / s
        p = (e.reshape(B, -1)[:, :C] * inv[:, None]).astype(f)
        t = np.full((B, C), base, dtype=f)
        t[rows, ya] = t[rows, ya] + wa
        t[rows, yb] = t[rows, yb] + wb
        dl = f(g) * (p - t)
    assert loss.dtype == lse.dtype == dl.dtype == f
    return loss, lse, dl


def softce_errors(got, ref, g):
    """-> (worst |got - ref| / max(1, |ref|) over loss and lse, worst (|got - ref| - 2^-7 |ref|) / g over dlogits, at least 0)."""
    k = 0.0
    for a, b in zip(got[:2], ref[:2]):
        k = max(k, float(((a.double() - b).abs() / b.abs().clamp_min(1.0)).max()))
    kg = float((((got[2].double() - ref[2]).abs() - 2.0 ** -7 * ref[2].abs()) / g).clamp_min(0.0).max())
    return k, kg


def kappas():
    """Twice the worst error of the fp32 restatement (its gradient rounded to bf16) against fp64 over the table (CPU)."""
    k = kg = 0.0
    for c in SOFTCE:
        buf, ya, yb, lam = softce_operands(c)
        g = 1.0 / c["B"]
        ref = softce_reference(buf[:, :c["C"]], ya, yb, lam, c["eps"], g)
        loss, lse, dl = softce_sweeps(buf.numpy(), c["C"], ya, yb, lam, c["eps"], g)
        got = (torch.from_numpy(loss), torch.from_numpy(lse), torch.from_numpy(dl).to(torch.bfloat16))
        a, b = softce_errors(got, ref, g)
        k, kg = max(k, a), max(kg, b)
    return 2 * k, 2 * kg


def check_softce(ops, dev, case, kappa=KAPPA, kappa_g=KAPPA_G, **kw):
    buf, ya, yb, lam = softce_operands(case)
    C, B = case["C"], case["B"]
    g = 1.0 / B
    ref = softce_reference(buf[:, :C], ya, yb, lam, case["eps"], g)
    dbuf = buf.to(dev)
    put = lambda t: None if t is None else t.to(dev)
    loss, lse, dl = ops.soft_target_ce(dbuf[:, :C], put(ya), put(yb), put(lam), smoothing=case["eps"], gscale=g, **kw)
    ops.check_token_ids(wait=True)
    assert tuple(loss.shape) == (B,) and tuple(lse.shape) == (B,) and tuple(dl.shape) == (B, C) and dl.dtype == torch.bfloat16
    got = (loss.cpu(), lse.cpu(), dl.cpu())
    for name, t in zip(("loss", "lse", "dlogits"), got):
        assert torch.isfinite(t).all(), f"{name} is not finite"
    k, kg = softce_errors(got, ref, g)
    print(f"[softce {case}] loss/lse error {k:.3e} (bound {kappa:.2e}), dlogits excess {kg:.3e} (bound {kappa_g:.2e})")
    assert k <= kappa, f"loss / lse error {k:.3e} above {kappa:.3e}"
    assert kg <= kappa_g, f"dlogits error beyond 2^-7 |ref| is {kg:.3e} g, above {kappa_g:.3e} g"
    # the zero padding of the gradient buffer, the untouched NaN padding of the logits
    ldd = dl.stride(0)
    assert ldd % 8 == 0 and ldd >= C
    full = dl.as_strided((B, ldd), (ldd, 1)).cpu()
    assert not full[:, C:].float().abs().any()
    assert torch.isnan(dbuf[:, C:]).all()
    # without a gradient: the same loss bits
    loss2, lse2, none = ops.soft_target_ce(dbuf[:, :C], put(ya), put(yb), put(lam), smoothing=case["eps"], **kw)
    assert none is None and torch.equal(loss2.cpu(), got[0]) and torch.equal(lse2.cpu(), got[1])
    return got


def check_softce_refuses(ops, dev):
    """Labels outside [0, C) and lam outside [0, 1] raise."""
    z = torch.zeros(3, 12).to(dev)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32).to(dev)
    good_lam = torch.tensor([0.5, 0.5, 0.5]).to(dev)
    for ya, yb, lam in ((i32(0, 12, 1), None, None), (i32(0, -1, 1), None, None), (i32(0, 1, 2), i32(0, 12, 1), good_lam),
                        (i32(0, 1, 2), i32(2, 1, 0), torch.tensor([0.5, 1.25, 0.5]).to(dev)),
                        (i32(0, 1, 2), i32(2, 1, 0), torch.tensor([0.5, float("nan"), 0.5]).to(dev))):
        with pytest.raises(RuntimeError, match="soft_target_ce"):
            ops.soft_target_ce(z, ya, yb, lam, gscale=1.0)
            ops.check_token_ids(wait=True)
    ops.check_token_ids(wait=True)
    for bad in (dict(yb=i32(0, 1, 2)), dict(smoothing=1.5)):
        with pytest.raises(RuntimeError):
            ops.soft_target_ce(z, i32(0, 1, 2), **bad)
    with pytest.raises(RuntimeError):
        ops.soft_target_ce(z[:, :1], i32(0, 0, 0))


# ---- the toy model ---------------------------------------------------------------------------------------------------------
TOY = {"embed_dim": 64,
       "vision_cfg": {"image_size": 32, "layers": 2, "width": 128, "patch_size": 16},
       "text_cfg": {"context_length": 8, "vocab_size": 64, "width": 64, "heads": 1, "layers": 1}}
MODEL_CASES = ("plain10", "normalized10", "padded1001")
# relative L2 error |d - ref| / |ref| of the head's two gradients against the fp32 oracle, as the bf16 restatement of the head on
# the CPU stand-ins measures it (tests/test_finetune_cpu.py prints and checks the figures); the GPU bound is twice that
HEAD_DW_MEASURED_CPU = {"plain10": 0.0061, "normalized10": 0.0058, "padded1001": 0.0063}
HEAD_DF_MEASURED_CPU = {"plain10": 0.0029, "normalized10": 0.0033, "padded1001": 0.0025}
MIX_LAM = (1.0, 0.95, 0.9, 1.0, 0.05, 0.97, 1.0, 0.92)       # near 0 / 1: the targets' entropy leaves the loss room to fall


def toy(name, B=8, seed=11):
    """-> dict(sd: the CLIP state dict from oracle.clip_oracle.make_state_dict, head [C, E], images uint8 [B,3,32,32], ya, yb,
    lam, C, normalize, smoothing)."""
    import clipa_amd
    from oracle import clip_oracle as O
    C = 1001 if name == "padded1001" else 10
    shapes = {k: tuple(v.shape) for k, v in clipa_amd.CLIP(**TOY).state_dict().items()}
    sd = O.make_state_dict(shapes, seed)
    rng = np.random.RandomState(seed + 1)
    E = TOY["embed_dim"]
    head = rng.standard_normal((C, E)) * E ** -0.5
    if name == "normalized10":                   # the WiSE-FT start: unit-norm class embeddings times a logit scale
        head = 10.0 * head / np.linalg.norm(head, axis=1, keepdims=True)
    images = torch.from_numpy(rng.randint(0, 256, size=(B, 3, 32, 32), dtype=np.uint8))
    ya = torch.from_numpy(rng.randint(0, C, size=B).astype(np.int32))
    lam = torch.tensor((MIX_LAM * ((B + 7) // 8))[:B], dtype=torch.float32)
    return dict(name=name, sd=sd, head=torch.from_numpy(head.astype(np.float32)), images=images, ya=ya, yb=ya.flip(0), lam=lam,
                C=C, normalize=name == "normalized10", smoothing=0.1)


def build_classifier(t, device="cpu"):
    import clipa_amd
    clip = clipa_amd.CLIP(**TOY)
    clip.load_state_dict(t["sd"], strict=True)
    clip.to(device)
    clip.set_grad_checkpointing(True)
    m = clipa_amd.ImageClassifier(clip.visual, t["C"], normalize=t["normalize"], init=t["head"])
    return m.train()


def oracle_step(t, sd=None, head=None, dtype=torch.float32):
    """The fp32 (or fp64) oracle: oracle.clip_oracle.encode_image, the head and the soft-target cross-entropy in torch.
    -> (logits, features, loss, {name: gradient} with 'head.weight' and the tower's keys under 'visual.', feature gradient)."""
    from oracle import clip_oracle as O
    sd = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in (sd or t["sd"]).items() if k.startswith("visual.")}
    w = (t["head"] if head is None else head).detach().clone().to(dtype).requires_grad_(True)
    cfg = O.oracle_cfg(TOY)
    f = O.encode_image(sd, cfg, O.normalize_images(t["images"], dtype=dtype))
    if t["normalize"]:
        f = O.l2_normalize(f)
    f.retain_grad()
    logits = f @ w.T
    B, C = logits.shape
    tgt = torch.zeros(B, C, dtype=dtype)
    rows = torch.arange(B)
    tgt[rows, t["ya"].long()] += t["lam"].to(dtype)
    tgt[rows, t["yb"].long()] += 1 - t["lam"].to(dtype)
    tgt = (1 - t["smoothing"]) * tgt + t["smoothing"] / C
    loss = (torch.logsumexp(logits, 1) - (tgt * logits).sum(1)).mean()
    loss.backward()
    grads = {k: v.grad for k, v in sd.items() if v.grad is not None}
    grads["head.weight"] = w.grad
    return logits.detach(), f.detach(), float(loss.detach()), grads, f.grad


def engine_step(m, t, dev="cpu"):
    """One step of the engine (or of its stand-ins) with mixup targets -> (logits, features, loss, gradients, feature gradient)."""
    import clipa_amd
    m.zero_grad(set_to_none=True)
    f = m.features(t["images"].to(dev))
    f.retain_grad()
    logits = m.head_logits(f)
    loss = clipa_amd.SoftTargetCrossEntropy(t["smoothing"])(logits, (t["ya"].to(dev), t["yb"].to(dev), t["lam"].to(dev)))
    loss.backward()
    grads = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    return logits.detach(), f.detach(), loss.detach(), grads, f.grad


TRAIN_LR = 2e-3
# the mean of n row losses: each within KAPPA, plus the fixed-order fp32 sums over two batches of 8 - a sum of n terms carries at
# most (n - 1) 2^-24 relative
EVAL_LOSS_BOUND = KAPPA + 16 * 2.0 ** -24


def check_evaluation(m, t, got, dev="cpu"):
    """evaluate_classification against the fp64 restatement on the engine's own features and logits: counts exact, the loss
    within the softce bound."""
    was = m.training
    m.eval()
    with torch.no_grad():
        f = m.features(t["images"].to(dev))
        logits = m.head_logits(f).double().cpu()
        v = f.double().cpu() @ m.head.weight.detach().double().cpu().T
    m.train(was)
    lab = t["ya"].long()
    n = lab.numel()
    gt = (v > v.gather(1, lab[:, None])).sum(1)
    ref_loss = float(torch.nn.functional.cross_entropy(logits, lab))
    assert sorted(got) == ["count", "loss", "prec@1", "top5"] and got["count"] == n
    assert got["prec@1"] == int((gt < 1).sum()) / n and got["top5"] == int((gt < 5).sum()) / n
    print(f"evaluation: prec@1 {got['prec@1']:.4f}, top5 {got['top5']:.4f}, loss {got['loss']:.6f} (fp64 {ref_loss:.6f})")
    assert abs(got["loss"] - ref_loss) <= EVAL_LOSS_BOUND * max(1.0, abs(ref_loss))


def rel_l2(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm())
