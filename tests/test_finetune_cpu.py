"""Image-tower fine-tuning without a GPU: the case tables of tests/finetune_cases.py through the stand-ins of
tests/finetune_cpu_ops.py (so the stand-ins keep the contract tests/test_finetune_gpu.py holds the kernels to), the constants of
the softce bounds against the function that derives them, the four wrong kernels the comparison has to refuse, the host logic
(sample_mixcut, ImageClassifier's surface) and clipa_amd.finetune on the stand-ins against torch autograd - whose error on the
head's gradients is the figure the GPU test's bound is built on (it is printed here)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import clipa_amd
from clipa_amd import finetune, lib

from . import finetune_cases as C
from . import finetune_cpu_ops as cpu_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the kernels' contract on the stand-ins --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.MIXCUT, ids=C.names(C.MIXCUT))
def test_mixcut_standin(case):
    C.check_mixcut(cpu_ops, "cpu", case)


def test_mixcut_standin_refuses_bad_descriptors():
    C.check_mixcut_refuses(cpu_ops, "cpu")


def test_mixcut_table_covers_the_issue():
    S = 18
    assert 3 * S * S % 16 == 12 and 3 * 16 * 16 % 16 == 0
    for B in (2, 5):
        for mode, n in (("mixup", len(C.LAMS)), ("cutmix", len(C.boxes(S)))):
            seen = {(b + c["rot"]) % n for c in C.MIXCUT if c["B"] == B and c["mode"] == mode and c["S"] == S for b in range(B)}
            assert seen == set(range(n)), (B, mode)
    bx = C.boxes(S)
    assert bx[0][0] == bx[0][1] and bx[1] == (0, S, 0, S) and bx[6] == (0, 1, 0, 1)
    assert bx[2][0] == 0 and bx[3][1] == S and bx[4][2] == 0 and bx[5][3] == S


def test_mixup_restatement_rounds_half_up_and_keeps_the_ends():
    img = C.position_coded(2, 16)
    for lam, want in ((1.0, img), (0.0, img[::-1])):
        assert np.array_equal(C.mixcut_reference(img, np.full(2, lam, dtype=np.float32)), want)
    a = np.array([[[[3]], [[0]], [[255]]], [[[4]], [[1]], [[0]]]], dtype=np.uint8)       # 3.5 -> 4, 0.5 -> 1, 127.5 -> 128
    assert C.mixcut_reference(a, np.array([0.5, 0.5], dtype=np.float32))[0].reshape(-1).tolist() == [4, 1, 128]


def test_softce_constants_are_what_the_standin_measures():
    k, kg = C.kappas()
    print(f"kappa = {k:.3e} (stated {C.KAPPA:.2e}), kappa_g = {kg:.3e} (stated {C.KAPPA_G:.2e})")
    assert 0.9 * C.KAPPA <= k <= C.KAPPA
    assert 0.9 * C.KAPPA_G <= kg <= C.KAPPA_G


@pytest.mark.parametrize("case", C.SOFTCE, ids=C.names(C.SOFTCE))
def test_softce_standin(case):
    C.check_softce(cpu_ops, "cpu", case)


def test_softce_standin_refuses_bad_targets():
    C.check_softce_refuses(cpu_ops, "cpu")


@pytest.mark.parametrize("bug", ["smooth_ld", "swap", "once", "pad_lse"])
def test_comparison_refuses_wrong_kernels(bug):
    """Smoothing spread over ld instead of C, the ya / yb weights swapped, the ya == yb term counted once, pad columns in the
    LSE: each fails check_softce on the table."""
    class Wrong:
        check_token_ids = staticmethod(cpu_ops.check_token_ids)
        soft_target_ce = staticmethod(functools.partial(cpu_ops.soft_target_ce, _bug=bug))
    refused = 0
    for case in C.SOFTCE:
        try:
            C.check_softce(Wrong, "cpu", case)
        except AssertionError:
            refused += 1
    print(f"{bug}: refused on {refused} of {len(C.SOFTCE)} cases")
    assert refused >= 4


def test_softce_table_covers_the_issue():
    assert {c["C"] for c in C.SOFTCE} >= {2, 63, 64, 65, 1000, 1001, 4099}
    assert any(c["C"] == 1001 and c["ld"] == 1008 for c in C.SOFTCE)
    assert {c["B"] for c in C.SOFTCE} == {1, 5} and {c["eps"] for c in C.SOFTCE} == {0.0, 0.1}
    assert all(c["ld"] > c["C"] and c["ld"] % 4 == 0 for c in C.SOFTCE)
    buf, ya, yb, lam = C.softce_operands(dict(C=65, ld=72, B=5, eps=0.1, targets="mix", rows="mixed"))
    z = buf[:, :65]
    assert torch.isnan(buf[:, 65:]).all() and torch.isfinite(z).all()
    assert float(z[0].max()) == float(z[0].min()) and 90 < float(z[1].abs().max()) <= 100
    assert int(ya[2]) == int(z[2].argmax()) and int(ya[3]) == int(z[3].argmin()) and int(ya[4]) == int(yb[4])
    assert sorted(set(lam.tolist())) == [0.0, pytest.approx(0.3), 1.0]


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    header = open(os.path.join(ROOT, "include", "clipa_hip.h")).read()
    declared = set(re.findall(r"\b(clipa_[a-z0-9_]+)\s*\(", header))
    assert {"clipa_mixcut_u8", "clipa_softce"} <= declared and {"clipa_mixcut_u8", "clipa_softce"} <= set(lib.SIGNATURES)
    assert declared == set(lib.SIGNATURES)
    for cite in ("transforms/mixup.py:141-201", "losses/common.py:104-109", "mixup.py:203-211", "random_erasing.py:25-61"):
        assert cite in header, cite
    from clipa_amd import build
    assert "mixcut.hip" in build.SOURCES and "softce.hip" in build.SOURCES


def test_capi_reports_argument_errors():
    h = lib.load()
    p = ctypes.c_void_p(16)
    assert h.clipa_mixcut_u8(p, p, None, 0, 16, 0, 0, None, None) == 0
    assert h.clipa_mixcut_u8(p, p, None, 2, 0, 0, 0, None, None) < 0 and "S = 0" in lib.last_error()
    assert h.clipa_mixcut_u8(p, p, None, 2, 5000, 0, 0, None, None) < 0 and "out of range" in lib.last_error()
    assert h.clipa_mixcut_u8(p, p, None, 2, 16, 0, 2, None, None) < 0 and "mode = 2" in lib.last_error()
    assert h.clipa_mixcut_u8(p, None, None, 2, 16, 0, 0, None, None) < 0 and "no lam" in lib.last_error()
    assert h.clipa_mixcut_u8(p, p, None, 2, 16, 0, 1, None, None) < 0 and "no box" in lib.last_error()
    assert h.clipa_mixcut_u8(p, p, None, 200000, 16, 0, 0, None, None) < 0 and "131070" in lib.last_error()
    sce = lambda B=4, Cn=10, ld=12, yb=None, lam=None, eps=0.0, dl=None, ldd=16, mw=0, z=p: h.clipa_softce(
        z, B, Cn, ld, p, yb, lam, eps, 1.0, p, p, dl, ldd, mw, None, None)
    assert sce(B=0) == 0
    assert sce(Cn=1) < 0 and "out of range" in lib.last_error()
    assert sce(Cn=32769, ld=32772) < 0 and "out of range" in lib.last_error()
    assert sce(ld=8) < 0 and "ld = 8" in lib.last_error()
    assert sce(ld=14) < 0 and "multiple of 4" in lib.last_error()
    assert sce(eps=1.5) < 0 and "smoothing" in lib.last_error()
    assert sce(yb=p) < 0 and "yb comes with lam" in lib.last_error()
    assert sce(mw=-1) < 0 and "max_workgroups" in lib.last_error()
    assert sce(dl=p, ldd=12) < 0 and "multiple of 8" in lib.last_error()
    assert sce(z=ctypes.c_void_p(20)) < 0 and "16-byte aligned" in lib.last_error()


def test_no_cpu_fallback():
    from clipa_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mixcut_u8(torch.zeros(2, 3, 16, 16, dtype=torch.uint8), lam=torch.ones(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.soft_target_ce(torch.zeros(2, 8), torch.zeros(2, dtype=torch.int32))


# ---- host logic ------------------------------------------------------------------------------------------------------------
def test_sample_mixcut_geometry_and_label_weights():
    S, B = 32, 64
    gen = torch.Generator().manual_seed(3)
    modes = set()
    for _ in range(40):
        mode, lam, box = clipa_amd.sample_mixcut(B, S, generator=gen)
        modes.add(mode)
        assert lam.dtype == torch.float32 and tuple(lam.shape) == (B,) and box.dtype == torch.int32 and tuple(box.shape) == (B, 4)
        assert bool(((lam >= 0) & (lam <= 1)).all())
        y0, y1, x0, x1 = box.long().unbind(1)
        assert bool(((0 <= y0) & (y0 <= y1) & (y1 <= S) & (0 <= x0) & (x0 <= x1) & (x1 <= S)).all())       # inside the image
        if mode == "cutmix":
            pasted = ((y1 - y0) * (x1 - x0)).double()
            assert torch.equal(lam, (1.0 - pasted / (S * S)).float())                # the label matches the pixels, exactly
        else:
            assert not box.any()
    assert modes == {"mixup", "cutmix"}
    # correct_lam=False: the reference's 1 - cut^2 / S^2 of the unclipped size, from the same draws
    a = clipa_amd.sample_mixcut(B, S, mixup_alpha=0.0, generator=torch.Generator().manual_seed(5))
    b = clipa_amd.sample_mixcut(B, S, mixup_alpha=0.0, correct_lam=False, generator=torch.Generator().manual_seed(5))
    assert a[0] == b[0] == "cutmix" and torch.equal(a[2], b[2])
    # the clipped box (sides 2 (cut // 2), less at a border) never holds more pixels than cut^2
    assert bool((b[1] <= a[1]).all()) and bool((b[1] < a[1]).any())


def test_sample_mixcut_unclipped_formula_and_switches():
    S, B = 16, 32
    gen = torch.Generator().manual_seed(9)
    mode, lam, box = clipa_amd.sample_mixcut(B, S, mixup_alpha=0.0, correct_lam=False, generator=gen)
    # replay the draws: u[2], two gammas, the centres
    gen = torch.Generator().manual_seed(9)
    torch.rand(2, generator=gen)
    al = torch.ones(B)
    ga, gb = torch._standard_gamma(al, generator=gen), torch._standard_gamma(al, generator=gen)
    l0 = ga / (ga + gb)
    cut = (torch.sqrt(1 - l0) * float(S)).to(torch.int32)
    assert mode == "cutmix" and torch.equal(lam, (1.0 - cut.double() * cut.double() / (S * S)).float())
    cy = torch.randint(0, S, (B,), generator=gen, dtype=torch.int32)
    assert torch.equal(box[:, 0], (cy - cut // 2).clamp(min=0)) and torch.equal(box[:, 1], (cy + cut // 2).clamp(max=S))
    # prob = 0 leaves the batch alone; an alpha of 0 disables its arm; both 0: nothing
    for seed in range(20):
        g = torch.Generator().manual_seed(seed)
        mode, lam, box = clipa_amd.sample_mixcut(B, S, prob=0.0, generator=g)
        assert mode == "none" and bool((lam == 1).all()) and not box.any()
        assert clipa_amd.sample_mixcut(B, S, cutmix_alpha=0.0, generator=g)[0] == "mixup"
        assert clipa_amd.sample_mixcut(B, S, mixup_alpha=0.0, generator=g)[0] == "cutmix"
        assert clipa_amd.sample_mixcut(B, S, mixup_alpha=0.0, cutmix_alpha=0.0, generator=g)[0] == "none"
        assert clipa_amd.sample_mixcut(B, S, switch_prob=1.0, generator=g)[0] == "cutmix"
        assert clipa_amd.sample_mixcut(B, S, switch_prob=0.0, generator=g)[0] == "mixup"
    # the same seed, the same draws
    a = clipa_amd.sample_mixcut(B, S, generator=torch.Generator().manual_seed(1))
    b = clipa_amd.sample_mixcut(B, S, generator=torch.Generator().manual_seed(1))
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_image_classifier_surface():
    clip = clipa_amd.CLIP(**C.TOY)
    E = C.TOY["embed_dim"]
    m = clipa_amd.ImageClassifier(clip.visual, 10)
    sd = m.state_dict()
    assert list(sd) == ["visual." + k for k in clip.visual.state_dict()] + ["head.weight"]
    assert tuple(sd["head.weight"].shape) == (10, E) and sd["head.weight"].dtype == torch.float32
    # the tower is shared with the CLIP, not copied
    assert m.visual is clip.visual and m._cache is clip._cache
    assert all(p is q for p, q in zip(m.visual.parameters(), clip.visual.parameters()))
    assert len(list(m.parameters())) == len(list(clip.visual.parameters())) + 1
    # inits
    big = clipa_amd.ImageClassifier(clip.visual, 4000)
    assert abs(float(big.head.weight.detach().std()) - E ** -0.5) < 0.02 * E ** -0.5 and abs(float(big.head.weight.detach().mean())) < 1e-3
    assert not clipa_amd.ImageClassifier(clip.visual, 10, init="zeros").head.weight.any()
    w = torch.randn(10, E)
    wise = clipa_amd.ImageClassifier(clip.visual, 10, normalize=True, init=w)
    assert torch.equal(wise.head.weight.detach(), w) and wise.normalize and wise.head.weight.requires_grad
    for bad in ("ones", torch.zeros(9, E)):
        with pytest.raises(ValueError):
            clipa_amd.ImageClassifier(clip.visual, 10, init=bad)
    with pytest.raises(ValueError):
        clipa_amd.ImageClassifier(clip.visual, 1)
    # strict round trip, lock, grad checkpointing, train / eval reach the tower
    other = clipa_amd.ImageClassifier(clipa_amd.CLIP(**C.TOY).visual, 10)
    res = other.load_state_dict(sd, strict=True)
    assert res.missing_keys == [] and res.unexpected_keys == []
    m.lock()
    assert m.head.weight.requires_grad and not any(p.requires_grad for p in m.visual.parameters())
    m.lock(unlocked_groups=1)
    assert m.visual.proj.requires_grad and not m.visual.conv1.weight.requires_grad
    m.set_grad_checkpointing(True)
    assert m.visual.transformer.grad_checkpointing
    m.eval()
    assert not m.visual.training
    m.train()
    assert m.visual.training
    # the factory
    f = clipa_amd.create_classifier(clip, 7, normalize=True, init="zeros")
    assert isinstance(f, clipa_amd.ImageClassifier) and f.visual is clip.visual and f.num_classes == 7 and f.normalize
    g = clipa_amd.create_classifier("ViT-S-16", 5, force_image_size=32)
    assert tuple(g.head.weight.shape) == (5, g.visual.output_dim) and g.visual.image_size == (32, 32)
    with pytest.raises(TypeError):
        clipa_amd.create_classifier(clip, 7, force_image_size=32)


# ---- clipa_amd.finetune on the stand-ins -------------------------------------------------------------------------------------
@pytest.fixture
def standins():
    restore = cpu_ops.swap_in()
    yield
    restore()


def test_loss_and_head_functions_equal_autograd_fp64(standins):
    gen = torch.Generator().manual_seed(2)
    B, Cn, E = 6, 13, 16
    feat = torch.randn(B, E, generator=gen).requires_grad_(True)
    w = torch.nn.Parameter(torch.randn(Cn, E, generator=gen) * 0.3)
    ya, yb = torch.randint(0, Cn, (B,), generator=gen), torch.randint(0, Cn, (B,), generator=gen)
    yb[0] = ya[0]
    lam = torch.rand(B, generator=gen)
    logits = finetune.HeadLinearFn.apply(feat, w, clipa_amd.engine.WeightCache())
    assert tuple(logits.shape) == (B, Cn) and logits.stride(0) == 16          # the [B, C] view of the padded product
    loss = clipa_amd.soft_target_cross_entropy(logits, ya, yb, lam, smoothing=0.1)
    (3.0 * loss).backward()
    # fp64 autograd on the bf16-rounded operands the head multiplies
    f64 = feat.detach().to(torch.bfloat16).double().requires_grad_(True)
    w64 = w.detach().to(torch.bfloat16).double().requires_grad_(True)
    z = f64 @ w64.T
    t = torch.zeros(B, Cn, dtype=torch.float64)
    t[torch.arange(B), ya] += lam.double()
    t[torch.arange(B), yb] += 1 - lam.double()
    t = 0.9 * t + 0.1 / Cn
    ref = (torch.logsumexp(z, 1) - (t * z).sum(1)).mean()
    (3.0 * ref).backward()
    assert abs(float(loss.detach()) - float(ref.detach())) < 1e-5 * float(ref.detach())
    assert (logits.detach().double() - z.detach()).abs().max() < 1e-5
    assert C.rel_l2(feat.grad, f64.grad) < 8e-3 and C.rel_l2(w.grad, w64.grad) < 8e-3      # dlogits and its operand are bf16
    assert feat.grad.dtype == torch.float32 and w.grad.dtype == torch.float32 and tuple(w.grad.shape) == (Cn, E)
    # hard labels, no gradient wanted, the module form
    hard = clipa_amd.SoftTargetCrossEntropy()(logits.detach(), ya)
    assert abs(float(hard) - float(torch.nn.functional.cross_entropy(z.detach(), ya))) < 1e-5
    mod = clipa_amd.SoftTargetCrossEntropy(0.1)(logits.detach(), (ya, yb, lam))
    assert float(mod) == float(loss.detach())
    with pytest.raises(RuntimeError, match="come together"):
        clipa_amd.soft_target_cross_entropy(logits, ya, yb)
    # a frozen head: no weight gradient, the feature gradient unchanged
    w.requires_grad_(False)
    f2 = feat.detach().clone().requires_grad_(True)
    clipa_amd.soft_target_cross_entropy(finetune.HeadLinearFn.apply(f2, w, clipa_amd.engine.WeightCache()), ya, yb, lam, 0.1).backward()
    assert C.rel_l2(f2.grad * 3.0, feat.grad) < 8e-3                  # 3 dlogits and dlogits round to bf16 apart


@pytest.mark.parametrize("name", C.MODEL_CASES)
def test_engine_on_standins_matches_oracle(name, standins):
    """One step with mixup targets: logits, loss and every tower gradient against the fp32 oracle at the figures of
    tests/test_model_gpu.py; prints the relative L2 error of the head's weight and feature gradients of this bf16 restatement:
    the figures behind the GPU test's bounds (tests/finetune_cases.py states them)."""
    from .test_model_gpu import _compare_gradients
    t = C.toy(name)
    m = C.build_classifier(t)
    logits, f, loss, got, df = C.engine_step(m, t)
    rl, rf, rloss, ref, rdf = C.oracle_step(t)
    assert (logits - rl).abs().max() < 2e-2 * max(1.0, float(rl.abs().max()))
    assert abs(float(loss) - rloss) < 2e-2 * rloss
    assert sorted(got) == sorted(ref)
    _compare_gradients(got, ref, name + " (stand-ins)")
    dw, dfe = C.rel_l2(got["head.weight"], ref["head.weight"]), C.rel_l2(df, rdf)
    print(f"[{name}] bf16 restatement on the stand-ins: relative L2 error of d head.weight {dw:.5f}, of d features {dfe:.5f}")
    assert 0.5 * C.HEAD_DW_MEASURED_CPU[name] <= dw <= C.HEAD_DW_MEASURED_CPU[name], "tests/finetune_cases.py states another figure"
    assert 0.5 * C.HEAD_DF_MEASURED_CPU[name] <= dfe <= C.HEAD_DF_MEASURED_CPU[name], "tests/finetune_cases.py states another figure"


def test_oracle_trajectory_falls_below_a_quarter():
    """Ten AdamW steps of the fp32 oracle on the fixed batch: the loss falls below a quarter of the first, so the GPU test's
    'below half' has room."""
    t = C.toy("plain10")
    sd = {k: v.clone() for k, v in t["sd"].items() if k.startswith("visual.")}
    head = t["head"].clone()
    params = [p.requires_grad_(True) for p in list(sd.values()) + [head]]
    opt = torch.optim.AdamW(params, lr=C.TRAIN_LR, betas=(0.9, 0.95), eps=1e-6, weight_decay=0.0)
    losses = []
    for _ in range(10):
        opt.zero_grad(set_to_none=True)
        _, _, loss, grads, _ = C.oracle_step(t, sd, head)
        for k, p in sd.items():
            p.grad = grads.get(k)
        head.grad = grads["head.weight"]
        opt.step()
        losses.append(loss)
    print("oracle trajectory:", [round(v, 4) for v in losses])
    assert losses[-1] < 0.25 * losses[0]


def test_evaluate_classification_on_standins(standins):
    t = C.toy("plain10", B=16)
    m = C.build_classifier(t)
    labels = t["ya"].long()
    batches = [(t["images"][:8], labels[:8]), (t["images"][8:], labels[8:])]
    got = clipa_amd.evaluate_classification(m, batches)
    assert m.training and m.visual.training                          # the previous mode is back
    C.check_evaluation(m, t, got)
    for bad in (labels[:8] + 10, torch.full((8,), -1)):
        with pytest.raises(RuntimeError, match="outside"):
            clipa_amd.evaluate_classification(m, [(t["images"][:8], bad)])
    with pytest.raises(RuntimeError, match="no batches"):
        clipa_amd.evaluate_classification(m, [])
