"""Dual PatchNorm (input_patchnorm, open_clip/transformer.py:362-371,483-489) without a GPU: the fold / unfold algebra, the
case tables of tests/patchnorm_cases.py through the torch stand-ins of tests/patchnorm_cpu_ops.py (so the stand-ins keep the
contract tests/test_patchnorm_gpu.py holds the kernels to), PatchNormOracle against the fixtures the real reference generated
(tests/golden/patchnorm_*.npz, tools/make_patchnorm_golden.py), the module surface (state dict, strict load, lock) and the
engine's PatchNorm stem on the stand-ins - whose error on dgamma / dbeta against the fp32 oracle is the figure the GPU test's
bound is built on (it is printed here)."""
import numpy as np
import pytest
import torch

import clipa_amd

from . import patchnorm_cases as C
from . import patchnorm_cpu_ops as cpu_ops
from .test_oracle_cpu import _check_oracle_against_golden


# ---- the algebra ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 3])
def test_fold_unfold_algebra_equals_autograd(P):
    """pe = LayerNorm_K(x; gamma, beta) W^T + b == xhat (W diag(gamma))^T + (b + W beta), and with G = dPE^T xhat, s = colsum(dPE):
    db = s, dW = gamma G + beta s, dgamma = sum_n W G, dbeta = sum_n W s - against autograd of the reference formula, fp64."""
    gen = torch.Generator().manual_seed(P)
    K, N, M = 3 * P * P, 5, 17
    x, dpe = torch.randn(M, K, generator=gen, dtype=torch.float64), torch.randn(M, N, generator=gen, dtype=torch.float64)
    w, b, gamma, beta = (torch.randn(s, generator=gen, dtype=torch.float64).requires_grad_(True) for s in ((N, K), (N,), (K,), (K,)))
    pe = torch.nn.functional.layer_norm(x, (K,), gamma, beta, 1e-5) @ w.T + b
    pe.backward(dpe)
    xhat = torch.nn.functional.layer_norm(x, (K,), None, None, 1e-5)
    with torch.no_grad():
        assert torch.allclose(xhat @ (w * gamma).T + (b + w @ beta), pe, atol=1e-12)
        G, s = dpe.T @ xhat, dpe.sum(0)
        assert torch.allclose(b.grad, s, atol=1e-12)
        assert torch.allclose(w.grad, gamma * G + beta * s[:, None], atol=1e-12)
        assert torch.allclose(gamma.grad, (w * G).sum(0), atol=1e-12)
        assert torch.allclose(beta.grad, (w * s[:, None]).sum(0), atol=1e-12)
        # the stand-ins (and so the kernels' contract) in the engine's column order, Kp > K
        Kp = (K + 7) // 8 * 8
        wf, bf = cpu_ops.patchnorm_fold(w.float(), b.float(), gamma.float(), beta.float(), P, Kp)
        perm = cpu_ops._perm(P)
        assert torch.allclose(wf.double()[:, :K], (w * gamma)[:, perm], rtol=2.0 ** -8) and not wf[:, K:].any()
        assert torch.allclose(bf.double(), b + w @ beta, atol=1e-5)
        Gp = torch.nn.functional.pad(G[:, perm], (0, Kp - K), value=99.0).float()
        dw, dg, db = cpu_ops.patchnorm_unfold(Gp, s.float(), w.float(), gamma.float(), beta.float(), P)
        assert torch.allclose(dw.double(), w.grad, atol=1e-4) and torch.allclose(dg.double(), gamma.grad, atol=1e-4)
        assert torch.allclose(db.double(), beta.grad, atol=1e-4)


@pytest.mark.parametrize("case", C.FOLD, ids=C.names(C.FOLD))
def test_patchnorm_fold_standin(case):
    C.check_fold(cpu_ops, "cpu", case)


@pytest.mark.parametrize("case", C.UNFOLD, ids=C.names(C.UNFOLD))
def test_patchnorm_unfold_standin(case):
    C.check_unfold(cpu_ops, "cpu", case)


def test_patchify_ln_standin_and_kappa():
    """The stand-in through the GPU test's case table, with the GPU test's own absolute term: kappa = twice the worst error of
    the fp32 statistics against fp64 over the table (tests/test_patchnorm_gpu.py states the figure)."""
    from .test_patchnorm_gpu import KAPPA, kappa
    k = kappa()
    print(f"kappa = {k:.3e} (stated {KAPPA:.1e})")
    assert 0.5 * KAPPA <= k <= KAPPA
    for c in C.PATCHIFY:
        C.check_patchify_ln(cpu_ops, "cpu", c, KAPPA)


def test_capi_reports_argument_errors():
    from clipa_amd import lib
    h = lib.load()
    import ctypes
    p = ctypes.c_void_p(16)
    assert h.clipa_patchify_ln(p, p, 1, 16, 8, 196, 0, 0, 0, None, None, 1e-5, None) < 0 and "bad geometry" in lib.last_error()
    assert h.clipa_patchify_ln(p, p, 1, 64, 40, 4800, 0, 0, 0, None, None, 1e-5, None) < 0 and "bad geometry" in lib.last_error()
    assert h.clipa_patchify_ln(p, p, 1, 16, 8, 192, 7, 0, 0, None, None, 1e-5, None) < 0 and "dtype" in lib.last_error()
    assert h.clipa_patchify_ln(p, p, 1, 16, 8, 192, 0, 0, 1, None, None, 1e-5, None) < 0 and "mean/std" in lib.last_error()
    assert h.clipa_patchify_ln(p, p, 0, 16, 8, 192, 0, 0, 0, None, None, 1e-5, None) == 0
    assert h.clipa_patchnorm_fold(None, 1, p, p, p, p, p, 1, 8, 192, None) < 0 and "null operand" in lib.last_error()
    assert h.clipa_patchnorm_fold(p, 1, p, p, p, p, p, 1, 8, 188, None) < 0 and "bad geometry" in lib.last_error()
    assert h.clipa_patchnorm_fold(p, 1, p, p, p, p, p, 0, 8, 192, None) == 0
    assert h.clipa_patchnorm_unfold(p, None, p, 1, p, p, p, 1, p, p, 1, 8, 192, None) < 0 and "only the outputs" in lib.last_error()
    assert h.clipa_patchnorm_unfold(p, p, p, 1, p, p, None, 1, None, None, 1, 8, 192, None) == 0      # nothing wanted


# ---- the oracle against the real reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.MODEL_CASES)
def test_oracle_reproduces_the_fixtures(name, monkeypatch):
    """PatchNormOracle at the tolerances tests/test_oracle_cpu.py holds the oracle to on the other toy goldens (features 3e-6,
    logits 5e-5, loss 1e-5, gradient digests 2e-4), and the stem's full gradients element by element."""
    from . import test_oracle_cpu as T
    monkeypatch.setattr(T, "O", C.PatchNormOracle())
    g = C.load(name)
    _check_oracle_against_golden(g)
    _, grads, _, _ = C.oracle_grads(g)
    assert sorted(g.stem_grads) == sorted(k for k in (C.PN_W, C.PN_B, C.CONV_W, C.CONV_B, "visual.class_embedding",
                                                      "visual.positional_embedding") if k not in g.frozen)
    for k, ref in g.stem_grads.items():
        assert grads[k].shape == ref.shape, k
        assert (grads[k] - ref).abs().max() <= 2e-4 * float(ref.norm()) + 1e-7, k


def test_fixture_stem_tensors_are_not_the_init_values():
    for name in C.MODEL_CASES:
        g = C.load(name)
        gamma, beta, b = g.stem[C.PN_W], g.stem[C.PN_B], g.stem[C.CONV_B]
        assert 0.5 <= float(gamma.abs().min()) and float(gamma.abs().max()) <= 1.5 and 0.3 < float((gamma > 0).float().mean()) < 0.7
        assert 0.3 < float(beta.abs().max()) <= 0.5 and float(b.abs().min()) > 0


# ---- the module surface ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.MODEL_CASES)
def test_state_dict_is_the_references(name):
    """create_model / CLIP with input_patchnorm builds on the CPU; keys, order and shapes are the reference's (the fixture's name
    list), and a reference-shaped dict loads strictly."""
    g = C.load(name)
    m = clipa_amd.CLIP(**g.cfg, output_dict=True)
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in g.z["keys"]]
    assert {k: tuple(v.shape) for k, v in sd.items()} == g.shapes
    P = g.cfg["vision_cfg"]["patch_size"]
    K, D = 3 * P * P, g.cfg["vision_cfg"]["width"]
    assert tuple(sd[C.PN_W].shape) == (K,) and tuple(sd[C.PN_B].shape) == (K,)
    assert tuple(sd[C.CONV_W].shape) == (D, K) and tuple(sd[C.CONV_B].shape) == (D,)
    res = m.load_state_dict(g.sd, strict=True)
    assert res.missing_keys == [] and res.unexpected_keys == []
    assert all(torch.equal(m.state_dict()[k], v) for k, v in g.stem.items())
    # torch's default initialisation, as in the reference: LayerNorm at (1, 0), the Linear uniform within 1 / sqrt(K)
    fresh = clipa_amd.CLIP(**g.cfg).state_dict()
    assert torch.equal(fresh[C.PN_W], torch.ones(K)) and torch.equal(fresh[C.PN_B], torch.zeros(K))
    assert float(fresh[C.CONV_W].abs().max()) <= K ** -0.5 and float(fresh[C.CONV_B].abs().max()) <= K ** -0.5


def test_without_the_flag_nothing_changes():
    g = C.load("patchnorm_cls_erf")
    cfg = dict(g.cfg, vision_cfg={k: v for k, v in g.cfg["vision_cfg"].items() if k != "input_patchnorm"})
    m = clipa_amd.CLIP(**cfg)
    assert not any("patchnorm" in k for k in m.state_dict()) and "visual.conv1.bias" not in m.state_dict()
    assert m.state_dict()[C.CONV_W].dim() == 4 and isinstance(m.visual.patchnorm_pre_ln, torch.nn.Identity)


def test_builtin_config_and_neighbours():
    cfg = clipa_amd.get_model_config("ViT-B-16-patchnorm")
    assert cfg["vision_cfg"] == {"image_size": 224, "layers": 12, "width": 768, "patch_size": 16, "input_patchnorm": True}
    assert cfg["text_cfg"] == clipa_amd.get_model_config("ViT-B-16")["text_cfg"]
    m = clipa_amd.create_model("ViT-B-16-patchnorm")
    assert tuple(m.visual.conv1.weight.shape) == (768, 768) and tuple(m.visual.patchnorm_pre_ln.weight.shape) == (768,)
    with pytest.raises(NotImplementedError, match="attentional pool"):
        clipa_amd.CLIP(cfg["embed_dim"], dict(cfg["vision_cfg"], attentional_pool=True), cfg["text_cfg"])
    with pytest.raises(NotImplementedError, match="input_patchnorm together with ls_init_value"):      # no fixture covers both folds
        clipa_amd.CLIP(cfg["embed_dim"], dict(cfg["vision_cfg"], ls_init_value=1e-4), cfg["text_cfg"])
    clipa_amd.CLIP(cfg["embed_dim"], dict(cfg["vision_cfg"], layers=1), dict(cfg["text_cfg"], layers=1, ls_init_value=1e-4))
    with pytest.raises(NotImplementedError, match="3072"):
        clipa_amd.CLIP(cfg["embed_dim"], dict(cfg["vision_cfg"], patch_size=56), cfg["text_cfg"])


@pytest.mark.parametrize("unlocked", [0, 1, 3, 4])
def test_lock_leaves_patchnorm_pre_ln_frozen(unlocked):
    """transformer.py:415-446: the first group lists conv1, class_embedding, positional_embedding and ln_pre - not
    patchnorm_pre_ln, which therefore stays frozen even when every group is unlocked (2 blocks: 4 groups)."""
    m = clipa_amd.CLIP(**C.load("patchnorm_cls_erf").cfg)
    m.lock_image_tower(unlocked_groups=unlocked)
    v = m.visual
    first = unlocked >= 4
    assert v.conv1.weight.requires_grad == first and v.conv1.bias.requires_grad == first
    assert v.class_embedding.requires_grad == first and v.ln_pre.weight.requires_grad == first
    assert not v.patchnorm_pre_ln.weight.requires_grad and not v.patchnorm_pre_ln.bias.requires_grad
    assert v.proj.requires_grad == (unlocked >= 1)


def test_weight_decay_split():
    """training/main.py:311-316: the LayerNorm affine and the Linear's bias take no weight decay, the Linear's matrix does."""
    m = clipa_amd.CLIP(**C.load("patchnorm_cls_erf").cfg)
    exclude = lambda n, p: p.ndim < 2 or "bn" in n or "ln" in n or "bias" in n or "logit_scale" in n
    named = dict(m.named_parameters())
    assert all(exclude(k, named[k]) for k in (C.PN_W, C.PN_B, C.CONV_B)) and not exclude(C.CONV_W, named[C.CONV_W])


# ---- the engine path on the stand-ins --------------------------------------------------------------------------------------
@pytest.fixture
def standins():
    restore = cpu_ops.swap_in()
    yield
    restore()


def _model(g, precision="fp32", recompute=True):
    m = clipa_amd.CLIP(**g.cfg, output_dict=True)
    m.load_state_dict(g.sd, strict=True)
    if precision != "fp32":
        clipa_amd.convert_weights_to_lp(m, torch.bfloat16)
    for t in (m.visual.transformer, m.transformer):
        t.fp8 = precision == "fp8"
    m.set_grad_checkpointing(recompute)
    return m


def _step(m, g):
    m.zero_grad(set_to_none=True)
    out = m(g.images_u8, g.texts)
    loss = clipa_amd.ClipLoss()(**out, output_dict=True)["contrastive_loss"]
    loss.backward()
    return out, loss, {k: p.grad for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("name", C.MODEL_CASES)
def test_engine_on_standins_matches_reference_golden(name, standins):
    """Features and loss against the real reference's, every gradient against PatchNormOracle, itself pinned to the reference's
    gradient digests; tolerances of tests/test_model_gpu.py.  Prints the relative L2 error of dgamma and dbeta of this bf16
    restatement of the stem against the fp32 oracle: the figures behind tests/test_patchnorm_gpu.py's DGAMMA_TOL / DBETA_TOL (DESIGN)."""
    from .test_model_gpu import _compare_gradients
    g = C.load(name)
    out, loss, got = _step(_model(g), g)
    assert (out["image_features"].float() - g.t("image_features")).abs().max() < 2e-2
    assert (out["text_features"].float() - g.t("text_features")).abs().max() < 2e-2
    assert abs(float(loss) - float(g.t("loss"))) < 2e-2 * float(g.t("loss"))
    ref_loss, ref, _, _ = C.oracle_grads(g)
    assert abs(ref_loss - float(g.t("loss"))) < 3e-5
    names = [str(n) for n in g.z["grad_names"]]
    assert sorted(got) == names
    _compare_gradients(got, ref, name + " (stand-ins)", digest=(names, g.z["grad_norms"]))
    dg, db = C.affine_grad_error(got, ref)
    print(f"[{name}] bf16 restatement on the stand-ins: relative L2 error of dgamma {dg:.5f}, of dbeta {db:.5f}")
    from .test_patchnorm_gpu import DBETA_MEASURED_CPU, DGAMMA_MEASURED_CPU
    assert dg <= DGAMMA_MEASURED_CPU and db <= DBETA_MEASURED_CPU, "tests/test_patchnorm_gpu.py states smaller figures than this run measures"


@pytest.mark.parametrize("precision", ["bf16", "fp8"])
def test_engine_on_standins_low_precision_modes(precision, standins):
    """bf16 parameters (the Linear bf16, the LayerNorm fp32: the unfold writes a bf16 weight gradient) and the fp8 engine (the
    stem stays bf16): every gradient is there in its parameter's dtype and close to the oracle on the rounded weights."""
    g = C.load("patchnorm_cls_erf")
    m = _model(g, precision)
    assert m.visual.conv1.weight.dtype == torch.bfloat16 and m.visual.patchnorm_pre_ln.weight.dtype == torch.float32
    _, loss, got = _step(m, g)
    sd = {k: v.detach().float() for k, v in m.state_dict().items()}
    ref_loss, ref, _, _ = C.oracle_grads(g, sd)
    assert abs(float(loss) - ref_loss) < (0.04 if precision == "fp8" else 0.02) * ref_loss
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == p.dtype, k
        a, b = p.grad.double().reshape(-1), ref[k].double().reshape(-1)
        if a.numel() > 1 and float(b.norm()) > 1e-7:
            cos = float(torch.dot(a, b) / (a.norm() * b.norm()))
            assert cos > (0.9 if precision == "fp8" else 0.99), (k, cos)


def test_recompute_and_frozen_parameters(standins):
    """grad_checkpointing on / off give the same bits; with the reference's lock (every group unlocked) patchnorm_pre_ln gets no
    gradient and every other gradient is the unfrozen model's; a frozen stem computes nothing."""
    g = C.load("patchnorm_cls_erf")
    _, l0, ref = _step(_model(g), g)
    _, l1, kept = _step(_model(g, recompute=False), g)
    assert float(l0) == float(l1) and all(torch.equal(v, kept[k]) for k, v in ref.items())
    m = _model(g)
    m.lock_image_tower(unlocked_groups=4)
    _, _, got = _step(m, g)
    assert C.PN_W not in got and C.PN_B not in got and C.CONV_W in got and C.CONV_B in got
    assert all(torch.equal(v, ref[k]) for k, v in got.items())
    m = _model(g)
    m.lock_image_tower(unlocked_groups=1)
    _, _, got = _step(m, g)
    assert not any(k.startswith("visual.") and k != "visual.proj" for k in got)


def test_folded_operands_follow_the_parameters(standins):
    """The cached fold is rebuilt when gamma, beta, W or b changes version; a `p.data` write is seen after
    invalidate_weight_cache()."""
    g = C.load("patchnorm_p14_gap")
    m = _model(g)
    img = g.images_u8
    v = m.visual
    with torch.no_grad():
        for p in (v.patchnorm_pre_ln.weight, v.patchnorm_pre_ln.bias, v.conv1.weight, v.conv1.bias):
            before = m.encode_image(img, normalize=True).clone()
            p.mul_(0.5)                                            # in place: bumps the version counter
            after = m.encode_image(img, normalize=True)
            assert not torch.equal(before, after)
        fresh = _model(g)
        fresh.load_state_dict(m.state_dict(), strict=True)
        assert torch.equal(fresh.encode_image(img, normalize=True), after)
        v.patchnorm_pre_ln.bias.data.mul_(-2.0)                    # no version bump: the stale fold is still in use ...
        assert torch.equal(m.encode_image(img, normalize=True), after)
        m.invalidate_weight_cache()                                # ... until the cache is dropped
        f1 = m.encode_image(img, normalize=True)
        assert not torch.equal(f1, after)
        fresh.load_state_dict(m.state_dict(), strict=True)
        assert torch.equal(fresh.encode_image(img, normalize=True), f1)


def test_patch_dropout_with_patchnorm(standins):
    """patch_dropout > 0 together with patchnorm: the engine draws the kept indices as the reference does, and matches the oracle
    run with those indices."""
    from clipa_amd.model import patch_dropout_indices
    from .test_model_gpu import _compare_gradients
    g = C.load("patchnorm_cls_erf")
    cfg = dict(g.cfg, vision_cfg=dict(g.cfg["vision_cfg"], patch_dropout=0.5))
    m = clipa_amd.CLIP(**cfg, output_dict=True)
    m.load_state_dict(g.sd, strict=True)
    m.train()
    torch.manual_seed(99)
    keep = patch_dropout_indices(g.images_u8.shape[0], 9, 0.5)
    torch.manual_seed(99)
    out, loss, got = _step(m, g)
    ref_loss, ref, fi, _ = C.oracle_grads(g, patch_keep=keep)
    assert (out["image_features"].float() - fi).abs().max() < 2e-2 and abs(float(loss) - ref_loss) < 2e-2 * ref_loss
    _compare_gradients(got, ref, "patchnorm + patch dropout (stand-ins)")
    assert np.isfinite(float(loss))
