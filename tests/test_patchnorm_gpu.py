"""Dual PatchNorm (input_patchnorm, open_clip/transformer.py:362-371,483-489) on the device: the three kernels of
csrc/patchnorm.hip against the case tables of tests/patchnorm_cases.py, and the engine with the LayerNorm's affine folded into
the stem GEMM against the fixtures the real reference generated (tests/golden/patchnorm_*.npz, tools/make_patchnorm_golden.py;
gamma of magnitude 0.5 - 1.5 and mixed sign, beta up to 0.5, a non-zero Linear bias, so a wrong fold cannot hide behind the
init values).

patchify_ln: |got - ref| <= 2^-7 |ref| + KAPPA against the fp64 restatement of the same statistics.  bf16 rounds to 2^-9
relative; KAPPA is the absolute term for values near zero: twice the worst error that the fp32 torch stand-in of the kernel's
statistics (tests/patchnorm_cpu_ops.py: xhat) shows against fp64 over the whole case table, computed on the CPU by kappa() below
and never taken from the kernel.  kappa() gives 1.46e-6; KAPPA states it rounded up to 1.5e-6, and tests/test_patchnorm_cpu.py
checks the statement against kappa().

fold / unfold: exact-sum inputs, compared bit for bit.

The model: the helpers and figures of tests/test_model_gpu.py (features 2e-2, loss 2 %, per-tensor gradient cosine 0.99 and norm
within 5 %; the bf16-parameter mode 0.99 / 8 %) and tests/test_fp8_gpu.py (_check_fp8_model with
test_fp8_model_matches_reference_golden's figures), which see patchnorm_cases.PatchNormOracle in place of the oracle.  dgamma and
dbeta are sums over every patch of the batch and had no precedent, so besides the cosine / norm check they get a bound on the
relative L2 error |d - ref| / |ref| against the fp32 oracle (fp32 parameters): twice what the bf16 restatement of the stem on the
CPU stand-ins measures (tests/test_patchnorm_cpu.py prints it): dgamma 0.02145 / dbeta 0.01474 on patchnorm_cls_erf, 0.01550 /
0.02392 on patchnorm_p14_gap -> DGAMMA_MEASURED_CPU = 0.0215, DBETA_MEASURED_CPU = 0.0240, the bounds 0.0430 and 0.0480
(DESIGN 3).  The engine on an MI355X measures dgamma 0.01959 / dbeta 0.01351 and 0.01528 / 0.02601 on the two fixtures."""
import pytest
import torch

import clipa_amd
from clipa_amd import ops

from . import patchnorm_cases as C
from . import test_fp8_gpu as F
from . import test_model_gpu as M

pytestmark = pytest.mark.gpu
DEV = "cuda"

KAPPA = 1.5e-6
DGAMMA_MEASURED_CPU, DBETA_MEASURED_CPU = 0.0215, 0.0240
DGAMMA_TOL, DBETA_TOL = 2 * DGAMMA_MEASURED_CPU, 2 * DBETA_MEASURED_CPU


def kappa():
    """Twice the worst |fp32 stand-in - fp64| of xhat over the case table (CPU)."""
    worst = 0.0
    for c in C.PATCHIFY:
        _, img64, _ = C.patchify_input(c)
        worst = max(worst, C.patchify_reference(c, img64)[1])
    return 2 * worst


# ---- kernels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.PATCHIFY, ids=C.names(C.PATCHIFY))
def test_patchify_ln(case):
    C.check_patchify_ln(ops, DEV, case, KAPPA)


def test_patchify_ln_matches_patchify_geometry():
    """The same element order as patchify: un-normalising xhat with the row's own statistics gives patchify's matrix back."""
    c = dict(P=16, S=40, B=2, layout="u8_nhwc", norm="openai")
    t, _, _ = C.patchify_input(c)
    mean, std = C.NORMS["openai"]
    x = ops.patchify(t.to(DEV), 16, 768, mean, std).float()
    xh = ops.patchify_ln(t.to(DEV), 16, 768, mean, std).float()
    ref = torch.nn.functional.layer_norm(x, (768,), None, None, 1e-5)
    assert (xh - ref).abs().max() < 0.05


@pytest.mark.parametrize("case", C.FOLD, ids=C.names(C.FOLD))
def test_patchnorm_fold(case):
    C.check_fold(ops, DEV, case)


@pytest.mark.parametrize("case", C.UNFOLD, ids=C.names(C.UNFOLD))
def test_patchnorm_unfold(case):
    C.check_unfold(ops, DEV, case)


def test_wrappers_check_their_arguments():
    C.check_argument_checks(ops, DEV)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        ops.patchify_ln(torch.zeros(1, 3, 16, 16), 8, 192)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.patchnorm_fold(torch.zeros(4, 192), torch.zeros(4), torch.ones(192), torch.zeros(192), 8, 192)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.patchnorm_unfold(torch.zeros(4, 192), torch.zeros(4), torch.zeros(4, 192), torch.ones(192), torch.zeros(192), 8)


def test_unfold_is_reproducible_on_random_data():
    """Fixed summation order, no atomics: the same bits on every run, also where the sums are not exact."""
    gen = torch.Generator().manual_seed(5)
    N, P, K, Kp = 300, 14, 588, 592
    g, w = torch.randn(N, Kp, generator=gen).to(DEV), torch.randn(N, K, generator=gen).to(DEV)
    s, gamma, beta = torch.randn(N, generator=gen).to(DEV), torch.randn(K, generator=gen).to(DEV), torch.randn(K, generator=gen).to(DEV)
    a = ops.patchnorm_unfold(g, s, w, gamma, beta, P)
    for x, y in zip(a, ops.patchnorm_unfold(g, s, w, gamma, beta, P)):
        assert torch.equal(x, y)
    for x, r in zip(a, C.S.patchnorm_unfold(g.cpu(), s.cpu(), w.cpu(), gamma.cpu(), beta.cpu(), P)):
        assert (x.cpu().double() - r.double()).abs().max() < 1e-4 * r.abs().max()


# ---- the model ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def patchnorm_oracle(monkeypatch):
    """The helpers of test_model_gpu / test_fp8_gpu with the PatchNorm stem restated in front of the oracle they call."""
    monkeypatch.setattr(M, "O", C.PatchNormOracle())
    monkeypatch.setattr(F, "O", C.PatchNormOracle())


@pytest.fixture(params=C.MODEL_CASES)
def pn_golden(request):
    return C.load(request.param)


def test_fp32_forward_loss_match_reference_golden(pn_golden, patchnorm_oracle):
    M._check_forward_loss(pn_golden)


def test_fp32_every_gradient_matches_reference(pn_golden, patchnorm_oracle):
    g = pn_golden
    M._check_gradients(g)               # every parameter, the stem's among them (grad_names is the reference's list)
    m = M._engine(g)
    M._step(m, g)
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert C.PN_W in got and C.PN_B in got and C.CONV_B in got
    _, ref, _, _ = C.oracle_grads(g)
    dg, db = C.affine_grad_error(got, ref)
    print(f"[{g.name}] relative L2 error of dgamma {dg:.5f} (bound {DGAMMA_TOL:.4f}), of dbeta {db:.5f} (bound {DBETA_TOL:.4f})")
    assert dg < DGAMMA_TOL and db < DBETA_TOL, (dg, db)
    # and the real reference's own full arrays of the stem
    for k, r in g.stem_grads.items():
        a = got[k].double().cpu().reshape(-1)
        assert float(torch.dot(a, r.double().reshape(-1)) / (a.norm() * r.double().norm())) > 0.99, k


def test_bf16_mode_matches_oracle(pn_golden, patchnorm_oracle):
    """precision="bf16": the Linear bf16, the LayerNorm fp32; the unfold kernel reads the bf16 matrix and writes the bf16 weight
    gradient.  The check of test_full_dims_bf16_mode_matches_oracle (the oracle on the bf16-rounded weights, 2e-2 / 2 % / 0.99 /
    8 %) at the fixture."""
    g = pn_golden
    m, sd = M._bf16_mode_state(g)
    assert m.state_dict()[C.CONV_W].dtype == torch.bfloat16 and m.state_dict()[C.PN_W].dtype == torch.float32
    out, loss = M._step(m, g)
    ref_loss, ref, fi, ft = C.oracle_grads(g, sd)
    i, t = out["image_features"].float().cpu(), out["text_features"].float().cpu()
    assert (i - fi).abs().max() < 2e-2 and (t - ft).abs().max() < 2e-2
    assert abs(float(loss) - ref_loss) < 2e-2 * ref_loss
    got = {}
    for k, p in m.named_parameters():
        if p.grad is not None:
            assert p.grad.dtype == p.dtype, k
            got[k] = p.grad
    assert sorted(got) == sorted(ref)
    M._compare_gradients(got, ref, g.name + " bf16 mode", norm_rtol=0.08)


def test_fp8_model_matches_reference_golden(pn_golden, patchnorm_oracle):
    """precision="fp8" (the stem itself stays on the bf16 GEMMs): test_fp8_gpu's toy-golden check and figures, unchanged."""
    F._check_fp8_model(pn_golden, 6e-2, 0.04, 0.95, 0.97, 0.22)


def test_recompute_equals_stored_activations():
    """grad_checkpointing on and off: the stem recomputes xhat in its backward either way, and the loss and every gradient agree
    bit for bit; a second run of the same model gives the same bits again (no atomics in the unfold)."""
    g = C.load("patchnorm_p14_gap")

    def run(recompute):
        m = M._engine(g, recompute=recompute)
        _, loss = M._step(m, g)
        first = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
        _, loss2 = M._step(m, g)
        assert float(loss) == float(loss2) and all(torch.equal(v, dict(m.named_parameters())[k].grad) for k, v in first.items())
        return float(loss), first

    a, b = run(True), run(False)
    assert a[0] == b[0] and C.PN_W in a[1]
    for k, v in a[1].items():
        assert torch.equal(v, b[1][k]), k


def test_optimizer_steps_and_data_writes_reach_the_folded_operands():
    """Two AdamW steps change gamma, beta, W and b: the forward after them is the forward of a fresh model with the stepped
    weights, bit for bit.  A `p.data` write bumps no version counter: it is seen after invalidate_weight_cache()."""
    g = C.load("patchnorm_cls_erf")
    m = M._engine(g)
    img, txt = g.images_u8.to(DEV), g.texts.to(DEV)
    opt = M._reference_adamw(m, 1e-3)
    keys = (C.PN_W, C.PN_B, C.CONV_W, C.CONV_B)
    before = {k: m.state_dict()[k].clone() for k in keys}
    for _ in range(2):
        M._train_step(m, opt, img, txt)
    assert all(not torch.equal(before[k], m.state_dict()[k]) for k in keys)

    def fresh_forward():
        f = clipa_amd.CLIP(**g.cfg, output_dict=True)
        f.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
        with torch.no_grad():
            return f.to(DEV)(img, txt)

    with torch.no_grad():
        out, ref = m(img, txt), fresh_forward()
        assert torch.equal(out["image_features"], ref["image_features"])
        for p in (m.visual.patchnorm_pre_ln.weight, m.visual.patchnorm_pre_ln.bias, m.visual.conv1.weight, m.visual.conv1.bias):
            p.data.mul_(-1.5)
            stale = m(img, txt)
            assert torch.equal(stale["image_features"], out["image_features"])          # the cached fold: documented contract
            m.invalidate_weight_cache()
            out, ref = m(img, txt), fresh_forward()
            assert not torch.equal(out["image_features"], stale["image_features"])
            assert torch.equal(out["image_features"], ref["image_features"])


def test_reference_state_dict_loads_strictly():
    for name in C.MODEL_CASES:
        g = C.load(name)
        m = clipa_amd.CLIP(**g.cfg, output_dict=True).to(DEV)
        assert list(m.state_dict()) == [str(k) for k in g.z["keys"]]
        assert m.load_state_dict(g.sd, strict=True).missing_keys == []


def test_lock_image_tower():
    """Every group unlocked: patchnorm_pre_ln alone stays frozen (transformer.py:420-426) and gets no gradient; every gradient
    that is computed is the unfrozen model's bit for bit."""
    g = C.load("patchnorm_cls_erf")
    full = M._engine(g)
    M._step(full, g)
    ref = {k: p.grad.clone() for k, p in full.named_parameters()}
    m = M._engine(g)
    m.lock_image_tower(unlocked_groups=4)
    M._step(m, g)
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert sorted(set(ref) - set(got)) == sorted((C.PN_W, C.PN_B))
    for k, v in got.items():
        assert torch.equal(v, ref[k]), k


def test_patch_dropout_with_patchnorm():
    """patch_dropout > 0 together with patchnorm: the kept indices are drawn as the reference draws them, and the step matches
    the oracle run with the same indices (features 2e-2, loss 2 %, gradients 0.99 / 5 %)."""
    from clipa_amd.model import patch_dropout_indices
    g = C.load("patchnorm_cls_erf")
    cfg = dict(g.cfg, vision_cfg=dict(g.cfg["vision_cfg"], patch_dropout=0.5))
    m = clipa_amd.CLIP(**cfg, output_dict=True)
    m.load_state_dict(g.sd, strict=True)
    m.to(DEV).train()
    m.set_grad_checkpointing(True)
    torch.manual_seed(99)
    keep = patch_dropout_indices(g.images_u8.shape[0], 9, 0.5)
    torch.manual_seed(99)
    out, loss = M._step(m, g)
    ref_loss, ref, fi, _ = C.oracle_grads(g, patch_keep=keep)
    assert (out["image_features"].float().cpu() - fi).abs().max() < 2e-2 and abs(float(loss) - ref_loss) < 2e-2 * ref_loss
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert sorted(got) == sorted(ref)
    M._compare_gradients(got, ref, "patchnorm + patch dropout")


def test_vit_b_16_patchnorm_runs_a_step():
    """The built-in config through the factory: one training step at batch 4, finite loss and gradients, every stem parameter
    moved by the optimizer."""
    torch.manual_seed(0)
    m = clipa_amd.create_model("ViT-B-16-patchnorm", device=DEV, output_dict=True)
    m.set_grad_checkpointing(True)
    img, txt = C.O.synthetic_batch(4, 224, 77, 49408, seed=3)
    opt = M._reference_adamw(m, 1e-4)
    before = {k: m.state_dict()[k].clone() for k in (C.PN_W, C.PN_B, C.CONV_W, C.CONV_B)}
    opt.zero_grad(set_to_none=True)
    out = m(img.to(DEV).contiguous(memory_format=torch.channels_last), txt.to(DEV))
    loss = clipa_amd.ClipLoss()(**out, output_dict=True)["contrastive_loss"]
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(out["image_features"]).all()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert all(float(dict(m.named_parameters())[k].grad.abs().max()) > 0 for k in before)
    opt.step()
    torch.cuda.synchronize()
    assert all(not torch.equal(v, m.state_dict()[k]) for k, v in before.items())
