"""LayerScale without a GPU: the case table of tests/layerscale_cases.py through the torch stand-ins of
tests/layerscale_cpu_ops.py (so the stand-ins keep the contract tests/test_layerscale_gpu.py holds the kernels to), and the
engine's LayerScale path - folded operands, the multi-tensor weight cache, the unfold after the weight gradients, the two extra
gradients - on those stand-ins against the fixtures the real reference generated.  Host-side properties that need no kernel
(state_dict keys, lock, the config registry, the C entries' argument errors) are checked here too."""
import pytest
import torch

import clipa_amd
from clipa_amd import lib

from . import layerscale_cases as C
from . import layerscale_cpu_ops as cpu_ops

DEV = "cpu"


@pytest.mark.parametrize("case", C.UNFOLD, ids=C.names(C.UNFOLD))
def test_layerscale_unfold(case):
    C.check_unfold(cpu_ops, DEV, case)


@pytest.mark.parametrize("case", C.FOLD, ids=C.names(C.FOLD))
def test_layerscale_fold(case):
    C.check_fold(cpu_ops, DEV, case)


def test_capi_argument_errors():
    """The C entries report bad arguments through the return code and clipa_last_error (no launch, no GPU needed)."""
    h = lib.load()
    one = torch.zeros(8)
    p = one.data_ptr()
    assert h.clipa_layerscale_fold(None, 1, p, p, p, p, 1, 8, None) < 0 and "layerscale_fold: null operand" in lib.last_error()
    assert h.clipa_layerscale_fold(p, 1, p, None, p, p, 1, 8, None) < 0 and "layerscale_fold: null operand" in lib.last_error()
    assert h.clipa_layerscale_fold(p, 1, p, p, p, p, 1, 0, None) < 0 and "K=0" in lib.last_error()
    assert h.clipa_layerscale_fold(p, 1, p, p, p, p, 0, 8, None) == 0
    assert h.clipa_layerscale_unfold(None, p, 1, p, p, p, p, 1, None, None, 1, 8, None) < 0
    assert "layerscale_unfold: null operand" in lib.last_error()
    assert h.clipa_layerscale_unfold(p, p, 1, p, None, p, None, 1, None, p, 1, 8, None) < 0 and "only the outputs" in lib.last_error()
    assert h.clipa_layerscale_unfold(p, p, 1, p, p, p, p, 1, None, None, 1, 0, None) < 0 and "K=0" in lib.last_error()
    assert h.clipa_layerscale_unfold(p, p, 1, p, p, p, None, 1, None, None, 1, 8, None) == 0      # nothing wanted


# ---- host side of the model -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.MODEL_CASES)
def test_state_dict_interchanges_with_the_reference(name):
    """The key set, shapes and dtypes are the reference's (stored in the fixture), `...resblocks.N.ls_1.gamma` included; the
    reference's state dict loads strictly, and this model's loads back into a fresh one."""
    g = C.load(name)
    m = clipa_amd.CLIP(**g.cfg, output_dict=True)
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in g.z["keys"]]
    assert {k: tuple(v.shape) for k, v in sd.items()} == g.shapes
    for k in g.gammas:
        assert sd[k].dtype == torch.float32 and torch.equal(sd[k], torch.full_like(sd[k], 1e-4))
    m.load_state_dict(g.sd, strict=True)
    m2 = clipa_amd.CLIP(**g.cfg, output_dict=True)
    m2.load_state_dict(m.state_dict(), strict=True)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, g.sd[k]), k
    # LayerScale in the image tower only: the text tower holds no gamma
    if "ls_init_value" not in g.cfg["text_cfg"]:
        assert all(k.startswith("visual.") for k in g.gammas)
        assert all(len(b.param_tuple()) == 12 for b in m.transformer.resblocks)
    assert all(len(b.param_tuple()) == 14 for b in m.visual.transformer.resblocks)
    clipa_amd.convert_weights_to_lp(m, torch.bfloat16)          # model.py:329-351 leaves LayerScale in fp32
    assert all(m.state_dict()[k].dtype == torch.float32 for k in g.gammas)


def test_without_layer_scale_nothing_changes():
    g = C.load_golden("cls_erf")
    m = clipa_amd.CLIP(**g.cfg)
    assert list(m.state_dict()) == [str(k) for k in g.z["keys"]]
    assert not any("ls_" in k for k in m.state_dict())
    assert all(len(b.param_tuple()) == 12 for b in list(m.visual.transformer.resblocks) + list(m.transformer.resblocks))


def test_unsupported_neighbours_stay_rejected():
    g = C.load("layerscale_cls_erf")
    for extra in ({"attentional_pool": True}, {"input_patchnorm": True}):
        with pytest.raises(NotImplementedError, match="attentional pool / patchnorm"):
            clipa_amd.CLIP(g.cfg["embed_dim"], dict(g.cfg["vision_cfg"], **extra), g.cfg["text_cfg"])


def test_vit_m_16_alt_is_registered_and_builds():
    cfg = clipa_amd.get_model_config("ViT-M-16-alt")
    assert cfg == {"embed_dim": 384,
                   "vision_cfg": {"image_size": 224, "layers": 12, "width": 512, "patch_size": 16, "ls_init_value": 1e-4},
                   "text_cfg": {"context_length": 77, "vocab_size": 49408, "width": 384, "heads": 6, "layers": 12}}
    m = clipa_amd.create_model("ViT-M-16-alt")
    gammas = {k: v for k, v in m.state_dict().items() if k.endswith(".gamma")}
    assert len(gammas) == 24 and all(k.startswith("visual.") and v.shape == (512,) for k, v in gammas.items())
    assert all(torch.equal(v, torch.full((512,), 1e-4)) for v in gammas.values())


def test_weight_decay_split_puts_gamma_with_the_vectors():
    """training/main.py:311-316: p.ndim < 2 -> no weight decay."""
    m = clipa_amd.CLIP(**C.load("layerscale_cls_erf").cfg)
    exclude = lambda n, p: p.ndim < 2 or "bn" in n or "ln" in n or "bias" in n or "logit_scale" in n
    gam = [n for n, p in m.named_parameters() if n.endswith(".gamma")]
    assert len(gam) == 8 and all(exclude(n, dict(m.named_parameters())[n]) for n in gam)


@pytest.mark.parametrize("unlocked", [0, 1, 2])
def test_lock_freezes_gammas_with_their_block(unlocked):
    m = clipa_amd.CLIP(**C.load("layerscale_cls_erf").cfg)
    m.lock_image_tower(unlocked_groups=unlocked)
    blocks = m.visual.transformer.resblocks
    for i, blk in enumerate(blocks):
        free = unlocked >= 2 and i == len(blocks) - 1          # groups from the back: proj, then [last block, ln_post]
        assert blk.ls_1.gamma.requires_grad == free and blk.ls_2.gamma.requires_grad == free, (unlocked, i)
        assert all(p.requires_grad == free for p in blk.parameters())
    assert all(p.requires_grad for p in m.transformer.parameters())


# ---- the engine path on the stand-ins --------------------------------------------------------------------------------------
@pytest.fixture
def standins():
    restore = cpu_ops.swap_in()
    yield
    restore()


def _model(g, precision="fp32", **tiers):
    m = clipa_amd.CLIP(**g.cfg, output_dict=True)
    m.load_state_dict(g.sd, strict=True)
    if precision != "fp32":
        clipa_amd.convert_weights_to_lp(m, torch.bfloat16)
    for t in (m.visual.transformer, m.transformer):
        t.fp8 = precision == "fp8"
        for k, v in tiers.items():
            setattr(t, k, t.layers if v == "all" else v)
    m.set_grad_checkpointing(True)
    return m


def _step(m, g):
    m.zero_grad(set_to_none=True)
    out = m(g.images_u8, g.texts)
    loss = clipa_amd.ClipLoss()(**out, output_dict=True)["contrastive_loss"]
    loss.backward()
    return out, loss, {k: p.grad for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("name", C.MODEL_CASES)
def test_engine_on_standins_matches_reference_golden(name, standins):
    """Features and loss against the real reference's, every gradient - the gammas too - against the oracle with the scale
    folded in, itself pinned to the reference's gradient digests; tolerances of tests/test_model_gpu.py.  Prints the dgamma
    figure of this bf16 restatement of the block."""
    from .test_model_gpu import _compare_gradients
    g = C.load(name)
    out, loss, got = _step(_model(g), g)
    assert (out["image_features"].float() - g.t("image_features")).abs().max() < 2e-2
    assert (out["text_features"].float() - g.t("text_features")).abs().max() < 2e-2
    assert abs(float(loss) - float(g.t("loss"))) < 2e-2 * float(g.t("loss"))
    ref_loss, ref, _, _ = C.oracle_grads(g)
    assert abs(ref_loss - float(g.t("loss"))) < 3e-5
    names = [str(n) for n in g.z["grad_names"]]
    assert sorted(got) == names and all(k in got for k in g.gammas)
    _compare_gradients(got, ref, name + " (stand-ins)", digest=(names, g.z["grad_norms"]))
    print(f"[{name}] bf16 restatement on the stand-ins: worst dgamma relative error", C.dgamma_error(got, ref))


@pytest.mark.parametrize("precision", ["bf16", "fp8"])
def test_engine_on_standins_low_precision_modes(precision, standins):
    """The wiring of the other two modes (bf16 parameters: the unfold writes bf16 weight gradients; fp8: the folded matrices go
    through the row quantisers): every gradient is there in its parameter's dtype and close to the oracle on the rounded weights."""
    g = C.load("layerscale_cls_erf")
    m = _model(g, precision)
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


@pytest.mark.parametrize("precision", ["fp32", "fp8"])
def test_recompute_tiers_agree_bit_for_bit(precision, standins):
    g = C.load("layerscale_cls_erf")
    runs = [_step(_model(g, precision, **t), g) for t in ({}, {"keep_blocks": "all"}, {"keep_blocks": 1, "medium_blocks": 1})]
    for _, loss, grads in runs[1:]:
        assert float(loss) == float(runs[0][1])
        for k, v in runs[0][2].items():
            assert torch.equal(v, grads[k]), k


def test_folded_operands_follow_gamma(standins):
    """The cached fold is rebuilt when gamma (or W, or b) changes version; a `p.data` write is seen after
    invalidate_weight_cache()."""
    g = C.load("layerscale_cls_erf")
    m = _model(g)
    img = g.images_u8
    with torch.no_grad():
        f0 = m.encode_image(img, normalize=True).clone()
        gam = m.visual.transformer.resblocks[0].ls_2.gamma
        for p in (gam, m.visual.transformer.resblocks[1].attn.out_proj.bias, m.visual.transformer.resblocks[0].mlp.c_proj.weight):
            before = m.encode_image(img, normalize=True).clone()
            p.mul_(0.5)                                            # in place: bumps the version counter
            after = m.encode_image(img, normalize=True)
            assert not torch.equal(before, after)
        fresh = _model(g)
        fresh.load_state_dict(m.state_dict(), strict=True)
        assert torch.equal(fresh.encode_image(img, normalize=True), after)
        gam.data.mul_(2.0)                                         # no version bump: the stale fold is still in use ...
        assert torch.equal(m.encode_image(img, normalize=True), after)
        m.invalidate_weight_cache()                                # ... until the cache is dropped
        f1 = m.encode_image(img, normalize=True)
        assert not torch.equal(f1, after)
        fresh.load_state_dict(m.state_dict(), strict=True)
        assert torch.equal(fresh.encode_image(img, normalize=True), f1)
    assert not torch.equal(f0, f1)


def test_locked_tower_gammas_get_no_gradient(standins):
    """unlocked_groups=2 frees proj and [last block, ln_post]: of the image tower's gammas only the last block's get a gradient,
    and it is the unfrozen model's."""
    g = C.load("layerscale_cls_erf")
    _, _, ref = _step(_model(g), g)
    m = _model(g)
    m.lock_image_tower(unlocked_groups=2)
    _, _, got = _step(m, g)
    vis = sorted(k for k in got if k.startswith("visual.") and k.endswith(".gamma"))
    assert vis == ["visual.transformer.resblocks.1.ls_1.gamma", "visual.transformer.resblocks.1.ls_2.gamma"]
    for k, v in got.items():
        assert torch.equal(v, ref[k]), k
