"""Multihead attention pooling (pool_style="big_vision_map") without a GPU: the host side of the model (construction, state_dict
keys, lock groups, low-precision conversion, the config registry, the header), the algebra of the fold in fp64, the case table
of tests/mappool_cases.py through the torch stand-ins of tests/mappool_cpu_ops.py - which must stay inside a quarter of the
bounds tests/test_mappool_gpu.py holds the kernels to, while deliberately wrong variants must fall outside them - and the whole
toy model on those stand-ins against the unfused definition in fp64."""
import os

import pytest
import torch

import clipa_amd
from clipa_amd import lib, model as model_mod

from . import mappool_cases as C
from . import mappool_cpu_ops as cpu_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_KEYS = ["probe", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "ln.weight",
            "ln.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias"]


# ---- host side of the model ---------------------------------------------------------------------------------------------------
def test_map_model_builds_with_the_specified_state_dict():
    m = clipa_amd.CLIP(**C.TOY)
    sd = m.state_dict()
    assert not any(k.startswith("visual.ln_post") for k in sd)
    assert [k[len("visual.map_head."):] for k in sd if k.startswith("visual.map_head.")] == MAP_KEYS
    D, W = 128, 512
    shapes = {"probe": (1, 1, D), "attn.in_proj_weight": (3 * D, D), "attn.in_proj_bias": (3 * D,), "attn.out_proj.weight": (D, D),
              "attn.out_proj.bias": (D,), "ln.weight": (D,), "ln.bias": (D,), "mlp.c_fc.weight": (W, D), "mlp.c_fc.bias": (W,),
              "mlp.c_proj.weight": (D, W), "mlp.c_proj.bias": (D,)}
    assert {k: tuple(sd["visual.map_head." + k].shape) for k in MAP_KEYS} == shapes
    # initialisation: xavier-uniform matrices and probe (bounded by sqrt(6 / (fan_in + fan_out)), not all zero), zero biases, LN 1 / 0
    h = m.visual.map_head
    for t, fan in ((h.probe, 2 * D), (h.attn.in_proj_weight[:D], 2 * D), (h.attn.in_proj_weight[D:2 * D], 2 * D),
                   (h.attn.in_proj_weight[2 * D:], 2 * D), (h.attn.out_proj.weight, 2 * D), (h.mlp.c_fc.weight, D + W),
                   (h.mlp.c_proj.weight, D + W)):
        bound = (6.0 / fan) ** 0.5
        assert 0.8 * bound < float(t.detach().abs().max()) <= bound
    for b in (h.attn.in_proj_bias, h.attn.out_proj.bias, h.mlp.c_fc.bias, h.mlp.c_proj.bias, h.ln.bias):
        assert torch.equal(b, torch.zeros_like(b))
    assert torch.equal(h.ln.weight, torch.ones(D))
    # every other key of the model is the CLS model's
    other = clipa_amd.CLIP(C.TOY["embed_dim"], dict(C.TOY["vision_cfg"], pool_style="open_clip"), C.TOY["text_cfg"])
    assert [k for k in sd if ".map_head." not in k] == [k for k in other.state_dict() if ".ln_post." not in k]


def test_other_pool_styles_are_unchanged():
    from .layerscale_cases import load_golden
    g = load_golden("cls_erf")
    m = clipa_amd.CLIP(**g.cfg)
    assert list(m.state_dict()) == [str(k) for k in g.z["keys"]]
    assert not hasattr(m.visual, "map_head") and "visual.ln_post.weight" in m.state_dict()


def test_vit_b_16_map_bigvision_is_registered_and_builds():
    cfg = clipa_amd.get_model_config("ViT-B-16-MAP-BigVision")
    base = clipa_amd.get_model_config("ViT-B-16")
    assert cfg["text_cfg"] == base["text_cfg"] and cfg["embed_dim"] == base["embed_dim"]
    assert cfg["vision_cfg"] == dict(base["vision_cfg"], pool_style="big_vision_map", gelu_approximate="tanh")
    m = clipa_amd.create_model("ViT-B-16-MAP-BigVision")
    assert m.visual.pool_style == "big_vision_map" and m.visual.map_head.probe.shape == (1, 1, 768)
    assert m.visual.map_head.mlp.c_fc.weight.shape == (3072, 768) and m.visual.transformer.act == clipa_amd.ops.ACT_GELU_TANH


def test_global_average_pool_with_map_is_refused():
    with pytest.raises(ValueError, match="global_average_pool"):
        clipa_amd.CLIP(C.TOY["embed_dim"], dict(C.TOY["vision_cfg"], global_average_pool=True), C.TOY["text_cfg"])
    with pytest.raises(ValueError):
        clipa_amd.CLIP(C.TOY["embed_dim"], dict(C.TOY["vision_cfg"], pool_style="big_vision_mapp"), C.TOY["text_cfg"])


@pytest.mark.parametrize("unlocked", [0, 1, 2, 3])
def test_lock_groups_put_map_head_with_the_last_block(unlocked):
    m = clipa_amd.CLIP(**C.TOY)
    m.lock_image_tower(unlocked_groups=unlocked)
    v = m.visual
    assert v.proj.requires_grad == (unlocked >= 1)
    assert all(p.requires_grad == (unlocked >= 2) for p in v.map_head.parameters())
    assert all(p.requires_grad == (unlocked >= 2) for p in v.transformer.resblocks[-1].parameters())
    assert all(p.requires_grad == (unlocked >= 3) for p in v.transformer.resblocks[0].parameters())
    assert not v.conv1.weight.requires_grad and all(p.requires_grad for p in m.transformer.parameters())


def test_convert_weights_to_lp_dtypes():
    m = clipa_amd.CLIP(**C.TOY)
    clipa_amd.convert_weights_to_lp(m, torch.bfloat16)
    sd = m.state_dict()
    fp32 = {"probe", "ln.weight", "ln.bias"}
    for k in MAP_KEYS:
        assert sd["visual.map_head." + k].dtype == (torch.float32 if k in fp32 else torch.bfloat16), k
    assert sd["visual.class_embedding"].dtype == torch.float32 and sd["visual.proj"].dtype == torch.bfloat16


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "clipa_hip.h")).read()
    for name in ("clipa_mappool_fwd", "clipa_mappool_bwd", "clipa_mappool_bwd_workspace"):
        assert f"{name}(" in text and name in lib.SIGNATURES
    doc = text[:text.index("int64_t clipa_mappool_bwd_workspace(")]
    assert "clipa_jax/models/vit.py:187-207" in doc[doc.rindex("/*"):]
    assert "vit.py:187-207" in open(os.path.join(ROOT, "clipa_amd", "lib.py")).read()


def test_capi_argument_errors_and_zero_batch():
    """The C entries refuse unsupported shapes through the return code (no launch, no GPU needed); B = 0 returns OK."""
    h = lib.load()
    buf = torch.zeros(64)
    p = buf.data_ptr()
    assert p % 16 == 0
    assert h.clipa_mappool_fwd(p, p, p, p, 1, 1, 128, 17, 128, 0, None) < 0 and "H = 17" in lib.last_error()
    assert h.clipa_mappool_fwd(p, p, p, p, 1, 1, 128, 0, 128, 0, None) < 0 and "H = 0" in lib.last_error()
    assert h.clipa_mappool_fwd(p, p, p, p, 1, 1, 96, 2, 96, 0, None) < 0 and "D = 96" in lib.last_error()
    assert h.clipa_mappool_fwd(p, p, p, p, 1, 1, 2112, 2, 2112, 0, None) < 0 and "D = 2112" in lib.last_error()
    assert h.clipa_mappool_fwd(p, p, p, p, 1, 0, 128, 2, 128, 0, None) < 0 and "L = 0" in lib.last_error()
    assert h.clipa_mappool_fwd(p, p, p, p, 1, 1, 128, 2, 64, 0, None) < 0 and "row stride" in lib.last_error()
    assert h.clipa_mappool_fwd(p + 2, p, p, p, 1, 1, 128, 2, 128, 0, None) < 0 and "16-byte aligned" in lib.last_error()
    assert h.clipa_mappool_fwd(p, p, p, p, 0, 1, 128, 2, 128, 0, None) == 0
    assert h.clipa_mappool_bwd(p, p, p, p, p, p, p, 1, 1, 128, 17, 128, 128, 0, p, 1 << 30, None) < 0 and "H = 17" in lib.last_error()
    assert h.clipa_mappool_bwd(p, p, p, p, p, p, p, 1, 1, 128, 2, 128, 128, 0, p, 16, None) < 0 and "workspace" in lib.last_error()
    assert h.clipa_mappool_bwd_workspace(5, 2, 128, 2) == 128 * 32 + 5 * 128 * 32 + 2 * 2 * 128 * 4
    assert h.clipa_mappool_bwd_workspace(5, 2, 128, 0) == 128 * 32 + 5 * 128 * 32 + 5 * 2 * 128 * 4


def test_standins_refuse_unsupported_shapes():
    x, u = torch.zeros(4, 96, dtype=torch.bfloat16), torch.zeros(2, 96, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="D=96"):
        cpu_ops.mappool_fwd(x, u, 2, 2, 2)
    with pytest.raises(RuntimeError, match="H=17"):
        cpu_ops.mappool_fwd(torch.zeros(4, 128, dtype=torch.bfloat16), torch.zeros(17, 128, dtype=torch.bfloat16), 2, 2, 17)


# ---- the algebra of the fold, fp64 -----------------------------------------------------------------------------------------------
def test_fold_equals_the_unfused_head_in_fp64():
    """Outputs and every gradient of the folded head agree with torch's multi_head_attention_forward restatement to 1e-10; the K
    bias has no gradient at all in the fold (it never enters) and ~1e-17 in the unfused head: the bk . q term cancels."""
    torch.manual_seed(3)
    B, L, D, H, E = 3, 7, 24, 3, 10
    pre = "h."
    shapes = {"probe": (1, 1, D), "attn.in_proj_weight": (3 * D, D), "attn.in_proj_bias": (3 * D,), "attn.out_proj.weight": (D, D),
              "attn.out_proj.bias": (D,), "ln.weight": (D,), "ln.bias": (D,), "mlp.c_fc.weight": (2 * D, D),
              "mlp.c_fc.bias": (2 * D,), "mlp.c_proj.weight": (D, 2 * D), "mlp.c_proj.bias": (D,)}
    base = {pre + k: torch.randn(s, dtype=torch.float64) * 0.5 for k, s in shapes.items()}
    x0, proj0, dout = torch.randn(B, L, D, dtype=torch.float64), torch.randn(D, E, dtype=torch.float64), torch.randn(B, E, dtype=torch.float64)
    res = []
    for fn in (C.head_unfused, C.head_folded):
        sd = {k: v.clone().requires_grad_(True) for k, v in base.items()}
        x, proj = x0.clone().requires_grad_(True), proj0.clone().requires_grad_(True)
        out = fn(x, sd, pre, H, "gelu_tanh", proj)
        out.backward(dout)
        res.append((out.detach(), x.grad, proj.grad, {k: v.grad for k, v in sd.items()}))
    (o1, dx1, dp1, g1), (o2, dx2, dp2, g2) = res
    assert (o1 - o2).abs().max() < 1e-10 and (dx1 - dx2).abs().max() < 1e-10 and (dp1 - dp2).abs().max() < 1e-10
    for k in g1:
        assert (g1[k] - g2[k]).abs().max() < 1e-10, k
    dbk = g2[pre + "attn.in_proj_bias"][D:2 * D]
    assert torch.equal(dbk, torch.zeros_like(dbk)) and g1[pre + "attn.in_proj_bias"][D:2 * D].abs().max() < 1e-12
    assert g2[pre + "attn.in_proj_bias"][:D].abs().max() > 1e-3 and g2[pre + "attn.in_proj_bias"][2 * D:].abs().max() > 1e-3


# ---- the stand-ins on the case table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.TABLE, ids=C.names(C.TABLE))
def test_standins_within_a_quarter_of_the_bounds(case):
    """kappa = 4 x the stand-in's worst normalised error: every case stays within kappa / 4 (and z within its stated bound)."""
    C.check(cpu_ops, "cpu", case, kdx=C.KAPPA_DX / 4, kdu=C.KAPPA_DU / 4)


@pytest.mark.parametrize("case", C.ROUTED, ids=C.names(C.ROUTED))
def test_routed_expectations_are_proven(case):
    """The expectation itself, before the kernel is held to it: in fp64 every winner leads by more than 104, fp32's exp of such a
    gap is exactly zero, the fp64 outputs agree with the expected ones to 1e-40 relative, and the stand-in gives them bit for bit."""
    inp, win, z_want, dx_want = C.routed(case)
    B, L, D, H = case["B"], case["L"], case["D"], case["H"]
    x = inp["x"].double().reshape(B, L, D)
    s = torch.einsum("bld,hd->blh", x, inp["u"].double())
    top = s.gather(1, win[:, None, :])[:, 0]
    rest = s.scatter(1, win[:, None, :], float("-inf")).amax(1)
    assert float((top - rest).min()) > 104.0
    assert float(torch.exp(torch.tensor(-104.0, dtype=torch.float32))) == 0.0
    ref = C.reference(dict(case, kind="routed"), inp)
    assert (ref["z"] - z_want.double()).abs().max() <= 1e-40 * 8 and (ref["dx"].reshape(B * L, D) - dx_want.double()).abs().max() <= 1e-40 * 64
    assert ref["du"].abs().max() <= 1e-40 * 1e6
    rows = {(b, int(win[b, h])) for b in range(B) for h in range(H)}
    assert len(rows) < B * H if case.get("pair") else len(rows) == B * H
    C.check_routed(cpu_ops, "cpu", case)


def test_routed_winners_walk_over_every_row_of_a_chunk():
    seen = set()
    for case in C.ROUTED:
        seen |= {int(w) % C.CHUNK for w in C.routed(case)[1].reshape(-1)}
    assert seen == set(range(C.CHUNK))


MUTANTS = {      # name -> (which op, a case that must refuse it)
    "drop_last_row": ("fwd", "L32_D128_H2_B3"),
    "neighbour_head": ("fwd", "L50_D128_H2_B3"),
    "no_rescale": ("fwd", "spread_L197_D128_H2_B3"),
    "no_delta": ("bwd", "L50_D128_H2_B3"),
    "skip_second_sample": ("bwd", "second_sample_L33_D128_H2_B5_wg2"),
    "heads_minus_one": ("bwd", "L50_D128_H2_B3"),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_comparison_refuses_wrong_kernels(mutant):
    """Each deliberately wrong stand-in falls outside the GPU test's bounds on its case (and the same case passes without it)."""
    which, name = MUTANTS[mutant]
    case = next(c for c in C.TABLE if c["name"] == name)
    C.check(cpu_ops, "cpu", case)
    with pytest.raises(AssertionError):
        C.check(cpu_ops, "cpu", case, **{which: {"mutant": mutant}})


def test_mutants_are_also_refused_by_the_routed_cases():
    for mutant, which in (("drop_last_row", "fwd"), ("neighbour_head", "fwd"), ("heads_minus_one", "bwd")):
        class Ops:
            mappool_fwd = staticmethod(lambda *a, **k: cpu_ops.mappool_fwd(*a, **k, **({"mutant": mutant} if which == "fwd" else {})))
            mappool_bwd = staticmethod(lambda *a, **k: cpu_ops.mappool_bwd(*a, **k, **({"mutant": mutant} if which == "bwd" else {})))
        refused = 0
        for case in C.ROUTED:
            try:
                C.check_routed(Ops, "cpu", case)
            except AssertionError:
                refused += 1
        assert refused > 0, mutant


# ---- the engine path on the stand-ins ----------------------------------------------------------------------------------------------
@pytest.fixture
def standins():
    restore = cpu_ops.swap_in()
    yield
    restore()


def _step(m, images, texts, seed=None, loss=None):
    m.zero_grad(set_to_none=True)
    if seed is not None:
        torch.manual_seed(seed)
    out = m(images, texts)
    val = (loss or clipa_amd.ClipLoss())(**out, output_dict=True)["contrastive_loss"]
    val.backward()
    return out, val, {k: p.grad for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("patch_dropout", [0.0, 0.5])
def test_toy_model_on_standins_matches_fp64(patch_dropout, standins):
    """Features, ClipLoss and every parameter gradient of the whole toy model through the engine (MapHeadFn on the stand-ins)
    against the unfused fp64 restatement, tolerances of tests/test_model_gpu.py; with patch_dropout the head sees 1 + kept tokens."""
    from .test_model_gpu import _compare_gradients
    m, images, texts = C.toy_model(patch_dropout)
    m.train()
    out, loss, got = _step(m, images, texts, seed=11)
    keep = None
    if patch_dropout:
        torch.manual_seed(11)
        keep = model_mod.patch_dropout_indices(C.TOY_BATCH, 49, patch_dropout)
        assert keep.shape == (C.TOY_BATCH, 24)
    fi, ft, ref_loss, ref = C.toy_reference(m, images, texts, keep)
    assert (out["image_features"].double() - fi).abs().max() < 2e-2
    assert (out["text_features"].double() - ft).abs().max() < 2e-2
    assert abs(float(loss) - ref_loss) < 2e-2 * ref_loss
    assert sorted(got) == sorted(ref) == sorted(k for k, _ in m.named_parameters())
    _compare_gradients(got, ref, f"toy MAP model on the stand-ins, patch_dropout={patch_dropout}")
    dbk = got["visual.map_head.attn.in_proj_bias"][128:256]
    assert torch.equal(dbk, torch.zeros_like(dbk))


def test_u_follows_the_weights(standins):
    """The cached fold is rebuilt when the probe or the in-projection changes version."""
    m, images, _ = C.toy_model()
    with torch.no_grad():
        f0 = m.encode_image(images).clone()
        assert torch.equal(m.encode_image(images), f0)
        for p in (m.visual.map_head.probe, m.visual.map_head.attn.in_proj_weight, m.visual.map_head.attn.in_proj_bias):
            before = m.encode_image(images).clone()
            p.mul_(1.5) if p.ndim > 1 else p.add_(0.3)
            assert not torch.equal(m.encode_image(images), before)


def test_locked_tower_trains_the_head_alone(standins):
    m, images, texts = C.toy_model()
    _, _, ref = _step(m, images, texts)
    m.lock_image_tower(unlocked_groups=2)
    _, _, got = _step(m, images, texts)
    vis = sorted(k for k in got if k.startswith("visual."))
    assert vis == sorted(["visual.proj"] + [k for k in ref if ".map_head." in k or "visual.transformer.resblocks.1." in k])
    for k in got:
        assert torch.equal(got[k], ref[k]), k
