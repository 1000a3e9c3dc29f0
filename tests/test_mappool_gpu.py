"""The attention-pooling kernels (csrc/mappool.hip) and the MAP head of the image tower on the GPU: every case of
tests/mappool_cases.py forward and backward inside the stated bounds (fp64 unfused reference; kappa from the CPU stand-ins), the
routed cases bit for bit, run-to-run bit-identity, argument handling, the head's memory footprint, and the whole toy model
against the unfused fp64 restatement at the model tolerance of tests/test_model_gpu.py."""
import pytest
import torch

import clipa_amd
from clipa_amd import engine, lib, model as model_mod, ops

from . import mappool_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", C.TABLE, ids=C.names(C.TABLE))
def test_table_case_forward_backward(case):
    C.check(ops, DEV, case)


@pytest.mark.parametrize("case", C.ROUTED, ids=C.names(C.ROUTED))
def test_routed_case_is_bit_exact(case):
    C.check_routed(ops, DEV, case)


@pytest.mark.parametrize("name", ["second_sample_L50_D384_H6_B5_wg2", "L257_D1408_H16_B1", "L197_D128_H2_B3"])
def test_two_runs_are_bit_identical(name):
    case = next(c for c in C.TABLE if c["name"] == name)
    a, b = C.run(ops, DEV, case), C.run(ops, DEV, case)
    for s, t in zip(a, b):
        assert torch.equal(s, t)


def test_zero_batch_returns_ok():
    x, u = torch.zeros(0, 128, device=DEV, dtype=torch.bfloat16), torch.zeros(2, 128, device=DEV, dtype=torch.bfloat16)
    z, stats = ops.mappool_fwd(x, u, 0, 50, 2)
    assert z.shape == (0, 2, 128) and stats.shape == (0, 2, 2)
    dx, du = ops.mappool_bwd(x, u, z, stats, torch.zeros(0, 2, 128, device=DEV), 0, 50, 2)
    torch.cuda.synchronize()
    assert dx.shape == (0, 128) and torch.equal(du.cpu(), torch.zeros(2, 128))
    p = u.data_ptr()
    assert lib.load().clipa_mappool_fwd(p, p, p, p, 0, 50, 128, 2, 128, 0, None) == 0


def test_unsupported_shapes_raise_from_ops():
    def args(D, H):
        return torch.zeros(4, D, device=DEV, dtype=torch.bfloat16), torch.zeros(H, D, device=DEV, dtype=torch.bfloat16), 2, 2, H
    with pytest.raises(RuntimeError, match=r"H=17, D=128"):
        ops.mappool_fwd(*args(128, 17))
    with pytest.raises(RuntimeError, match=r"H=2, D=96"):
        ops.mappool_fwd(*args(96, 2))
    x, u, B, L, H = args(96, 2)
    with pytest.raises(RuntimeError, match=r"H=2, D=96"):
        ops.mappool_bwd(x, u, torch.zeros(2, 2, 96, device=DEV), torch.zeros(2, 2, 2, device=DEV), torch.zeros(2, 2, 96, device=DEV), B, L, H)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.mappool_fwd(torch.zeros(4, 128, dtype=torch.bfloat16), torch.zeros(2, 128, dtype=torch.bfloat16), 2, 2, 2)


def test_head_memory_stays_under_twice_x():
    """B = 256, L = 197, D = 768: the peak of MapHeadFn forward + backward over the level before it is <= 2.0 x bytes(x) - dx is
    1.0 x, z / dz / the B-row tensors / the kernel's workspace / the weight gradients the rest; an unfused head would hold K, V,
    dK, dV and dx, at least 3 x.  (The bf16 operand copies of the weights belong to the weight cache, filled by a small call
    before the measurement.)"""
    B, L, D, H, E = 256, 197, 768, 12, 512
    torch.manual_seed(0)
    head = model_mod._MapHeadParams(D, H).to(DEV)
    proj = torch.nn.Parameter(torch.randn(D, E, device=DEV) * D ** -0.5)
    cache = engine.WeightCache()

    def step(b):
        x = (torch.randn(b * L, D, device=DEV) * 0.5).to(torch.bfloat16).requires_grad_(True)
        dfeat = torch.randn(b, E, device=DEV)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        feat = engine.MapHeadFn.apply(x, engine.MapHeadCfg(B=b, L=L, H=H, act=ops.ACT_GELU_TANH, eps=1e-5), cache,
                                      *head.param_tuple(), proj)
        feat.backward(dfeat)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        assert x.grad is not None and x.grad.shape == x.shape and torch.isfinite(x.grad.float()).all()
        return peak, x.numel() * 2
    step(2)
    for p in list(head.parameters()) + [proj]:
        p.grad = None
    peak, xbytes = step(B)
    print(f"MapHeadFn forward + backward at B={B}, L={L}, D={D}: peak {peak / 2 ** 20:.1f} MiB over the level before = "
          f"{peak / xbytes:.3f} x bytes(x) ({xbytes / 2 ** 20:.1f} MiB)")
    assert peak <= 2.0 * xbytes


# ---- the whole toy model ---------------------------------------------------------------------------------------------------------
def _step(m, images, texts, seed=None, loss=None):
    m.zero_grad(set_to_none=True)
    if seed is not None:
        torch.manual_seed(seed)
    out = m(images.to(DEV), texts.to(DEV))
    val = (loss or clipa_amd.ClipLoss())(**out, output_dict=True)["contrastive_loss"]
    val.backward()
    torch.cuda.synchronize()
    return out, val, {k: p.grad for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("patch_dropout", [0.0, 0.5])
def test_toy_model_matches_fp64(patch_dropout):
    from .test_model_gpu import _compare_gradients
    m, images, texts = C.toy_model(patch_dropout)
    m.to(DEV).train()
    out, loss, got = _step(m, images, texts, seed=11)
    keep = None
    if patch_dropout:
        torch.manual_seed(11)
        keep = model_mod.patch_dropout_indices(C.TOY_BATCH, 49, patch_dropout)
    fi, ft, ref_loss, ref = C.toy_reference(m, images, texts, keep)
    assert (out["image_features"].double().cpu() - fi).abs().max() < 2e-2
    assert (out["text_features"].double().cpu() - ft).abs().max() < 2e-2
    assert abs(float(loss) - ref_loss) < 2e-2 * ref_loss
    assert sorted(got) == sorted(ref)
    _compare_gradients(got, ref, f"toy MAP model, patch_dropout={patch_dropout}")
    dbk = got["visual.map_head.attn.in_proj_bias"][128:256]
    assert torch.equal(dbk, torch.zeros_like(dbk))


def test_grad_checkpointing_on_and_off_agree_bit_for_bit():
    runs = []
    for ckpt in (False, True):
        m, images, texts = C.toy_model()
        m.to(DEV)
        m.set_grad_checkpointing(ckpt)
        out, loss, got = _step(m, images, texts)
        runs.append((out["image_features"].clone(), float(loss), got))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    for k, v in runs[0][2].items():
        assert torch.equal(v, runs[1][2][k]), k


def test_fp8_precision_runs_the_head_in_bf16():
    """precision="fp8": the blocks run on the fp8 path, the head's operands stay bf16 - its features follow from the tower's
    output exactly as in the bf16 engine, and every head parameter gets a finite gradient."""
    m, images, texts = C.toy_model()
    m.to(DEV)
    clipa_amd.convert_weights_to_lp(m, torch.bfloat16)
    for t in (m.visual.transformer, m.transformer):
        t.fp8 = True
    out, loss, got = _step(m, images, texts)
    assert torch.isfinite(loss) and all(torch.isfinite(v.float()).all() for v in got.values())
    assert all(p.grad is not None and p.grad.dtype == p.dtype for p in m.visual.map_head.parameters())
    # the head alone, on the fp8 tower's own output, through the bf16 ops: bit for bit what the model returned
    v = m.visual
    with torch.no_grad():
        B, S = images.shape[0], images.shape[2]
        L = (S // 16) ** 2 + 1
        cfg = engine.StemCfg(B=B, L=L, P=16, Kp=768, eps=1e-5, ln_pre=True, mean=v.image_mean, std=v.image_std)
        x0 = engine.VisionStemFn.apply(images.to(DEV), cfg, v._cache, v.conv1.weight, v.class_embedding, v.positional_embedding,
                                       v.ln_pre.weight, v.ln_pre.bias)
        xL = v.transformer.run(x0, B, L, False, v._cache)
        assert xL.dtype == torch.bfloat16
        feat = engine.MapHeadFn.apply(xL, engine.MapHeadCfg(B=B, L=L, H=2, act=v.transformer.act, eps=1e-5), v._cache,
                                      *v.map_head.param_tuple(), v.proj)
        assert torch.equal(engine.L2NormFn.apply(feat), out["image_features"])
    bf = C.toy_model()[0].to(DEV)
    clipa_amd.convert_weights_to_lp(bf, torch.bfloat16)
    ref = _step(bf, images, texts)[0]["image_features"]
    assert (ref - out["image_features"]).abs().max() < 5e-2 and not torch.equal(ref, out["image_features"])


def test_siglip_training_step_reaches_every_head_parameter():
    """One end-to-end step with SigLipLoss and a logit bias: finite, non-zero gradients on every map_head parameter - except the K
    third of attn.in_proj_bias, which is exactly zero (bk cancels in the softmax) - against the fp64 restatement of the same loss."""
    from .test_model_gpu import _compare_gradients
    m, images, texts = C.toy_model(init_logit_bias=-10.0)
    m.to(DEV).train()
    out, loss, got = _step(m, images, texts, loss=clipa_amd.SigLipLoss())
    assert torch.isfinite(loss)
    for k, p in m.visual.map_head.named_parameters():
        g = p.grad
        assert g is not None and torch.isfinite(g).all(), k
        if k == "attn.in_proj_bias":
            assert torch.equal(g[128:256], torch.zeros_like(g[128:256]))
            assert float(g[:128].abs().max()) > 0 and float(g[256:].abs().max()) > 0
        else:
            assert float(g.abs().max()) > 0, k
    _, _, ref_loss, ref = C.toy_reference(m, images, texts, loss="siglip")
    assert abs(float(loss) - ref_loss) < 2e-2 * ref_loss
    _compare_gradients({k: v for k, v in got.items() if ".map_head." in k}, {k: v for k, v in ref.items() if ".map_head." in k},
                       "toy MAP model, SigLipLoss: head gradients")
