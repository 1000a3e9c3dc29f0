"""Image-tower fine-tuning on the device: the kernels of csrc/mixcut.hip and csrc/softce.hip against the case tables of
tests/finetune_cases.py, and clipa_amd.finetune - classifier head, fused loss, Mixup / CutMix, evaluator - on a 2-layer tower.

mixcut: bit for bit against the numpy float32 restatement (position-coded images, both memory layouts, the 16-byte path with and
without its tail, every lam and box of the table, bad descriptors).
softce: row losses and lse |got - ref| <= KAPPA max(1, |ref|), dlogits |got - ref| <= 2^-7 |ref| + KAPPA_G g against fp64; the
constants are derived on the CPU (finetune_cases.kappas: 6.083e-7 and 1.827e-7, stated as 6.1e-7 and 1.9e-7).
The model: logits 2e-2 max(1, max |ref|), loss 2 %, every tower gradient by tests/test_model_gpu.py's _compare_gradients (cosine
0.99, norm within 5 %) against the fp32 oracle (oracle.clip_oracle.encode_image, the head and the loss in torch); the head's
weight and feature gradients additionally within twice the relative L2 error that the bf16 restatement on the CPU stand-ins
measures (tests/test_finetune_cpu.py prints it; finetune_cases.HEAD_DW_MEASURED_CPU / HEAD_DF_MEASURED_CPU state it)."""
import numpy as np
import pytest
import torch

import clipa_amd
from clipa_amd import ops
from clipa_amd.optim import AdamW

from . import finetune_cases as C
from . import test_model_gpu as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- mixcut ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.MIXCUT, ids=C.names(C.MIXCUT))
def test_mixcut(case):
    C.check_mixcut(ops, DEV, case)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("mode", ["mixup", "cutmix"])
def test_mixcut_at_224(mode, layout):
    """The production size: 150528 bytes per image, 37 workgroups per pair, 16-byte aligned images."""
    C.check_mixcut(ops, DEV, dict(mode=mode, B=3, S=224, layout=layout, rot=2))


def test_mixcut_refuses_bad_descriptors():
    C.check_mixcut_refuses(ops, DEV)


def test_mixcut_wrapper_checks_its_arguments():
    img = torch.zeros(4, 3, 16, 16, dtype=torch.uint8, device=DEV)
    lam = torch.ones(4, device=DEV)
    box = torch.zeros(4, 4, dtype=torch.int32, device=DEV)
    for bad in (dict(), dict(lam=lam, box=box), dict(lam=lam[:3]), dict(lam=lam.double()), dict(box=box[:, :3]), dict(box=box.long())):
        with pytest.raises(RuntimeError):
            ops.mixcut_u8(img, **bad)
    for bad in (img.float(), img[:, :, :, :8], img[:, :, ::2, ::2], torch.zeros(4, 1, 16, 16, dtype=torch.uint8, device=DEV)):
        with pytest.raises(RuntimeError):
            ops.mixcut_u8(bad, lam=lam)
    assert ops.mixcut_u8(img[:0], lam=lam[:0]).shape[0] == 0


def test_device_mixcut_on_an_augmented_batch():
    """DeviceMixCut on what DeviceAugment returns (a channels_last view of an NHWC batch): the images are the restatement's for
    the replayed draws, the triple is (labels, labels.flip(0), lam)."""
    B, S = 6, 32
    rng = np.random.RandomState(4)
    staged = torch.from_numpy(rng.randint(0, 256, size=(B, 40, 48, 3), dtype=np.uint8)).to(DEV)
    labels = torch.arange(B, device=DEV) * 3
    seen = set()
    for seed in range(6):
        images = clipa_amd.DeviceAugment(S, seed=seed)(staged)
        assert not images.is_contiguous() and images.is_contiguous(memory_format=torch.channels_last)
        before = images.clone()
        mix = clipa_amd.DeviceMixCut(seed=seed)
        out, (ya, yb, lam) = mix(images, labels)
        ops.check_token_ids(wait=True)
        mode, rlam, rbox = clipa_amd.sample_mixcut(B, S, generator=torch.Generator().manual_seed(seed))
        seen.add(mode)
        ref = C.mixcut_reference(before.cpu().numpy(), rlam.numpy() if mode == "mixup" else None, rbox.numpy() if mode == "cutmix" else None)
        assert out is images and np.array_equal(out.cpu().numpy(), ref)
        assert ya.dtype == torch.int32 and torch.equal(ya.long(), labels) and torch.equal(yb, ya.flip(0))
        assert torch.equal(lam.cpu(), rlam)
        logits = torch.randn(B, 20, device=DEV)
        loss = clipa_amd.SoftTargetCrossEntropy(0.1)(logits, (ya, yb, lam))
        ref = C.softce_reference(logits.cpu(), ya.cpu(), yb.cpu(), lam.cpu(), 0.1, 1.0)[0].mean()
        assert abs(float(loss) - float(ref)) < 1e-5 * float(ref)
    assert seen == {"mixup", "cutmix"}


# ---- softce ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.SOFTCE, ids=C.names(C.SOFTCE))
def test_softce(case):
    C.check_softce(ops, DEV, case)


@pytest.mark.parametrize("C_", [65, 1001, 1025, 4099])
def test_softce_bits_do_not_depend_on_the_grid(C_):
    """37 rows through one workgroup per four rows, through a single workgroup and through three: the same bits."""
    gen = torch.Generator().manual_seed(C_)
    B = 37
    z = (torch.randn(B, C_, generator=gen) * 6).to(DEV)
    ya = torch.randint(0, C_, (B,), generator=gen, dtype=torch.int32).to(DEV)
    yb = torch.randint(0, C_, (B,), generator=gen, dtype=torch.int32).to(DEV)
    lam = torch.rand(B, generator=gen).to(DEV)
    runs = [ops.soft_target_ce(z, ya, yb, lam, smoothing=0.1, gscale=1.0 / B, _max_workgroups=g) for g in (0, 1, 3)]
    ops.check_token_ids(wait=True)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    ref = C.softce_reference(z.cpu(), ya.cpu(), yb.cpu(), lam.cpu(), 0.1, 1.0 / B)
    k, kg = C.softce_errors(tuple(t.cpu() for t in runs[0]), ref, 1.0 / B)
    print(f"[C = {C_}, B = 37] loss/lse error {k:.3e} (bound {C.KAPPA:.2e}), dlogits excess {kg:.3e} (bound {C.KAPPA_G:.2e})")
    assert k <= C.KAPPA and kg <= C.KAPPA_G


def test_softce_refuses_bad_targets():
    C.check_softce_refuses(ops, DEV)


def test_softce_wrapper_copies_misaligned_operands():
    """A logits view at an odd column offset, labels at an odd element offset: copied, the same result as the aligned call."""
    gen = torch.Generator().manual_seed(8)
    B, C_ = 5, 63
    buf = torch.randn(B, 70, generator=gen).to(DEV)
    lab = torch.randint(0, C_, (B + 1,), generator=gen, dtype=torch.int32).to(DEV)
    a = ops.soft_target_ce(buf[:, 1:1 + C_], lab[1:], gscale=0.2)
    b = ops.soft_target_ce(buf[:, 1:1 + C_].contiguous(), lab[1:].clone(), gscale=0.2)
    ops.check_token_ids(wait=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(RuntimeError):
        ops.soft_target_ce(buf.double(), lab[1:])
    with pytest.raises(RuntimeError):
        ops.soft_target_ce(buf, lab[1:].long())
    with pytest.raises(RuntimeError):
        ops.soft_target_ce(buf, lab)


# ---- the model -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.MODEL_CASES)
def test_step_matches_oracle(name):
    t = C.toy(name)
    m = C.build_classifier(t, DEV)
    logits, f, loss, got, df = C.engine_step(m, t, DEV)
    torch.cuda.synchronize()
    ops.check_token_ids(wait=True)
    rl, rf, rloss, ref, rdf = C.oracle_step(t)
    assert tuple(logits.shape) == (8, t["C"]) and logits.dtype == torch.float32
    err = float((logits.cpu() - rl).abs().max())
    print(f"[{name}] logits error {err:.4f} (bound {2e-2 * max(1.0, float(rl.abs().max())):.4f}), loss {float(loss):.5f} (oracle {rloss:.5f})")
    assert err < 2e-2 * max(1.0, float(rl.abs().max()))
    assert abs(float(loss) - rloss) < 2e-2 * rloss
    assert sorted(got) == sorted(ref)
    M._compare_gradients(got, ref, name)
    dw, dfe = C.rel_l2(got["head.weight"], ref["head.weight"]), C.rel_l2(df, rdf)
    tol_w, tol_f = 2 * C.HEAD_DW_MEASURED_CPU[name], 2 * C.HEAD_DF_MEASURED_CPU[name]
    print(f"[{name}] relative L2 error of d head.weight {dw:.5f} (bound {tol_w:.4f}), of d features {dfe:.5f} (bound {tol_f:.4f})")
    assert dw < tol_w and dfe < tol_f, (dw, dfe)
    # the same model again: the same bits (no atomics anywhere on the path)
    logits2, _, loss2, got2, _ = C.engine_step(m, t, DEV)
    assert torch.equal(logits, logits2) and float(loss) == float(loss2)
    assert all(torch.equal(got[k], got2[k]) for k in got)


def test_clip_and_classifier_share_the_tower():
    """A step on the classifier moves the CLIP's image tower (shared parameters, shared weight cache)."""
    t = C.toy("plain10")
    clip = clipa_amd.CLIP(**C.TOY)
    clip.load_state_dict(t["sd"], strict=True)
    clip.to(DEV)
    m = clipa_amd.create_classifier(clip, 10, init=t["head"])
    assert m.head.weight.is_cuda
    img = t["images"].to(DEV)
    with torch.no_grad():
        before = clip.encode_image(img).clone()
    opt = AdamW(m.parameters(), lr=1e-2, betas=(0.9, 0.95), eps=1e-6, weight_decay=0.0)
    loss = clipa_amd.soft_target_cross_entropy(m(img), t["ya"].to(DEV))
    loss.backward()
    opt.step()
    with torch.no_grad():
        after = clip.encode_image(img)
    assert not torch.equal(before, after)


def _train():
    t = C.toy("plain10")
    m = C.build_classifier(t, DEV)
    opt = AdamW(m.parameters(), lr=C.TRAIN_LR, betas=(0.9, 0.95), eps=1e-6, weight_decay=0.0)
    crit = clipa_amd.SoftTargetCrossEntropy(t["smoothing"])
    img, target = t["images"].to(DEV), (t["ya"].to(DEV), t["yb"].to(DEV), t["lam"].to(DEV))
    losses = []
    for _ in range(10):
        opt.zero_grad(set_to_none=True)
        loss = crit(m(img), target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def test_ten_adamw_steps_reduce_the_loss_reproducibly():
    """One fixed batch: the final loss is below half the first (the fp32 oracle's trajectory falls below a quarter:
    tests/test_finetune_cpu.py), and two runs give identical losses."""
    a, b = _train(), _train()
    print("losses:", [round(v, 4) for v in a])
    assert a == b
    assert all(np.isfinite(a)) and a[-1] < 0.5 * a[0]


def test_evaluate_classification():
    t = C.toy("plain10", B=16)
    m = C.build_classifier(t, DEV)
    labels = t["ya"].long().to(DEV)
    img = t["images"].to(DEV)
    got = clipa_amd.evaluate_classification(m, [(img[:8], labels[:8]), (img[8:], labels[8:])])
    assert m.training and m.visual.training
    C.check_evaluation(m, t, got, DEV)
    with pytest.raises(RuntimeError, match="outside"):
        clipa_amd.evaluate_classification(m, [(img[:8], labels[:8] + 10)])
    ops.check_token_ids(wait=True)
