"""CPU tests of the distillation surface: create_loss's DistillClipLoss branch (open_clip/factory.py:262-270), the
teacher-is-a-constant rule, the C-ABI declarations of the fused kernel pair, and the golden fixture's provenance."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import clipa_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Args:
    local_loss, gather_with_grad, rank, world_size, horovod, distill, model = True, False, 2, 4, False, True, "ViT-B-16"


def test_create_loss_distill_returns_distill_clip_loss_with_reference_arguments():
    loss = clipa_amd.create_loss(_Args)
    assert isinstance(loss, clipa_amd.DistillClipLoss)
    assert isinstance(loss, clipa_amd.ClipLoss)
    assert (loss.local_loss, loss.gather_with_grad, loss.rank, loss.world_size, loss.cache_labels, loss.use_horovod) == \
        (True, False, 2, 4, True, False)


def test_create_loss_coca_still_refused():
    class A(_Args):
        distill, model = False, "coca_ViT-B-32"
    with pytest.raises(NotImplementedError, match="CoCa"):
        clipa_amd.create_loss(A)


@pytest.mark.parametrize("which", ["dist_image_features", "dist_text_features", "dist_logit_scale"])
def test_teacher_input_that_requires_grad_is_refused(which):
    args = {"image_features": torch.randn(8, 16), "text_features": torch.randn(8, 16), "logit_scale": torch.tensor(10.0),
            "dist_image_features": torch.randn(8, 24), "dist_text_features": torch.randn(8, 24),
            "dist_logit_scale": torch.tensor(100.0)}
    args[which].requires_grad_(True)
    with pytest.raises(RuntimeError, match="teacher"):
        clipa_amd.DistillClipLoss()(**args)


def test_capi_header_declares_the_distill_entries():
    header = open(os.path.join(ROOT, "include", "clipa_hip.h")).read()
    declared = set(re.findall(r"\b(clipa_[a-z0-9_]+)\s*\(", header))
    for name in ("clipa_simce_distill_workspace", "clipa_simce_distill_fwd", "clipa_simce_distill_bwd"):
        assert name in declared, name
    assert "loss.py:202-238" in header


def test_distill_golden_regenerates_exactly():
    """tools/make_distill_golden.py run against the live reference reproduces the committed fixture bit for bit."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import ref_loader
    if not ref_loader.available():
        pytest.skip("the reference checkout is not available on this machine")
    from tools import make_distill_golden
    fresh = make_distill_golden.generate(port=29763)
    z = np.load(os.path.join(ROOT, "tests", "golden", "distill_loss.npz"))
    assert set(z.files) == set(fresh), set(z.files) ^ set(fresh)
    for k in z.files:
        a, b = np.asarray(fresh[k]), z[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(a, b), k
