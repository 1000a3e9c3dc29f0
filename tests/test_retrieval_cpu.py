"""CPU tests of the validation surface (training/train.py:317-449 restated in clipa_amd/evaluate.py): the host reduction
from ranks to the reference's metrics against the reference fixture, the argument checks of the rank kernel's C ABI, and
the rule that there is no CPU fallback."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import clipa_amd
from clipa_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "retrieval_metrics.npz")


@pytest.mark.parametrize("case", ["A", "B"])
def test_metrics_from_reference_preds_match_reference_metrics(case):
    z = np.load(FIXTURE)
    got = clipa_amd.metrics_from_ranks(z[f"{case}_i2t"], z[f"{case}_t2i"])
    keys = [str(k) for k in z[f"{case}_metric_keys"]]
    assert sorted(got) == sorted(keys)
    for k, v in zip(keys, z[f"{case}_metrics"]):
        assert isinstance(got[k], np.float64), k
        assert got[k] == v, (k, got[k], v)


def test_metrics_formulas_on_small_ranks():
    m = clipa_amd.metrics_from_ranks(np.array([0, 0, 3, 9, 12]), torch.tensor([1, 1, 1, 2], dtype=torch.int32))
    assert m["image_to_text_mean_rank"] == np.mean([0, 0, 3, 9, 12]) + 1
    assert m["image_to_text_median_rank"] == 4.0
    assert (m["image_to_text_R@1"], m["image_to_text_R@5"], m["image_to_text_R@10"]) == (0.4, 0.6, 0.8)
    assert m["text_to_image_median_rank"] == 2.0
    assert m["text_to_image_R@1"] == 0.0 and m["text_to_image_R@5"] == 1.0


def _call(N, E, lda, ldb, ptr=4096):
    p = ctypes.c_void_p(ptr)
    return lib.load().clipa_retrieval_ranks(p, p, N, E, lda, ldb, None, p, p, p, p, p, 1 << 20, None)


@pytest.mark.parametrize("N,E,lda,ldb,what", [(16, 64, 66, 64, "lda"), (16, 64, 64, 70, "ldb"), (16, 64, 60, 64, "lda"),
                                              (0, 64, 64, 64, "N"), (16, 0, 64, 64, "E")])
def test_rank_kernel_refuses_bad_arguments(N, E, lda, ldb, what):
    rc = _call(N, E, lda, ldb)
    assert rc < 0
    assert "retrieval_ranks" in lib.last_error() and what in lib.last_error()


def test_rank_kernel_refuses_misaligned_pointers():
    assert _call(16, 64, 64, 64, ptr=4096 + 4) < 0
    assert "16-byte aligned" in lib.last_error()


def test_get_clip_metrics_refuses_cpu_features():
    f = torch.nn.functional.normalize(torch.randn(8, 16), dim=-1)
    with pytest.raises(RuntimeError, match="GPU"):
        clipa_amd.get_clip_metrics(f, f, torch.tensor(100.0))


def test_capi_header_declares_the_rank_entries():
    header = open(os.path.join(ROOT, "include", "clipa_hip.h")).read()
    declared = set(re.findall(r"\b(clipa_[a-z0-9_]+)\s*\(", header))
    assert {"clipa_retrieval_ranks", "clipa_retrieval_ranks_workspace"} <= declared
    assert "train.py:432-449" in header
