"""CPU tests of multi-caption image-text retrieval (clipa_amd/retrieval_eval.py on csrc/retrieval_multi.hip): the argument
checks of the C ABI, the Recall@k formulas against the reference fixture, the id -> correspondence step of the
reference's Evaluator, and the rule that there is no CPU fallback."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import clipa_amd
from clipa_amd import lib
from clipa_amd.retrieval_eval import correspondence_from_ids, recalls_from_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "multicaption_retrieval.npz")


def _call(Ni, Nt, E, lda, ldb, ptr=4096, cptr=None, ws_bytes=1 << 20):
    p = ctypes.c_void_p(ptr)
    c = p if cptr is None else ctypes.c_void_p(cptr)
    return lib.load().clipa_retrieval_ranks_multi(p, p, c, Ni, Nt, E, lda, ldb, None, p, p, p, p, p, ws_bytes, None)


@pytest.mark.parametrize("Ni,Nt,E,lda,ldb,what", [(16, 40, 64, 66, 64, "lda"), (16, 40, 64, 64, 70, "ldb"),
                                                  (16, 40, 64, 60, 64, "lda"), (0, 40, 64, 64, 64, "Ni"),
                                                  (16, 0, 64, 64, 64, "Nt"), (16, 40, 0, 64, 64, "E")])
def test_multi_rank_kernel_refuses_bad_arguments(Ni, Nt, E, lda, ldb, what):
    assert _call(Ni, Nt, E, lda, ldb) < 0
    assert "retrieval_ranks_multi" in lib.last_error() and what in lib.last_error()


def test_multi_rank_kernel_refuses_misaligned_pointers():
    assert _call(16, 40, 64, 64, 64, ptr=4096 + 4) < 0
    assert "16-byte aligned" in lib.last_error()
    assert _call(16, 40, 64, 64, 64, cptr=4096 + 8) < 0                 # the correspondence too
    assert "16-byte aligned" in lib.last_error()


def test_multi_rank_kernel_refuses_small_workspace():
    need = lib.load().clipa_retrieval_ranks_multi_workspace(1000, 5000)
    assert need >= (1000 + 5000) * 4
    assert _call(1000, 5000, 64, 64, 64, ws_bytes=need - 1) < 0
    assert "workspace too small" in lib.last_error()


def test_capi_header_declares_the_multi_rank_entries():
    header = open(os.path.join(ROOT, "include", "clipa_hip.h")).read()
    declared = set(re.findall(r"\b(clipa_[a-z0-9_]+)\s*\(", header))
    names = {"clipa_retrieval_ranks_multi", "clipa_retrieval_ranks_multi_workspace"}
    assert names <= declared
    assert names <= set(lib.SIGNATURES)
    assert "image_text_retrieval.py" in header


@pytest.mark.parametrize("case", ["A", "B"])
def test_recalls_from_reference_ranks_match_reference_recalls(case):
    z = np.load(FIXTURE)
    ni = int(z[f"{case}_ni"])
    has = np.bincount(z[f"{case}_c"], minlength=ni) > 0
    assert not has.all()                                               # captionless images are part of the case
    ks = tuple(int(k) for k in z[f"{case}_thresholds"])
    got = recalls_from_ranks(z[f"{case}_i2t"], z[f"{case}_t2i"], has, ks)
    for d in ("img2txt", "txt2img"):
        assert list(got[d]) == [f"Recall@{k}" for k in ks]
        for k, want in zip(ks, z[f"{case}_{d}"]):
            assert isinstance(got[d][f"Recall@{k}"], np.float64)
            assert got[d][f"Recall@{k}"] == want, (case, d, k, got[d][f"Recall@{k}"], want)


def test_captionless_image_misses_at_every_k():
    # 3 images, 2 texts, both of image 0: image 2 has no caption; k = 5, 10 exceed Nt, image 1 and 2 still miss
    got = recalls_from_ranks(np.array([0, 2, 2]), np.array([0, 1]), np.array([True, False, False]))
    assert got["img2txt"] == {"Recall@1": 1 / 3, "Recall@5": 1 / 3, "Recall@10": 1 / 3}
    assert got["txt2img"] == {"Recall@1": 0.5, "Recall@5": 1.0, "Recall@10": 1.0}


def test_correspondence_from_ids():
    assert correspondence_from_ids([7, 3, 9], [9, 9, 3, 7, 3]).tolist() == [2, 2, 1, 0, 1]
    with pytest.raises(RuntimeError, match="appears twice"):
        correspondence_from_ids([7, 3, 7], [3])
    with pytest.raises(RuntimeError, match="no image has"):
        correspondence_from_ids([7, 3], [3, 4])


def test_image_text_retrieval_refuses_cpu_features():
    f = torch.nn.functional.normalize(torch.randn(8, 16), dim=-1)
    with pytest.raises(RuntimeError, match="GPU"):
        clipa_amd.image_text_retrieval(f, f, list(range(8)))
