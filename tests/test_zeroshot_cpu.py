"""Fused zero-shot classification without a GPU: the fixture of tools/make_zeroshot_golden.py against the restatements that made
it (tests/zeroshot_cases.py) and against the two references' accuracy rules, the host side of the prompt ensemble, the counting
rules of clipa_amd/zero_shot.py on a host stand-in for the two kernels, the argument errors of the C entry points (returned
before any launch) and of the Python functions."""
import os
from unittest import mock

import numpy as np
import pytest
import torch

import clipa_amd
from clipa_amd import zero_shot
from tools import make_zeroshot_golden as G

from . import zeroshot_cases as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "zeroshot.npz")
NAMES = ("S", "M", "L")


@pytest.fixture(scope="module")
def golden():
    return np.load(FIXTURE, allow_pickle=False)


@pytest.fixture(scope="module")
def cases(golden):
    """name -> (features, classifier, labels, fp64 logits): computed once, shared, never written to."""
    out = {}
    for name in NAMES:
        f, w, lab = G.case_inputs(name, golden[f"{name}_redraws"])
        out[name] = (f, w, lab, Z.logits_fp64(f, w))
    return out


class HostOps:
    """Stands in for clipa_amd.ops on CPU tensors: the two kernels by their restatements."""
    calls = 0

    def zeroshot_ranks(self, f, w, labels):
        self.calls += 1
        assert labels.dtype == torch.int32 and labels.dim() == 2
        with np.errstate(all="ignore"):                        # non-finite inputs are reported by the caller, after the launch
            gt, eq, pred = Z.ranks_from_logits(Z.chain_fp32(f.numpy(), w.numpy()), labels.numpy())
        return tuple(torch.from_numpy(a.astype(np.int32)) for a in (gt, eq, pred))

    def zeroshot_class_mean(self, emb, offsets, eps=0.0):
        return torch.from_numpy(Z.class_mean_fp32(emb.numpy(), list(offsets), eps))


@pytest.fixture
def host_engine():
    """CPU tensors claim to be on the GPU and the kernels are the host stand-ins: the Python glue runs as it does on the device."""
    ops = HostOps()
    with mock.patch.object(torch.Tensor, "is_cuda", True), mock.patch.object(zero_shot, "ops", ops):
        yield ops


def test_functions_are_exported():
    for name in ("build_classifier", "class_mean_embeddings", "zero_shot_ranks", "zero_shot_counts", "zero_shot_metrics",
                 "evaluate_zero_shot"):
        assert getattr(clipa_amd, name) is getattr(zero_shot, name)
    assert clipa_amd.zero_shot is zero_shot


@pytest.mark.parametrize("name", NAMES)
def test_restatements_reproduce_the_fixture(golden, cases, name):
    z, k = golden, G.CASES[name]
    for key in ("c", "e", "b", "seed", "noise"):
        assert float(z[f"{name}_{key}"]) == float(k[key]), key
    f, w, lab, v = cases[name]
    assert f.dtype == w.dtype == np.float32 and f.shape == (k["b"], k["e"]) and w.shape == (k["c"], k["e"])
    assert np.array_equal(lab.reshape(k["b"], -1), z[f"{name}_labels"].reshape(k["b"], -1))
    assert np.abs(np.linalg.norm(f, axis=1) - 1).max() < 1e-6 and np.abs(np.linalg.norm(w, axis=1) - 1).max() < 1e-6
    gt, eq, pred = Z.ranks_from_logits(v, lab)
    assert np.array_equal(gt, z[f"{name}_gt"]) and np.array_equal(eq, z[f"{name}_eq"]) and np.array_equal(pred, z[f"{name}_pred"])
    # the float32 chain (the engine's arithmetic) must land on the same ranks: nothing sits inside the margin
    v32 = Z.chain_fp32(f, w)
    dev = float(z[f"{name}_dev"])
    assert np.abs(v32.astype(np.float64) - v).max() == dev
    g32, e32, p32 = Z.ranks_from_logits(v32, lab)
    assert np.array_equal(g32, gt) and np.array_equal(e32, eq) and np.array_equal(p32, pred)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_meets_its_own_conditions(golden, name):
    z = golden
    dev, margin = float(z[f"{name}_dev"]), float(z[f"{name}_margin"])
    assert 0 < dev < 1e-6 and margin == G.MARGIN_FACTOR * dev == 64 * dev
    assert z[f"{name}_gap"].min() >= margin and (z[f"{name}_eq"] == 0).all() and int(z[f"{name}_ties"]) == 0
    assert z[f"{name}_redraws"].max() <= 2                    # the rule converges in at most two rounds
    b, c = int(z[f"{name}_b"]), int(z[f"{name}_c"])
    counts = Z.counts_from_ranks(z[f"{name}_gt"], z[f"{name}_eq"], c, (1, 5))
    assert counts == {"count": b, "ties": 0, "hits1": int(z[f"{name}_hits1"]), "hits5": int(z[f"{name}_hits5"])}
    assert 0.1 <= float(z[f"{name}_top1"]) == counts["hits1"] / b <= 0.9 and float(z[f"{name}_top5"]) == counts["hits5"] / b < 0.95
    lab = z[f"{name}_labels"]
    if name == "M":                                           # one, two and three labels, -1 padding
        assert lab.shape == (b, 3) and sorted(set((lab >= 0).sum(1).tolist())) == [1, 2, 3] and lab.min() == -1
        assert (z["M_gt"] == 0).sum() > (lab[:, 0] == z["M_pred"]).sum()      # the extra labels decide some rows
    else:
        assert lab.shape == (b,) and lab.min() >= 0


@pytest.mark.parametrize("name", ["S", "L"])
def test_counts_equal_the_torch_reference_accuracy(golden, cases, name):
    """Single label, no ties: gt < k is exactly "the target is among the k largest logits" (zero_shot.py:47-50, on the
    reference's 100 * logits)."""
    _, _, lab, v = cases[name]
    want = Z.accuracy_torch_reference(torch.from_numpy(100.0 * v), torch.from_numpy(lab), topk=(1, 5))
    assert want == [float(golden[f"{name}_hits1"]), float(golden[f"{name}_hits5"])]


def test_multi_label_top1_equals_the_jax_reference(golden, cases):
    _, _, lab, v = cases["M"]
    assert Z.any_match_jax_reference(v, lab) == int(golden["M_hits1"])
    # an image without labels is counted and wrong, with and without the reference's mask of real rows
    lab2 = lab.copy()
    lab2[:7] = -1
    gt, eq, _ = Z.ranks_from_logits(v, lab2)
    assert (gt[:7] == v.shape[1]).all() and (eq[:7] == 0).all()
    assert Z.counts_from_ranks(gt, eq, v.shape[1], (1,))["hits1"] == Z.any_match_jax_reference(v, lab2)


def test_k_above_the_class_count_is_the_references_clipped_k(host_engine):
    """C = 3 with top-5: `run` clips k to C, so every labelled image is a hit - and an image without labels still is none."""
    rng = np.random.RandomState(0)
    f, w = rng.standard_normal((40, 8)).astype(np.float32), rng.standard_normal((3, 8)).astype(np.float32)
    y = rng.randint(0, 3, size=40)
    want = Z.accuracy_torch_reference(torch.from_numpy(Z.logits_fp64(f, w)), torch.from_numpy(y), topk=(1, 3))
    got = zero_shot.zero_shot_metrics(torch.from_numpy(f), torch.from_numpy(w), torch.from_numpy(y), topk=(1, 5))
    assert [got["hits1"], got["hits5"]] == want and got["hits5"] == 40 and 0 < got["hits1"] < 40
    y[:4] = -1
    got = zero_shot.zero_shot_counts(torch.from_numpy(f), torch.from_numpy(w), y, topk=(5, 7))
    assert got == {"count": 40, "ties": 0, "hits5": 36, "hits7": 36}


def test_counts_metrics_types_ties_and_additivity(host_engine, golden, cases):
    f, w, lab, _ = cases["S"]
    ft, wt = torch.from_numpy(f), torch.from_numpy(w)
    met = zero_shot.zero_shot_metrics(ft, wt, lab)
    assert {k: met[k] for k in ("count", "ties", "hits1", "hits5")} == {"count": 300, "ties": 0, "hits1": int(golden["S_hits1"]),
                                                                        "hits5": int(golden["S_hits5"])}
    assert all(type(met[k]) is int for k in ("count", "ties", "hits1", "hits5"))
    assert type(met["top1"]) is np.float64 and met["top1"] == float(golden["S_top1"]) and met["top5"] == float(golden["S_top5"])
    # shards add up
    parts = [zero_shot.zero_shot_counts(ft[a:b], wt, lab[a:b]) for a, b in ((0, 130), (130, 300))]
    total = {k: parts[0][k] + parts[1][k] for k in parts[0]}
    assert zero_shot.metrics_from_counts(total) == met
    # classes that copy the rows of classes 3 and 11 tie with them: counted in `ties`, and the label still wins
    w2 = np.concatenate([w, w[[3, 11]]])
    got = zero_shot.zero_shot_counts(ft, torch.from_numpy(w2), lab)
    assert got["ties"] == int(np.isin(lab, [3, 11]).sum()) > 5 and got["hits1"] == met["hits1"]
    # no rows: no launch, zero counts, NaN accuracies
    before = host_engine.calls
    ranks = zero_shot.zero_shot_ranks(ft[:0], wt, lab[:0])
    assert all(tuple(ranks[k].shape) == (0,) and ranks[k].dtype == torch.int32 for k in ("gt", "eq", "pred"))
    empty = zero_shot.zero_shot_metrics(ft[:0], wt, lab[:0])
    assert empty["count"] == 0 and empty["hits1"] == 0 and np.isnan(empty["top1"]) and type(empty["top1"]) is np.float64
    assert host_engine.calls == before + 2


def test_prompt_order_is_a_stable_sort_and_merges_aliases():
    # classes 0..3; class 2 has two names (aliases) of two templates each, given far apart and out of order
    pc = np.array([3, 2, 0, 2, 1, 0, 3, 2, 2, 1])
    order, offsets = zero_shot.prompt_order(pc, 4)
    assert order.tolist() == [2, 5, 4, 9, 1, 3, 7, 8, 0, 6]      # within a class: the caller's order
    assert offsets.tolist() == [0, 2, 4, 8, 10]
    assert zero_shot.prompt_order(np.sort(pc), 4)[0] is None and zero_shot.prompt_order(torch.from_numpy(pc), 4)[1].tolist() == offsets.tolist()
    with pytest.raises(RuntimeError, match=r"Classes without embeddings: \[4\]"):
        zero_shot.prompt_order(pc, 5)
    with pytest.raises(RuntimeError, match=r"\[0, 3\)"):
        zero_shot.prompt_order(pc, 3)
    with pytest.raises(RuntimeError, match="one integer class per prompt"):
        zero_shot.prompt_order(pc.astype(np.float32), 4)


def test_class_mean_embeddings_in_any_prompt_order(host_engine):
    emb, offsets = G.classmean_inputs()
    pc = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    want = Z.class_mean_fp32(emb, offsets, 1e-8)
    perm = np.random.RandomState(3).permutation(len(pc))
    got = zero_shot.class_mean_embeddings(torch.from_numpy(emb[perm]), pc[perm], len(offsets) - 1, eps=1e-8).numpy()
    stable = perm[np.argsort(pc[perm], kind="stable")]         # within a class the rows keep the caller's order
    assert np.array_equal(got, Z.class_mean_fp32(emb[stable], offsets, 1e-8))
    dev_w = float(np.load(FIXTURE)["W_dev"])
    assert np.abs(want.astype(np.float64) - Z.class_mean_fp64(emb, offsets, 1e-8)).max() <= dev_w
    assert np.abs(got.astype(np.float64) - Z.class_mean_fp64(emb, offsets, 1e-8)).max() <= 4 * dev_w      # another row order


def test_c_entry_argument_errors_come_back_as_codes():
    """Null pointers, bad leading dimensions and Lmax: CLIPA_ERR_ARG plus clipa_last_error, before any device is touched."""
    from clipa_amd import lib
    h = lib.load()
    p = 4096                                                    # an aligned, never dereferenced address
    assert h.clipa_zeroshot_ranks(p, p, p, 0, 5, 8, 1, 8, 8, None, None, None, None) == 0            # B = 0: nothing to do
    assert h.clipa_zeroshot_ranks(None, p, p, 3, 5, 8, 1, 8, 8, p, p, p, None) < 0 and "pointer argument 0 is null" in lib.last_error()
    assert h.clipa_zeroshot_ranks(p, p, p, 3, 5, 8, 1, 8, 8, p, None, p, None) < 0 and "pointer argument 4 is null" in lib.last_error()
    assert h.clipa_zeroshot_ranks(p, p + 4, p, 3, 5, 8, 1, 8, 8, p, p, p, None) < 0 and "not 16-byte aligned" in lib.last_error()
    assert h.clipa_zeroshot_ranks(p, p, p, 3, 5, 8, 1, 7, 8, p, p, p, None) < 0 and "lda = 7" in lib.last_error()
    assert h.clipa_zeroshot_ranks(p, p, p, 3, 5, 8, 1, 8, 10, p, p, p, None) < 0 and "multiples of 4" in lib.last_error()
    for lmax in (0, 33):
        assert h.clipa_zeroshot_ranks(p, p, p, 3, 5, 8, lmax, 8, 8, p, p, p, None) < 0 and f"Lmax = {lmax}" in lib.last_error()
    assert h.clipa_zeroshot_ranks(p, p, p, 3, 0, 8, 1, 8, 8, p, p, p, None) < 0 and "nothing to rank" in lib.last_error()
    assert h.clipa_zeroshot_ranks(p, p, p, 3, 1 << 20, 8, 1, 8, 8, p, p, p, None) < 0 and "too large" in lib.last_error()
    assert h.clipa_zeroshot_class_mean(None, None, 0, 0, 8, 8, 0.0, None, 8, None) == 0                # C = 0: nothing to do
    assert h.clipa_zeroshot_class_mean(None, p, 5, 2, 8, 8, 0.0, p, 8, None) < 0 and "pointer argument 0 is null" in lib.last_error()
    assert h.clipa_zeroshot_class_mean(p, p, 5, 2, 8, 8, 0.0, None, 8, None) < 0 and "pointer argument 2 is null" in lib.last_error()
    assert h.clipa_zeroshot_class_mean(p, p, 5, 2, 8, 7, 0.0, p, 8, None) < 0 and "lde = 7" in lib.last_error()
    assert h.clipa_zeroshot_class_mean(p, p, 5, 2, 8, 8, 0.0, p, 6, None) < 0 and "ldw = 6" in lib.last_error()
    assert h.clipa_zeroshot_class_mean(p, p, 1, 2, 8, 8, 0.0, p, 8, None) < 0 and "empty class" in lib.last_error()
    assert h.clipa_zeroshot_class_mean(p, p, 5, 2, 8, 8, -1.0, p, 8, None) < 0 and "eps" in lib.last_error()


def test_cpu_tensors_raise():
    f, w, y = torch.zeros(4, 8), torch.zeros(3, 8), torch.zeros(4, dtype=torch.int64)
    for call in (lambda: zero_shot.zero_shot_ranks(f, w, y), lambda: zero_shot.zero_shot_counts(f, w, y),
                 lambda: zero_shot.zero_shot_metrics(f.numpy(), w, y), lambda: zero_shot.class_mean_embeddings(f, [0, 1, 2, 2], 3),
                 lambda: zero_shot.build_classifier(None, torch.zeros(4, 8, dtype=torch.int64), [0, 1, 2, 2], 3),
                 lambda: zero_shot.evaluate_zero_shot(None, w, {})):
        with pytest.raises(RuntimeError, match="GPU"):
            call()


def test_argument_errors_are_raised(host_engine):
    rng = np.random.RandomState(1)
    f, w = torch.from_numpy(rng.standard_normal((6, 8)).astype(np.float32)), torch.from_numpy(rng.standard_normal((3, 8)).astype(np.float32))
    y = torch.tensor([0, 1, 2, 0, 1, 2])
    nan = torch.where(torch.eye(6, 8) > 0, torch.tensor(float("nan")), f)
    bad = [("non-finite values in 6 image feature rows", lambda: (nan, w, y)),
           ("non-finite values in 0 image feature rows / 8 classifier", lambda: (f, torch.cat([w[:2], w[2:] * float("inf")]), y)),
           (r"1 labels values outside \[-1, C\)", lambda: (f, w, torch.tensor([0, 1, 3, 0, 1, 2]))),
           (r"2 labels values outside \[-1, C\)", lambda: (f, w, torch.tensor([[0, -2], [1, -1], [2, -1], [0, 1 << 40], [1, -1], [2, -1]]))),
           ("labels must be integers", lambda: (f, w, y.float())),
           (r"\[B\] or \[B, Lmax\]", lambda: (f, w, y[:-1])),
           (r"\[B\] or \[B, Lmax\]", lambda: (f, w, y.reshape(6, 1, 1))),
           ("Lmax = 33", lambda: (f, w, torch.full((6, 33), -1))),
           (r"must be \[B, E\] and", lambda: (f, w[:, :7], y)),
           ("2-D float GPU tensor", lambda: (f[0], w, y)),
           ("2-D float GPU tensor", lambda: (f, w.long(), y))]
    for match, make in bad:
        for fn in (zero_shot.zero_shot_ranks, zero_shot.zero_shot_counts, zero_shot.zero_shot_metrics):
            with pytest.raises(RuntimeError, match=match):
                fn(*make())
    with pytest.raises(RuntimeError, match="topk"):
        zero_shot.zero_shot_counts(f, w, y, topk=(0,))
    with pytest.raises(RuntimeError, match="topk"):
        zero_shot.zero_shot_metrics(f, w, y, topk=())
    with pytest.raises(RuntimeError, match="Classes without embeddings"):
        zero_shot.class_mean_embeddings(f, [0, 0, 1, 1, 3, 3], 4)
    with pytest.raises(RuntimeError, match="one row of E >= 1 columns per entry"):
        zero_shot.class_mean_embeddings(f, [0, 1, 2], 3)
    with pytest.raises(RuntimeError, match="non-finite"):
        zero_shot.class_mean_embeddings(nan, [0, 0, 1, 1, 2, 2], 3)
    with pytest.raises(RuntimeError, match="yielded no batches"):
        zero_shot.evaluate_zero_shot(torch.nn.Identity(), w, {"empty": []})
