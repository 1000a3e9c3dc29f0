"""The few-shot linear probe without a GPU: the host-side task sampling against the reference's recipe, the fixture of
tools/make_fewshot_golden.py against the two restatements that made it (tests/fewshot_cases.py) and against its own
conditions, the route switch, and every argument error of clipa_amd/fewshot.py (raised before any kernel is reached)."""
import os
from unittest import mock

import numpy as np
import pytest
import torch

import clipa_amd
from clipa_amd import fewshot
from tools import make_fewshot_golden as G

from . import fewshot_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "fewshot_lsr.npz")
NAMES = ("A1", "A2", "B1", "B2", "E")


@pytest.fixture(scope="module")
def golden():
    return np.load(FIXTURE, allow_pickle=False)


def test_module_is_exported():
    assert clipa_amd.fewshot is fewshot and clipa_amd.fewshot_lsr is fewshot.fewshot_lsr
    assert clipa_amd.fewshot_metrics is fewshot.fewshot_metrics and clipa_amd.evaluate_fewshot is fewshot.evaluate_fewshot


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_class_indices_follow_the_numpy_recipe(seed):
    labels = np.random.RandomState(seed).randint(0, 9, size=200)
    labels[labels == 4] = 5                               # an empty class draws from the generator too
    rng = np.random.default_rng(seed)
    want = [rng.permutation(np.where(labels == c)[0]) for c in range(9)]
    for got in (fewshot.class_indices(labels, 9, seed), fewshot.class_indices(torch.from_numpy(labels), 9, seed)):
        assert len(got) == 9 and len(got[4]) == 0
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert sorted(np.concatenate(want).tolist()) == list(range(200))
    sub = F.subsets(labels, 9, seed, (1, 3))
    assert np.array_equal(sub[3][0], np.concatenate([w[:3] for w in want])) and (np.diff(sub[3][1]) >= 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_restatements_agree_with_the_fixture(golden, name):
    """Pins the fixture: the fp64 restatement reproduces the stored predictions and maxima, the fp32 one (the stand-in for the
    reference's arithmetic; its LAPACK may differ from the generating machine's) stays inside the bound the engine gets."""
    z, k = golden, G.CASES[name]
    for key in ("c", "d", "shots", "l2", "seed", "noise"):
        assert float(z[f"{name}_{key}"]) == float(k[key]), key
    x, y, xt, yt = G.case_inputs(name, z[f"{name}_redraws"])
    assert x.dtype == np.float32 and x.shape == (k["c"] * k["shots"], k["d"]) and xt.shape == (G.NT, k["d"])
    assert np.array_equal(yt, z[f"{name}_y_test"])
    l64 = F.lsr_fp64(x, y, xt, k["c"], k["l2"])
    assert np.array_equal(np.argmax(l64, axis=1), z[f"{name}_pred"])
    assert np.abs(l64.max(1) - z[f"{name}_best"]).max() <= 1e-9
    l32, route = F.lsr_fp32(x, y, xt, k["c"], k["l2"])
    dev = float(z[f"{name}_dev"])
    assert route == str(z[f"{name}_route"])
    assert np.array_equal(np.argmax(l32, axis=1), z[f"{name}_pred"])
    assert np.abs(l32.astype(np.float64) - l64).max() <= 8 * dev


@pytest.mark.parametrize("name", NAMES)
def test_fixture_meets_its_own_conditions(golden, name):
    z = golden
    dev, margin = float(z[f"{name}_dev"]), float(z[f"{name}_margin"])
    assert dev > 0 and margin == G.MARGIN_FACTOR * dev == 64 * dev
    assert z[f"{name}_gap"].min() >= margin                 # no row inside the margin
    acc = float(z[f"{name}_accuracy"])
    assert 0.5 <= acc <= 0.97
    assert int(z[f"{name}_correct"]) == int((z[f"{name}_pred"] == z[f"{name}_y_test"]).sum()) == round(acc * G.NT)
    n, dim = int(z[f"{name}_c"]) * int(z[f"{name}_shots"]), int(z[f"{name}_d"]) + 1
    assert str(z[f"{name}_route"]) == ("A" if n >= dim else "B") == {"A1": "A", "A2": "A", "B1": "B", "B2": "B", "E": "A"}[name]
    if name == "E":
        assert n == dim


def test_route_switch_at_the_boundary():
    assert fewshot.route(60, 60) == "A" and fewshot.route(59, 60) == "B" and fewshot.route(61, 60) == "A"
    rng = np.random.RandomState(0)
    y = np.repeat(np.arange(4), 5)
    for d, want in ((19, "A"), (20, "B")):                  # N = 20: dim = 20 -> A, dim = 21 -> B
        x = rng.standard_normal((20, d)).astype(np.float32)
        logits, route = F.lsr_fp32(x, y, x, 4, 2.0)
        assert route == want == fewshot.route(20, d + 1)
        assert np.abs(logits - F.lsr_fp64(x, y, x, 4, 2.0)).max() < 1e-3      # the two routes are one solution


def test_c_entries_on_zero_sized_inputs():
    """Nothing to write: CLIPA_OK before any pointer is looked at or any launch is made (so it runs without a GPU).  The one
    documented exception is an argmax over no classes."""
    from clipa_amd import lib
    h = lib.load()
    assert h.clipa_fewshot_moments(None, None, 0, 0, 0, 0, None, None, None) == 0
    assert h.clipa_fewshot_moments(None, None, 5, 5, 0, 0, None, None, None) == 0
    assert h.clipa_fewshot_whiten(None, None, 0, 0, 7, 7, None, None, None, 8, None, 0, None) == 0
    assert h.clipa_fewshot_gram(None, 0, 5, 8, None, 0, None) == 0
    assert h.clipa_fewshot_class_sums(None, None, 0, 0, 3, 0, None, 3, None) == 0
    assert h.clipa_fewshot_class_sums(None, None, 4, 5, 0, 8, None, 0, None) == 0
    assert h.clipa_fewshot_predict(None, None, 0, 0, 0, 0, 0, None, None, None) == 0
    assert h.clipa_fewshot_predict(None, None, 3, 0, 4, 4, 4, None, None, None) < 0 and "argmax over nothing" in lib.last_error()
    assert h.clipa_fewshot_gram(None, 3, 5, 8, None, 3, None) < 0 and "null" in lib.last_error()
    assert h.clipa_fewshot_whiten(None, None, 2, 2, 7, 7, None, None, None, 7, None, 0, None) < 0 and "ldz" in lib.last_error()


def _problem():
    rng = np.random.RandomState(1)
    return (torch.from_numpy(rng.standard_normal((12, 6)).astype(np.float32)), np.repeat(np.arange(3), 4),
            torch.from_numpy(rng.standard_normal((5, 6)).astype(np.float32)), np.array([0, 1, 2, 0, 1]))


def test_cpu_features_raise():
    x, y, xt, yt = _problem()
    with pytest.raises(RuntimeError, match="GPU"):
        fewshot.fewshot_lsr(x, y, xt, yt, 3, 1.0)
    with pytest.raises(RuntimeError, match="GPU"):
        fewshot.fewshot_metrics(x, y, xt, yt, 3, (1,), 1.0, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        fewshot.fewshot_lsr(x.numpy(), y, xt, yt, 3, 1.0)


def test_argument_errors_are_raised_before_any_kernel():
    """The checks behind the device check, reached here by letting CPU tensors claim to be on the GPU; ops is replaced by a
    mock that fails the test if a kernel wrapper is reached."""
    x, y, xt, yt = _problem()
    bad = [("non-finite", lambda: (torch.where(torch.eye(12, 6) > 0, torch.tensor(float("nan")), x), y, xt, yt)),
           ("non-finite", lambda: (x, y, xt * float("inf"), yt)),
           (r"\[0, 3\)", lambda: (x, np.where(y == 2, 3, y), xt, yt)),
           (r"\[0, 3\)", lambda: (x, y, xt, np.array([0, 1, -1, 0, 1]))),
           ("one integer label per row", lambda: (x, y[:-1], xt, yt)),
           ("one integer label per row", lambda: (x, y.astype(np.float32), xt, yt)),
           ("empty", lambda: (x[:0], y[:0], xt, yt)),
           ("empty", lambda: (x, y, xt[:0], yt[:0])),
           ("2-D float GPU tensor", lambda: (x[0], y, xt, yt)),
           ("2-D float GPU tensor", lambda: (x.long(), y, xt, yt)),
           ("widths differ", lambda: (x, y, xt[:, :5], yt))]
    with mock.patch.object(torch.Tensor, "is_cuda", True), mock.patch.object(fewshot, "ops", None):
        for match, make in bad:
            with pytest.raises(RuntimeError, match=match):
                fewshot.fewshot_lsr(*make(), 3, 1.0)
            with pytest.raises(RuntimeError, match=match):
                fewshot.fewshot_metrics(*make(), 3, (1, 2), 1.0, 0)
        with pytest.raises(RuntimeError, match="l2_reg"):
            fewshot.fewshot_lsr(x, y, xt, yt, 3, 0.0)
        with pytest.raises(RuntimeError, match="num_classes"):
            fewshot.fewshot_lsr(x, y, xt, yt, 0, 1.0)
        with pytest.raises(RuntimeError, match="representation"):
            list(fewshot.evaluate_fewshot(None, {}, representation="pooled"))
