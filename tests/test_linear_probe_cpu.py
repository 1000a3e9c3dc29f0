"""The logistic-regression linear probe without a GPU: the host L-BFGS of clipa_amd/linear_probe.py on fp64 closures against
scikit-learn, its "line_search" stop, the sweep's visiting order and tie rule on a stubbed fit, the fixture of
tools/make_linear_probe_golden.py against the restatement that made it, and every argument error (raised before any kernel
is reached)."""
import os
from unittest import mock

import numpy as np
import pytest
import torch

import clipa_amd
from clipa_amd import linear_probe as P

from . import linear_probe_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "linear_probe.npz")
K = L.FIXTURE
SHAPE = (K["c"], K["d"] + 1)


@pytest.fixture(scope="module")
def golden():
    return np.load(FIXTURE, allow_pickle=False)


@pytest.fixture(scope="module")
def fp64_fit(golden):
    """The package's L-BFGS on the exact objective of the fixture problem, at gtol = 1e-9."""
    value, grad = L.closures(L.objective_fp64, golden["x"], golden["y"], SHAPE, float(golden["l2"]))
    x, f, gmax, its, evals, status = P.lbfgs(value, grad, np.zeros(SHAPE).reshape(-1), gtol=1e-9)
    return x.reshape(SHAPE), f, gmax, its, evals, status


def test_module_is_exported():
    assert clipa_amd.linear_probe is P and callable(P.linear_probe)
    assert clipa_amd.fit_logreg is P.fit_logreg and clipa_amd.logreg_objective is P.logreg_objective
    assert clipa_amd.sweep_l2 is P.sweep_l2 and clipa_amd.evaluate_linear_probe is P.evaluate_linear_probe


def test_fixture_is_what_the_restatement_gives(golden):
    z = golden
    x, y, xt, yt = L.fixture_inputs()
    for got, want in ((x, z["x"]), (y, z["y"]), (xt, z["x_test"]), (yt, z["y_test"])):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert x.shape == (K["n"], K["d"]) and xt.shape == (K["nt"], K["d"]) and float(z["l2"]) == K["l2"]
    assert z["theta_star"].shape == SHAPE and abs(z["theta_star"][:, -1].mean()) < 1e-15
    f, g, _ = L.objective_fp64(x, y, z["theta_star"], K["l2"])
    assert abs(f - float(z["f_star"])) <= 1e-14 and np.abs(g).max() <= 2 * float(z["g_star"]) <= 1e-7
    stable, pred = L.stable_rows(z["theta_star"], xt, float(z["sim_delta"]))
    assert np.array_equal(pred, z["pred"]) and 0.5 <= float(z["accuracy"]) == np.mean(pred == yt) <= 0.97
    assert 1.0 - stable.mean() == float(z["sim_left_out"]) <= 0.05       # the condition the golden tool refuses to break


def test_lbfgs_matches_scikit_learn_on_the_fixture_problem(golden, fp64_fit):
    """Both minimise one strictly convex function (up to the common bias shift, removed from both).  With mu the smallest
    non-zero eigenvalue of the exact Hessian at the solution, |theta_a - theta_b|_2 <= (|g_a|_2 + |g_b|_2) / mu and
    f_a - f* <= |g_a|_2^2 / (2 mu); the Hessian moves between two points this close by far less than the factor 2 allowed
    below.  Nothing else enters the bounds."""
    sk = pytest.importorskip("sklearn.linear_model")
    x, y, l2 = golden["x"], golden["y"], float(golden["l2"])
    theta, f, gmax, its, evals, status = fp64_fit
    assert status == "converged" and gmax <= 1e-9 and its < 200 and evals < 2 * its + 30
    clf = sk.LogisticRegression(C=1.0 / (l2 * len(y)), tol=1e-12, max_iter=100000, solver="lbfgs").fit(x.astype(np.float64), y)
    theta_sk = L.centre_bias(np.concatenate([clf.coef_, clf.intercept_[:, None]], axis=1))
    eig = np.linalg.eigvalsh(L.hessian_fp64(x, theta, l2))
    assert abs(eig[0]) < 1e-12 and eig[1] > 1e-3         # one null direction, the bias shift
    mu = eig[1] / 2
    for name, other in (("live scikit-learn", theta_sk), ("stored theta_star", golden["theta_star"])):
        f_o, g_o, _ = L.objective_fp64(x, y, other, l2)
        g_a = L.objective_fp64(x, y, theta, l2)[1]
        bound = (np.linalg.norm(g_a) + np.linalg.norm(g_o)) / mu
        dist = np.linalg.norm(L.centre_bias(theta) - other)
        fbound = (np.linalg.norm(g_a) ** 2 + np.linalg.norm(g_o) ** 2) / (2 * mu) + 64 * np.finfo(np.float64).eps * abs(f_o)
        print(f"{name}: |theta - theta_sk|_2 = {dist:.3g} (bound {bound:.3g}), max {np.abs(L.centre_bias(theta) - other).max():.3g}; "
              f"|f - f_sk| = {abs(f - f_o):.3g} (bound {fbound:.3g}); {its} iterations")
        assert dist <= bound and abs(f - f_o) <= fbound


def test_line_search_stop_when_no_step_decreases_f():
    """A gradient of the wrong sign: every probe goes uphill.  One start value and 1 + 25 probes, then "line_search" with the
    start point returned - not a loop that keeps halving."""
    calls = []

    def value(x):
        calls.append(x.copy())
        return 1.0 + float(np.sum(x ** 2))

    x0 = np.array([1.0, -2.0])
    x, f, gmax, its, evals, status = P.lbfgs(value, lambda: -2.0 * calls[-1], x0, gtol=1e-9)
    assert status == "line_search" and its == 0 and evals == len(calls) == 2 + P.MAX_HALVINGS == 27
    assert np.array_equal(x, x0) and f == 6.0 and gmax == 4.0
    steps = [np.linalg.norm(c - x0) for c in calls[1:]]
    assert np.allclose(np.array(steps[:-1]) / np.array(steps[1:]), 2.0)


def test_line_search_stop_at_the_float32_noise_floor(golden, fp64_fit):
    """The fixture problem in simulated float32 with a gtol far below what float32 can reach: the fit ends "line_search"
    after a bounded number of evaluations and returns its best iterate, close to the exact solution; at the default gtol the
    same simulation converges."""
    x, y, l2 = golden["x"], golden["y"], float(golden["l2"])
    seen = []
    value, grad = L.closures(L.objective_fp32, x, y, SHAPE, l2)
    xs, f, gmax, its, evals, status = P.lbfgs(lambda v: (seen.append(value(v)), seen[-1])[1], grad, np.zeros(SHAPE).reshape(-1),
                                              gtol=1e-12)
    print(f"fp32 simulation, gtol 1e-12: {status} after {its} iterations / {evals} evaluations at max |g| = {gmax:.3g}")
    assert status == "line_search" and evals == len(seen) < 1000 and gmax < 1e-5
    assert f == min(seen)                                # the best iterate
    assert np.abs(L.centre_bias(xs.reshape(SHAPE)) - L.centre_bias(fp64_fit[0])).max() < 1e-4
    out = P.lbfgs(value, grad, np.zeros(SHAPE).reshape(-1))
    assert out[5] == "converged" and out[2] <= P.DEFAULT_GTOL == 1e-5 and out[3] == int(golden["sim_iterations"])


def test_lbfgs_skips_pairs_without_positive_curvature_and_honours_max_iter():
    """f = -cos on [-1, 1]-ish starts is convex there; a concave stretch (f = cos) gives s.y < 0: the pair is dropped and the
    iteration goes on downhill instead of dividing by a negative curvature."""
    at = {}
    value = lambda v: (at.update(x=v.copy()), float(np.sum(np.cos(v))))[1]      # noqa: E731
    out = P.lbfgs(value, lambda: -np.sin(at["x"]), np.array([0.3, -0.2, 0.1]), gtol=1e-10)
    assert out[5] == "converged" and np.allclose(np.abs(out[0]), np.pi) and abs(out[1] + 3.0) < 1e-12
    out = P.lbfgs(value, lambda: -np.sin(at["x"]), np.array([0.3, -0.2, 0.1]), gtol=1e-10, max_iter=2)
    assert out[5] == "max_iter" and out[3] == 2
    assert P.lbfgs(value, lambda: -np.sin(at["x"]), np.array([np.pi]), gtol=1e-10)[3:] == (0, 1, "converged")


def test_search_grid_visits_the_papers_order_with_warm_starts_and_ties_to_the_larger_lambda():
    grid = np.logspace(-6, 6, 97)
    calls = []
    acc = lambda i: 0.9 - 0.01 * abs(i - 45)      # noqa: E731     peak at index 45
    best, seen = P.search_grid(97, 16, lambda i, warm: (calls.append((i, warm)), acc(i))[1])
    coarse = [0, 16, 32, 48, 64, 80, 96]
    assert np.allclose(grid[coarse], [1e-6, 1e-4, 1e-2, 1, 1e2, 1e4, 1e6])
    # 48 wins the coarse pass; 40 / 56 -> 48; 44 / 52 -> 44; 42 / 46 -> 46 (tie at 0.89 with 44: the larger); 45 / 47 -> 45
    assert list(seen) == [i for i, _ in calls] == coarse + [40, 56, 44, 52, 42, 46, 45, 47]
    assert best == 45 and seen[45] == acc(45)
    # each fit starts from the nearest index already solved, the larger of two equally near
    assert [w for _, w in calls] == [None, 0, 16, 32, 48, 64, 80, 48, 64, 48, 56, 44, 48, 46, 48]
    # a plateau: ties go to the larger lambda at every stage
    best, seen = P.search_grid(97, 16, lambda i, warm: 0.5)
    assert best == 96 and list(seen) == coarse + [88, 92, 94, 95]
    # edges of the grid are not stepped over
    best, seen = P.search_grid(97, 16, lambda i, warm: -float(i))
    assert best == 0 and list(seen) == coarse + [8, 4, 2, 1]
    assert P.search_grid(1, 16, lambda i, warm: 1.0) == (0, {0: 1.0})
    with pytest.raises(RuntimeError, match="power of two"):
        P.search_grid(97, 12, lambda i, warm: 0.0)


def test_sweep_l2_returns_lambdas_and_warm_starts_from_solved_ones():
    """sweep_l2 with the fit and the kernels stubbed out: what it hands to the fit and what it returns."""
    x, y, xt, yt = _problem()
    fits = []

    def fit(prep, yd, c, l2, max_iter, gtol, history, theta0):
        fits.append((l2, None if theta0 is None else float(theta0[0, 0])))
        return {"theta": np.full((c, 7), l2), "f": 0.0, "gnorm": 0.0, "iterations": 1, "evaluations": 1, "status": "converged"}

    score = lambda theta, xp, yv: (int(5 - min(5, abs(np.log10(theta[0, 0]) - 0.5))), None, None)      # noqa: E731   peak near 10^0.5
    with mock.patch.object(torch.Tensor, "is_cuda", True), mock.patch.object(P, "ops", mock.MagicMock()), \
            mock.patch.object(P, "Prepared", mock.MagicMock()), mock.patch.object(P, "_on", lambda d, v: v), \
            mock.patch.object(P, "_fit", fit), mock.patch.object(P, "_score", score), \
            mock.patch.object(torch.Tensor, "to", lambda self, *a, **k: self):
        best, seen = P.sweep_l2(x, y, xt, yt, 3)
    grid = np.logspace(-6, 6, 97)
    assert list(seen)[:7] == [float(v) for v in grid[::16]] and best in seen and best == max(k for k, v in seen.items() if v == max(seen.values()))
    assert [l for l, _ in fits] == list(seen) and fits[0][1] is None
    assert all(w in seen for _, w in fits[1:])            # warm starts are solutions of lambdas already visited
    assert all(isinstance(v, np.float64) for v in seen.values())


def test_c_entries_on_zero_sized_inputs_and_bad_arguments():
    """Nothing to write: CLIPA_OK before any pointer is looked at or any launch is made (so it runs without a GPU); argument
    errors are loud."""
    from clipa_amd import lib
    h = lib.load()
    assert h.clipa_logreg_prepare(None, 0, 7, 7, None, 8, None, 0, None) == 0
    assert h.clipa_logreg_logits(None, None, 0, 0, 8, 8, 8, None, 0, None, None, None, None) == 0
    assert h.clipa_logreg_logits(None, None, 3, 0, 8, 8, 8, None, 0, None, None, None, None) == 0
    assert h.clipa_logreg_residual(None, None, None, 3, 0, 0, None, 1, None) == 0
    assert h.clipa_logreg_grad(None, None, 0, 8, 5, 8, 8, None, 8, 0, 0, None, 0, None) == 0
    assert h.clipa_logreg_grad(None, None, 3, 0, 5, 8, 8, None, 0, 0, 0, None, 0, None) == 0
    assert h.clipa_logreg_logits(None, None, 0, 5, 8, 8, 8, None, 8, None, None, None, None) < 0 and "softmax over nothing" in lib.last_error()
    assert h.clipa_logreg_residual(None, None, None, 0, 5, 8, None, 1, None) < 0 and "C = 0" in lib.last_error()
    assert h.clipa_logreg_logits(None, None, 3, 1 << 21, 8, 8, 8, None, 1 << 21, None, None, None, None) < 0 and "below 2^21" in lib.last_error()
    assert h.clipa_logreg_prepare(None, 1 << 21, 7, 7, None, 8, None, 1 << 21, None) < 0 and "below 2^21" in lib.last_error()
    assert h.clipa_logreg_logits(None, None, 3, 5, 8, 8, 8, None, 8, None, None, None, None) < 0 and "null" in lib.last_error()
    assert h.clipa_logreg_logits(None, None, 3, 5, 7, 7, 8, None, 8, None, None, None, None) < 0 and "multiples of 4" in lib.last_error()
    assert h.clipa_logreg_logits(None, None, 3, 5, 8, 8, 8, None, 4, None, None, None, None) < 0 and "ldz" in lib.last_error()
    assert h.clipa_logreg_prepare(None, 5, 7, 7, None, 7, None, 8, None) < 0 and "ld = 7" in lib.last_error()
    assert h.clipa_logreg_grad(None, None, 3, 8, 5, 8, 8, None, 8, 6, 0, None, 0, None) < 0 and "slice" in lib.last_error()
    assert h.clipa_logreg_grad(None, None, 3, 8, 5, 8, 8, None, 4, 0, 0, None, 0, None) < 0 and "ldg" in lib.last_error()
    assert h.clipa_logreg_grad(None, None, 3, 8, 5, 4, 8, None, 8, 0, 0, None, 0, None) < 0 and "lda" in lib.last_error()
    # three slices of 128 over N = 300: [C, dim rounded up to 4] floats each; a single slice needs none
    assert h.clipa_logreg_grad_workspace(130, 71, 300, 128) == 3 * 130 * 72 * 4 and h.clipa_logreg_grad_workspace(130, 71, 300, 0) == 0 == h.clipa_logreg_grad_workspace(130, 71, 4096, 0)
    assert h.clipa_logreg_grad_workspace(1000, 1025, 1281167, 0) == 313 * 1000 * 1028 * 4


def _problem():
    rng = np.random.RandomState(1)
    return (torch.from_numpy(rng.standard_normal((12, 6)).astype(np.float32)), np.repeat(np.arange(3), 4),
            torch.from_numpy(rng.standard_normal((5, 6)).astype(np.float32)), np.array([0, 1, 2, 0, 1]))


def test_cpu_features_raise():
    x, y, xt, yt = _problem()
    with pytest.raises(RuntimeError, match="GPU"):
        P.linear_probe(x, y, xt, yt, 3, 1.0)
    with pytest.raises(RuntimeError, match="GPU"):
        P.fit_logreg(x, y, 3, 1.0)
    with pytest.raises(RuntimeError, match="GPU"):
        P.sweep_l2(x, y, xt, yt, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        P.prepare(x.numpy())
    with pytest.raises(RuntimeError, match="GPU"):
        clipa_amd.ops.logreg_prepare(x)
    with pytest.raises(RuntimeError, match="GPU"):
        clipa_amd.ops.logreg_logits(torch.zeros(3, 7), torch.zeros(12, 7))


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
    with mock.patch.object(torch.Tensor, "is_cuda", True), mock.patch.object(P, "ops", None):
        for match, make in bad:
            with pytest.raises(RuntimeError, match=match):
                P.linear_probe(*make(), 3, 1.0)
            with pytest.raises(RuntimeError, match=match):
                P.sweep_l2(*make(), 3)
        for make in (bad[0][1], bad[2][1], bad[4][1], bad[6][1]):
            with pytest.raises(RuntimeError, match="non-finite|0, 3|one integer|empty"):
                P.fit_logreg(*make()[:2], 3, 1.0)
        for l2 in (0.0, -1.0, float("nan")):
            with pytest.raises(RuntimeError, match="l2"):
                P.linear_probe(x, y, xt, yt, 3, l2)
            with pytest.raises(RuntimeError, match="l2"):
                P.fit_logreg(x, y, 3, l2)
            with pytest.raises(RuntimeError, match="l2"):
                list(P.evaluate_linear_probe(None, {}, l2=l2))
        with pytest.raises(RuntimeError, match="num_classes"):
            P.linear_probe(x, y, xt, yt, 0, 1.0)
        with pytest.raises(RuntimeError, match="ascending"):
            P.sweep_l2(x, y, xt, yt, 3, grid=[1.0, 0.5])
        with pytest.raises(RuntimeError, match="ascending"):
            P.sweep_l2(x, y, xt, yt, 3, grid=[0.0, 0.5])
        with pytest.raises(RuntimeError, match="representation"):
            list(P.evaluate_linear_probe(None, {}, representation="pooled"))
        with pytest.raises(RuntimeError, match="no validation split"):
            list(P.evaluate_linear_probe(None, {"a": ([], None, [], 3)}))
