"""Generate tests/golden/linear_probe.npz: the end-to-end problem of the logistic-regression linear probe
(clipa_amd/linear_probe.py) with its solution from scikit-learn.  Run (numpy and scikit-learn; only this tool needs the latter):
    python tools/make_linear_probe_golden.py

The problem (tests/linear_probe_cases.py: FIXTURE, fixture_inputs): N = 600 train rows, D = 48, C = 10, l2 = 0.1, 400 test
rows; class prototypes plus noise.  theta_star is scikit-learn's LogisticRegression(C = 1 / (l2 * N), tol = 1e-12) on the
float64 features - the same objective, tests/linear_probe_cases.py: objective_fp64 - with the common bias shift removed.  Its
own float64 gradient (printed, and stored as g_star) is where scikit-learn's stopping rule left it, near 2e-8.

What the tests ask of a fit at the default gtol is decided here, with the device's arithmetic simulated in float32 on the CPU
(objective_fp32) and fitted by the package's own L-BFGS: with delta = max |theta - theta_star| after bias centring, a test
row whose top-two logit gap under theta_star exceeds 2 delta ||x~||_1 cannot change its argmax (stable_rows); the other rows
are left out of the comparison, and they may be at most 5 % of the test set.  The tool refuses to write a fixture whose
simulated fit leaves out more, or does not end "converged".  It prints the simulated max |g_fp64 - g_fp32| at the solution,
the number `fit_logreg`'s docstring quotes.
Stored: x, y, x_test, y_test (as generated), l2, theta_star, f_star, the fp64 test predictions and top-two gaps, and the
simulated fit's delta, left-out fraction, iterations and gradient difference (records, not expectations).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import linear_probe_cases as L      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "linear_probe.npz")
MAX_LEFT_OUT = 0.05


def solve(x, y, c, l2):
    from sklearn.linear_model import LogisticRegression
    n = len(y)
    clf = LogisticRegression(C=1.0 / (l2 * n), tol=1e-12, max_iter=100000, solver="lbfgs").fit(x.astype(np.float64), y)
    assert list(clf.classes_) == list(range(c))
    return L.centre_bias(np.concatenate([clf.coef_, clf.intercept_[:, None]], axis=1))


def main():
    from clipa_amd import linear_probe as P
    k = L.FIXTURE
    x, y, xt, yt = L.fixture_inputs()
    c, l2, shape = k["c"], k["l2"], (k["c"], k["d"] + 1)
    theta = solve(x, y, c, l2)
    f_star, g_star, _ = L.objective_fp64(x, y, theta, l2)
    print(f"theta_star: f = {f_star:.15g}, max |g_fp64| = {np.abs(g_star).max():.3g}")
    assert np.abs(g_star).max() < 1e-6

    value, grad = L.closures(L.objective_fp32, x, y, shape, l2)
    sim, _, gmax, its, evals, status = P.lbfgs(value, grad, np.zeros(shape).reshape(-1), gtol=P.DEFAULT_GTOL)
    sim = sim.reshape(shape)
    gdiff = np.abs(L.objective_fp64(x, y, sim, l2)[1] - L.objective_fp32(x, y, sim, l2)[1]).max()
    delta = np.abs(L.centre_bias(sim) - theta).max()
    stable, pred = L.stable_rows(theta, xt, delta)
    left_out = 1.0 - stable.mean()
    print(f"simulated fp32 fit at gtol {P.DEFAULT_GTOL:g}: {status} after {its} iterations / {evals} evaluations, max |g| = {gmax:.3g}, "
          f"max |g_fp64 - g_fp32| = {gdiff:.3g}, delta = {delta:.3g}, rows left out {left_out:.2%}")
    if status != "converged" or left_out > MAX_LEFT_OUT:
        raise SystemExit(f"refusing to write {OUT}: the simulated fit ended {status!r} and leaves out {left_out:.2%} of the test "
                         f"rows (at most {MAX_LEFT_OUT:.0%})")
    sim_pred = np.argmax(L.with_ones(xt.astype(np.float64)) @ sim.T, axis=1)
    assert np.array_equal(sim_pred[stable], pred[stable])
    z = L.with_ones(xt.astype(np.float64)) @ theta.T
    top = np.sort(z, axis=1)
    acc = float(np.mean(pred == yt))
    print(f"fp64 test accuracy {acc:.4f}")
    assert 0.5 <= acc <= 0.97, "a saturated or hopeless problem would show nothing"
    np.savez_compressed(OUT, x=x, y=y, x_test=xt, y_test=yt, l2=np.float64(l2), theta_star=theta, f_star=np.float64(f_star), g_star=np.float64(np.abs(g_star).max()),
                        pred=pred.astype(np.int64), gap=top[:, -1] - top[:, -2], accuracy=np.float64(acc),
                        sim_delta=np.float64(delta), sim_left_out=np.float64(left_out), sim_iterations=np.int64(its),
                        sim_gdiff=np.float64(gdiff))
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
