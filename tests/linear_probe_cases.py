"""Host restatements of the logistic-regression linear probe (clipa_amd/linear_probe.py, csrc/logreg.hip; Radford et al. 2021,
appendix A.3), shared by tools/make_linear_probe_golden.py and the linear-probe tests.

  objective   f(theta) = (1 / N) sum_n (lse_n - z_{n, y_n}) + (l2 / 2) ||theta[:, :-1]||^2 with z_n = theta [x_n, 1] and
              lse_n = log sum_c exp z_{n, c}; theta [C, D + 1], the last column the (unpenalised) bias;
  gradient    (1 / N) (softmax(z) - onehot(y))^T [x, 1] + l2 [theta[:, :-1], 0].

`objective_fp64` is the ground truth.  `objective_fp32` does the same steps in float32 - products, exp, log and sums - with
only the sum over n, the 1 / N and the L2 term in float64, as the engine splits them: it stands in for the device when no
GPU is there (its summation orders are numpy's, not the kernels').  `SHAPES` is the case table of the kernel tests.
"""
import numpy as np

# (N, D, C): N = 300 is three sample tiles, the last with 44 rows, and no multiple of the gradient product's 32-wide k stage;
# D = 70 gives dim = 71, ragged against 32 and padded to 72; C = 130 is two class tiles, the second with 2 classes.
SHAPES = {"two class tiles": (300, 70, 130), "few classes": (300, 70, 3), "few rows": (5, 70, 130)}

# unit noise around prototypes of scale 0.4: features of order one, as an encoder's, and a Hessian whose eigenvalues span
# 0.026 .. 0.58 - at gtol = 1e-5 the fit stops well above the float32 noise floor of the objective
FIXTURE = dict(n=600, d=48, c=10, l2=0.1, nt=400, proto=0.4, noise=1.0, seed=9301)


def with_ones(x):
    return np.concatenate([x, np.ones((len(x), 1), dtype=x.dtype)], axis=1)


def lse_fp64(z):
    """log sum exp over the last axis of a float64 array."""
    z = np.asarray(z, dtype=np.float64)
    m = z.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))[..., 0]


def objective_fp64(x, y, theta, l2):
    """-> (f, g [C, D + 1], logits [N, C]) in float64."""
    xt = with_ones(np.asarray(x, dtype=np.float64))
    theta = np.asarray(theta, dtype=np.float64)
    z = xt @ theta.T
    lse = lse_fp64(z)
    n = len(y)
    f = float(np.mean(lse - z[np.arange(n), y]) + 0.5 * l2 * np.sum(theta[:, :-1] ** 2))
    p = np.exp(z - lse[:, None])
    p[np.arange(n), y] -= 1.0
    g = p.T @ xt / n
    g[:, :-1] += l2 * theta[:, :-1]
    return f, g, z


def objective_fp32(x, y, theta, l2):
    """-> (f, g) with the device's split of precisions: float32 products, exp, log and residual; float64 from the sum over n on."""
    f32 = np.float32
    xt = with_ones(np.asarray(x, dtype=f32))
    th = np.asarray(theta, dtype=np.float64)
    z = xt @ th.astype(f32).T
    m = z.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True, dtype=f32)))[:, 0]
    n = len(y)
    assert z.dtype == f32 and lse.dtype == f32
    ce = lse - z[np.arange(n), y]
    f = float(ce.astype(np.float64).sum() / n + 0.5 * l2 * np.sum(th[:, :-1] ** 2))
    p = np.exp(z - lse[:, None])
    p[np.arange(n), y] -= f32(1.0)
    g = (p.T @ xt).astype(np.float64) / n
    g[:, :-1] += l2 * th[:, :-1]
    return f, g


def closures(objective, x, y, shape, l2):
    """(value, grad) as clipa_amd.linear_probe.lbfgs takes them, on flat float64 vectors."""
    at = {}

    def value(v):
        at["f"], at["g"] = objective(x, y, v.reshape(shape), l2)[:2]
        return at["f"]

    return value, lambda: at["g"].reshape(-1)


def centre_bias(theta):
    """Softmax is invariant to a common shift of the biases, and they are unpenalised: solutions compare after removing it."""
    theta = np.array(theta, dtype=np.float64)
    theta[:, -1] -= theta[:, -1].mean()
    return theta


def hessian_fp64(x, theta, l2):
    """The [C * dim, C * dim] Hessian of the objective at theta (float64): block (c, c') = X~^T diag(p_c (delta_cc' - p_c')) X~ / N,
    plus l2 on the weights.  Its only null direction is the common bias shift."""
    xt = with_ones(np.asarray(x, dtype=np.float64))
    n, dim = xt.shape
    z = xt @ np.asarray(theta, dtype=np.float64).T
    p = np.exp(z - lse_fp64(z)[:, None])
    c = p.shape[1]
    h = np.zeros((c, dim, c, dim))
    for a in range(c):
        for b in range(a, c):
            w = p[:, a] * ((a == b) - p[:, b])
            h[a, :, b, :] = h[b, :, a, :] = (xt * w[:, None]).T @ xt / n
        h[a, np.arange(dim - 1), a, np.arange(dim - 1)] += l2
    return h.reshape(c * dim, c * dim)


def fixture_inputs():
    """The end-to-end problem: class prototypes plus noise.  -> x [N, D] f32, y int64, x_test [Nt, D] f32, y_test int64."""
    k = FIXTURE
    rng = np.random.RandomState(k["seed"])
    proto = k["proto"] * rng.standard_normal((k["c"], k["d"]))
    y = rng.randint(0, k["c"], size=k["n"])
    yt = rng.randint(0, k["c"], size=k["nt"])
    x = proto[y] + k["noise"] * rng.standard_normal((k["n"], k["d"]))
    xt = proto[yt] + k["noise"] * rng.standard_normal((k["nt"], k["d"]))
    return x.astype(np.float32), y.astype(np.int64), xt.astype(np.float32), yt.astype(np.int64)


def stable_rows(theta_star, x_test, delta):
    """Rows whose argmax under theta_star no theta within delta (max norm, after bias centring) can change: a logit moves by
    at most delta * ||x~||_1, so a top-two gap above 2 delta ||x~||_1 keeps its winner.  -> (mask [Nt], predictions [Nt])."""
    xt = with_ones(np.asarray(x_test, dtype=np.float64))
    z = xt @ centre_bias(theta_star).T
    top = np.sort(z, axis=1)
    gap = top[:, -1] - top[:, -2]
    return gap > 2.0 * delta * np.abs(xt).sum(axis=1), np.argmax(z, axis=1)
