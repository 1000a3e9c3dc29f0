"""Logistic-regression linear-probe evaluation through the MI355X engine: the linear probe of Radford et al. 2021 ("Learning
Transferable Visual Models From Natural Language Supervision", section 3.2 and appendix A.3) - an L2-regularised multinomial
logistic regression on frozen image features, fitted with L-BFGS for at most 1000 iterations, the regularisation strength found
by a sweep on a validation split.  The reference has no such evaluator; users ran it by copying `encode_image` outputs to the
host and waiting for scikit-learn.

Here the features stay on the GPU.  With x~ = [x, 1] and theta [C, D + 1] (class-major, the last column the bias) the objective is

    f(theta) = (1 / N) sum_n (lse_n - z_{n, y_n}) + (l2 / 2) ||theta[:, :-1]||^2,    z_n = theta x~_n,  lse_n = log sum_c exp z_{n, c}

whose two [N, C, D + 1] products per evaluation (the logits and the gradient) are fp32 HIP kernels on the project's bit-
reproducible 128 x 128 tile (`ops.logreg_*`, csrc/logreg.hip).  The optimiser - L-BFGS with Armijo backtracking - runs on the
host in numpy fp64 and sees the device as a function: theta goes down and the gradient comes back ((C * (D + 1) values each),
once per evaluation; features never travel.  The sum over n, the 1 / N and the L2 term are fp64 on the host.

`l2` is the coefficient of the formula above.  scikit-learn's `LogisticRegression(C=C_sklearn)` minimises
sum_n ce_n + ||W||^2 / (2 C_sklearn), the same problem with  l2 = 1 / (C_sklearn * N).  The bias is not penalised in either.
There is no scipy / scikit-learn dependency and no host fallback.
"""
import numpy as np
import torch

from . import ops
from ._eval_common import _features, _inference
from .fewshot import _labels, _represent
from .ops import LOGREG_MAX_N

DEFAULT_GTOL = 1e-5
ARMIJO_C1 = 1e-4
MAX_HALVINGS = 25


# ---- the device objective --------------------------------------------------------------------------------------------------
class Prepared:
    """The device operands of one training set (ops.logreg_prepare): xp [N, dim] = [x, 1], xt [dim, N] its transpose, and the
    [C, N] logits buffer every evaluation writes (C * N * 4 bytes, allocated at the first evaluation with C classes)."""

    def __init__(self, x):
        self.xp, self.xt = ops.logreg_prepare(x)
        self.n, self.dim = self.xp.shape
        self.device = x.device
        self._zt = None

    def logits_buffer(self, num_classes):
        if self._zt is None or self._zt.shape[0] != num_classes:
            self._zt = torch.empty((num_classes, (self.n + 3) // 4 * 4), device=self.device, dtype=torch.float32)[:, :self.n]
        return self._zt


def _check_features(x, name, who):
    x = _features(x, name, who, check_finite=True)
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise RuntimeError(f"clipa_amd.{who}: {name} is empty: shape {tuple(x.shape)}")
    if x.shape[0] >= LOGREG_MAX_N:
        raise RuntimeError(f"clipa_amd.{who}: {name} has {x.shape[0]} rows; the probe takes fewer than 2^21 = {LOGREG_MAX_N}")
    return x


def prepare(x, name="x", who="prepare"):
    """x: 2-D float GPU tensor [N, D] of finite features -> Prepared.  Once per fit (or per sweep)."""
    return Prepared(_check_features(x, name, who))


def _device_labels(y, n, num_classes, name, who, device):
    """Labels validated on the host (one integer in [0, num_classes) per row) -> int32 device tensor."""
    return torch.from_numpy(_labels(y, n, num_classes, name, who).astype(np.int32)).to(device)


def _check_problem(x_train, y_train, x_test, y_test, num_classes, l2, who, other="test"):
    """Every argument check of a fit-and-score call, before any kernel: -> (x_train, y_train, x_test, y_test), the features
    fp32 GPU tensors, the labels host int64 arrays."""
    if int(num_classes) < 1 or not float(l2) > 0.0:
        raise RuntimeError(f"clipa_amd.{who}: num_classes = {num_classes} must be >= 1 and l2 = {l2} > 0")
    x_train, x_test = _check_features(x_train, "x_train", who), _check_features(x_test, f"x_{other}", who)
    if x_train.shape[1] != x_test.shape[1]:
        raise RuntimeError(f"clipa_amd.{who}: feature widths differ: {x_train.shape[1]} vs {x_test.shape[1]}")
    return (x_train, _labels(y_train, x_train.shape[0], int(num_classes), "y_train", who), x_test,
            _labels(y_test, x_test.shape[0], int(num_classes), f"y_{other}", who))


def _on(device, y):
    return torch.from_numpy(y.astype(np.int32)).to(device)


def _theta_device(theta, device):
    """fp64 [C, dim] -> the fp32 [C, dim] view of a [C, dim rounded up to 4] device buffer (rows 16-byte aligned)."""
    c, dim = theta.shape
    buf = np.zeros((c, (dim + 3) // 4 * 4), dtype=np.float32)
    buf[:, :dim] = theta
    return torch.from_numpy(buf).to(device)[:, :dim]


class _Objective:
    """f and its gradient at one point after another.  value(theta) runs the logits product and the cross entropies and leaves
    the logits in place; grad() turns them into the residual and runs the gradient product - so a rejected line-search probe
    costs one product, an accepted one two."""

    def __init__(self, prep, y, num_classes, l2):
        self.prep, self.y, self.c, self.l2 = prep, y, int(num_classes), float(l2)
        self.evaluations = 0
        self._state = None

    def value(self, theta):
        p = self.prep
        theta = np.asarray(theta, dtype=np.float64).reshape(self.c, p.dim)
        zt, lse, pred, _ = ops.logreg_logits(_theta_device(theta, p.device), p.xp, out=p.logits_buffer(self.c))
        ce = ops.logreg_residual(zt, lse, self.y, overwrite=False)
        both = torch.stack([ce.sum(dtype=torch.float64), (pred == self.y).sum().double()]).tolist()      # one transfer
        self._state = (theta, zt, lse, pred)
        self.evaluations += 1
        self.ncorrect = int(both[1])
        return both[0] / p.n + 0.5 * self.l2 * float(np.sum(theta[:, :-1] ** 2))

    def grad(self):
        """The gradient at the point of the last value(): fp64 [C, dim], the bias column unpenalised."""
        theta, zt, lse, _ = self._state
        ops.logreg_residual(zt, lse, self.y, overwrite=True)
        g = ops.logreg_grad(zt, self.prep.xt).cpu().numpy().astype(np.float64) / self.prep.n
        g[:, :-1] += self.l2 * theta[:, :-1]
        self._state = None                         # the logits are gone
        return g


def logreg_objective(prep, y, theta, l2, need_grad=True):
    """One evaluation at theta (array-like [C, D + 1], the last column the bias) on the prepared training rows with labels y
    (host or device integers): -> (f, g, ncorrect) with f = mean(ce) + (l2 / 2) ||theta[:, :-1]||^2
    a Python float (the cross entropies fp32 from the device, their sum and the rest fp64), g its gradient as fp64 numpy
    [C, D + 1] with the bias column unpenalised (None without need_grad), ncorrect the training rows whose argmax is their label
    (lowest class on ties).  Bit-reproducible: the same inputs give the same f, g and predictions."""
    theta = np.asarray(theta, dtype=np.float64)
    if theta.ndim != 2 or theta.shape[1] != prep.dim or theta.shape[0] < 1 or not np.isfinite(theta).all():
        raise RuntimeError(f"clipa_amd.logreg_objective: theta must be a finite [C >= 1, {prep.dim}] array, got {theta.shape}")
    if not float(l2) > 0.0:
        raise RuntimeError(f"clipa_amd.logreg_objective: l2 = {l2} must be > 0")
    obj = _Objective(prep, _device_labels(y, prep.n, theta.shape[0], "y", "logreg_objective", prep.device), theta.shape[0], l2)
    f = obj.value(theta)
    return f, (obj.grad() if need_grad else None), obj.ncorrect


# ---- L-BFGS on the host ----------------------------------------------------------------------------------------------------
def _direction(g, pairs):
    """The two-loop recursion: -H g for the stored (s, y, 1 / s.y) pairs, oldest first; H0 = (s.y / y.y) I of the newest."""
    q = g.copy()
    alphas = []
    for s, y, rho in reversed(pairs):
        a = rho * np.dot(s, q)
        q -= a * y
        alphas.append(a)
    if pairs:
        s, y, _ = pairs[-1]
        q *= np.dot(s, y) / np.dot(y, y)
    for (s, y, rho), a in zip(pairs, reversed(alphas)):
        q += (a - rho * np.dot(y, q)) * s
    return -q


def lbfgs(value, grad, x0, max_iter=1000, gtol=DEFAULT_GTOL, history=10):
    """Minimise a smooth function given as two closures: value(x) -> f(x), and grad() -> the gradient at the x of the last
    value() call (fp64 vectors).  L-BFGS with `history` pairs (a pair is skipped unless s.y > 1e-10 |s| |y|), the step by Armijo
    backtracking from 1 (first iteration: 1 / max(1, |g|)) with at most 25 halvings.  Stops with status
      "converged"    max |g_i| <= gtol
      "line_search"  no step of the backtracking decreased f enough - with an objective that carries rounding noise this is
                     where the noise floor shows; the iterate is the best one seen, as f only ever decreases
      "max_iter"     after max_iter iterations.
    -> (x, f, max |g_i|, iterations, evaluations, status)."""
    x = np.asarray(x0, dtype=np.float64).copy()
    f = value(x)
    g = grad()
    evaluations = 1
    pairs = []
    for it in range(max_iter + 1):
        gmax = float(np.max(np.abs(g))) if g.size else 0.0
        if gmax <= gtol:
            return x, f, gmax, it, evaluations, "converged"
        if it == max_iter:
            break
        d = _direction(g, pairs)
        gd = float(np.dot(g, d))
        if not gd < 0.0:                           # not a descent direction: steepest descent, the history dropped
            pairs, d = [], -g
            gd = -float(np.dot(g, g))
        t = 1.0 if pairs else 1.0 / max(1.0, float(np.linalg.norm(g)))
        for _ in range(MAX_HALVINGS + 1):
            xn = x + t * d
            fn = value(xn)
            evaluations += 1
            if fn <= f + ARMIJO_C1 * t * gd:
                break
            t *= 0.5
        else:
            return x, f, gmax, it, evaluations, "line_search"
        gn = grad()
        s, y = xn - x, gn - g
        sy = float(np.dot(s, y))
        if sy > 1e-10 * float(np.linalg.norm(s)) * float(np.linalg.norm(y)):
            pairs.append((s, y, 1.0 / sy))
            del pairs[:-history]
        x, f, g = xn, fn, gn
    return x, f, gmax, max_iter, evaluations, "max_iter"


def _fit(prep, y, num_classes, l2, max_iter, gtol, history, theta0):
    obj = _Objective(prep, y, num_classes, l2)
    shape = (num_classes, prep.dim)
    x0 = np.zeros(shape) if theta0 is None else np.asarray(theta0, dtype=np.float64)
    if x0.shape != shape or not np.isfinite(x0).all():
        raise RuntimeError(f"clipa_amd.fit_logreg: theta0 must be a finite {shape} array, got {x0.shape}")
    x, f, gmax, it, ev, status = lbfgs(lambda v: obj.value(v.reshape(shape)), lambda: obj.grad().reshape(-1), x0.reshape(-1),
                                       max_iter, gtol, history)
    return {"theta": x.reshape(shape), "f": f, "gnorm": gmax, "iterations": it, "evaluations": ev, "status": status}


def _check_fit_args(num_classes, l2, who):
    if int(num_classes) < 1 or not float(l2) > 0.0:
        raise RuntimeError(f"clipa_amd.{who}: num_classes = {num_classes} must be >= 1 and l2 = {l2} > 0")


def fit_logreg(x, y, num_classes, l2, max_iter=1000, gtol=DEFAULT_GTOL, history=10, theta0=None):
    """Fit the probe: x 2-D float GPU tensor [N, D] (or a `Prepared`), y integer labels in [0, num_classes) (host or device),
    l2 > 0 the coefficient of the module docstring's formula (l2 = 1 / (C_sklearn * N)).  L-BFGS from theta0 (default 0) in
    numpy fp64 on the host (`lbfgs`), every evaluation on the device.  -> {"theta": fp64 [C, D + 1] (last column the bias), "f",
    "gnorm": max |g_i|, "iterations", "evaluations", "status": "converged" | "line_search" | "max_iter"}.

    gtol: the device's gradient differs from the exact fp64 gradient of the same theta by fp32 rounding; at the solution of
    tests/golden/linear_probe.npz (N = 600, D = 48, C = 10, l2 = 0.1) that difference is max |g_fp64 - g_device| = 2.7e-8, on the
    MI355X (tests/test_linear_probe_gpu.py prints and bounds it) as in a CPU simulation of the fp32 arithmetic
    (tools/make_linear_probe_golden.py prints that one).  The default gtol = 1e-5 is about 400 times that: below roughly 1e-6 the fp32 objective's
    noise (near 1e-8) stops every line search ("line_search"), and asking for less buys nothing."""
    who = "fit_logreg"
    _check_fit_args(num_classes, l2, who)
    if isinstance(x, Prepared):
        y = _device_labels(y, x.n, int(num_classes), "y", who, x.device)
        prep = x
    else:
        x = _check_features(x, "x", who)
        y = _device_labels(y, x.shape[0], int(num_classes), "y", who, x.device)
        prep = Prepared(x)
    return _fit(prep, y, int(num_classes), float(l2), int(max_iter), float(gtol), int(history), theta0)


# ---- probe and sweep -------------------------------------------------------------------------------------------------------
def _score(theta, xp_test, y_test_dev):
    """-> (correct, pred, best) of theta on prepared test rows: ops.fewshot_predict, which forms no [Nt, C] logits and gives
    what the `pred` / `best` of ops.logreg_logits would, bit for bit."""
    pred, best = ops.fewshot_predict(xp_test, _theta_device(theta, xp_test.device))
    return int((pred == y_test_dev).sum()), pred, best


def linear_probe(x_train, y_train, x_test, y_test, num_classes, l2, return_predictions=False, max_iter=1000,
                 gtol=DEFAULT_GTOL, theta0=None):
    """Fit on the train rows (fit_logreg), score on the test rows: features 2-D float GPU tensors of one width, labels host or
    device integers.  -> {"accuracy": np.float64, "correct", "num_test", "iterations", "status"}; return_predictions adds "pred"
    (int32 [Nt]) and "best" (the winning logit, f32 [Nt]), GPU tensors, and "theta".  CPU features, non-finite features, labels
    out of range, empty sets and l2 <= 0 raise: there is no host fallback."""
    who = "linear_probe"
    x_train, y, x_test, yt = _check_problem(x_train, y_train, x_test, y_test, num_classes, l2, who)
    prep = Prepared(x_train)
    xp_test, yt = ops.logreg_prepare(x_test)[0], torch.from_numpy(yt).to(x_test.device)
    fit = _fit(prep, _on(prep.device, y), int(num_classes), float(l2), int(max_iter), float(gtol), 10, theta0)
    correct, pred, best = _score(fit["theta"], xp_test, yt)
    out = {"accuracy": np.float64(correct) / np.float64(len(yt)), "correct": correct, "num_test": len(yt),
           "iterations": fit["iterations"], "status": fit["status"]}
    if return_predictions:
        out.update(pred=pred, best=best, theta=fit["theta"])
    return out


def search_grid(n, first_step, score):
    """The paper's parametric binary search over grid indices 0 .. n - 1 (ascending lambda): first every first_step-th index
    (a power of two), then the step halved again and again around the best index so far - its lower neighbour, then its upper
    one - down to step 1.  The best index is the one with the highest score, ties going to the larger index.
    score(i, warm) -> the score of index i, warm being the nearest index already scored (the larger one of two equally near;
    None for the first).  -> (best index, {index: score} in visiting order)."""
    if n < 1 or first_step < 1 or first_step & (first_step - 1):
        raise RuntimeError(f"clipa_amd.sweep_l2: a grid of {n} values and a first step of {first_step} (must be a power of two)")
    seen = {}

    def visit(i):
        if 0 <= i < n and i not in seen:
            seen[i] = score(i, min(seen, key=lambda j: (abs(j - i), -j)) if seen else None)

    for i in range(0, n, first_step):
        visit(i)
    best = max(seen, key=lambda i: (seen[i], i))
    step = first_step // 2
    while step >= 1:
        visit(best - step)
        visit(best + step)
        best = max((i for i in (best - step, best, best + step) if i in seen), key=lambda i: (seen[i], i))
        step //= 2
    return best, seen


def sweep_l2(x_train, y_train, x_val, y_val, num_classes, grid=None, first_step=16, max_iter=1000, gtol=DEFAULT_GTOL):
    """The regularisation sweep of Radford et al. A.3 on a validation split: a parametric binary search (`search_grid`) over
    `grid` (ascending; default np.logspace(-6, 6, 97), 8 steps per decade) that starts with every first_step-th value - 1e-6,
    1e-4, ..., 1e6 - and halves the step around the best validation accuracy down to the grid's spacing.  Every fit is warm-
    started from the solution of the nearest lambda already solved; ties go to the larger lambda.  The train rows are prepared
    once.  -> (best lambda, {lambda: validation accuracy} in visiting order)."""
    who = "sweep_l2"
    grid = np.logspace(-6, 6, 97) if grid is None else np.asarray(grid, dtype=np.float64)
    if grid.ndim != 1 or len(grid) < 1 or not (grid > 0).all() or not (np.diff(grid) > 0).all():
        raise RuntimeError(f"clipa_amd.{who}: grid must be a 1-D ascending array of positive values")
    x_train, y, x_val, yv = _check_problem(x_train, y_train, x_val, y_val, num_classes, grid[0], who, other="val")
    prep = Prepared(x_train)
    y = _on(prep.device, y)
    xp_val, yv = ops.logreg_prepare(x_val)[0], torch.from_numpy(yv).to(x_val.device)
    thetas = {}

    def score(i, warm):
        fit = _fit(prep, y, int(num_classes), float(grid[i]), int(max_iter), float(gtol), 10, None if warm is None else thetas[warm])
        thetas[i] = fit["theta"]
        return np.float64(_score(fit["theta"], xp_val, yv)[0]) / np.float64(len(yv))

    best, seen = search_grid(len(grid), int(first_step), score)
    return float(grid[best]), {float(grid[i]): acc for i, acc in seen.items()}


def evaluate_linear_probe(model, datasets, l2=None, grid=None, representation="features", max_iter=1000, gtol=DEFAULT_GTOL):
    """The linear-probe protocol of Radford et al. A.3 on one process, shaped like `evaluate_fewshot`.  datasets: {name:
    (train_batches, val_batches, test_batches, num_classes)}, the batches yielding (images, labels) with the images already on the
    device in the form `model.encode_image` accepts; val_batches may be None when l2 is given.  Every dataset is encoded once
    (no_grad, eval mode - the model's previous mode is put back after each dataset's encoding; representation "features":
    encode_image(normalize=False), "normalized": normalize=True) and its features stay on the GPU.  With l2=None lambda is
    swept on the validation split (`sweep_l2` over `grid`), then the probe is fitted on train + validation rows, as the paper
    does; with a number it is fitted on the train rows (and the validation rows, where given) with that lambda.
    Yields, per dataset in order, ("{name}_linear_probe_l2", lambda) and ("{name}_linear_probe", test accuracy), np.float64."""
    who = "evaluate_linear_probe"
    if representation not in ("features", "normalized"):
        raise RuntimeError(f"clipa_amd.{who}: representation must be 'features' or 'normalized', got {representation!r}")
    if l2 is not None and not float(l2) > 0.0:
        raise RuntimeError(f"clipa_amd.{who}: l2 = {l2} must be > 0 (or None: sweep it on the validation split)")
    norm = representation == "normalized"
    for name, (train_batches, val_batches, test_batches, num_classes) in datasets.items():
        if l2 is None and val_batches is None:
            raise RuntimeError(f"clipa_amd.{who}: dataset {name!r} has no validation split to sweep l2 on")
        with _inference(model) as m:
            xtr, ytr = _represent(m, train_batches, norm, who)
            xva, yva = _represent(m, val_batches, norm, who) if val_batches is not None else (None, None)
            xte, yte = _represent(m, test_batches, norm, who)
        lam = np.float64(l2) if l2 is not None else np.float64(sweep_l2(xtr, ytr, xva, yva, num_classes, grid=grid,
                                                                        max_iter=max_iter, gtol=gtol)[0])
        if xva is not None:
            xtr, ytr = torch.cat([xtr, xva]), np.concatenate([ytr, yva])
        out = linear_probe(xtr, ytr, xte, yte, num_classes, float(lam), max_iter=max_iter, gtol=gtol)
        yield f"{name}_linear_probe_l2", lam
        yield f"{name}_linear_probe", out["accuracy"]
