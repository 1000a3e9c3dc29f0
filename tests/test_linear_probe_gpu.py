"""GPU tests of the logistic-regression linear probe (clipa_amd/linear_probe.py, csrc/logreg.hip; Radford et al. 2021, A.3).
Kernel level: exactly representable inputs (small integers, every sum below 2^24), so the two products compare for equality;
the log-sum-exp and the residual against fp64 on those exact logits within bounds derived from the arithmetic, not measured.
End to end: the fixture of tools/make_linear_probe_golden.py (theta_star from scikit-learn), where the test asks for what the
stopping rule promises and for every prediction that theta's distance from theta_star cannot change."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import clipa_amd
from clipa_amd import linear_probe as P
from clipa_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import clip_oracle as O                 # noqa: E402
from . import linear_probe_cases as L               # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(ROOT, "tests", "golden", "linear_probe.npz")
U = 2.0 ** -24
SENTINEL = 7.0


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _host(t):
    return t.detach().cpu().numpy()


def _padded(a, extra=0, fill=0.0):
    """[R, K] host array -> the [R, K] view of a [R, K rounded up to 4, plus extra] device buffer whose other columns hold fill."""
    r, k = a.shape
    buf = torch.full((r, (k + 3) // 4 * 4 + extra), fill, device=DEV, dtype=torch.float32)
    buf[:, :k] = _dev(a)
    return buf[:, :k]


def absent_class(c):
    return 1 if c > 3 else 0


def _exact_case(name):
    """Integer theta and x of SHAPES[name] with planted ties and planted logits of +-100, labels that include the last two
    classes and leave one class (absent_class) without an example.  -> (x [N, D], theta [C, dim], y [N], logits int64 [N, C])."""
    n, d, c = L.SHAPES[name]
    rng = np.random.RandomState(n + c)
    x = rng.randint(-3, 4, size=(n, d)).astype(np.int64)
    theta = rng.randint(-3, 4, size=(c, d + 1)).astype(np.int64)
    theta[:, 0] = -10                                 # feature 0 carries the +-100: x = +-10 there, theta = +-10
    theta[[c - 1, min(4, c - 2)], 0] = 10
    if c > 128:                                        # equal weight rows: ties inside a lane, across lanes, waves and class tiles
        for group in ((5, 37), (6, 9), (7, 100), (11, 128), (40, 41, 129)):
            theta[list(group)] = theta[group[0]]
    else:
        theta[2] = theta[0]
    for r, s in ((1, 10), (2, -10), (n - 1, 10)):     # rows of the first and of the ragged last sample tile
        x[r] = 0
        x[r, 0] = s
    if c <= 128:
        theta[:, 0] = -10                             # C = 3: every logit of the planted rows is -100 or +100 at once
    y = rng.randint(0, c, size=n)
    y[y == absent_class(c)] = c - 1
    y[::7] = c - 1
    y[3::7] = c - 2
    logits = L.with_ones(x) @ theta.T
    assert np.abs(logits).max() < 2 ** 24 and np.abs(logits[[1, 2, n - 1]]).min() >= 97
    return x, theta, y, logits


@pytest.fixture(scope="module", params=list(L.SHAPES))
def exact(request):
    """The case, its device operands and one run of the logits kernel into a wider, sentinel-filled buffer."""
    x, theta, y, logits = _exact_case(request.param)
    n, d, c = L.SHAPES[request.param]
    xp, xt = ops.logreg_prepare(_dev(x))
    out = _padded(np.full((c, n), SENTINEL), extra=8, fill=SENTINEL)
    zt, lse, pred, best = ops.logreg_logits(_padded(theta), xp, out=out)
    return dict(name=request.param, x=x, theta=theta, y=y, logits=logits, xp=xp, xt=xt, zt=zt, lse=lse, pred=pred, best=best,
                lse64=L.lse_fp64(logits))


# ---- 1. prepare ------------------------------------------------------------------------------------------------------------
def test_prepare_appends_ones_pads_with_zeros_and_transposes(exact):
    x, xp, xt = exact["x"], exact["xp"], exact["xt"]
    n, d = x.shape
    pb, tb = _host(xp._base), _host(xt._base)
    assert pb.shape == (n, (d + 4) // 4 * 4) and tb.shape == (d + 1, (n + 3) // 4 * 4)
    assert np.array_equal(pb[:, :d + 1], L.with_ones(x).astype(np.float32)) and not pb[:, d + 1:].any()
    assert np.array_equal(tb[:, :n], pb[:, :d + 1].T) and not tb[:, n:].any()


# ---- 2. logits -------------------------------------------------------------------------------------------------------------
def test_logits_equal_the_integer_product_and_leave_padding_untouched(exact):
    zb = _host(exact["zt"]._base)
    n, c = exact["logits"].shape
    assert zb.dtype == np.float32 and np.array_equal(zb[:, :n].astype(np.int64), exact["logits"].T)
    assert zb.shape[1] >= n + 8 and (zb[:, n:] == SENTINEL).all()      # columns [N, ldz): untouched, as the header says


def test_pred_and_best_equal_fewshot_predict_bit_for_bit_ties_included(exact):
    logits = exact["logits"]
    want = np.argmax(logits, axis=1)                       # the lowest index among equal maxima
    tied = (logits == logits.max(1, keepdims=True)).sum(1)
    assert (tied > 1).sum() >= 1 and (tied == 1).sum() >= 1
    pred, best = ops.fewshot_predict(exact["xp"], _padded(exact["theta"]))
    assert torch.equal(exact["pred"], pred) and torch.equal(exact["best"], best)
    assert exact["pred"].dtype == torch.int32 and np.array_equal(_host(exact["pred"]), want)
    assert np.array_equal(_host(exact["best"]).astype(np.int64), logits.max(1))


def test_lse_within_16_ulp_of_fp64_with_logits_of_plus_minus_100(exact):
    """|lse - lse64| <= 16 * 2^-24 * max(1, |lse64|): at most 2 ulp per expf, half an ulp per add, and at most
    2 * ceil(C / 128) + 6 sequential merges; the logits themselves are exact.  exp(100) overflows fp32 and exp(-100) underflows:
    the planted rows pass only with the running maximum subtracted."""
    lse, lse64 = _host(exact["lse"]).astype(np.float64), exact["lse64"]
    n = len(lse64)
    assert np.isfinite(lse).all() and np.abs(lse64[[1, 2, n - 1]]).min() > 90
    err = np.abs(lse - lse64) / np.maximum(1.0, np.abs(lse64))
    print(f"lse {exact['name']}: max |lse - lse64| / max(1, |lse64|) = {err.max() / U:.2f} * 2^-24 (bound 16)")
    assert err.max() <= 16 * U


# ---- 3. residual -----------------------------------------------------------------------------------------------------------
def test_residual_reads_ce_before_the_overwrite_and_is_within_32_ulp(exact):
    """g = exp(z - lse) - [c == y] and ce = lse - z_y against fp64 on the exact logits: |. - fp64| <= 32 * 2^-24 *
    max(1, |lse64|) (the lse's 16, carried through one more expf or subtraction; the subtraction's own half ulp of ce stays
    inside it for these logits).  Measured on an MI355X: ce 24.0 * 2^-24 at most (C = 3, where |ce| reaches 60 times |lse|), g 1.03.  Labels c - 1 and c - 2 sit in the second
    class tile and class block: a ce read after the overwrite would come out as lse - (p - 1)."""
    logits, y, lse64 = exact["logits"].astype(np.float64), exact["y"], exact["lse64"]
    n, c = logits.shape
    assert (y == c - 1).any() and (y == c - 2).any() and not (y == absent_class(c)).any()
    zt = _padded(_host(exact["zt"]))                        # a copy: the module's logits stay as they are
    yd = _dev(y, torch.int32)
    ce0 = ops.logreg_residual(zt, exact["lse"], yd, overwrite=False)
    assert torch.equal(zt, exact["zt"])                     # the line-search mode writes ce alone
    ce = ops.logreg_residual(zt, exact["lse"], yd, overwrite=True)
    assert torch.equal(ce, ce0)
    scale = np.maximum(1.0, np.abs(lse64))
    ce64 = lse64 - logits[np.arange(n), y]
    g64 = np.exp(logits - lse64[:, None])
    g64[np.arange(n), y] -= 1.0
    ce_err = (np.abs(_host(ce).astype(np.float64) - ce64) / scale).max()
    g_err = (np.abs(_host(zt).astype(np.float64).T - g64) / scale[:, None]).max()
    print(f"residual {exact['name']}: ce {ce_err / U:.2f}, g {g_err / U:.2f} (* 2^-24, bound 32)")
    assert ce_err <= 32 * U and g_err <= 32 * U
    with pytest.raises(RuntimeError, match="int32"):
        ops.logreg_residual(zt, exact["lse"], yd.long())


# ---- 4. gradient product ---------------------------------------------------------------------------------------------------
def test_grad_equals_the_integer_product_for_any_slicing_and_grid(exact):
    """Integer Gt: every partial and every sum is exact, so three slices of 128 (the last with 44 samples), one slice, and two
    grid shapes all give the integer product; between repeated calls and grids the results are bit-identical in any case."""
    n, c = exact["logits"].shape
    rng = np.random.RandomState(c)
    g = rng.randint(-3, 4, size=(c, n)).astype(np.int64)
    want = g @ L.with_ones(exact["x"])
    gt = _padded(g)
    runs = [ops.logreg_grad(gt, exact["xt"], _slice=128), ops.logreg_grad(gt, exact["xt"], _slice=128),
            ops.logreg_grad(gt, exact["xt"], _slice=128, _max_workgroups=2), ops.logreg_grad(gt, exact["xt"], _slice=128, _max_workgroups=5),
            ops.logreg_grad(gt, exact["xt"]), ops.logreg_grad(gt, exact["xt"], _max_workgroups=1)]
    from clipa_amd import lib
    assert lib.query("clipa_logreg_grad_workspace", c, want.shape[1], n, 128) == (0 if n <= 128 else 3 * c * 72 * 4)
    for r in runs:
        assert r.dtype == torch.float32 and np.array_equal(_host(r).astype(np.int64), want)
        assert torch.equal(r, runs[0])


def test_grad_is_bit_identical_across_grids_on_inexact_data():
    """Random fp32 operands, where another summation order would show: repeated calls and three grid shapes agree bit for bit,
    with three slices and with one; the sliced sum is the ascending-order sum of the three slice products."""
    g = torch.Generator(device=DEV).manual_seed(5)
    gt, xt = torch.randn(130, 300, device=DEV, generator=g), torch.randn(71, 300, device=DEV, generator=g)
    for s in (128, 0):
        a = ops.logreg_grad(gt, xt, _slice=s)
        for mw in (0, 1, 3):
            assert torch.equal(a, ops.logreg_grad(gt, xt, _slice=s, _max_workgroups=mw))
    parts = [ops.logreg_grad(gt[:, lo:hi].contiguous(), xt[:, lo:hi].contiguous()) for lo, hi in ((0, 128), (128, 256), (256, 300))]
    assert torch.equal(ops.logreg_grad(gt, xt, _slice=128), (parts[0] + parts[1]) + parts[2])
    want, lim = gt.double() @ xt.double().t(), 300 * U * (gt.abs().double() @ xt.abs().double().t())      # gamma_n sum |a| |b|
    assert bool(((ops.logreg_grad(gt, xt).double() - want).abs() <= lim).all())


# ---- 5. one whole evaluation -----------------------------------------------------------------------------------------------
def test_objective_is_deterministic_and_close_to_fp64():
    n, d, c = L.SHAPES["two class tiles"]
    rng = np.random.RandomState(12)
    x = rng.standard_normal((n, d)).astype(np.float32)
    theta = 0.3 * rng.standard_normal((c, d + 1)).astype(np.float32).astype(np.float64)
    y = rng.randint(0, c, size=n)
    prep = P.prepare(_dev(x))
    f, g, k = P.logreg_objective(prep, y, theta, 0.01)
    f2, g2, k2 = P.logreg_objective(prep, torch.from_numpy(y).to(DEV), theta, 0.01)
    assert f == f2 and k == k2 and g.dtype == np.float64 and np.array_equal(g, g2)
    p1 = ops.logreg_logits(P._theta_device(theta, DEV), prep.xp)
    p2 = ops.logreg_logits(P._theta_device(theta, DEV), prep.xp)
    assert all(torch.equal(a, b) for a, b in zip(p1, p2)) and k == int((_host(p1[2]) == y).sum())
    f64, g64, z64 = L.objective_fp64(x, y, theta, 0.01)
    assert k == int((np.argmax(z64, axis=1) == y).sum())
    assert P.logreg_objective(prep, y, theta, 0.01, need_grad=False) == (f, None, k)
    # a logit is a dim-term fp32 chain: |error| <= dim * 2^-24 * sum_d |theta| |x~|, as is that of the fp32 rounding of theta;
    # it passes into lse, ce and the softmax one to one, next to the 32 * 2^-24 * max(1, |lse|) of the steps after the product.
    # The gradient averages residuals times x~, with one more n-term chain
    xa = np.abs(L.with_ones(x.astype(np.float64)))
    e = 2 * (d + 1) * U * (xa @ np.abs(theta).T).max() + 32 * U * max(1.0, np.abs(L.lse_fp64(z64)).max())
    g_tol = e * xa.mean(0).max() + n * U * xa.max()
    print(f"objective: |f - f64| = {abs(f - f64):.3g} (bound {e:.3g}), max |g - g64| = {np.abs(g - g64).max():.3g} (bound {g_tol:.3g})")
    assert abs(f - f64) <= e and np.abs(g - g64).max() <= g_tol
    assert np.array_equal(g[:, -1], g2[:, -1]) and abs(g[:, -1].sum()) < 1e-6      # the bias gradients sum to 0: softmax rows sum to 1


# ---- 6. end to end on the fixture ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(FIXTURE, allow_pickle=False)


@pytest.fixture(scope="module")
def probe(golden):
    z = golden
    return P.linear_probe(_dev(z["x"]), z["y"], _dev(z["x_test"]), z["y_test"], L.FIXTURE["c"], float(z["l2"]),
                          return_predictions=True)


def test_fit_converges_at_the_default_gtol_to_a_point_whose_exact_gradient_is_small(golden, probe):
    """fit_logreg stops when the device's max |g| <= gtol; the exact gradient at that theta then obeys
    max |g64| <= gtol + max |g64 - g_device|, a triangle inequality with no free constant."""
    z = golden
    x, y, l2 = z["x"], z["y"], float(z["l2"])
    fit = P.fit_logreg(_dev(x), y, L.FIXTURE["c"], l2)
    assert fit["status"] == "converged" and fit["gnorm"] <= P.DEFAULT_GTOL and fit["iterations"] < 100
    assert np.array_equal(fit["theta"], probe["theta"]) and fit["iterations"] == probe["iterations"]      # the same fit, bit for bit
    f_dev, g_dev, _ = P.logreg_objective(P.prepare(_dev(x)), y, fit["theta"], l2)
    f64, g64, _ = L.objective_fp64(x, y, fit["theta"], l2)
    gdiff = np.abs(g64 - g_dev).max()
    print(f"fit: {fit['status']} after {fit['iterations']} iterations / {fit['evaluations']} evaluations, device max |g| = "
          f"{fit['gnorm']:.3g}, max |g64| = {np.abs(g64).max():.3g}, max |g64 - g_device| = {gdiff:.3g}, |f64 - f_device| = "
          f"{abs(f64 - f_dev):.3g}, f - f_star = {f64 - float(z['f_star']):.3g}")
    assert f_dev == fit["f"] and np.abs(g_dev).max() == fit["gnorm"]
    assert np.abs(g64).max() <= P.DEFAULT_GTOL + gdiff
    assert gdiff * 10 <= P.DEFAULT_GTOL                     # the default sits at least 10 times above the device's gradient error


def test_probe_predictions_match_theta_star_wherever_they_are_determined(golden, probe):
    """With delta = max |theta - theta_star| after bias centring, a test row whose top-two logit gap under theta_star exceeds
    2 delta ||x~||_1 cannot change its argmax: those rows must match exactly, and the rows left out may be at most 5 % of the
    test set - a condition, not a measurement (the golden tool's float32 simulation left out 0.5 %)."""
    z = golden
    assert probe["status"] == "converged" and probe["num_test"] == L.FIXTURE["nt"]
    delta = np.abs(L.centre_bias(probe["theta"]) - z["theta_star"]).max()
    stable, want = L.stable_rows(z["theta_star"], z["x_test"], delta)
    pred = _host(probe["pred"])
    left_out = 1.0 - stable.mean()
    print(f"probe: delta = {delta:.3g}, rows left out {left_out:.2%}, rows off among the rest {(pred != want)[stable].sum()}, "
          f"accuracy {probe['accuracy']:.4f} (theta_star {float(z['accuracy']):.4f})")
    assert left_out <= 0.05
    assert np.array_equal(pred[stable], want[stable])
    assert probe["correct"] == int((pred == z["y_test"]).sum()) and probe["accuracy"] == np.float64(probe["correct"]) / 400
    # the two ways to predict agree bit for bit
    xp = ops.logreg_prepare(_dev(z["x_test"]))[0]
    _, _, pred2, best2 = ops.logreg_logits(P._theta_device(probe["theta"], DEV), xp)
    assert torch.equal(pred2, probe["pred"]) and torch.equal(best2, probe["best"])


def test_sweep_l2_on_a_small_grid(golden):
    z = golden
    x, y = z["x"], z["y"]
    grid = np.logspace(-4, 0, 9)
    best, seen = P.sweep_l2(_dev(x[:450]), y[:450], _dev(x[450:]), y[450:], L.FIXTURE["c"], grid=grid, first_step=4)
    assert list(seen)[:3] == [float(grid[0]), float(grid[4]), float(grid[8])] and 5 <= len(seen) <= 7
    top = max(seen.values())
    assert best == max(k for k, v in seen.items() if v == top) and 0.5 < top <= 1.0
    one = P.linear_probe(_dev(x[:450]), y[:450], _dev(x[450:]), y[450:], L.FIXTURE["c"], float(grid[0]))
    assert one["accuracy"] == seen[float(grid[0])]          # the sweep's first fit starts cold, as this one


# ---- 7. evaluate_linear_probe ----------------------------------------------------------------------------------------------
TOY = {"embed_dim": 64,
       "vision_cfg": {"image_size": 32, "layers": 2, "width": 128, "patch_size": 16},
       "text_cfg": {"context_length": 16, "vocab_size": 512, "width": 128, "heads": 2, "layers": 2}}


def test_evaluate_linear_probe_names_order_and_mode(tmp_path):
    path = os.path.join(str(tmp_path), "probe-toy.json")
    json.dump(TOY, open(path, "w"))
    clipa_amd.add_model_config(path)
    torch.manual_seed(0)
    m = clipa_amd.create_model("probe-toy", device=DEV, output_dict=True)
    rng = np.random.RandomState(8)

    def batches(n, c, seed):
        images = O.synthetic_batch(n, 32, 16, 512, seed=seed)[0].to(DEV)
        labels = rng.randint(0, c, size=n)
        cut = n // 2 + 3
        return [(images[:cut], torch.from_numpy(labels[:cut]).to(DEV)), (images[cut:], labels[cut:].tolist())], images, labels

    sets, raw = {}, {}
    for name, c in (("pets", 5), ("birds", 3)):
        tr, xtr, ytr = batches(48, c, 100 + c)
        va, xva, yva = batches(24, c, 300 + c)
        te, xte, yte = batches(32, c, 200 + c)
        sets[name] = (iter(tr), iter(va) if name == "pets" else None, iter(te), c)      # one-shot iterators: encoded once
        raw[name] = (xtr, ytr, xva if name == "pets" else None, yva, xte, yte, c)
    calls, modes = [], []
    encode = m.encode_image
    m.encode_image = lambda *a, **k: (calls.append(k.get("normalize")), modes.append(m.training), encode(*a, **k))[-1]
    m.train()
    got = list(P.evaluate_linear_probe(m, sets, l2=0.01, representation="normalized", max_iter=30))
    m.encode_image = encode
    assert calls == [True] * 10 and modes == [False] * 10 and m.training      # pets 3 x 2 batches, birds 2 x 2; mode put back
    assert [n for n, _ in got] == ["pets_linear_probe_l2", "pets_linear_probe", "birds_linear_probe_l2", "birds_linear_probe"]
    assert all(isinstance(v, np.float64) for _, v in got) and got[0][1] == got[2][1] == 0.01
    m.eval()
    with torch.no_grad():
        enc = lambda x: torch.cat([m.encode_image(x[:len(x) // 2 + 3], normalize=True),      # noqa: E731
                                   m.encode_image(x[len(x) // 2 + 3:], normalize=True)]).float()
        for (name, acc) in (got[1], got[3]):
            xtr, ytr, xva, yva, xte, yte, c = raw[name.split("_")[0]]
            ftr, ytr = (torch.cat([enc(xtr), enc(xva)]), np.concatenate([ytr, yva])) if xva is not None else (enc(xtr), ytr)
            want = P.linear_probe(ftr, ytr, enc(xte), yte, c, 0.01, max_iter=30)
            assert acc == want["accuracy"] and 0.0 <= acc <= 1.0, (name, acc, want)
    # l2 = None: swept on the validation split, here over a three-value grid
    sets = {"pets": ([(raw["pets"][0], raw["pets"][1])], [(raw["pets"][2], raw["pets"][3])], [(raw["pets"][4], raw["pets"][5])], 5)}
    m.eval()
    got = dict(P.evaluate_linear_probe(m, sets, grid=[0.01, 0.1, 1.0], representation="normalized", max_iter=30))
    assert list(got) == ["pets_linear_probe_l2", "pets_linear_probe"] and got["pets_linear_probe_l2"] in (0.01, 0.1, 1.0)
    assert not m.training
