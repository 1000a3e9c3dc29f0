"""GPU tests of the few-shot linear probe (clipa_amd/fewshot.py, csrc/fewshot.hip; the reference's
clipa_jax/evaluators/fewshot_lsr.py).  Kernel level: exactly representable inputs (small integers, every sum below 2^24, after
tests/glue_cases.py), so every comparison is for equality - the std of the moments excepted, whose square root and 1e-5 add
are one rounding each.  End to end: the fixture of tools/make_fewshot_golden.py, whose margin rule makes every per-row
prediction well defined; the reference's task sampling; evaluate_fewshot on a toy engine model."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import clipa_amd
from clipa_amd import fewshot, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import clip_oracle as O                 # noqa: E402
from tools import make_fewshot_golden as G          # noqa: E402
from . import fewshot_cases as F                    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(ROOT, "tests", "golden", "fewshot_lsr.npz")


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _host(t):
    return t.detach().cpu().numpy()


# ---- 1. moments ------------------------------------------------------------------------------------------------------------
def test_moments_exact_mean_and_two_ulp_std():
    """Integers in [-3, 3]; 256 rows of a 300-row matrix through a permuting, subsampling index list.  Every column's sum over
    the selected rows is made a multiple of 16, so mean = k / 16, x - mean is a multiple of 1/16 below 6, its square a multiple
    of 1/256 below 36 and the 256-term sum below 2^24 / 256: all of it exact in fp32 in any order.  What is left is the
    rounding of the root and of the 1e-5 add: 2 ulp."""
    rng = np.random.RandomState(11)
    x = rng.randint(-3, 4, size=(300, 70)).astype(np.int64)
    idx = rng.permutation(300)[:256]
    for d in range(70):
        r = int(x[idx, d].sum() % 16)
        rows = idx[x[idx, d] > -3][:r]               # lower r of the selected entries by one
        x[rows, d] -= 1
    assert (x[idx].sum(0) % 16 == 0).all() and x.min() >= -3 and x.max() <= 3
    xs = x[idx].astype(np.float64)
    mean64 = xs.mean(0)
    var64 = ((xs - mean64) ** 2).mean(0)
    assert len(np.unique(mean64)) > 8 and (var64 > 0).all()
    want_std = np.float32(np.sqrt(var64)).astype(np.float32) + np.float32(1e-5)
    xd, idxd = _dev(x), _dev(idx, torch.int64)
    mean, std = ops.fewshot_moments(xd, idxd)
    mean2, std2 = ops.fewshot_moments(xd, idxd)
    assert torch.equal(mean, mean2) and torch.equal(std, std2)
    assert np.array_equal(_host(mean), mean64.astype(np.float32))
    ulps = np.abs(_host(std).view(np.int32).astype(np.int64) - want_std.view(np.int32).astype(np.int64))
    print("moments: std ulp distances", np.bincount(ulps))
    assert ulps.max() <= 2, ulps.max()
    # no index list: all rows, in order
    mean_all, _ = ops.fewshot_moments(xd[:256])
    assert np.array_equal(_host(mean_all), x[:256].astype(np.float64).mean(0).astype(np.float32))


# ---- 2. whiten -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,ntot", [(130, 70, 200), (5, 199, 9)])
def test_whiten_exact_with_gather_bias_column_and_padding(N, D, ntot):
    rng = np.random.RandomState(N)
    x = rng.randint(-8, 9, size=(ntot, D)).astype(np.float32)
    idx = rng.randint(0, ntot, size=N)               # any order, repeats allowed
    mean = rng.randint(-2, 3, size=D).astype(np.float32)
    std = (2.0 ** rng.randint(-2, 3, size=D)).astype(np.float32)
    dim = D + 1
    want = np.concatenate([(x[idx] - mean) / std, np.full((N, 1), 100.0, dtype=np.float32)], axis=1)
    z, zt = ops.fewshot_whiten(_dev(x), _dev(mean), _dev(std), _dev(idx, torch.int64), transpose=True)
    assert tuple(z.shape) == (N, dim) and tuple(zt.shape) == (dim, N)
    zb, tb = _host(z._base), _host(zt._base)          # the padded buffers
    assert zb.shape == (N, (dim + 3) // 4 * 4) and tb.shape == (dim, (N + 3) // 4 * 4)
    assert np.array_equal(zb[:, :dim], want)
    assert np.array_equal(zb[:, dim:], np.zeros((N, zb.shape[1] - dim), dtype=np.float32))
    assert np.array_equal(tb[:, :N], zb[:, :dim].T)
    assert np.array_equal(tb[:, N:], np.zeros((dim, tb.shape[1] - N), dtype=np.float32))
    # without an index list and without the transposed copy
    z2 = ops.fewshot_whiten(_dev(x), _dev(mean), _dev(std))
    assert np.array_equal(_host(z2)[:, :D], (x - mean) / std) and (_host(z2)[:, D] == 100.0).all()


def test_moments_and_whiten_on_a_misaligned_column_slice():
    """x = big[:, 1:]: base 4 bytes off a 16-byte boundary, row stride 8 for 7 columns.  The wrappers copy it into an aligned
    dense buffer; the row stride passed to the kernels must be the copy's."""
    rng = np.random.RandomState(9)
    big = rng.randint(-3, 4, size=(37, 8)).astype(np.float32)
    x = big[:, 1:]
    idx = rng.permutation(37)[:16]
    big[idx[:8], 1:] = -big[idx[8:], 1:] + 2                          # selected rows: column sums 16, mean exactly 1
    xd = _dev(big)[:, 1:]
    assert xd.data_ptr() % 16 == 4 and xd.stride() == (8, 1)
    idxd = _dev(idx, torch.int64)
    mean, std = ops.fewshot_moments(xd, idxd)
    assert np.array_equal(_host(mean), np.ones(7, dtype=np.float32))
    var64 = ((x[idx].astype(np.float64) - 1.0) ** 2).mean(0)
    want_std = np.sqrt(var64).astype(np.float32) + np.float32(1e-5)
    assert np.abs(_host(std).view(np.int32).astype(np.int64) - want_std.view(np.int32).astype(np.int64)).max() <= 2
    mean_all, _ = ops.fewshot_moments(_dev(big[:32])[:, 1:])
    assert np.array_equal(_host(mean_all), x[:32].astype(np.float64).mean(0).astype(np.float32))      # 32 rows: exact
    mu = rng.randint(-2, 3, size=7).astype(np.float32)
    sd = (2.0 ** rng.randint(-2, 3, size=7)).astype(np.float32)
    z, zt = ops.fewshot_whiten(xd, _dev(mu), _dev(sd), idxd, transpose=True)
    want = np.concatenate([(x[idx] - mu) / sd, np.full((16, 1), 100.0, dtype=np.float32)], axis=1)
    assert np.array_equal(_host(z), want) and np.array_equal(_host(zt), want.T)
    assert np.array_equal(_host(ops.fewshot_whiten(xd, _dev(mu), _dev(sd)))[:, :7], (x - mu) / sd)
    # and through the public entry: a sliced view gives what its dense copy gives
    g = np.load(FIXTURE, allow_pickle=False)
    xs, y, xt, yt = G.case_inputs("E", g["E_redraws"])
    pad = lambda a: _dev(np.concatenate([np.zeros((len(a), 1), dtype=np.float32), a], axis=1))[:, 1:]      # noqa: E731
    a = fewshot.fewshot_lsr(pad(xs), y, pad(xt), yt, 20, 64.0, return_predictions=True)
    b = fewshot.fewshot_lsr(_dev(xs), y, _dev(xt), yt, 20, 64.0, return_predictions=True)
    assert torch.equal(a["pred"], b["pred"]) and torch.equal(a["best"], b["best"])


# ---- 3. gram ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,E", [(71, 130), (200, 71)])
def test_gram_exact_on_integers(M, E):
    a = np.random.RandomState(M).randint(-3, 4, size=(M, E)).astype(np.int64)
    S = _host(ops.fewshot_gram(_dev(a)))
    assert np.array_equal(S.astype(np.int64), a @ a.T) and S.dtype == np.float32


def test_gram_is_bitwise_symmetric_across_mirrored_tiles():
    """M = 257: three tile rows, six computed tiles, three mirrored; random fp32 data, so a tile and its mirror image agree
    only if both come from one accumulator chain."""
    g = torch.Generator(device=DEV).manual_seed(3)
    a = torch.randn(257, 100, device=DEV, generator=g)
    S = ops.fewshot_gram(a)
    assert torch.equal(S, S.t().contiguous())
    want = a.double().cpu().numpy()
    want = want @ want.T
    assert np.abs(_host(S) - want).max() <= 100 * 2.0 ** -23 * np.abs(a.cpu().numpy()).max() ** 2 * 4


# ---- 4. class sums ---------------------------------------------------------------------------------------------------------
def test_class_sums_exact_with_an_empty_class():
    rng = np.random.RandomState(4)
    counts = np.array([5, 1, 0, 17, 3, 140, 9])         # C = 7, class 2 empty
    n, dim = int(counts.sum()), 71
    z = rng.randint(-3, 4, size=(n, dim)).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    seg = np.stack([z[off[c]:off[c + 1]].sum(0) for c in range(7)], axis=1)      # [dim, C]
    want = 2 * seg - z.sum(0)[:, None]
    R = _host(ops.fewshot_class_sums(_dev(z), off))
    assert R.shape == (dim, 7) and np.array_equal(R.astype(np.int64), want)
    assert np.array_equal(R[:, 2].astype(np.int64), -z.sum(0))
    y = -np.ones((n, 7), dtype=np.int64)
    y[np.arange(n), np.repeat(np.arange(7), counts)] = 1
    assert np.array_equal(want, z.T @ y)                  # it is z^T Y


# ---- 5. predict ------------------------------------------------------------------------------------------------------------
# pairs / triples of classes with identical weight rows; lane L of column wave wn holds classes tile * 128 + wn * 64 + ni * 32 + L
TIES = {"within a lane": (5, 37), "across lanes": (6, 9), "across the column waves": (7, 100),
        "one lane, across class tiles": (11, 139), "across lanes and class tiles": (10, 200),
        "into the ragged last tile": (250, 256), "three ways": (40, 41, 180), "higher tile first in value order": (129, 3)}


def test_predict_matches_int64_argmax_with_planted_ties():
    rng = np.random.RandomState(5)
    nt, dim, C = 300, 71, 257
    w = rng.randint(-3, 4, size=(C, dim)).astype(np.int64)
    z = rng.randint(-3, 4, size=(nt, dim)).astype(np.int64)
    groups = list(TIES.values())
    for g, classes in enumerate(groups):
        v = 3 * (2 * rng.randint(0, 2, size=dim) - 1)      # +-3 everywhere: v . v = 639 beats every other row of w
        w[list(classes)] = v
        z[g::2 * len(groups)] = v                          # rows g, g + 16, ...: through all three row tiles
    logits = z @ w.T
    want = np.argmax(logits, axis=1)                       # the lowest index among equal maxima
    tied = (logits == logits.max(1, keepdims=True)).sum(1)
    for g, classes in enumerate(groups):
        rows = np.arange(nt)[g::2 * len(groups)]
        assert (tied[rows] == len(classes)).all() and (want[rows] == min(classes)).all()
    assert (tied == 1).sum() > 100                         # and plenty of rows without a tie
    pred, best = ops.fewshot_predict(_dev(z), _dev(w))
    pred, best = _host(pred), _host(best)
    assert pred.dtype == np.int32 and best.dtype == np.float32
    bad = np.nonzero(pred != want)[0]
    assert len(bad) == 0, (bad[:10], pred[bad[:10]], want[bad[:10]])
    assert np.array_equal(best.astype(np.int64), logits.max(1))


def test_predict_single_class_and_single_row():
    z = _dev(np.array([[1, -2, 3, 100]]))
    pred, best = ops.fewshot_predict(z, _dev(np.array([[2, 2, 2, 1]])))
    assert _host(pred).tolist() == [0] and _host(best).tolist() == [104.0]


def test_predict_writes_every_row_to_its_own_output():
    """Every row has its own winning logit, n + 1, so a reduction that hands a row's result to another row cannot pass (the
    planted ties above repeat one value across many rows)."""
    nt, C, dim = 130, 3, 8
    n = np.arange(nt)
    z = np.zeros((nt, dim), dtype=np.int64)
    z[n, n % C] = n + 1                                    # class n % 3 wins row n with n + 1; the other classes get 0
    pred, best = ops.fewshot_predict(_dev(z), _dev(np.eye(C, dim, dtype=np.int64)))
    assert np.array_equal(_host(pred), n % C)
    assert np.array_equal(_host(best), (n + 1).astype(np.float32))


def test_zero_sized_inputs_give_the_empty_computation():
    """The C entry points on zero-sized inputs (include/clipa_hip.h): OK, with what the empty sum or mean is."""
    from clipa_amd import lib
    st, p = ops._stream(), ops._p
    mean, std = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
    lib.call("clipa_fewshot_moments", None, None, 0, 0, 5, 8, p(mean), p(std), st)
    assert torch.isnan(mean[:5]).all() and torch.isnan(std[:5]).all() and (mean[5:] == 0).all() and (std[5:] == 0).all()
    a, S = torch.ones(3, 4, device=DEV), torch.ones(3, 4, device=DEV)
    lib.call("clipa_fewshot_gram", p(a), 3, 0, 4, p(S), 4, st)
    assert (S[:, :3] == 0).all() and (S[:, 3] == 1).all()
    pred, best = torch.full((4,), 7, device=DEV, dtype=torch.int32), torch.ones(4, device=DEV)
    lib.call("clipa_fewshot_predict", p(a), p(a), 3, 2, 0, 0, 0, p(pred), p(best), st)
    assert pred.tolist() == [0, 0, 0, 7] and best.tolist() == [0.0, 0.0, 0.0, 1.0]


# ---- 6. fewshot_lsr on the fixture -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(FIXTURE, allow_pickle=False)


@pytest.mark.parametrize("name", ["A1", "A2", "B1", "B2", "E"])
def test_fewshot_lsr_matches_fixture_on_every_row(golden, name):
    z = golden
    x, y, xt, yt = G.case_inputs(name, z[f"{name}_redraws"])
    assert np.array_equal(yt, z[f"{name}_y_test"])
    out = fewshot.fewshot_lsr(_dev(x), y, _dev(xt), yt, int(z[f"{name}_c"]), float(z[f"{name}_l2"]), return_predictions=True)
    dev = float(z[f"{name}_dev"])
    pred, best = _host(out["pred"]), _host(out["best"]).astype(np.float64)
    wrong = np.nonzero(pred != z[f"{name}_pred"])[0]
    err = np.abs(best - z[f"{name}_best"]).max()
    print(f"fewshot_lsr {name}: route {out['route']} rows off {len(wrong)} max |best - fp64| {err:.3g} = {err / dev:.2f} dev "
          f"(bound 8 dev = {8 * dev:.3g}) correct {out['correct']} / {out['num_test']}")
    assert out["route"] == str(z[f"{name}_route"]) == {"A1": "A", "A2": "A", "B1": "B", "B2": "B", "E": "A"}[name]
    assert len(wrong) == 0, (wrong[:10], pred[wrong[:10]], z[f"{name}_pred"][wrong[:10]])
    assert err <= 8 * dev, (err, dev)
    assert out["correct"] == int(z[f"{name}_correct"]) and out["num_test"] == G.NT
    assert isinstance(out["accuracy"], np.float64) and out["accuracy"] == float(z[f"{name}_accuracy"])


def test_fewshot_lsr_sorts_unordered_rows_and_takes_other_dtypes(golden):
    """Rows in shuffled order give the class-sorted task (stable order), bf16 features are used as fp32."""
    x, y, xt, yt = G.case_inputs("A1", golden["A1_redraws"])
    perm = np.random.RandomState(0).permutation(len(y))
    xb, xtb = _dev(x).bfloat16(), _dev(xt).bfloat16()
    a = fewshot.fewshot_lsr(xb[_dev(perm, torch.int64)], y[perm], xtb, torch.from_numpy(yt).to(DEV), 20, 1024.0, True)
    order = perm[np.argsort(y[perm], kind="stable")]
    b = fewshot.fewshot_lsr(xb.float()[_dev(order, torch.int64)], y[order], xtb.float(), yt, 20, 1024.0, True)
    assert torch.equal(a["pred"], b["pred"]) and torch.equal(a["best"], b["best"]) and a["correct"] == b["correct"]


# ---- 7. fewshot_metrics ----------------------------------------------------------------------------------------------------
def _pool(seed, n_train=260, n_test=400, c=12, d=40):
    rng = np.random.RandomState(seed)
    proto = rng.standard_normal((c, d))
    ytr = rng.randint(0, c, size=n_train)
    rare = np.nonzero(ytr == 3)[0]
    ytr[rare[2:]] = 4                                       # class 3 keeps only 2 training rows
    yte = rng.randint(0, c, size=n_test)
    xtr = (proto[ytr] + 1.5 * rng.standard_normal((n_train, d))).astype(np.float32)
    xte = (proto[yte] + 1.5 * rng.standard_normal((n_test, d))).astype(np.float32)
    return xtr, ytr, xte, yte, c


def test_fewshot_metrics_equals_per_task_calls_on_the_reference_subsets():
    xtr, ytr, xte, yte, c = _pool(21)
    assert (ytr == 3).sum() == 2
    shots, l2, seed = (1, 3, 10), 8.0, 5
    got = fewshot.fewshot_metrics(_dev(xtr), ytr, _dev(xte), yte, c, shots, l2, seed)
    assert list(got) == list(shots)
    subsets = F.subsets(ytr, c, seed, shots)
    routes = set()
    for k in shots:
        idx, yk = subsets[k]
        assert len(idx) == sum(min(k, int((ytr == cls).sum())) for cls in range(c))
        one = fewshot.fewshot_lsr(_dev(xtr[idx]), yk, _dev(xte), yte, c, l2)
        routes.add(one["route"])
        assert isinstance(got[k], np.float64) and got[k] == one["accuracy"], (k, got[k], one)
    assert routes == {"A", "B"}                             # 12 and 35 rows < dim = 41 <= 112 rows


# ---- 8. evaluate_fewshot ---------------------------------------------------------------------------------------------------
TOY = {"embed_dim": 64,
       "vision_cfg": {"image_size": 32, "layers": 2, "width": 128, "patch_size": 16},
       "text_cfg": {"context_length": 16, "vocab_size": 512, "width": 128, "heads": 2, "layers": 2}}


def test_evaluate_fewshot_names_values_and_one_encoding_per_dataset(tmp_path):
    path = os.path.join(str(tmp_path), "fewshot-toy.json")
    json.dump(TOY, open(path, "w"))
    clipa_amd.add_model_config(path)
    torch.manual_seed(0)
    m = clipa_amd.create_model("fewshot-toy", device=DEV, output_dict=True)
    rng = np.random.RandomState(8)

    def batches(n, c, seed):
        images = O.synthetic_batch(n, 32, 16, 512, seed=seed)[0].to(DEV)
        labels = rng.randint(0, c, size=n)
        cut = n // 2 + 3
        return [(images[:cut], torch.from_numpy(labels[:cut]).to(DEV)), (images[cut:], labels[cut:].tolist())], images, labels

    sets, raw = {}, {}
    for name, c in (("pets", 5), ("birds", 3)):
        tr, xtr, ytr = batches(60, c, 100 + c)
        te, xte, yte = batches(40, c, 200 + c)
        sets[name], raw[name] = (iter(tr), iter(te), c), (xtr, ytr, xte, yte, c)      # one-shot iterators: a second pass would fail
    calls = []
    encode = m.encode_image
    modes = []
    m.encode_image = lambda *a, **k: (calls.append(k.get("normalize")), modes.append(m.training), encode(*a, **k))[-1]
    m.train()
    shots, l2 = (1, 5), 4.0
    got = list(fewshot.evaluate_fewshot(m, sets, shots=shots, l2_reg=l2, num_seeds=2, display_first=(("birds", 5),)))
    m.encode_image = encode
    assert calls == [False] * 8                            # 2 datasets x (2 train + 2 test batches), once
    assert m.training and modes == [False] * 8             # encoded in eval mode, the caller's mode put back
    names = [f"{'a/' if (n, k) == ('birds', 5) else 'z/'}{n}_{k}shot-seed-{s}" for s in range(2) for n in ("pets", "birds") for k in shots]
    assert [n for n, _ in got] == names
    with torch.no_grad():
        enc = lambda x: torch.cat([m.encode_image(x[:33], normalize=False), m.encode_image(x[33:], normalize=False)]).float() \
            if len(x) == 60 else torch.cat([m.encode_image(x[:23], normalize=False), m.encode_image(x[23:], normalize=False)]).float()  # noqa: E731
        feats = {n: (enc(r[0]), enc(r[2])) for n, r in raw.items()}      # the same batches as above
    it = iter(got)
    for s in range(2):
        for n in ("pets", "birds"):
            _, ytr, _, yte, c = raw[n]
            want = fewshot.fewshot_metrics(feats[n][0], ytr, feats[n][1], yte, c, shots, l2, s)
            for k in shots:
                name, v = next(it)
                assert isinstance(v, np.float64) and v == want[k], (name, v, want[k])
    # the other representation: normalised features, encoded as such
    calls.clear()
    m.encode_image = lambda *a, **k: (calls.append(k.get("normalize")), encode(*a, **k))[1]
    xtr, ytr, xte, yte, c = raw["birds"]
    one = dict(fewshot.evaluate_fewshot(m, {"birds": ([(xtr, ytr)], [(xte, yte)], c)}, shots=(5,), l2_reg=l2, num_seeds=1,
                                        representation="normalized"))
    m.encode_image = encode
    assert calls == [True, True] and list(one) == ["z/birds_5shot-seed-0"]
