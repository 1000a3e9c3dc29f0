"""GPU tests of the fused fp32 retrieval-rank kernel (csrc/retrieval.hip) and of the validation pass built on it
(clipa_amd/evaluate.py, training/train.py:317-449): exact counts on exactly representable data, identical arithmetic at
every tile position, fp64 brackets on random data, the reference fixture, O(N) memory at N = 65 536, and evaluate() end
to end on a small engine model."""
import os
import sys

import numpy as np
import pytest
import torch

import clipa_amd
from clipa_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import clip_oracle as O            # noqa: E402
from tools import make_retrieval_golden as G   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(ROOT, "tests", "golden", "retrieval_metrics.npz")


def _counts_np(v):
    """Exact int64 counts from a [N, N] float64 matrix of exactly computed logits."""
    n = v.shape[0]
    d = np.diag(v)
    off = ~np.eye(n, dtype=bool)
    return ((v > d[:, None]) & off).sum(1), ((v == d[:, None]) & off).sum(1), \
        ((v > d[None, :]) & off).sum(0), ((v == d[None, :]) & off).sum(0)


def _ranks(img, txt, scale=None):
    s = None if scale is None else torch.tensor([scale], device=DEV, dtype=torch.float32)
    return [t.cpu().numpy().astype(np.int64) for t in ops.retrieval_ranks(img, txt, s)]


@pytest.mark.parametrize("E", [64, 200, 768])
@pytest.mark.parametrize("N", [1, 7, 128, 1000, 4099])
@pytest.mark.parametrize("scale", [1.0, 100.0])
def test_exact_counts_on_integer_features(N, E, scale):
    """|v| <= 8 integers: every dot product and every s * x is exact in fp32, so the counts have one right answer.
    Planted duplicate image rows, duplicate text rows and positives that tie with other entries."""
    rng = np.random.RandomState(N * 1000 + E + int(scale))
    img = rng.randint(-8, 9, size=(N, E)).astype(np.float32)
    txt = rng.randint(-8, 9, size=(N, E)).astype(np.float32)
    if N >= 7:
        k = max(N // 10, 2)
        src, dst = rng.choice(N, k, replace=False), rng.choice(N, k, replace=False)
        img[dst] = img[src]                                  # duplicate image rows
        src, dst = rng.choice(N, k, replace=False), rng.choice(N, k, replace=False)
        txt[dst] = txt[src]                                  # duplicate text rows
        for i in rng.choice(N, k, replace=False):            # positives that tie with another column: text j := text i
            j = (i + 1 + rng.randint(N - 1)) % N
            txt[j] = txt[i]
        for i in rng.choice(N, 3, replace=False):            # a positive of 0 ties with every orthogonal entry
            img[i] = 0.0
    x = img.astype(np.float64) @ txt.astype(np.float64).T
    assert np.abs(x).max() * scale < 2 ** 24                 # exact in fp32
    want = _counts_np(x * scale)
    got = _ranks(torch.from_numpy(img).to(DEV), torch.from_numpy(txt).to(DEV), scale)
    for name, g, w in zip(("i2t_gt", "i2t_eq", "t2i_gt", "t2i_eq"), got, want):
        assert np.array_equal(g, w), (name, np.nonzero(g != w)[0][:10])
    if N >= 7:
        assert want[1].sum() > 0 and want[3].sum() > 0       # the ties really are there


def test_same_arithmetic_at_every_tile_position():
    """All rows equal to one random non-integer vector: every x_ij must be bitwise the same value, the diagonal pass
    included, so every gt is 0 and every eq is N - 1 in both directions."""
    N, E = 1000, 1000
    g = torch.Generator().manual_seed(3)
    row = torch.randn(E, generator=g) * 0.37
    img = row.expand(N, E).contiguous().to(DEV)
    txt = (torch.randn(E, generator=g) * 1.3).expand(N, E).contiguous().to(DEV)
    for scale in (None, 1.0 / 0.07):
        i2t_gt, i2t_eq, t2i_gt, t2i_eq = _ranks(img, txt, scale)
        assert (i2t_gt == 0).all() and (t2i_gt == 0).all()
        assert (i2t_eq == N - 1).all() and (t2i_eq == N - 1).all()


def _bracket(x64, r, rows=None, cols=None, tau=1e-5):
    """#{x_ij > x_ii + tau} <= gt and gt + eq <= #{x_ij >= x_ii - tau} (j != i) for every selected row (i2t) and
    column (t2i)."""
    n = x64.shape[0]
    idx = torch.arange(n, device=x64.device)
    for axis, sel, g, e in (("row", rows, r[0], r[1]), ("col", cols, r[2], r[3])):
        sel = idx if sel is None else sel
        vals = x64[sel] if axis == "row" else x64[:, sel].t()
        d = x64[sel, sel][:, None]
        off = idx[None, :] != sel[:, None]
        lo = ((vals > d + tau) & off).sum(1).cpu().numpy()
        hi = ((vals >= d - tau) & off).sum(1).cpu().numpy()
        s_np = sel.cpu().numpy()
        gs, es = g[s_np], e[s_np]
        assert (lo <= gs).all(), (axis, s_np[np.nonzero(lo > gs)[0][:10]])
        assert (gs + es <= hi).all(), (axis, s_np[np.nonzero(gs + es > hi)[0][:10]])


def test_random_normalised_features_bracketed_by_fp64():
    N, E, s = 4133, 1024, 1.0 / 0.07
    g = torch.Generator(device=DEV).manual_seed(11)
    base = torch.randn(N, E, device=DEV, generator=g)
    img = torch.nn.functional.normalize(base + 3.0 * torch.randn(N, E, device=DEV, generator=g), dim=-1)
    txt = torch.nn.functional.normalize(base + 3.0 * torch.randn(N, E, device=DEV, generator=g), dim=-1)
    r = _ranks(img, txt, s)
    _bracket(s * (img.double() @ txt.double().t()), r)
    assert 0.05 < np.mean(r[0] == 0) < 0.99                 # a meaningful spread of ranks


def _fixture_inputs(z, case):
    c = G.CASES[case]
    assert (int(z[f"{case}_n"]), int(z[f"{case}_e"]), int(z[f"{case}_seed"])) == (c["n"], c["e"], c["seed"])
    (img, txt), dup = G.case_inputs(case, z[f"{case}_redraws"].astype(np.int64))
    return torch.from_numpy(img).to(DEV), torch.from_numpy(txt).to(DEV), float(z[f"{case}_scale"])


def test_reference_fixture_case_a_exact():
    z = np.load(FIXTURE)
    img, txt, s = _fixture_inputs(z, "A")
    i2t, _, t2i, _ = _ranks(img, txt, s)
    assert np.array_equal(i2t, z["A_i2t"].astype(np.int64))
    assert np.array_equal(t2i, z["A_t2i"].astype(np.int64))
    got = clipa_amd.get_clip_metrics(img, txt, torch.tensor(s, device=DEV))
    for k, v in zip([str(k) for k in z["A_metric_keys"]], z["A_metrics"]):
        assert got[k] == v, (k, got[k], v)


def test_reference_fixture_case_b_within_tie_range():
    z = np.load(FIXTURE)
    img, txt, s = _fixture_inputs(z, "B")
    i2t_gt, i2t_eq, t2i_gt, t2i_eq = _ranks(img, txt, s)
    for ref, gt, eq in ((z["B_i2t"], i2t_gt, i2t_eq), (z["B_t2i"], t2i_gt, t2i_eq)):
        ref = ref.astype(np.int64)
        assert ((gt <= ref) & (ref <= gt + eq)).all(), np.nonzero((gt > ref) | (ref > gt + eq))[0][:10]
    assert i2t_eq.sum() > 0                                  # the duplicated captions do tie


def test_scale_n65536_memory_is_linear():
    N, E, s = 65536, 1024, 1.0 / 0.07
    g = torch.Generator(device=DEV).manual_seed(5)
    base = torch.randn(N, E, device=DEV, generator=g)
    img = torch.nn.functional.normalize(base + 3.0 * torch.randn(N, E, device=DEV, generator=g), dim=-1)
    txt = torch.nn.functional.normalize(base + 3.0 * torch.randn(N, E, device=DEV, generator=g), dim=-1)
    del base
    scale = torch.tensor(s, device=DEV)
    clipa_amd.get_clip_metrics(img[:256], txt[:256], scale)              # load the library outside the measurement
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    metrics = clipa_amd.get_clip_metrics(img, txt, scale)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert rise < 16 * 2 ** 20, rise
    assert 0.0 < metrics["image_to_text_R@1"] < 1.0
    r = _ranks(img, txt, s)
    sel = torch.from_numpy(np.random.RandomState(0).choice(N, 256, replace=False)).to(DEV)
    # fp64 rows / columns of the sampled entries only: [256, N] each
    rows64 = s * (img[sel].double() @ txt.double().t())
    cols64 = s * (img.double() @ txt[sel].double().t())
    d_rows = s * (img[sel].double() * txt[sel].double()).sum(1)
    off = torch.arange(N, device=DEV)[None, :] != sel[:, None]
    for vals, g_, e_ in ((rows64, r[0], r[1]), (cols64.t(), r[2], r[3])):
        lo = ((vals > d_rows[:, None] + 1e-5) & off).sum(1).cpu().numpy()
        hi = ((vals >= d_rows[:, None] - 1e-5) & off).sum(1).cpu().numpy()
        sn = sel.cpu().numpy()
        assert (lo <= g_[sn]).all() and (g_[sn] + e_[sn] <= hi).all()


def test_evaluate_end_to_end():
    torch.manual_seed(0)
    m = clipa_amd.create_model("ViT-S-16", device=DEV, force_image_size=112, output_dict=True)
    m.positional_embedding = torch.nn.Parameter(m.positional_embedding[:32].clone())
    sizes = (64, 64, 37)
    batches = []
    for b, B in enumerate(sizes):
        img, txt = O.synthetic_batch(B, 112, 32, 49408, seed=90 + b)
        batches.append((img.to(DEV), txt.to(DEV)))
    out = clipa_amd.evaluate(m, batches, epoch=3)
    z = np.load(FIXTURE)
    assert set(out) == set(str(k) for k in z["A_metric_keys"]) | {"clip_val_loss", "epoch", "num_samples"}
    assert out["num_samples"] == 165 and out["epoch"] == 3
    assert not m.training
    # fp64 maths on the same features
    feats, want, n = [], 0.0, 0
    with torch.no_grad():
        for img, txt in batches:
            o = m(img, txt)
            i64, t64 = o["image_features"].double(), o["text_features"].double()
            s = o["logit_scale"].double().mean()
            lg = s * i64 @ t64.t()
            lab = torch.arange(img.shape[0], device=DEV)
            loss = (torch.nn.functional.cross_entropy(lg, lab) + torch.nn.functional.cross_entropy(lg.t(), lab)) / 2
            want += float(loss) * img.shape[0]
            n += img.shape[0]
            feats.append((o["image_features"].float(), o["text_features"].float(), o["logit_scale"]))
    want /= n
    assert abs(out["clip_val_loss"] - want) <= 1e-3 * abs(want), (out["clip_val_loss"], want)
    img = torch.cat([f[0] for f in feats])
    txt = torch.cat([f[1] for f in feats])
    s = float(feats[-1][2].mean())
    r = _ranks(img, txt, s)
    _bracket(s * (img.double() @ txt.double().t()), r)
    want_metrics = clipa_amd.metrics_from_ranks(r[0], r[2])       # a second forward: equal up to near ties
    for k, v in want_metrics.items():
        assert abs(out[k] - v) <= 0.02 * max(1.0, abs(v)), (k, out[k], v)
