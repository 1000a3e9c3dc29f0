"""GPU parity tests of the three fused similarity-loss kernels (csrc/simce.hip, simce_distill.hip, simsig.hip on
csrc/sim_tile.h) through clipa_amd.ops: element-wise against fp64 at the tile, K-tail, ring hand-over and stride edges.
The cases, their inputs, the fp64 references, the tolerances (and where each comes from) and the comparisons live in
tests/loss_cases.py; tests/test_loss_cases_cpu.py runs the same table through the fp32 stand-ins and shows that the
comparisons refuse seven kinds of wrong kernel.  Each test is parametrised by case name, so a failure names its branch;
run with -s for the error / tolerance figures.  Below the table: the three loss modules at a batch that is no multiple of 8.
"""
import pytest
import torch
import torch.nn.functional as F

from . import loss_cases as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
bf16, f64 = torch.bfloat16, torch.float64


def ops():
    from clipa_amd import ops as _ops
    return _ops


def _show(kind, c, figs):
    print(f"[loss_kernels {kind}/{c.name}] error / tolerance: " + ", ".join(f"{k} {v:.3g}" for k, v in figs.items() if k != "kappa_needed")
          + f"; kappa needed {figs['kappa_needed']:.3g} of {c.kappa:.3g}")


@pytest.mark.parametrize("case", L.SIMCE, ids=L.names(L.SIMCE))
def test_simce(case):
    _show("simce", case, L.check_simce(ops(), DEV, case))


@pytest.mark.parametrize("case", L.DISTILL, ids=L.names(L.DISTILL))
def test_simce_distill(case):
    _show("distill", case, L.check_distill(ops(), DEV, case))


@pytest.mark.parametrize("case", L.SIMSIG, ids=L.names(L.SIMSIG))
def test_simsig(case):
    _show("simsig", case, L.check_simsig(ops(), DEV, case))


def test_argument_errors():
    L.check_argument_errors(ops(), DEV)
    torch.cuda.synchronize()


def test_misaligned_base_equals_contiguous_copy():
    L.check_misaligned_base(ops(), DEV)


# ---- the loss modules at W = 1, B = 13: _pad_rows8 and the four gradient GEMMs at K = 16 and an 8-ragged M --------------
B, E, ET = 13, 72, 40


def _features():
    g = torch.Generator().manual_seed(4242)
    unit = lambda e: F.normalize(torch.randn(B, e, generator=g), dim=-1)      # noqa: E731
    img, dimg = unit(E), unit(ET)
    return img, F.normalize(unit(E) + img, dim=-1), dimg, F.normalize(unit(ET) + dimg, dim=-1)


def _leaves(img, txt, *scalars):
    return (img.to(bf16).double().requires_grad_(True), txt.to(bf16).double().requires_grad_(True),
            *(torch.tensor(v, dtype=f64, requires_grad=True) for v in scalars))


def _assert_loss_and_grads(got, ref):
    """The bounds of test_siglip_gpu._assert_loss_and_grads; got / ref = (values, d image, d text, scalar gradients)."""
    for a, r in zip(got[0], ref[0]):
        assert abs(a - r) <= 1e-4 * abs(r) + 2e-4, (a, r)
    for a, r in zip(got[1:3], ref[1:3]):
        assert a.shape == r.shape
        assert float((a.double() - r).norm()) <= 2.0 ** -7 * float(r.norm()), float((a.double() - r).norm() / r.norm())
    for a, r in zip(got[3], ref[3]):
        assert abs(a - r) <= 2e-3 * abs(r) + 2e-5, (a, r)


def _run(fn, img, txt, scalars, extra=()):
    i = img.clone().to(DEV).requires_grad_(True)
    t = txt.clone().to(DEV).requires_grad_(True)
    ps = [torch.nn.Parameter(torch.tensor(v, device=DEV)) for v in scalars]
    out = fn(i, t, *ps, *extra)
    values = out if isinstance(out, tuple) else (out,)
    sum(values).backward()
    torch.cuda.synchronize()
    assert all(p.grad.shape == () for p in ps)
    return [float(v.detach()) for v in values], i.grad.cpu(), t.grad.cpu(), [float(p.grad) for p in ps]


def _ce2(z):
    lab = torch.arange(z.shape[0])
    return (F.cross_entropy(z, lab) + F.cross_entropy(z.T, lab)) / 2


def test_clip_loss_at_a_batch_of_13():
    import clipa_amd
    img, txt, _, _ = _features()
    I, T, s = _leaves(img, txt, 14.3)
    loss = _ce2(s * I @ T.T)
    gi, gt, gs = torch.autograd.grad(loss, (I, T, s))
    _assert_loss_and_grads(_run(clipa_amd.ClipLoss(), img, txt, (14.3,)), ([float(loss.detach())], gi, gt, [float(gs)]))


def test_distill_clip_loss_at_a_batch_of_13():
    import clipa_amd
    img, txt, dimg, dtxt = _features()
    I, T, s = _leaves(img, txt, 14.3)
    z = s * I @ T.T
    y = 30.0 * dimg.to(bf16).double() @ dtxt.to(bf16).double().T
    h = lambda y, z: -(y.softmax(1) * z.log_softmax(1)).sum(1).mean()      # noqa: E731
    con, dis = _ce2(z), (h(y, z) + h(y.T, z.T)) / 2
    gi, gt, gs = torch.autograd.grad(con + dis, (I, T, s))
    got = _run(clipa_amd.DistillClipLoss(), img, txt, (14.3,), (dimg.to(DEV), dtxt.to(DEV), torch.tensor(30.0, device=DEV)))
    _assert_loss_and_grads(got, ([float(con.detach()), float(dis.detach())], gi, gt, [float(gs)]))


def test_siglip_loss_at_a_batch_of_13():
    import clipa_amd
    img, txt, _, _ = _features()
    I, T, s, b = _leaves(img, txt, 10.0, -10.0)
    y = 2.0 * torch.eye(B, dtype=f64) - 1.0
    loss = -F.logsigmoid(y * (s * I @ T.T + b)).sum() / B
    gi, gt, gs, gb = torch.autograd.grad(loss, (I, T, s, b))
    _assert_loss_and_grads(_run(clipa_amd.SigLipLoss(), img, txt, (10.0, -10.0)), ([float(loss.detach())], gi, gt, [float(gs), float(gb)]))
