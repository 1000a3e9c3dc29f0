"""The case table of tests/loss_cases.py through tests/cpu_ops, the fp32 torch stand-ins of the fused similarity-loss
kernels.  Three things are established here without a GPU:
  * the stand-ins keep the contract tests/test_loss_kernels_gpu.py holds the kernels to (same cases, same comparisons);
  * the kappa of every case: `kappa_fp32` in the table is what the stand-in needs against the fp64 reference (printed per
    case, run with -s) and `kappa` follows from it by loss_cases.kappa_rule - never from a kernel;
  * the comparisons can fail: seven stand-ins that are wrong in one way each are refused on at least one case, and the one
    that drops the teacher term off the diagonal passes the comparison test_distill_gpu.py used to make.
"""
import types

import pytest
import torch

from . import cpu_ops
from . import loss_cases as L

DEV = "cpu"
bf16 = torch.bfloat16


def _show(kind, c, figs):
    print(f"[loss_cases {kind}/{c.name}] kappa needed by the fp32 stand-in {figs['kappa_needed']:.3g} (table "
          f"{c.kappa_fp32:.3g}, used {c.kappa:.3g}); error / tolerance: "
          + ", ".join(f"{k} {v:.3g}" for k, v in figs.items() if k != "kappa_needed"))


@pytest.mark.parametrize("case", L.SIMCE, ids=L.names(L.SIMCE))
def test_simce(case):
    _show("simce", case, L.check_simce(cpu_ops, DEV, case))


@pytest.mark.parametrize("case", L.DISTILL, ids=L.names(L.DISTILL))
def test_simce_distill(case):
    _show("distill", case, L.check_distill(cpu_ops, DEV, case))


@pytest.mark.parametrize("case", L.SIMSIG, ids=L.names(L.SIMSIG))
def test_simsig(case):
    _show("simsig", case, L.check_simsig(cpu_ops, DEV, case))


def test_argument_errors():
    L.check_argument_errors(cpu_ops, DEV)


def test_misaligned_base():
    L.check_misaligned_base(cpu_ops, DEV)


def test_ops_copy_an_operand_whose_base_is_not_16_byte_aligned():
    """The host side of test_misaligned_base_equals_contiguous_copy: what the similarity wrappers hand to the kernels."""
    from clipa_amd import ops
    buf = torch.arange(16 * 216, dtype=torch.float32).reshape(16, 216).to(bf16)
    for view, copied in ((buf[:, 4:76], True), (buf[:, 8:80], False), (buf[:, 72:144], False), (buf, False),
                         (buf.reshape(-1)[4:4 + 4 * 72].view(4, 72), True), (buf[3:4, 4:76], True)):
        t, ld = ops._aligned16(view)
        assert t.data_ptr() % 16 == 0 and ld % 8 == 0 and torch.equal(t, view)
        assert (t.data_ptr() != view.data_ptr()) == copied
        assert ld == (72 if copied else max(view.stride(0), view.shape[1]))


@pytest.mark.parametrize("kind", ["simce", "distill", "simsig"])
def test_kappa_follows_the_rule(kind):
    """kappa = max(4 x the fp32 stand-in's need, 2^-20), and the recorded need is not below today's measurement."""
    for c in L._TABLE[kind]:
        assert c.kappa == L.kappa_rule(c.kappa_fp32), c.name
        figs = getattr(L, {"simce": "check_simce", "distill": "check_distill", "simsig": "check_simsig"}[kind])(cpu_ops, DEV, c)
        assert figs["kappa_needed"] <= c.kappa_fp32 * 1.5 + 1e-12, (c.name, figs["kappa_needed"], c.kappa_fp32)


def test_every_case_is_live():
    """From the reference alone: half of dl above 1e-4 of its maximum, median label probability in [0.01, 0.99]."""
    for kind, cases in L._TABLE.items():
        for c in cases:
            ref = L._reference_of(kind, c.name)
            share, p_med = L.liveness(ref)
            print(f"[loss_cases {kind}/{c.name}] sigma {c.sigma} live share {share:.3f} median label probability {p_med:.4f} "
                  f"max |z| {ref['zmax']:.1f}")
            L.assert_live(c, ref)
    sat = L._reference_of("simce", "saturated")
    assert float(sat["loss_rows"].max()) > 100.0 and float(sat["mag"].min()) < 2.0 ** -126


# ---- negative controls: stand-ins that are wrong in one way each -----------------------------------------------------
def _wrap(**over):
    o = types.SimpleNamespace(**{k: getattr(cpu_ops, k) for k in ("simce", "simsig", "simce_distill", "simce_distill_bwd")})
    o.__dict__.update(over)
    return o


def _pads_in_softmax():
    """(a) the soft-max runs over the pad columns n_valid ... n8 as well."""
    n8 = lambda n: (n + 7) // 8 * 8      # noqa: E731
    return _wrap(simce=lambda r, c, n, *a, **k: cpu_ops.simce(r, c, n8(n), *a, **k),
                 simce_distill=lambda rs, cs, rt, ct, n, *a, **k: cpu_ops.simce_distill(rs, cs, rt, ct, n8(n), *a, **k),
                 simce_distill_bwd=lambda rs, cs, rt, ct, n, *a, **k: cpu_ops.simce_distill_bwd(rs, cs, rt, ct, n8(n), *a, **k))


def _k64(x):
    """x [n, E] as the kernel would read it with K rounded up to 64: the elements that follow each row in memory."""
    E64 = (x.shape[1] + 63) // 64 * 64
    base = x if x._base is None else x._base
    flat = torch.cat([base.reshape(-1), torch.zeros(64, dtype=x.dtype)])
    return flat.as_strided((x.shape[0], E64), (x.stride(0), 1), x.storage_offset())


def _k_rounded_up():
    """(b) K is rounded up to 64: a strided operand's neighbours enter the product."""
    return _wrap(simce=lambda r, c, *a, **k: cpu_ops.simce(_k64(r), _k64(c), *a, **k),
                 simsig=lambda r, c, *a, **k: cpu_ops.simsig(_k64(r), _k64(c), *a, **k),
                 simce_distill=lambda rs, cs, rt, ct, *a, **k: cpu_ops.simce_distill(rs, cs, _k64(rt), _k64(ct), *a, **k),
                 simce_distill_bwd=lambda rs, cs, rt, ct, *a, **k: cpu_ops.simce_distill_bwd(rs, cs, _k64(rt), _k64(ct), *a, **k))


def _label0_ignored():
    """(c) the labels are the plain diagonal."""
    return _wrap(simce=lambda r, c, n, l0, *a, **k: cpu_ops.simce(r, c, n, 0, *a, **k),
                 simce_distill=lambda rs, cs, rt, ct, n, l0, *a, **k: cpu_ops.simce_distill(rs, cs, rt, ct, n, 0, *a, **k),
                 simce_distill_bwd=lambda rs, cs, rt, ct, n, l0, *a, **k: cpu_ops.simce_distill_bwd(rs, cs, rt, ct, n, 0, *a, **k))


def _teacher_on_diagonal_only():
    """(d) distill: the teacher term of the off-diagonal entries is dropped (p_t only at the label)."""
    def bwd(rs, cs, rt, ct, n, l0, gscale, lse_s, lse_t, scale_s=None, scale_t=None, g_c=None, g_d=None):
        dl, ds = cpu_ops.simce_distill_bwd(rs, cs, rt, ct, n, l0, gscale, lse_s, lse_t, scale_s, scale_t, g_c, g_d)
        s, u, gd = (float(t[0]) if t is not None else 1.0 for t in (scale_s, scale_t, g_d))
        pt = torch.exp((rt.float() @ ct[:n].float().T) * u - lse_t[:, None])
        pt[torch.arange(rs.shape[0]), torch.arange(rs.shape[0]) + l0] = 0.0
        dl[:, :n] = (dl[:, :n].float() + s * gscale * gd * pt).to(bf16)
        return dl, ds
    return _wrap(simce_distill_bwd=bwd)


def _teacher_with_student_scale():
    """(e) distill: p_t is computed with s instead of u."""
    return _wrap(simce_distill=lambda rs, cs, rt, ct, n, l0, s=None, u=None: cpu_ops.simce_distill(rs, cs, rt, ct, n, l0, s, s),
                 simce_distill_bwd=lambda rs, cs, rt, ct, n, l0, gs, ls, lt, s=None, u=None, *a:
                 cpu_ops.simce_distill_bwd(rs, cs, rt, ct, n, l0, gs, ls, lt, s, s, *a))


def _on_dl(edit):
    def simce(*a, **k):
        out = cpu_ops.simce(*a, **k)
        return out if out[1] is None else (out[0], edit(out[1]), out[2])

    def simsig(*a, **k):
        out = cpu_ops.simsig(*a, **k)
        return out if out[1] is None else (out[0], edit(out[1])) + tuple(out[2:])

    def bwd(*a, **k):
        dl, ds = cpu_ops.simce_distill_bwd(*a, **k)
        return edit(dl), ds
    return _wrap(simce=simce, simsig=simsig, simce_distill_bwd=bwd)


def _one_column_zeroed():
    """(f) one column of dl is never written."""
    def edit(dl):
        dl = dl.clone()
        dl[:, dl.shape[1] // 2 - 1] = 0
        return dl
    return _on_dl(edit)


def _lane_halves_swapped():
    """(g) dl column j lands in column j ^ 4: the two lane halves of the fragment map exchanged."""
    return _on_dl(lambda dl: dl[:, torch.arange(dl.shape[1]) ^ 4])


def _refused(o, kinds=("simce", "distill", "simsig")):
    """-> the cases on which the comparison refuses the ops module `o`."""
    bad = []
    for kind, check in (("simce", L.check_simce), ("distill", L.check_distill), ("simsig", L.check_simsig)):
        for c in L._TABLE[kind] if kind in kinds else ():
            try:
                check(o, DEV, c)
            except AssertionError:
                bad.append(f"{kind}/{c.name}")
    return bad


@pytest.mark.parametrize("make,must", [
    (_pads_in_softmax, {"simce/ktail_72_step_plus_one_chunk_n_mod_8", "distill/teacher_1_step_student_2_both_k_tails"}),
    (_k_rounded_up, {"simce/packed_views", "distill/packed_views", "simsig/packed_views"}),
    (_label0_ignored, {"simce/labels_in_a_tile_of_8", "distill/teacher_2_steps_ends_on_slot_1"}),
    (_teacher_on_diagonal_only, {"distill/teacher_1_step_student_2_both_k_tails", "distill/sharp_teacher"}),
    (_teacher_with_student_scale, {"distill/teacher_3_steps_student_1_row_64_alone"}),
    (_one_column_zeroed, {"simce/ktail_72_step_plus_one_chunk_n_mod_8", "distill/scales_100_clustered", "simsig/packed_views"}),
    (_lane_halves_swapped, {"simce/one_row_k8_label_in_last_column", "distill/pure_distill", "simsig/packed_views"}),
], ids=["a_pads_in_softmax", "b_k_rounded_up", "c_label0_ignored", "d_teacher_on_diagonal_only", "e_teacher_with_student_scale",
        "f_one_column_zeroed", "g_lane_halves_swapped"])
def test_negative_control_is_refused(make, must):
    bad = _refused(make())
    print(f"[loss_cases {make.__name__}] refused on {len(bad)} cases: {bad}")
    assert must <= set(bad), (make.__doc__, sorted(must - set(bad)))


def test_the_old_distill_comparison_passes_the_dropped_teacher_term():
    """The gap this table closes: control (d) under the comparison test_simce_distill_kernel_matches_fp64 used to make
    (max |err| < 1e-2 max |dl| + 1e-6 s, cosine > 0.9999).  max |dl| is the diagonal term and an off-diagonal entry is
    about 1 / N of it, so the teacher's whole off-diagonal contribution fits under the bound."""
    c = L.case("distill", "sharp_teacher")
    rs, cs, rt, ct = L._distill_inputs(c.name)
    ref = L._reference_of("distill", c.name)
    o = _teacher_on_diagonal_only()
    s, u, gc, gd = (torch.tensor([v]) for v in (c.s, c.u, c.gc, c.gd))
    f = o.simce_distill(rs, cs, rt, ct, c.N, c.label0, s, u)
    dl, _ = o.simce_distill_bwd(rs, cs, rt, ct, c.N, c.label0, 0.5 / c.R, f[2], f[3], s, u, gc, gd)
    d, want = dl[:, :c.N].double(), ref["dl"]
    assert float((d - want).abs().max()) < 1e-2 * float(want.abs().max()) + 1e-6 * c.s
    assert float(d.reshape(-1) @ want.reshape(-1) / (d.norm() * want.norm())) > 0.9999
    wrong = int(((d - want).abs() > L.DL_RTOL * want.abs() + c.kappa * ref["mag"]).sum())
    print(f"[loss_cases] control (d) passes the old comparison with {wrong} of {d.numel()} entries outside the element-wise bound")
    assert wrong > 100
    with pytest.raises(AssertionError):
        L.check_distill(o, DEV, c)
