"""GPU parity tests of the fp8 path (clipa_quantize_rows, clipa_gemm_nt_f8, clipa_layernorm_fwd_q8) through the C ABI.

The reference has no fp8 mode (clipa_torch/training/params.py:195-200), so the oracle for these kernels is plain torch
on the CPU: torch.float8_e4m3fn / float8_e5m2 are the same OCP encodings, their casts round to nearest even, and a GEMM of
fp8 operands is checked against an fp64 product of the SAME de-quantised bytes - the only differences left are the fp32
accumulation order and the bf16 rounding of the output (<= 2^-8 relative), as for the bf16 GEMM tests.
"""
import math

import pytest
import torch

from oracle import clip_oracle as O
from . import tile_walk as TW
from .test_kernels_gpu import act_grad, check_dev, num_cu, ref_act, rows_by_tile      # shared with the bf16 multi-tile tests

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
DEV = "cuda"
F8 = {0: (torch.float8_e4m3fn, 448.0), 1: (torch.float8_e5m2, 57344.0)}


def ops():
    from clipa_amd import ops as _ops
    return _ops


def rnd(*shape, seed=0, scale=1.0, dtype=bf16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def cpu_quantize(x, fmt):
    """Row-scaled fp8 quantisation restated with torch CPU ops: -> (q fp8 tensor, dq f32 [rows])."""
    dt, fmax = F8[fmt]
    xf = x.float()
    amax = xf.abs().amax(dim=1)
    s = torch.where(amax > 0, torch.tensor(fmax) / amax, torch.ones_like(amax))
    dq = torch.where(amax > 0, amax / fmax, torch.zeros_like(amax))
    return (xf * s[:, None]).to(dt), dq


def check(name, got, ref, rtol, atol):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), (f"{name}: {int(bad.sum())}/{got.numel()} outside tol, max abs err {err.max().item():.4g}, "
                           f"ref scale {ref.abs().max().item():.4g}")


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("M,K", [(37, 64), (500, 776), (1030, 1024), (260, 1280), (129, 5120)])
def test_quantize_rows(M, K, fmt):
    g = torch.Generator().manual_seed(M + K)
    x = torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g) * 3.0)   # row magnitudes over ~5 decades
    x[M // 2] = 0.0                                                                          # an all-zero row (padding tokens)
    x = x.to(bf16)
    q, dq = ops().quantize_rows(x.to(DEV), fmt)
    qr, dqr = cpu_quantize(x, fmt)
    dt = F8[fmt][0]
    got = q.cpu().view(dt).float()
    assert torch.isfinite(got).all()
    torch.testing.assert_close(dq.cpu(), dqr, rtol=1e-6, atol=0)
    same = (q.cpu() == qr.view(torch.uint8)).float().mean().item()
    assert same > 0.999, f"only {same:.5f} of the fp8 bytes equal torch's cast"          # scale rounding may flip a tie
    half_ulp = 2.0 ** -4 if fmt == 0 else 2.0 ** -3
    deq = got * dq.cpu()[:, None]
    sub = dq.cpu()[:, None] * (2.0 ** -10 if fmt == 0 else 2.0 ** -17)                  # half a subnormal step
    assert ((deq - x.float()).abs() <= half_ulp * x.float().abs() * 1.001 + sub).all(), "quantisation error above half an ulp"
    assert (deq[M // 2] == 0).all() and dq[M // 2].item() == 0.0


# K = 512 (NCH - 1) + 8 puts one lane into the last 16-byte chunk of each of quantize_rows_colsum_kernel's eight instantiations
# (1, 2, 3, 4, 6, 8, 10, 16 chunks per lane) and reaches all five of quantize_rows_kernel (1, 2, 4, 8, 16); 8192 fills the
# widest.  (8200, 520): more rows than 4 x QUANT_COLSUM_BLOCKS, so the persistent loop and its prefetch run a second pass.
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("M,K", [(37, K) for K in (8, 520, 1032, 1544, 2568, 3592, 4616, 7688, 8192)] + [(8200, 520)])
def test_quantize_rows_every_instantiation(M, K, fmt):
    """Both row quantisers at every compiled chunk count.  Plain form against cpu_quantize and the input (the error bound
    fails any wrong byte); column-sum form: q, dq equal to the plain form's (same maximum, scale and conversion, only the
    row-to-wave mapping differs), column sums against fp64 within 1e-5 x the largest column's sum of magnitudes, row norms
    against the fp32 norms of the input, and a second call returning identical tensors (fixed-order reductions)."""
    g = torch.Generator().manual_seed(M + K)
    x = torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g) * 3.0)   # row magnitudes over ~5 decades
    x[M // 2] = 0.0                                                                          # an all-zero row (padding tokens)
    x = x.to(bf16)
    xd = x.to(DEV)
    q, dq = ops().quantize_rows(xd, fmt)
    _, dqr = cpu_quantize(x, fmt)
    got = q.cpu().view(F8[fmt][0]).float()
    assert torch.isfinite(got).all()
    torch.testing.assert_close(dq.cpu(), dqr, rtol=1e-6, atol=0)
    half_ulp = 2.0 ** -4 if fmt == 0 else 2.0 ** -3
    deq = got * dq.cpu()[:, None]
    sub = dq.cpu()[:, None] * (2.0 ** -10 if fmt == 0 else 2.0 ** -17)                  # half a subnormal step
    assert ((deq - x.float()).abs() <= half_ulp * x.float().abs() * 1.001 + sub).all(), "quantisation error above half an ulp"
    assert (q[M // 2] == 0).all() and dq[M // 2].item() == 0.0

    qc, dqc, cs, rn = ops().quantize_rows(xd, fmt, want_colsum=True, want_rownorm=True)
    assert torch.equal(qc, q) and torch.equal(dqc, dq)
    want = x.double().sum(0)
    scale = float(x.double().abs().sum(0).max())
    assert float((cs.cpu().double() - want).abs().max()) <= 1e-5 * scale
    torch.testing.assert_close(rn.cpu(), x.float().norm(dim=1), rtol=1e-5, atol=1e-6)
    again = ops().quantize_rows(xd, fmt, want_colsum=True, want_rownorm=True)
    assert all(torch.equal(a, b) for a, b in zip((qc, dqc, cs, rn), again))


def _f8_operands(M, N, K, fmt_a, fmt_b, seed):
    a = rnd(M, K, seed=seed) * torch.exp(rnd(M, 1, seed=seed + 1, dtype=f32))            # asymmetric, row-dependent scales
    b = rnd(N, K, seed=seed + 2, scale=0.05)
    qa, sa = cpu_quantize(a.to(bf16), fmt_a)
    qb, sb = cpu_quantize(b.to(bf16), fmt_b)
    ref = (qa.double() * sa.double()[:, None]) @ (qb.double() * sb.double()[:, None]).T
    return qa.view(torch.uint8), sa, qb.view(torch.uint8), sb, ref


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (300, 264, 144), (1000, 768, 1024), (77, 2304, 768), (512, 512, 3072),
                                    (2048, 256, 4096)])
def test_gemm_nt_f8_shapes(M, N, K):
    qa, sa, qb, sb, ref = _f8_operands(M, N, K, 0, 0, seed=M + N + K)
    bias = rnd(N, seed=3, dtype=f32)
    out = ops().gemm_nt_f8(qa.to(DEV), sa.to(DEV), qb.to(DEV), sb.to(DEV), bias.to(DEV), alpha=0.5)
    check("fp8 gemm", out, ref * 0.5 + bias.double(), 2 ** -7, 2e-3)
    out = ops().gemm_nt_f8(qa.to(DEV), None, qb.to(DEV), None)                           # raw byte product, no scales
    raw = qa.view(torch.float8_e4m3fn).double() @ qb.view(torch.float8_e4m3fn).double().T
    check("fp8 gemm, unit scales", out, raw, 2 ** -7, raw.abs().max().item() * 2 ** -9)


@pytest.mark.parametrize("fmt_a,fmt_b", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_gemm_nt_f8_formats(fmt_a, fmt_b):
    """e4m3 / e5m2 on either operand: a swapped format selector decodes the wrong exponent width and fails by orders of
    magnitude."""
    M, N, K = 520, 392, 272
    qa, sa, qb, sb, ref = _f8_operands(M, N, K, fmt_a, fmt_b, seed=11)
    out = ops().gemm_nt_f8(qa.to(DEV), sa.to(DEV), qb.to(DEV), sb.to(DEV), fmt_a=fmt_a, fmt_b=fmt_b)
    check(f"formats {fmt_a},{fmt_b}", out, ref, 2 ** -7, 2e-3)


@pytest.mark.parametrize("act", [0, 1, 2])
def test_gemm_nt_f8_epilogues(act):
    o = ops()
    M, N, K = 1000, 520, 784                      # several tiles per persistent workgroup, ragged M / N, K tail of 16
    qa, sa, qb, sb, lin = _f8_operands(M, N, K, 0, 0, seed=21)
    bias, aux = rnd(N, seed=8, dtype=f32), rnd(M, N, seed=9)
    v = (lin + bias.double()).to(bf16).double()
    A, SA, B, SB, BIAS, AUX = qa.to(DEV), sa.to(DEV), qb.to(DEV), sb.to(DEV), bias.to(DEV), aux.to(DEV)
    ref_act = lambda x: O.activation(x, {0: "gelu_erf", 1: "gelu_tanh", 2: "quick_gelu"}[act])
    prev = None
    for rep in range(2):                           # the second launch re-uses ring state
        out, pre = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_ACT, act=act, want_pre=True)
        one = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_ACT, act=act)
        add = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_ADD, aux=AUX)
        dact = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_DACT, act=act, aux=AUX)
        check("pre-activation", pre, v, 2 ** -7, 2e-3)
        check("act", out, ref_act(pre.double().cpu()), 2 ** -7, 2e-3)
        assert torch.equal(out, one), "activation epilogue with / without the pre-activation copy"
        check("residual add", add, v + aux.double(), 2 ** -6, 2e-2)
        x = aux.double().clone().requires_grad_(True)
        ref_act(x).sum().backward()
        check("act backward", dact, v * x.grad, 2 ** -6, 6e-3)
        got = (out, pre, add, dact)
        if prev is not None:
            assert all(torch.equal(x, y) for x, y in zip(prev, got)), "second launch differs"
        prev = got


def _debug_set(variant, abl):
    from clipa_amd import lib
    lib.debug_set(variant, abl)          # csrc/internal_hooks.h: not part of the C ABI, enabled per process through the environment
    return lib


@pytest.mark.parametrize("fmt_a", [0, 1])
@pytest.mark.parametrize("M,N,K", [(512, 256, 768), (1024, 768, 512), (768, 512, 1280)])
def test_gemm_f8a_matches_gemm_nt_f8(M, N, K, fmt_a):
    """Whole-tile shapes run on gemm_f8a (four waves, generated main loop, gemm_f8a.hip); every epilogue against the oracle and BIT
    FOR BIT against gemm_nt_f8_kernel (lib.debug_set(1, .) keeps that kernel), both A formats.  2-12 tiles: one tile per workgroup
    on a 256-CU part; workgroups that run a second and a third tile are test_gemm_f8a_past_one_tile_per_workgroup's subject."""
    o = ops()
    qa, sa, qb, sb, lin = _f8_operands(M, N, K, fmt_a, 0, seed=31 + fmt_a)
    bias, aux = rnd(N, seed=8, dtype=f32), rnd(M, N, seed=9)
    A, SA, B, SB, BIAS, AUX = qa.to(DEV), sa.to(DEV), qb.to(DEV), sb.to(DEV), bias.to(DEV), aux.to(DEV)

    def run():
        out, pre = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_ACT, act=0, want_pre=True, fmt_a=fmt_a, alpha=0.75)
        return (o.gemm_nt_f8(A, SA, B, SB, BIAS, fmt_a=fmt_a, alpha=0.75), out, pre,
                o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_ACT, act=2, fmt_a=fmt_a, alpha=0.75),
                o.gemm_nt_f8(A, SA, B, SB, None, epi=o.EPI_ADD, aux=AUX, fmt_a=fmt_a, alpha=0.75),
                o.gemm_nt_f8(A, None, B, SB, BIAS, epi=o.EPI_DACT, act=0, aux=AUX, fmt_a=fmt_a, alpha=0.75))
    try:
        h = _debug_set(1, 0)
        old = run()
        assert h.last_gemm() == 7
        _debug_set(0, 0)
        new = run()
        assert h.last_gemm() == 6, "the whole-tile shape did not reach gemm_f8a"
        again = run()
    finally:
        _debug_set(0, 0)
    check("bias", new[0], 0.75 * lin + bias.double(), 2 ** -7, 2e-3)
    for name, a, b, c in zip(("bias", "gelu", "pre", "quick_gelu", "residual", "gelu_bwd"), old, new, again):
        assert torch.equal(a, b), f"{name}: gemm_f8a differs from gemm_nt_f8_kernel"
        assert torch.equal(b, c), f"{name}: second launch differs"


# ---- the persistent fp8 NT GEMMs past one tile per workgroup ----------------------------------------------------------------
# The fp8 twin of test_kernels_gpu.py::test_gemm_nta_past_one_tile_per_workgroup: see the comment there and tests/tile_walk.py.
# Between two tiles gemm_f8a also reloads the tile's row scales, bias, column scales and output scales into its LDS window.
def _f8_tile_operands(M, N, K, fmt_a, seed):
    """_f8_operands with magnitudes that depend on the tile (tile_walk.tile_factors): the rows of a - and so their scales sa and
    every row-wise output scale derived from them - by M panel, the rows of b, sb and the bias by N tile.  Sized for matrices of
    17 000 rows and K up to 4096: row magnitudes exp(N(0, 1/4)) (e^-2 .. e^2 over that many rows) and weights of 0.05 sqrt(512 / K)
    keep every pre-activation below 60 in magnitude.  The polynomial erf-GELU has a documented tail error of 1.2e-5 |x| beyond
    |x| = 4.5 (csrc/common.h), which reaches the 2e-3 absolute tolerance of the activation checks at |x| = 166; _f8_operands' own
    exp(N(0, 1)) rows at K = 4096 put pre-activations of -170 among 17 million.
    -> bytes and scales of both operands, bias, the bf16 operands themselves (for the row-bound recipes)."""
    g = torch.Generator().manual_seed(seed)
    fa, fb = rows_by_tile(M, 7, 13), rows_by_tile(N, 5, 11)
    a = (torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g) * 0.5) * fa[:, None]).to(bf16)
    b = (torch.randn(N, K, generator=g) * (0.05 * math.sqrt(512.0 / K)) * fb[:, None]).to(bf16)
    bias = torch.randn(N, generator=g) * fb * 0.5
    qa, sa = cpu_quantize(a, fmt_a)
    qb, sb = cpu_quantize(b, 0)
    return qa, sa, qb, sb, bias, a, b


def _f8_product(qa, sa, qb, sb, rows=None):
    if rows is not None:
        qa, sa = qa[rows], sa[rows]
    return (qa.double() * sa.double()[:, None]) @ (qb.double() * sb.double()[:, None]).T


@pytest.mark.parametrize("name,fmt_a", [("S1", 0), ("S1", 1), ("S2", 0), ("S3", 0)])
def test_gemm_f8a_past_one_tile_per_workgroup(name, fmt_a):
    """gemm_f8a with two and three tiles per workgroup (tile_walk.SHAPES; the test FAILS where no workgroup gets a second tile).
    S1, both A formats: the 12 instantiations of its launcher - NONE, ACT without / with the bf16 / e4m3 pre-activation copy (the
    three activations), ADD, DACT from bf16 / e4m3 aux, the three producer-quantised activation forms, the producer-quantised DACT
    from e4m3 bytes with column sums, the emitting DACT (three activations).  S2, S3 (e4m3): plain, ACT with either copy, ADD, the
    emitting DACT, the quantised DACT with its per-tile column-sum partials.
      * dispatch: last_gemm and the exact gemm_counts of gemm_f8a and of its e4m3 / quantised / emitting forms, none on gemm_nt_f8_kernel;
      * the forms gemm_nt_f8_kernel has: bit for bit that kernel (lib.debug_set(1, 0)), itself multi-tile here;
      * the e4m3, quantised and emitting forms: bit for bit the launches they replace (cast_e4m3 / e4m3_to_bf16 / scale_quantize_rows
        around that kernel's outputs) - tanh-GELU emit: fewer than 1e-3 of the elements one bf16 step (2^-7) apart, as
        test_gemm_nt_f8_emit_matches_the_two_launches; column sums at rtol 2e-4 as test_gemm_f8a_producer_quantised_outputs;
      * bit for bit itself on a second launch and after launches of another shape in between;
      * plain, pre-activation and activation outputs against the fp64 product of the same de-quantised bytes at 2^-7 / 2e-3, every
        element (S3: the panels of test_gemm_nta_past_one_tile_per_workgroup)."""
    o = ops()
    from clipa_amd import lib
    M, N, K = TW.SHAPES[name]
    full = name == "S1"
    w = TW.walk(M, N, K, 1, num_cu())
    TW.require_second_tiles(w, f"gemm_f8a {name} on {num_cu()} CUs")
    qa, sa, qb, sb, bias, a16, b16 = _f8_tile_operands(M, N, K, fmt_a, seed=M + N + fmt_a)
    A, SA, B, SB, BIAS = qa.view(torch.uint8).to(DEV), sa.to(DEV), qb.view(torch.uint8).to(DEV), sb.to(DEV), bias.to(DEV)
    gd = torch.Generator(device=DEV).manual_seed(K)
    AUX = torch.randn(M, N, generator=gd, device=DEV, dtype=f32).to(bf16)
    one = torch.ones(1, device=DEV)
    # the recipes of test_gemm_f8a_producer_quantised_outputs / test_gemm_nt_f8_emit_matches_the_two_launches
    rn, wn = a16.float().norm(dim=1).to(DEV), o.rownorm_max(b16.to(DEV))
    _, inv = o.row_bound(rn, wn, o.absmax(BIAS), 1.13)
    _, sodh = o.row_bound(rn, wn, None, 1.13 * 1.13)
    sg = (torch.rand(M, generator=gd, device=DEV) * 0.02 + 1e-3)
    t = o.rowscale_max(SA, sg)
    kw = dict(fmt_a=fmt_a, alpha=0.75)
    acts = (0, 1, 2)
    # the e4m3 operand of the GELU-backward forms: this product's own pre-activation bytes (always written by gemm_f8a)
    _, H8 = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_ACT, act=0, want_pre="e4m3", **kw)
    HB = o.e4m3_to_bf16(H8)

    def both(r):           # the forms gemm_nt_f8_kernel has too
        r["bias"] = o.gemm_nt_f8(A, SA, B, SB, BIAS, **kw)
        r["act_pre"], r["pre"] = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_ACT, act=0, want_pre=True, **kw)
        r["residual"] = o.gemm_nt_f8(A, SA, B, SB, None, epi=o.EPI_ADD, aux=AUX, **kw)
        if full:
            for act in acts:
                r[f"act{act}"] = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_ACT, act=act, **kw)
            r["gelu_bwd"] = o.gemm_nt_f8(A, None, B, SB, BIAS, epi=o.EPI_DACT, act=0, aux=AUX, **kw)
        return r

    def composed(r):       # the launches the other forms replace, around gemm_nt_f8_kernel
        r["act_pre8"], r["pre8"] = r["act_pre"], o.cast_e4m3(r["pre"])
        dh = o.gemm_nt_f8(A, SA, B, SB, None, epi=o.EPI_DACT, act=0, aux=HB, **kw)
        r["q_gelu_bwd8"], r["colsum"] = o.scale_quantize_rows(dh, sodh, one), dh.double().sum(0)
        r["colsum_atol"] = 1e-6 * float(dh.float().abs().sum(0).max())
        for act in acts:
            r[f"emit_dh{act}"] = o.gemm_nt_f8(A, SA, B, SB, None, epi=o.EPI_DACT, act=act, aux=HB, fmt_a=fmt_a)
            r[f"emit_x8_{act}"] = o.scale_quantize_rows(H8, SA, t, act=act)
        if full:
            r["gelu_bwd8"] = dh
            r["q_act"] = r["q_act_pre"] = r["q_act_pre8"] = o.scale_quantize_rows(r["act0"], inv, one)
            r["q_pre"], r["q_pre8"] = r["pre"], r["pre8"]
        return r

    def fused(r):
        r["act_pre8"], r["pre8"] = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_ACT, act=0, want_pre="e4m3", **kw)
        r["q_gelu_bwd8"], r["colsum"] = o.gemm_nt_f8(A, SA, B, SB, None, epi=o.EPI_DACT, act=0, aux=H8, out_scale=sodh, want_colsum=True, **kw)
        for act in acts:
            r[f"emit_dh{act}"], r[f"emit_x8_{act}"] = o.gemm_nt_f8_emit(A, SA, B, SB, H8, t, act=act, fmt_a=fmt_a)
        if full:
            r["gelu_bwd8"] = o.gemm_nt_f8(A, SA, B, SB, None, epi=o.EPI_DACT, act=0, aux=H8, **kw)
            r["q_act"] = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_ACT, act=0, out_scale=inv, **kw)
            r["q_act_pre"], r["q_pre"] = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_ACT, act=0, want_pre=True, out_scale=inv, **kw)
            r["q_act_pre8"], r["q_pre8"] = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_ACT, act=0, want_pre="e4m3", out_scale=inv, **kw)
        return r

    loose = ("colsum", "colsum_atol", "emit_dh1")

    def same(what, x, y, skip=()):
        assert set(x) - {"colsum_atol"} == set(y) - {"colsum_atol"}
        for k in y:
            if k not in skip and k != "colsum_atol":
                assert x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]), f"{name} {k}: {what}"

    other = TW.SHAPES["S2" if name == "S1" else "S1"]
    qa2, sa2, qb2, sb2, bias2, _, _ = _f8_tile_operands(*other, 0, seed=5)
    A2, SA2, B2, SB2, BIAS2 = qa2.view(torch.uint8).to(DEV), sa2.to(DEV), qb2.view(torch.uint8).to(DEV), sb2.to(DEV), bias2.to(DEV)
    try:
        h = _debug_set(1, 0)
        lib.gemm_counts(reset=True)
        old = composed(both({}))
        c = lib.gemm_counts()
        assert h.last_gemm() == 7 and c[6] == 0, c
        _debug_set(0, 0)
        lib.gemm_counts(reset=True)
        new = fused(both({}))
        c = lib.gemm_counts()
        # gemm_f8a launches: [6] all, [12] with the e4m3 copy, [13] DACT from e4m3 bytes (the emitting ones included), [14] with a
        # quantised output, [0] emitting; [7] gemm_nt_f8_kernel
        want = (16, 1, 4, 4, 3, 0) if full else (8, 1, 3, 1, 3, 0)
        assert h.last_gemm() == 6 and (c[6], c[12], c[13], c[14], c[0], c[7]) == want, f"{name}: dispatch {c}"
        same("gemm_f8a differs from the launches around gemm_nt_f8_kernel", old, new, skip=loose)
        torch.testing.assert_close(new["colsum"].double(), old["colsum"], rtol=2e-4, atol=old["colsum_atol"])
        bad = new["emit_dh1"] != old["emit_dh1"]      # tanh-GELU: the table's act'(x) and the polynomial epilogue's differ in the last bit for a few codes
        assert float(bad.float().mean()) < 1e-3
        if bool(bad.any()):
            x, y = new["emit_dh1"].float(), old["emit_dh1"].float()
            assert float(((x - y).abs() / y.abs().clamp_min(1e-30))[bad].max()) <= 2 ** -7
        assert torch.equal(new["pre8"], H8)
        same("second launch differs", new, fused(both({})))
        # another shape in between: other tile counts, other descriptors, other vectors left in the LDS window
        o.gemm_nt_f8(A2, SA2, B2, SB2, BIAS2, epi=o.EPI_ACT, act=1, want_pre="e4m3")
        o.gemm_nt_f8(A2, None, B2, None)
        assert h.last_gemm() == 6
        same("differs after a launch of another shape", new, fused(both({})))
    finally:
        _debug_set(0, 0)
    del old, A2, B2

    if name == "S3":
        panels = TW.panels_to_check(w)
        assert len(panels) >= 8
        rows = torch.cat([torch.arange(256 * p, 256 * p + 256) for p in panels])
    else:
        rows = torch.arange(M)
    lin = (_f8_product(qa, sa, qb, sb, rows) * 0.75 + bias.double()).to(DEV)
    rows = rows.to(DEV)
    check_dev("bias", new["bias"][rows], lin, 2 ** -7, 2e-3)
    check_dev("pre", new["pre"][rows], lin, 2 ** -7, 2e-3)
    pre = new["pre"][rows].double()
    for act in (acts if full else ()):
        check_dev(f"act {act}", new[f"act{act}"][rows], ref_act(pre, act), 2 ** -7, 2e-3)
    check_dev("act (with the e4m3 copy)", new["act_pre8"][rows], ref_act(pre, 0), 2 ** -7, 2e-3)


def test_gemm_nt_f8_ragged_shape_past_one_tile_per_workgroup():
    """gemm_nt_f8_kernel, ragged in M, N and K, with 603 tiles: two and three per workgroup.  The epilogues and tolerances of
    test_gemm_nt_f8_epilogues, every element against the fp64 product of the same bytes, tile-dependent scales."""
    o = ops()
    from clipa_amd import lib
    M, N, K = TW.RAGGED_F8
    w = TW.walk(M, N, K, 1, num_cu())
    TW.require_second_tiles(w, f"gemm_nt_f8_kernel {(M, N, K)} on {num_cu()} CUs")
    qa, sa, qb, sb, bias, _, _ = _f8_tile_operands(M, N, K, 0, seed=21)
    A, SA, B, SB, BIAS = qa.view(torch.uint8).to(DEV), sa.to(DEV), qb.view(torch.uint8).to(DEV), sb.to(DEV), bias.to(DEV)
    AUX = torch.randn(M, N, generator=torch.Generator(device=DEV).manual_seed(9), device=DEV, dtype=f32).to(bf16)
    v = (_f8_product(qa, sa, qb, sb) + bias.double()).to(DEV).to(bf16).double()
    aux = AUX.double()
    for act in (0, 1, 2):
        prev = None
        for rep in range(2):                           # the second launch re-uses ring state
            out, pre = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_ACT, act=act, want_pre=True)
            assert lib.last_gemm() == 7
            one = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_ACT, act=act)
            add = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_ADD, aux=AUX)
            dact = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_DACT, act=act, aux=AUX)
            assert torch.equal(out, one), "activation epilogue with / without the pre-activation copy"
            got = (out, pre, add, dact)
            if prev is not None:
                assert all(torch.equal(x, y) for x, y in zip(prev, got)), "second launch differs"
            prev = got
        check_dev("pre-activation", pre, v, 2 ** -7, 2e-3)
        check_dev("act", out, ref_act(pre.double(), act), 2 ** -7, 2e-3)
        if act == 0:
            check_dev("residual add", add, v + aux, 2 ** -6, 2e-2)
        check_dev("act backward", dact, v * act_grad(aux, act), 2 ** -6, 6e-3)


def test_gemm_nt_f8_production_rows():
    """M = 806 912 rows (ViT-L/16 @ 224, local batch 4096): the real launch's buffer offsets on sampled rows."""
    o = ops()
    M, N, K = 806912, 256, 128
    g = torch.Generator().manual_seed(5)
    a = torch.randn(M, K, generator=g).to(bf16)
    b = (torch.randn(N, K, generator=g) * 0.1).to(bf16)
    qa, sa = o.quantize_rows(a.to(DEV))
    qb, sb = o.quantize_rows(b.to(DEV))
    out = o.gemm_nt_f8(qa, sa, qb, sb).cpu()
    rows = torch.cat([torch.arange(0, 300), torch.arange(M - 300, M), torch.randint(0, M, (4000,), generator=g),
                      torch.tensor([2 ** 18 - 1, 2 ** 18, 2 ** 19, 2 ** 19 + 255, 524288 + 131072])])
    e4 = torch.float8_e4m3fn      # reference from the DEVICE-quantised bytes: this test is about the GEMM's addressing
    qa_c, sa_c = qa[rows.to(DEV)].cpu().view(e4), sa[rows.to(DEV)].cpu()
    qb_c, sb_c = qb.cpu().view(e4), sb.cpu()
    ref = (qa_c.double() * sa_c.double()[:, None]) @ (qb_c.double() * sb_c.double()[:, None]).T
    check("sampled rows", out[rows], ref, 2 ** -7, 2e-3)
    assert torch.isfinite(out.float()).all()


def test_fp8_linear_is_close_to_bf16_linear():
    """End-to-end accuracy of the recipe on a layer-sized product: quantise(activation) x quantise(weight) against the bf16
    GEMM of the same operands.  e4m3 carries 3 mantissa bits: ~2.5-3.6 % rms relative rounding error per operand element,
    unbiased, so a dot product of independent terms lands ~4 % (rms) from the bf16 one whatever K is.  Stated bound:
    relative Frobenius error <= 6 %, mean signed error <= 0.5 % of the rms value (no bias)."""
    o = ops()
    M, N, K = 4096, 1024, 1024
    x, w = rnd(M, K, seed=1).to(DEV), rnd(N, K, seed=2, scale=0.03).to(DEV)
    ref = o.gemm_nt(x, w).float()
    qx, sx = o.quantize_rows(x)
    qw, sw = o.quantize_rows(w)
    got = o.gemm_nt_f8(qx, sx, qw, sw).float()
    rel = ((got - ref).norm() / ref.norm()).item()
    bias_rel = ((got - ref).mean() / ref.pow(2).mean().sqrt()).abs().item()
    print(f"fp8 linear: relative Frobenius error {rel:.4f}, relative mean error {bias_rel:.5f}")
    assert rel < 0.06, f"fp8 linear relative error {rel:.4f}"
    assert bias_rel < 0.005, f"fp8 linear is biased: {bias_rel:.5f}"


@pytest.mark.parametrize("D,rows", [(384, 1000), (768, 1000), (1024, 1000), (1280, 1000), (256, 40003),   # 40003 rows: more than one pass of the 8192-block grid
                                    (1408, 1000), (1544, 300), (1792, 300), (2048, 300)])   # ViT-g/14; four chunks per lane: one lane of the last (1544), ViT-e/14, all lanes
def test_layernorm_fwd_q8(D, rows):
    o = ops()
    x = (rnd(rows, D, seed=D, dtype=f32) * 2.0 + 0.3).to(bf16).to(DEV)
    gamma = (1.0 + 0.1 * rnd(D, seed=1, dtype=f32)).to(DEV)
    beta = (0.1 * rnd(D, seed=2, dtype=f32)).to(DEV)
    y_ref = o.layernorm_fwd(x, gamma, beta, 1e-5)
    q_ref, dq_ref = o.quantize_rows(y_ref)
    y, q, dq = o.layernorm_fwd_q8(x, gamma, beta, 1e-5, want_bf16=True)
    assert torch.equal(y, y_ref), "bf16 output differs from the plain LayerNorm kernel"
    assert torch.equal(q, q_ref) and torch.equal(dq, dq_ref), "fused fp8 output differs from quantize_rows(LayerNorm)"
    y2, q2, dq2 = o.layernorm_fwd_q8(x, gamma, beta, 1e-5)
    assert y2 is None and torch.equal(q2, q) and torch.equal(dq2, dq)


# ---- the whole model in fp8 mode --------------------------------------------------------------------------------------------
# Stated tolerance of precision="fp8" against the fp32 reference (golden vectors of the real reference / the fp32 oracle):
#   toy-dimension goldens (1-2 blocks, batch 8):       unit-norm features |err| <= 6e-2, loss <= 4 %, per-tensor gradient
#                                                      cosine >= 0.95, norm within 22 %
#   BASELINE dimensions (12-32 blocks, batch 2-4):     features |err| <= 5e-2, loss <= 3 %, per-tensor gradient cosine >= 0.85
#                                                      (median >= 0.92), norm within 25 %
# e4m3 rounding is ~3 % rms per operand element and unbiased.  That it "averages out over the tokens of a batch" in the per-tensor
# cosines was this comment's claim until it was measured (test_fp8_production_kernels_end_to_end: the same 2-layer model holds a
# median of ~0.990 at 8 and at 128 pairs, the larger batch 0.002 lower): what a 4096-pair batch sees at 12-32 blocks is not
# measured.  The same recipe run through the torch-CPU stand-in ops (tests/test_engine_cpu.py::test_fp8_orchestration) gives
# 0.92-0.95 at batch 2-4.
import clipa_amd  # noqa: E402
from .conftest import load_golden  # noqa: E402


def _fp8_engine(g, recompute=True, grad_fmt="e4m3", predict=False):
    m = clipa_amd.CLIP(**g.cfg, output_dict=True)
    m.load_state_dict(g.sd, strict=True)
    m.to(DEV)
    clipa_amd.convert_weights_to_lp(m, torch.bfloat16)
    for t in (m.visual.transformer, m.transformer):
        t.fp8, t.fp8_grad_format, t.fp8_predicted_scales = True, grad_fmt, predict
    m.set_grad_checkpointing(recompute)
    return m


def _fp8_step(m, g):
    m.zero_grad(set_to_none=True)
    out = m(g.images_u8.to(DEV), g.texts.to(DEV))
    loss = clipa_amd.ClipLoss()(**out, output_dict=True)["contrastive_loss"]
    loss.backward()
    torch.cuda.synchronize()
    return out, loss


def _oracle_grads(g):
    sd = {k: v.clone().requires_grad_(k not in g.frozen) for k, v in g.sd.items()}
    i, t, s = O.clip_forward(sd, g.ocfg, O.normalize_images(g.images_u8), g.texts)
    loss, _ = O.clip_loss(i, t, s)
    loss.backward()
    return {k: v.grad for k, v in sd.items() if v.grad is not None}


def _check_fp8_model(g, feat_tol, loss_tol, cos_min, cos_median, norm_tol, predict=False):
    m = _fp8_engine(g, predict=predict)
    out, loss = _fp8_step(m, g)
    i, t = out["image_features"].float().cpu(), out["text_features"].float().cpu()
    fi, ft = (i - g.t("image_features")).abs().max().item(), (t - g.t("text_features")).abs().max().item()
    lrel = abs(float(loss) - float(g.t("loss"))) / float(g.t("loss"))
    ref = _oracle_grads(g)
    coss, ratios = [], []
    for k, p in m.named_parameters():
        if p.grad is None or p.grad.numel() == 1:
            continue
        a, b = p.grad.double().cpu().reshape(-1), ref[k].double().reshape(-1)
        assert torch.isfinite(a).all(), k
        if float(b.norm()) < 1e-7:
            continue
        coss.append((float(torch.dot(a, b) / (a.norm() * b.norm())), k))
        ratios.append(float(a.norm() / b.norm()))
        if abs(ratios[-1] - 1.0) > 0.15:
            print(f"[fp8 {g.name}] norm ratio {ratios[-1]:.3f} cosine {coss[-1][0]:.4f} |ref| {float(b.norm()):.3e}: {k}")
    coss.sort()
    med = coss[len(coss) // 2][0]
    print(f"[fp8{' predicted scales' if predict else ''} {g.name}] feature err {fi:.4f} / {ft:.4f}, loss rel {lrel:.4f}, gradient cosine min {coss[0][0]:.4f} "
          f"({coss[0][1]}) median {med:.4f}, norm ratio {min(ratios):.3f}..{max(ratios):.3f}")
    assert fi < feat_tol and ft < feat_tol
    assert lrel < loss_tol
    assert coss[0][0] > cos_min, coss[0]
    assert med > cos_median
    assert max(abs(r - 1.0) for r in ratios) < norm_tol


def test_fp8_model_matches_reference_golden(golden):
    _check_fp8_model(golden, 6e-2, 0.04, 0.95, 0.97, 0.22)


def test_fp8_full_dims_match_reference_golden(golden_full):
    """fp8 block GEMMs at the BASELINE configurations' dimensions against the fp32 reference fixtures.  Tolerances follow what
    the five cases measure on an MI355X (profiles/r03_pytest_gpu_*.log: feature error <= 0.030, loss <= 1.3 %, per-tensor
    gradient cosine min 0.902..0.926 - always a LayerNorm gain or bias of the text tower - median 0.947..0.954, norm ratio
    0.81..1.15), with a margin; what that accuracy means for training is the convergence A/B of
    profiles/r03_fp8_convergence_S16_112.jsonl."""
    _check_fp8_model(golden_full, 4e-2, 0.02, 0.89, 0.94, 0.22)


def test_fp8_predicted_row_scales_full_dims(golden_full):
    """The engine knob fp8_predicted_scales (round 6; off by default): the MLP's 4 D-wide tensors leave their GEMMs as e4m3 operands with
    Cauchy-Schwarz row scales.  Measured against the fp32 reference fixtures (profiles/r06_pytest_fp8_parity.log): gradient cosine min
    0.898-0.927 (0.901-0.931 with the rows' true maxima), median 0.944-0.952 (0.947-0.954); the vectors that are sums over the batch of
    the pooled rows' gradients (last blocks' biases, the heads' LayerNorm bias) move by up to 30 % in norm at these batches of 2-4."""
    _check_fp8_model(golden_full, 4e-2, 0.02, 0.88, 0.935, 0.33, predict=True)


def test_fp8_predicted_row_scales_tiers_are_bit_identical():
    g = load_golden("cls_erf")
    ga = {}
    for rc in (True, False, "mixed"):
        m = _fp8_engine(g, recompute=bool(rc), predict=True)
        if rc == "mixed":
            for t in (m.visual.transformer, m.transformer):
                t.keep_blocks, t.medium_blocks = 1, 1
        _, loss = _fp8_step(m, g)
        ga[rc] = (float(loss), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    assert ga[True][0] == ga[False][0] == ga["mixed"][0]
    for k in ga[True][1]:
        assert torch.equal(ga[True][1][k], ga[False][1][k]), k
        assert torch.equal(ga[True][1][k], ga["mixed"][1][k]), k


def test_fp8_recompute_equals_stored_activations():
    """Row scales come from the data itself, so a block's backward-time recompute reproduces its forward bit for bit in
    fp8 mode too: all-recompute, all-stored and the light / medium keep tiers give identical losses and gradients."""
    g = load_golden("cls_erf")
    ga = {}
    for rc in (True, False, "mixed"):
        m = _fp8_engine(g, recompute=bool(rc))
        if rc == "mixed":
            for t in (m.visual.transformer, m.transformer):
                t.keep_blocks, t.medium_blocks = 1, 1
        _, loss = _fp8_step(m, g)
        ga[rc] = (float(loss), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    assert ga[True][0] == ga[False][0] == ga["mixed"][0]
    for k in ga[True][1]:
        assert torch.equal(ga[True][1][k], ga[False][1][k]), k
        assert torch.equal(ga[True][1][k], ga["mixed"][1][k]), k


def test_fp8_e5m2_gradient_operand_and_factory():
    """create_model(precision='fp8') switches both towers; the e5m2 gradient-operand variant trains the same model."""
    g = load_golden("cls_erf")
    m = _fp8_engine(g, grad_fmt="e5m2")
    _, loss = _fp8_step(m, g)
    assert abs(float(loss) - float(g.t("loss"))) < 0.04 * float(g.t("loss"))
    assert all(torch.isfinite(p.grad.float()).all() for p in m.parameters() if p.grad is not None)
    m2 = clipa_amd.create_model("ViT-S-16", precision="fp8", device=DEV) if "ViT-S-16" in clipa_amd.list_models() else None
    if m2 is not None:
        assert m2.visual.transformer.fp8 and m2.transformer.fp8
        assert m2.visual.transformer.resblocks[0].mlp.c_fc.weight.dtype == torch.bfloat16


# ---- fp8 weight gradients (round 6: clipa_gemm_tn_f8 and the operands it takes) ---------------------------------------------
def _tn8_operands(M, R, C, fmt_p, seed):
    """Random fp8 bytes of both operands (every finite code, asymmetric) + their fp64 product."""
    dt_p = F8[fmt_p][0]
    p = (rnd(M, R, seed=seed, dtype=f32) * torch.exp(rnd(M, 1, seed=seed + 1, dtype=f32))).to(dt_p)
    q = (rnd(M, C, seed=seed + 2, dtype=f32) * 3.0 + 0.25).to(torch.float8_e4m3fn)
    ref = p.double().T @ q.double()
    return p.view(torch.uint8), q.view(torch.uint8), ref


@pytest.mark.parametrize("M,R,C", [(128, 16, 16), (300, 72, 40), (1000, 264, 136), (515, 768, 256), (1028, 1280, 256)])
def test_gemm_tn_f8_generic_shapes(M, R, C):
    """Any shape runs on the byte-gather kernel: every element against the fp64 product of the same bytes (fp32 accumulation
    is the only difference), transposition-detecting (R != C, asymmetric data)."""
    o = ops()
    p8, q8, ref = _tn8_operands(M, R, C, 0, seed=M + R)
    out = o.gemm_tn_f8(p8.to(DEV), q8.to(DEV))
    check("tn f8 generic", out, ref, 1e-3, ref.abs().max().item() * 3e-4)     # the matrix pipe sums a 128-term dot product with aligned, truncated addends
    t = torch.tensor([0.375], device=DEV)
    outb = o.gemm_tn_f8(p8.to(DEV), q8.to(DEV), t=t, alpha=2.0, out_dtype=bf16)
    check("tn f8 generic, alpha x t, bf16", outb, ref * 0.75, 2 ** -7, ref.abs().max().item() * 2e-3)


@pytest.mark.parametrize("fmt_p", [0, 1])
@pytest.mark.parametrize("M,R,C", [(512, 256, 256), (1024, 512, 256), (4096 + 768, 256, 768), (8192 + 300, 768, 256),
                                    (65536, 1280, 256)])
def test_gemm_tn_f8_whole_tiles(M, R, C, fmt_p):
    """Whole 256 x 256 tiles: the four-wave kernel (tools/gen_gemm_tn8.py) on the sliceable rows + the byte-gather kernel on the
    remainder - bit-identical to the byte-gather kernel alone per slab order is not required (different split), so both are held
    to the fp64 product; every schedule of the generator must agree BIT FOR BIT with the default (same MFMA order per slab)."""
    o = ops()
    from clipa_amd import lib
    p8, q8, ref = _tn8_operands(M, R, C, fmt_p, seed=7 * M + R + fmt_p)
    P, Q = p8.to(DEV), q8.to(DEV)
    tol = ref.abs().max().item() * 3e-4
    out = o.gemm_tn_f8(P, Q, fmt_p=fmt_p)
    assert lib.last_gemm() == 8, "the four-wave kernel did not run"
    check("tn f8 four-wave", out, ref, 1e-3, tol)
    again = o.gemm_tn_f8(P, Q, fmt_p=fmt_p)
    assert torch.equal(out, again), "second launch differs"
    try:
        for sel in (1, 2, 3):                                   # schedules 0, 1, 2 (flag bits 26..27)
            _debug_set(0, sel << 26)
            alt = o.gemm_tn_f8(P, Q, fmt_p=fmt_p)
            check(f"tn f8 schedule {sel - 1}", alt, ref, 1e-3, tol)
    finally:
        _debug_set(0, 0)


def test_rowscale_max_and_scaled_quantisers():
    """The activation operand of an fp8 weight gradient: q = e4m3(act(x) * rowscale / t) with t = max(rowscale * sx) - against
    torch's own cast of the same fp32 expression (ties may flip on the scale rounding), never saturating, zero t -> zeros."""
    o = ops()
    M, K = 777, 1280
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))).to(bf16)
    ds = torch.exp(torch.randn(M, generator=g) * 2.0).float()
    sx = x.float().abs().amax(1) / 448.0
    t = o.rowscale_max(ds.to(DEV), sx.to(DEV))
    assert t.shape == (1,) and abs(t.item() - (ds * sx).max().item()) <= 1e-6 * t.item()
    assert o.rowscale_max(ds.to(DEV)).item() == ds.max().item()
    q = o.scale_quantize_rows(x.to(DEV), ds.to(DEV), t)
    want = (x.float() * (ds * (1.0 / t.cpu()))[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    got = q.cpu().view(torch.float8_e4m3fn).float()
    assert torch.isfinite(got).all() and got.abs().max().item() <= 448.0
    assert (q.cpu() == want.view(torch.uint8)).float().mean().item() > 0.999
    assert got.abs().max().item() >= 416.0, "the largest scaled element must land in the top binade"
    # the activation variant: gelu(x) rounded to bf16 first (what the forward GEMM's epilogue stored)
    for act, name in ((0, "gelu_erf"), (1, "gelu_tanh"), (2, "quick_gelu")):
        qa = o.scale_quantize_rows(x.to(DEV), ds.to(DEV), t, act=act)
        gx = O.activation(x.double(), name).to(bf16).float()
        wa = (gx * (ds * (1.0 / t.cpu()))[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
        d = (qa.cpu().view(torch.float8_e4m3fn).float() - wa.float()).abs()
        assert (d <= 0.0726 * wa.float().abs() + 2 ** -9 + 1e-3 * 448).all(), name        # one e4m3 step (polynomial GELU, bf16 ties)
    zero = torch.zeros(1, device=DEV)
    assert (o.scale_quantize_rows(x.to(DEV), ds.to(DEV), zero).view(torch.float8_e4m3fn).float() == 0).all()
    # LayerNorm variant == LayerNorm (bf16) followed by the plain scaled quantiser, bit for bit
    gam, bet = rnd(K, seed=1, dtype=f32).to(DEV) + 1.0, rnd(K, seed=2, dtype=f32).to(DEV)
    y = o.layernorm_fwd(x.to(DEV), gam, bet, 1e-5)
    sy = y.float().abs().amax(1) / 448.0
    ty = o.rowscale_max(ds.to(DEV), sy)
    assert torch.equal(o.layernorm_fwd_q8s(x.to(DEV), gam, bet, ds.to(DEV), ty, 1e-5), o.scale_quantize_rows(y, ds.to(DEV), ty))


@pytest.mark.parametrize("D", [1544, 1792])
def test_layernorm_quantisers_four_chunks_per_lane(D):
    """Rows of 1544 - 2048 elements (ViT-bigG/14 1664, ViT-e/14 1792) take the NCH = 4 instantiations of ln_fwd_q8s_kernel and
    ln_fwd_q8_kernel (1544: one lane active in the last chunk).  The equalities the narrower rows are held to above: the
    scaled LayerNorm quantiser == LayerNorm (bf16) + the plain scaled quantiser, bit for bit; the row-norm form returns the same
    y, q, dq as the plain one and ||y||_2 as tests/cpu_ops.layernorm_fwd_q8 states it (test_row_bound_helpers' tolerance)."""
    o = ops()
    M = 300
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(M, D, generator=g) * torch.exp(torch.randn(M, 1, generator=g))).to(bf16).to(DEV)
    ds = torch.exp(torch.randn(M, generator=g) * 2.0).float().to(DEV)
    gam, bet = rnd(D, seed=1, dtype=f32).to(DEV) + 1.0, rnd(D, seed=2, dtype=f32).to(DEV)
    y = o.layernorm_fwd(x, gam, bet, 1e-5)
    ty = o.rowscale_max(ds, y.float().abs().amax(1) / 448.0)
    assert torch.equal(o.layernorm_fwd_q8s(x, gam, bet, ds, ty, 1e-5), o.scale_quantize_rows(y, ds, ty))
    y2, q2, dq2 = o.layernorm_fwd_q8(x, gam, bet, 1e-5, want_bf16=True)
    y3, q3, dq3, rn = o.layernorm_fwd_q8(x, gam, bet, 1e-5, want_bf16=True, want_rownorm=True)
    assert torch.equal(y2, y) and torch.equal(y3, y) and torch.equal(q3, q2) and torch.equal(dq3, dq2)
    torch.testing.assert_close(rn.cpu(), y.float().norm(dim=1).cpu(), rtol=1e-5, atol=1e-6)
    _, q4, dq4, rn4 = o.layernorm_fwd_q8(x, gam, bet, 1e-5, want_rownorm=True)
    assert torch.equal(q4, q2) and torch.equal(dq4, dq2) and torch.equal(rn4, rn)


def test_fp8_weight_gradient_recipe_is_close_to_bf16():
    """dW = dY^T X through the recipe of engine._wgrad8 (row-quantised gradient, activation absorbing the row scale, one tensor
    scale) against the fp64 product of the bf16 operands: e4m3 rounding is ~3 % rms per element and averages out over the tokens."""
    o = ops()
    M, R, C = 4096, 512, 256
    g = torch.Generator().manual_seed(9)
    dy = (torch.randn(M, R, generator=g) * torch.exp(torch.randn(M, 1, generator=g) * 1.5) * 1e-3).to(bf16)
    x = (torch.randn(M, C, generator=g) * torch.exp(torch.randn(1, C, generator=g) * 0.5)).to(bf16)
    ref = dy.double().T @ x.double()
    for fmt in (0, 1):
        dq, ds = o.quantize_rows(dy.to(DEV), fmt)
        _, sx = o.quantize_rows(x.to(DEV))
        t = o.rowscale_max(ds, sx)
        x8 = o.scale_quantize_rows(x.to(DEV), ds, t)
        dw = o.gemm_tn_f8(dq, x8, t=t, fmt_p=fmt).double().cpu()
        rel = ((dw - ref).norm() / ref.norm()).item()
        cos = torch.nn.functional.cosine_similarity(dw.flatten(), ref.flatten(), dim=0).item()
        assert rel < (0.06 if fmt == 0 else 0.10) and cos > 0.995, (fmt, rel, cos)
        assert abs((dw - ref).mean().item()) < 1e-3 * ref.abs().mean().item() + 1e-9 or rel < 0.05


def test_gemm_f8a_e4m3_preactivation_epilogues():
    """CLIPA_EPI_ACT_PRE8 / CLIPA_EPI_DACT8 of the four-wave fp8 GEMM (round 6: the "h8" kept tensor in fp8 mode): the fused
    e4m3 copy is the cast of the bf16 pre-activation, the activation output is untouched, and the GELU-backward epilogue reading
    the bytes equals the one reading their bf16 decoding - all bit for bit; ragged shapes compose GEMM + cast."""
    o = ops()
    from clipa_amd import lib
    for act in (0, 1, 2):
        M, N, K = 512, 768, 512
        qa, sa, qb, sb, _ = _f8_operands(M, N, K, 0, 0, seed=31 + act)
        bias = rnd(N, seed=4, dtype=f32)
        A, SA, B, SB, BIAS = qa.to(DEV), sa.to(DEV), qb.to(DEV), sb.to(DEV), bias.to(DEV)
        g_ref, pre = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_ACT, act=act, want_pre=True)
        g8, pre8 = o.gemm_nt_f8(A, SA, B, SB, BIAS, epi=o.EPI_ACT, act=act, want_pre="e4m3")
        assert lib.last_gemm() == 6
        assert pre8.dtype == torch.uint8 and torch.equal(g8, g_ref)
        assert torch.equal(pre8, o.cast_e4m3(pre))
        dy8, sdy = o.quantize_rows(rnd(M, K, seed=9).to(DEV))
        w8, sw = o.quantize_rows(rnd(N, K, seed=10, scale=0.05).to(DEV))
        d8 = o.gemm_nt_f8(dy8, sdy, w8, sw, epi=o.EPI_DACT, act=act, aux=pre8)
        d16 = o.gemm_nt_f8(dy8, sdy, w8, sw, epi=o.EPI_DACT, act=act, aux=o.e4m3_to_bf16(pre8))
        assert torch.equal(d8, d16)
    # ragged: same values through GEMM + cast
    qa, sa, qb, sb, _ = _f8_operands(300, 264, 272, 0, 0, seed=77)
    A, SA, B, SB = qa.to(DEV), sa.to(DEV), qb.to(DEV), sb.to(DEV)
    g_ref, pre = o.gemm_nt_f8(A, SA, B, SB, epi=o.EPI_ACT, want_pre=True)
    g8, pre8 = o.gemm_nt_f8(A, SA, B, SB, epi=o.EPI_ACT, want_pre="e4m3")
    assert torch.equal(g8, g_ref) and torch.equal(pre8, o.cast_e4m3(pre))
    dy8, sdy = o.quantize_rows(rnd(300, 288, seed=9).to(DEV))
    w8, sw = o.quantize_rows(rnd(272, 288, seed=10, scale=0.05).to(DEV))
    pre8b = o.cast_e4m3(rnd(300, 272, seed=12).to(DEV))
    assert torch.equal(o.gemm_nt_f8(dy8, sdy, w8, sw, epi=o.EPI_DACT, aux=pre8b),
                       o.gemm_nt_f8(dy8, sdy, w8, sw, epi=o.EPI_DACT, aux=o.e4m3_to_bf16(pre8b)))


@pytest.mark.parametrize("name", ["cls_erf", "gap_sincos_tanh"])
def test_fp8_per_tensor_keep_sets(name):
    """bench.py's planner keeps a block's tensors one by one in fp8 mode too (round 6): any subset of the exact tensors (qkv,
    attention output, x1, bf16 pre-activation) reproduces the all-recompute step bit for bit; with the e4m3 pre-activation
    forward and loss stay bit-identical and the gradients stay within the tier's tolerance of the recomputed step."""
    g = load_golden(name)
    m = _fp8_engine(g)
    _, loss0 = _fp8_step(m, g)
    ref = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    for counts in ({"qkv": 2, "a": 1, "x1": 0, "h": 0, "h8": 0}, {"qkv": 0, "a": 2, "x1": 2, "h": 1, "h8": 0},
                   {"qkv": 1, "a": 0, "x1": 1, "h": 2, "h8": 0}):
        for t in (m.visual.transformer, m.transformer):
            t.keep_counts = dict(counts)
        _, loss = _fp8_step(m, g)
        assert float(loss) == float(loss0), counts
        for k, p in m.named_parameters():
            if p.grad is not None:
                assert torch.equal(p.grad, ref[k]), (counts, k)
    for t in (m.visual.transformer, m.transformer):
        t.keep_counts = {"qkv": 1, "a": 2, "x1": 2, "h": 0, "h8": 2}
    _, loss = _fp8_step(m, g)
    assert float(loss) == float(loss0)
    worst = 1.0
    for k, p in m.named_parameters():
        if p.grad is None or p.grad.numel() == 1 or float(ref[k].float().norm()) < 1e-7:
            continue
        a, b = p.grad.double().reshape(-1), ref[k].double().reshape(-1)
        worst = min(worst, float(torch.dot(a, b) / (a.norm() * b.norm())))
    print(f"[fp8 h8 tier, {name}] worst gradient cosine against the recomputed step {worst:.4f}")
    assert worst > 0.99


# ---- producer-fused quantisation with predicted row scales (round 6) --------------------------------------------------------
def test_row_bound_helpers():
    """rownorm_max / absmax / row_bound and the row norms the quantising kernels return: plain fp32 arithmetic against torch."""
    o = ops()
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(520, 1280, generator=g) * 0.03).to(bf16)
    b = torch.randn(520, generator=g)
    assert abs(o.rownorm_max(w.to(DEV)).item() - w.float().norm(dim=1).max().item()) < 1e-5 * w.float().norm(dim=1).max().item()
    assert o.absmax(b.to(DEV)).item() == b.abs().max().item()
    x = (torch.randn(300, 1280, generator=g) * torch.exp(torch.randn(300, 1, generator=g))).to(bf16)
    x[7] = 0
    q, dq, cs, rn = o.quantize_rows(x.to(DEV), want_colsum=True, want_rownorm=True)
    torch.testing.assert_close(rn.cpu(), x.float().norm(dim=1), rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(cs.cpu(), x.float().sum(0), rtol=1e-4, atol=1e-3)
    q2, dq2 = o.quantize_rows(x.to(DEV))
    assert torch.equal(q, q2) and torch.equal(dq, dq2)
    gam, bet = rnd(1280, seed=1, dtype=f32).to(DEV) + 1.0, rnd(1280, seed=2, dtype=f32).to(DEV)
    y, qy, sy, rny = o.layernorm_fwd_q8(x.to(DEV), gam, bet, want_bf16=True, want_rownorm=True)
    torch.testing.assert_close(rny.cpu(), y.float().norm(dim=1).cpu(), rtol=1e-5, atol=1e-6)
    wn, bm = o.rownorm_max(w.to(DEV)), o.absmax(b.to(DEV))
    sc, inv = o.row_bound(rn, wn, bm, 1.13)
    bound = 1.13 * x.float().norm(dim=1) * wn.item() + bm.item()
    torch.testing.assert_close(sc.cpu(), bound / 448.0, rtol=1e-5, atol=0)
    torch.testing.assert_close(inv.cpu(), 448.0 / bound, rtol=1e-5, atol=0)
    sc0, inv0 = o.row_bound(rn, wn, None, 1.0)
    assert sc0[7].item() == 0.0 and inv0[7].item() == 0.0             # a zero row: zero scale, zero multiplier


@pytest.mark.parametrize("act", [0, 2])
def test_gemm_f8a_producer_quantised_outputs(act):
    """clipa_gemm_nt_f8q: the epilogue writing the next GEMM's e4m3 operand with a caller-predicted row scale is bit-identical to the
    GEMM followed by the scaled quantiser (activation, with and without either pre-activation copy; GELU-backward from e4m3 bytes);
    the fused column sums are the sums of the bf16-rounded outputs; the Cauchy-Schwarz scale never saturates and the de-quantised
    bytes are the bf16 outputs to e4m3 precision."""
    o = ops()
    from clipa_amd import lib
    M, N, K = 768, 1024, 512
    x = rnd(M, K, seed=41) * torch.exp(rnd(M, 1, seed=42, dtype=f32) * 0.5)
    w = rnd(N, K, seed=43, scale=0.04)
    bias = rnd(N, seed=44, dtype=f32) * 0.1
    X, W, BIAS = x.to(bf16).to(DEV), w.to(bf16).to(DEV), bias.to(DEV)
    xq, xs, _, rn = o.quantize_rows(X, want_colsum=True, want_rownorm=True)
    wq, ws = o.quantize_rows(W)
    sc, inv = o.row_bound(rn, o.rownorm_max(W), o.absmax(BIAS), 1.13)
    one = torch.ones(1, device=DEV)
    for want_pre in (False, True, "e4m3"):
        lib.gemm_counts(reset=True)
        r = o.gemm_nt_f8(xq, xs, wq, ws, BIAS, epi=o.EPI_ACT, act=act, want_pre=want_pre, out_scale=inv)
        assert lib.gemm_counts()[14] == 1, "the producer-quantised epilogue did not run"
        ref = o.gemm_nt_f8(xq, xs, wq, ws, BIAS, epi=o.EPI_ACT, act=act, want_pre=want_pre)
        (q8, pre), (out, pre_ref) = (r if want_pre else (r, None)), (ref if want_pre else (ref, None))
        assert torch.equal(q8, o.scale_quantize_rows(out, inv, one)), want_pre
        if want_pre:
            assert torch.equal(pre, pre_ref)
        deq = q8.view(torch.float8_e4m3fn).float() * sc[:, None]
        assert q8.view(torch.float8_e4m3fn).float().abs().max().item() < 448.0, "the predicted scale saturated"
        err = (deq - out.float()).abs()
        assert (err <= 2.0 ** -4 * out.float().abs() + sc[:, None] * 2.0 ** -9).all()
    # GELU-backward from the e4m3 pre-activation, gradient rows of very different size, + column sums
    _, pre8 = o.gemm_nt_f8(xq, xs, wq, ws, BIAS, epi=o.EPI_ACT, act=act, want_pre="e4m3")
    dy = (rnd(M, 256, seed=45) * torch.exp(rnd(M, 1, seed=46, dtype=f32) * 2.0) * 1e-3).to(bf16).to(DEV)
    dy[5] = 0
    wt = rnd(N, 256, seed=47, scale=0.04).to(bf16).to(DEV)
    dq, ds, _, rnd_y = o.quantize_rows(dy, want_colsum=True, want_rownorm=True)
    wtq, wts = o.quantize_rows(wt)
    sdh, sodh = o.row_bound(rnd_y, o.rownorm_max(wt), None, 1.13 * 1.13)
    # K = 256 is below the four-wave kernel's minimum: pad the reduction to 512 with zeros (same product)
    pad = lambda t: torch.cat([t, torch.zeros_like(t)], dim=1).contiguous()
    lib.gemm_counts(reset=True)
    q8, cs = o.gemm_nt_f8(pad(dq), ds, pad(wtq), wts, epi=o.EPI_DACT, act=act, aux=pre8, out_scale=sodh, want_colsum=True)
    assert lib.gemm_counts()[14] == 1
    dh = o.gemm_nt_f8(pad(dq), ds, pad(wtq), wts, epi=o.EPI_DACT, act=act, aux=pre8)
    assert torch.equal(q8, o.scale_quantize_rows(dh, sodh, one))
    torch.testing.assert_close(cs, dh.float().sum(0), rtol=2e-4, atol=1e-6 * dh.float().abs().sum(0).max().item())
    assert (q8[5].view(torch.float8_e4m3fn).float() == 0).all() and q8.view(torch.float8_e4m3fn).float().abs().max().item() < 448.0
    # ragged shapes compose GEMM + scaled quantiser (+ column sums) with the same arithmetic
    xr = rnd(300, 272, seed=48).to(bf16).to(DEV)
    wr = rnd(264, 272, seed=49, scale=0.05).to(bf16).to(DEV)
    xrq, xrs, _, rnr = o.quantize_rows(xr, want_colsum=True, want_rownorm=True)
    wrq, wrs = o.quantize_rows(wr)
    scr, invr = o.row_bound(rnr, o.rownorm_max(wr), None, 1.13)
    qr = o.gemm_nt_f8(xrq, xrs, wrq, wrs, epi=o.EPI_ACT, act=act, out_scale=invr)
    assert torch.equal(qr, o.scale_quantize_rows(o.gemm_nt_f8(xrq, xrs, wrq, wrs, epi=o.EPI_ACT, act=act), invr, one))


@pytest.mark.parametrize("rows,D,fmt", [(1000, 1280, 0), (4099, 1024, 0), (777, 768, 1), (300, 384, 0), (2048, 2048, 1),
                                          (300, 1544, 0), (513, 1792, 1)])      # four chunks per lane with a ragged last one
def test_layernorm_bwd_with_quantised_output(rows, D, fmt):
    """ops.layernorm_bwd(q8_fmt=...) (clipa_layernorm_bwd_q8, round 6: the LayerNorm backward that hands the next linear layer its
    fp8 gradient operand): dx, dgamma, dbeta (and the emitted LayerNorm output) bit for bit those of the plain backward; q and
    the row scales bit for bit clipa_quantize_rows of that dx; column sums and row norms equal to the quantiser's up to the order
    of fp32 additions.  An all-zero gradient row (a padding token) gets scale 0 and zero bytes."""
    o = ops()
    g = torch.Generator().manual_seed(rows + D)
    x = (torch.randn(rows, D, generator=g) * 2 + 0.3).to(bf16).to(DEV)
    dy = (torch.randn(rows, D, generator=g) * 1e-2 * torch.exp(torch.randn(rows, 1, generator=g))).to(bf16).to(DEV)
    dres = (torch.randn(rows, D, generator=g) * 1e-2).to(bf16).to(DEV)
    x[5] = 0.0
    dy[5] = 0.0
    dres[5] = 0.0
    gam = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV)
    bet = (0.1 * torch.randn(D, generator=g)).to(DEV)
    for with_res in (True, False):
        for with_y in (False, True):
            ref = o.layernorm_bwd(x, gam, dy, dres=dres if with_res else None, beta=bet if with_y else None)
            got = o.layernorm_bwd(x, gam, dy, dres=dres if with_res else None, beta=bet if with_y else None, q8_fmt=fmt, want_rownorm=True)
            assert len(got) == len(ref) + 1
            for a, b in zip(ref, got[:-1]):
                assert torch.equal(a, b)
            q, dq, cs, rn = got[-1]
            q_ref, dq_ref, cs_ref, rn_ref = o.quantize_rows(ref[0], fmt, want_colsum=True, want_rownorm=True)
            assert torch.equal(q, q_ref) and torch.equal(dq, dq_ref)
            assert float(dq[5]) == 0.0 and int(q[5].to(torch.int32).abs().sum() & 0x7f) == 0
            want = ref[0].double().sum(0)
            scale = float(ref[0].double().abs().sum(0).max())
            assert float((cs.double() - want).abs().max()) <= 1e-5 * scale
            assert float((cs - cs_ref).abs().max()) <= 1e-5 * scale
            assert torch.allclose(rn, rn_ref, rtol=1e-5, atol=1e-12)
            again = o.layernorm_bwd(x, gam, dy, dres=dres if with_res else None, beta=bet if with_y else None, q8_fmt=fmt, want_rownorm=True)[-1]
            assert all(torch.equal(a, b) for a, b in zip(got[-1], again))      # fixed-order reductions


def test_fp8_block_chain_takes_the_operand_from_the_tower_handoff():
    """Two fp8 blocks in a row: the second block's LayerNorm-1 backward offers its dx as fp8 operand (engine.GradHandoff), the first
    block's backward takes it instead of launching the row quantiser - same gradients as with the hand-off disabled (the bytes
    and scales are identical; the bias gradient of c_proj differs by the order of fp32 additions only)."""
    from clipa_amd import engine
    torch.manual_seed(3)
    from clipa_amd.model import Transformer
    t = Transformer(256, 3, 4, mlp_ratio=4.0).to(DEV)
    t.fp8 = True
    cache = engine.WeightCache()
    B, L = 8, 32
    x0 = torch.randn(B * L, 256, device=DEV).to(bf16)

    def run(handoff):
        taken = []
        real_take, real_offer = engine.GradHandoff.take, engine.GradHandoff.offer
        engine.GradHandoff.take = lambda self, dy, fmt: (lambda r: (taken.append(r is not None), r)[1])(real_take(self, dy, fmt) if handoff else None)
        engine.GradHandoff.offer = real_offer if handoff else (lambda *a: None)
        try:
            for p in t.parameters():
                p.grad = None
            x = x0.clone().requires_grad_(True)
            y = t.run(x, B, L, False, cache)
            (y.float() * torch.linspace(-1, 1, y.numel(), device=DEV).reshape(y.shape)).sum().backward()
            return taken, x.grad.clone(), {n: p.grad.clone() for n, p in t.named_parameters()}
        finally:
            engine.GradHandoff.take, engine.GradHandoff.offer = real_take, real_offer
    taken, gx, grads = run(True)
    assert taken == [False, True, True], taken          # last block: nothing offered yet; blocks 1 and 0 start from the offer
    taken0, gx0, grads0 = run(False)
    assert taken0 == [False, False, False]
    assert torch.equal(gx, gx0)
    for n in grads:
        if n.endswith("mlp.c_proj.bias"):
            assert torch.allclose(grads[n].float(), grads0[n].float(), rtol=2e-2, atol=1e-6), n
        else:
            assert torch.equal(grads[n], grads0[n]), n


@pytest.mark.parametrize("M,N,K,fmt", [(512, 768, 512, 0), (768, 512, 1024, 1), (300, 520, 272, 0)])
def test_gemm_nt_f8_emit_matches_the_two_launches(M, N, K, fmt):
    """ops.gemm_nt_f8_emit (clipa_gemm_nt_f8_emit, round 6: gemm_f8a<DACT, PRE = 3, AUX8>): the GELU-backward input-gradient product
    from the kept e4m3 pre-activation that also emits the activation operand of the layer's fp8 weight gradient.  Both outputs bit
    for bit those of the two launches it replaces (gemm_nt_f8 with EPI_DACT on the bytes, scale_quantize_rows on the bytes), for the
    three activations, both gradient formats, every finite e4m3 code, a zero-scale row; the third shape is ragged (composed path)."""
    o = ops()
    from clipa_amd import lib as _lib
    g = torch.Generator().manual_seed(M + N + K)
    dy = (torch.randn(M, K, generator=g) * 1e-2 * torch.exp(torch.randn(M, 1, generator=g))).to(bf16).to(DEV)
    dy[3] = 0.0
    w = (torch.randn(N, K, generator=g) * 0.05).to(bf16).to(DEV)
    h8 = o.cast_e4m3((torch.randn(M, N, generator=g) * 2.0).to(bf16).to(DEV))
    codes = torch.arange(256, dtype=torch.uint8)
    codes = codes[(codes & 0x7f) != 0x7f]
    h8[0, :codes.numel()] = codes.to(DEV)
    sg = (torch.rand(M, generator=g) * 0.02 + 1e-3).to(DEV)
    dq, ds = o.quantize_rows(dy, fmt)
    wq, ws = o.quantize_rows(w)
    t = o.rowscale_max(ds, sg)
    whole = M % 256 == 0 and N % 256 == 0 and K % 256 == 0 and K >= 512
    for act in (0, 1, 2):
        _lib.gemm_counts(reset=True)
        dh, x8 = o.gemm_nt_f8_emit(dq, ds, wq, ws, h8, t, act=act, fmt_a=fmt)
        assert _lib.gemm_counts()[0] == (1 if whole else 0)
        ref = o.gemm_nt_f8(dq, ds, wq, ws, None, epi=o.EPI_DACT, act=act, aux=h8, fmt_a=fmt)
        if act == 1 and whole:
            # tanh-GELU: the table's act'(x) and the polynomial epilogue's differ in the last bit for a few codes (hipcc contracts the
            # two inlined copies differently): < 0.1 % of the products land on the neighbouring bf16 value
            bad = dh != ref
            assert float(bad.float().mean()) < 1e-3
            assert float(((dh.float() - ref.float()).abs() / ref.float().abs().clamp_min(1e-30))[bad].max() if bad.any() else 0.0) <= 2 ** -7
        else:
            assert torch.equal(dh, ref), act
        assert torch.equal(x8, o.scale_quantize_rows(h8, ds, t, act=act)), act
        assert int(x8[3].to(torch.int32).bitwise_and(0x7f).sum()) == 0                # zero gradient row: zero scale, zero bytes
        dh2, x82 = o.gemm_nt_f8_emit(dq, ds, wq, ws, h8, t, act=act, fmt_a=fmt)
        assert torch.equal(dh, dh2) and torch.equal(x8, x82)
    # a tensor scale of zero (every gradient row zero): zero bytes, as the unfused emission
    z = torch.zeros(1, device=DEV)
    _, xz = o.gemm_nt_f8_emit(dq, ds, wq, ws, h8, z, act=0, fmt_a=fmt)
    assert torch.equal(xz, o.scale_quantize_rows(h8, ds, z, act=0))


# ---- fp8 through the model with the production kernels dispatched -----------------------------------------------------------
def _fp8_parity_figures(m, out, loss, sd, cfg, images, texts):
    """Features, loss and every parameter gradient of one fp8 step against the fp32 oracle on the same weights and batch.
    -> dict of figures; the vectors that are plain sums over the batch of the pooled rows' gradients (the split of
    test_model_gpu.py::test_production_kernels_end_to_end) are reported apart from the other tensors."""
    osd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    fi, ft, s = O.clip_forward(osd, O.oracle_cfg(cfg), O.normalize_images(images), texts)
    lf, _ = O.clip_loss(fi, ft, s)
    lf.backward()
    i, t = out["image_features"].float().cpu(), out["text_features"].float().cpu()
    ref = {k: v.grad for k, v in osd.items() if v.grad is not None}
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert sorted(got) == sorted(ref)
    nv, nt = cfg["vision_cfg"]["layers"] - 1, cfg["text_cfg"]["layers"] - 1
    pooled_sum = ("ln_final.", "visual.ln_post.", f"transformer.resblocks.{nt}.mlp.c_proj.bias", f"transformer.resblocks.{nt}.attn.out_proj.bias",
                  f"visual.transformer.resblocks.{nv}.mlp.c_proj.bias", f"visual.transformer.resblocks.{nv}.attn.out_proj.bias")
    rows = {False: [], True: []}
    for n in sorted(ref):
        a, b = got[n].double().cpu().reshape(-1), ref[n].double().reshape(-1)
        assert torch.isfinite(a).all(), n
        if a.numel() == 1 or float(b.norm()) < 1e-7:
            continue
        rows[n.startswith(pooled_sum)].append((float(torch.dot(a, b) / (a.norm() * b.norm())), float(a.norm() / b.norm()), n))
    main, pooled = sorted(rows[False]), sorted(rows[True])
    mats = sorted(c for c, _, n in main if "resblocks" in n and n.endswith("weight") and got[n].dim() == 2)
    return {"feature": max(float((i - fi.detach()).abs().max()), float((t - ft.detach()).abs().max())),
            "loss": abs(float(loss) - float(lf)) / float(lf),
            "cos_min": main[0][0], "cos_min_name": main[0][2], "cos_median": main[len(main) // 2][0],
            "norm_lo": min(r for _, r, _ in main), "norm_hi": max(r for _, r, _ in main),
            "pooled_cos_min": pooled[0][0], "pooled_cos_min_name": pooled[0][2],
            "pooled_norm_lo": min(r for _, r, _ in pooled), "pooled_norm_hi": max(r for _, r, _ in pooled),
            "block_matrix_cos_median": mats[len(mats) // 2], "block_matrices": len(mats)}


def _fmt_figures(tag, f):
    return (f"[{tag}] feature err {f['feature']:.4f}, loss rel {f['loss']:.5f}, gradient cosine min {f['cos_min']:.4f} ({f['cos_min_name']}) "
            f"median {f['cos_median']:.4f}, norm ratio {f['norm_lo']:.3f}..{f['norm_hi']:.3f}; pooled-sum vectors: cosine min "
            f"{f['pooled_cos_min']:.4f} ({f['pooled_cos_min_name']}), norm ratio {f['pooled_norm_lo']:.3f}..{f['pooled_norm_hi']:.3f}; "
            f"median cosine of the {f['block_matrices']} block weight matrices {f['block_matrix_cos_median']:.4f}")


# name -> image size and what an MI355X measures at batch 128 (profiles/r07_pytest_fp8_production_end_to_end.log): feature error,
# relative loss error, minimum / median gradient cosine and largest norm deviation of the tensors that are not pooled sums, the
# same two of the pooled-sum vectors, median cosine of the 16 block weight matrices, and how far that median lies BELOW the one
# of the first 8 samples.  Every asserted bound is 1.5 x the measured distance from perfect (_cos_bound / _dev_bound), all of
# them inside the floors the full-dimension fixtures are held to (test_fp8_full_dims_match_reference_golden: 0.89 / 0.94 / 22 % /
# 4e-2 / 2 %).  The engine is bit-reproducible at a fixed seed: the margin is for later legitimate re-orderings of fp32 sums.
FP8_E2E = {
    "ViT-L-16": dict(image_size=112, feature=0.0148, loss=0.00005, cos_min=0.9588, cos_median=0.9899, norm=0.053,
                     pooled_cos_min=0.9904, pooled_norm=0.063, block_matrix_cos_median=0.9897, below_batch_8=0.0019),
    "ViT-H-14": dict(image_size=98, feature=0.0126, loss=0.00023, cos_min=0.9665, cos_median=0.9912, norm=0.028,
                     pooled_cos_min=0.9911, pooled_norm=0.028, block_matrix_cos_median=0.9905, below_batch_8=0.0015),
}
FP8_FLOORS = dict(feature=4e-2, loss=0.02, cos_min=0.89, cos_median=0.94, norm=0.22)


def _cos_bound(measured):
    return 1.0 - 1.5 * (1.0 - measured)


def _dev_bound(measured):
    return 1.5 * measured


@pytest.mark.parametrize("name", list(FP8_E2E))
def test_fp8_production_kernels_end_to_end(name):
    """The fp8 twin of test_model_gpu.py::test_production_kernels_end_to_end, at the smallest size that reaches the whole-tile
    kernels: 2 layers at the named model's widths, 7 x 7 patches + class token = 50 image tokens, 32 text tokens, batch 128 (50 is
    2 mod 4: B x 50 is a multiple of 256 from B = 128 on) - 6400 image rows, 4096 text rows, every block GEMM on gemm_f8a /
    gemm_tn8, the in-projection and c_fc products with 375-500 tiles (two tiles per workgroup on 256 CUs).  precision="fp8", keep
    plan from bench.plan_keep_tensors with bench.KEEP_VALUE_MS_PER_GB_FP8 (everything fits: each block keeps the e4m3 pre-activation),
    LastBlockFn on both towers.  Features, loss and every gradient against the fp32 oracle on the same weights and batch.

    The same model on the first 8 samples (400 image rows: ragged, gemm_nt_f8_kernel and gemm_tn8's byte-gather kernel; 256 text
    rows: one M panel of gemm_f8a) tests "e4m3 rounding averages out over the tokens of a batch" (VERDICT weak 1b).  It
    does NOT, at these sizes: the median cosine of the 16 block weight matrices is 0.9897 / 0.9905 (ViT-L-16 / ViT-H-14) at batch
    128 against 0.9916 / 0.9920 at batch 8, the minimum (block 0's c_proj.weight of the image tower, both batches) 0.9588 / 0.9665
    against 0.9719 / 0.9644.  Asserted is what is measured: batch 128 is not more than 1.5 x the measured 0.0019 / 0.0015 below
    batch 8 (that it is not above is a finding, not a requirement).

    Measured on an MI355X (profiles/r07_pytest_fp8_production_end_to_end.log), batch 128 | batch 8:
      ViT-L-16  feature error 0.0148 | 0.0134, loss 0.005 % | 0.19 %, cosine min 0.9588 | 0.9719 median 0.9899 | 0.9916, norm ratio
                0.998..1.053 | 0.990..1.017; pooled-sum vectors cosine min 0.9904 | 0.9913, norm ratio 1.021..1.063 | 0.970..1.005
      ViT-H-14  feature error 0.0126 | 0.0109, loss 0.023 % | 0.025 %, cosine min 0.9665 | 0.9644 median 0.9912 | 0.9917, norm ratio
                0.972..1.000 | 0.978..1.036; pooled-sum vectors cosine min 0.9911 | 0.9922, norm ratio 0.972..0.994 | 0.987..1.014"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench
    from clipa_amd import lib
    spec = FP8_E2E[name]
    cfg = clipa_amd.get_model_config(name)
    cfg["vision_cfg"]["layers"], cfg["text_cfg"]["layers"] = 2, 2
    cfg["vision_cfg"]["image_size"], cfg["text_cfg"]["context_length"] = spec["image_size"], 32
    B, Lv, Lt = 128, 50, 32
    torch.manual_seed(7)
    m = clipa_amd.CLIP(**cfg, output_dict=True)
    clipa_amd.convert_weights_to_lp(m, torch.bfloat16)
    sd = {k: v.detach().float().clone() for k, v in m.state_dict().items()}
    m.to(DEV)
    vt, tt = m.visual.transformer, m.transformer
    vt.fp8 = tt.fp8 = True                              # what create_model(precision="fp8") sets (factory.py)
    m.set_grad_checkpointing(True)
    images, texts = O.synthetic_batch(B, spec["image_size"], Lt, cfg["text_cfg"]["vocab_size"], seed=11)
    tok = {"v": B * Lv, "t": B * Lt}
    tb = {(tw, n): tr.tensor_keep_bytes(tok[tw], n) for tw, tr in (("v", vt), ("t", tt)) for n in ("h8", "h", "a", "x1", "qkv")}
    plan = bench.plan_keep_tensors(64 << 30, {"v": 2, "t": 2}, tb, bench.KEEP_VALUE_MS_PER_GB_FP8, ("v", "t"))
    assert all(plan[tw][n] == 2 for tw in ("v", "t") for n in ("h8", "a", "x1", "qkv")), plan
    vt.keep_counts, tt.keep_counts = dict(plan["v"]), dict(plan["t"])

    def step(b):
        lib.gemm_counts(reset=True)
        m.zero_grad(set_to_none=True)
        out = m(images[:b].to(DEV), texts[:b].to(DEV))
        loss = clipa_amd.ClipLoss()(**out, output_dict=True)["contrastive_loss"]
        loss.backward()
        torch.cuda.synchronize()
        c = lib.gemm_counts()
        print(f"[{name} fp8, batch {b}] launches: gemm_f8a {c[6]} (e4m3 copy {c[12]}, e4m3 operand {c[13]}, quantised output {c[14]}, emitting "
              f"{c[0]}), gemm_nt_f8_kernel {c[7]}, gemm_tn8 {c[8]}, its byte-gather kernel alone {c[9]}, gemm_nta {c[2]}, gemm_nt2 {c[1]}")
        return c, _fp8_parity_figures(m, out, loss, sd, cfg, images[:b], texts[:b])

    c, big = step(B)
    print(_fmt_figures(f"{name} x 2 layers, fp8, batch {B}: production kernels end to end", big))
    # gemm_f8a, per tower (everything kept, nothing recomputed):
    #   block 0 forward (engine._block_forward_fp8): in-projection, out-projection, c_fc with the e4m3 copy, c_proj            4
    #   block 0 backward (_block_backward_fp8): the emitting GELU-backward product of c_proj (reads the kept e4m3 bytes), the
    #     input gradients of c_fc, of the out-projection and of the in-projection                                              4
    #   block 1 (LastBlockFn): the in-projection and its input gradient; its B pooled rows take the bf16 GEMMs                  2
    # two towers: 20 launches, 2 with the e4m3 copy, 2 from e4m3 bytes - both of them emitting -, none with a quantised output
    # (fp8_predicted_scales is off), nothing left on gemm_nt_f8_kernel.  gemm_tn8: the 4 + 1 block weight gradients of a tower.
    assert (c[6], c[12], c[13], c[0], c[14]) == (20, 2, 2, 2, 0), c
    assert c[7] == 0, c
    assert c[8] >= 10, c
    c8, small = step(8)
    print(_fmt_figures(f"{name} x 2 layers, fp8, batch 8: generic kernels", small))
    # 8 x 50 = 400 image rows are ragged: the image tower's 10 products run on gemm_nt_f8_kernel; 8 x 32 = 256 text rows are one
    # whole M panel: the text tower's stay on gemm_f8a (one tile per workgroup)
    assert (c8[6], c8[7], c8[8]) == (10, 10, 0), c8
    for k in ("feature", "loss", "norm"):
        assert _dev_bound(spec[k]) <= FP8_FLOORS[k]
    assert _cos_bound(spec["cos_min"]) >= FP8_FLOORS["cos_min"] and _cos_bound(spec["cos_median"]) >= FP8_FLOORS["cos_median"]
    assert big["feature"] < _dev_bound(spec["feature"]) and big["loss"] < _dev_bound(spec["loss"]), (big["feature"], big["loss"])
    assert big["cos_min"] > _cos_bound(spec["cos_min"]), (big["cos_min"], big["cos_min_name"])
    assert big["cos_median"] > _cos_bound(spec["cos_median"]), big["cos_median"]
    assert max(1.0 - big["norm_lo"], big["norm_hi"] - 1.0) < _dev_bound(spec["norm"]), (big["norm_lo"], big["norm_hi"])
    assert big["pooled_cos_min"] > _cos_bound(spec["pooled_cos_min"]), (big["pooled_cos_min"], big["pooled_cos_min_name"])
    assert max(1.0 - big["pooled_norm_lo"], big["pooled_norm_hi"] - 1.0) < _dev_bound(spec["pooled_norm"]), (big["pooled_norm_lo"], big["pooled_norm_hi"])
    assert big["block_matrix_cos_median"] > _cos_bound(spec["block_matrix_cos_median"]), big["block_matrix_cos_median"]
    # the rounding does not average out over the batch (see the docstring): measured 0.0019 / 0.0015 BELOW the batch of 8
    assert big["block_matrix_cos_median"] >= small["block_matrix_cos_median"] - _dev_bound(spec["below_batch_8"]), \
        (big["block_matrix_cos_median"], small["block_matrix_cos_median"])
