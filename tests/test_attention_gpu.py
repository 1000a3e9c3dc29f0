"""Every compiled instantiation of the fused attention kernels (csrc/attention.hip, attention_wide.hip) against the fp64 oracle
(oracle/clip_oracle.attention), forward and backward, at both edge lengths of its key-tile count: 32 (NKT - 1) + 1 (one valid
row in the last tile) and 32 NKT (full last tile); the long kernels (L > 288) at lengths around their 256-row chunks; the packed
variable-length launches at both edges of all nine tile classes.  tests/attention_cases.py holds the table and the inputs.

Two kinds of input.  RANDOM: the N(0, 1.2^2) inputs and the tolerances of tests/test_kernels_gpu.py::test_attention (forward
2^-6 / 8e-3, gradients 2^-5 / 2e-2), plus the softmax statistics the forward hands the backward.  ROUTED: every query's
probability mass sits on ONE key chosen by a seeded map, values are small integers, and the result is known exactly
(tests/test_attention_cases_cpu.py proves that against the fp64 oracle); a key that is dropped, doubled, masked wrongly or read
from the wrong row / head / batch entry changes an output by >= 1, where the random inputs move by less than their tolerance.

What "exact" means for the routed inputs, from the kernels' arithmetic (csrc/attention_common.h softmax_rows, attention.hip):
  * the routed key's un-normalised probability is exp2(fma(s, c, -(max * c))) = 1 + O(1e-5) (the fma keeps the rounding residual
    of max * c), bf16(that) = 1 exactly; all others are below exp(-40), so out = bf16(V[pi] * (1 + O(1e-5))) = V[pi]: BITWISE.
  * dV = sum of bf16(P) * dO: the integer sum wherever that sum is not zero: BITWISE.  Where it is zero, "bitwise" is relaxed,
    for two reasons read from the code:
      - a key no query is routed to (under the causal mask and on the heads whose map has repeats there must be some): the
        probabilities of the other keys remain; they are below exp(-40) but not zero - bf16 keeps fp32's exponent range and
        pack_frag -> pack2bf rounds to nearest without a flush - so these entries are held to attention_cases.leak_bound(L)
        (< 1e-12) instead of to +0.0;
      - routed dO rows that cancel (+6 and -6 on one key): the sum runs inside the MFMA instruction (attention.hip, `dv[dt] =
        __builtin_amdgcn_mfma_f32_32x32x16_bf16(...)` of the key-major sweep), products exact, accumulation in fp32.  Measured on
        MI355X (dh 64, no mask, 2 - 13 entries of ~100 - 300 per case): such an entry comes out as -2^-24 * 2^floor(log2 |dO|),
        i.e. ONE unit of the accumulator's last place at the size of the addend that then cancels - a tiny addend of the other
        sign costs the running sum a unit, the cancellation exposes it.  That is the instruction's summation, not the kernel's
        logic (a wrong key, mask or row moves an entry by >= 1), so these entries are held to what an fp32 accumulation can
        lose: one unit in the last place (2^-23 relative) of the largest running sum, sum |dO| over the routed rows, per
        routed row - 2.9e-6 for a +-6 pair, nine orders below a wrong key and far inside one bf16 ulp of the addends.
    The forward has no exact zeros: V is never zero.
  * dS at the routed key is pe * (dp - Dq) with dp = <dO, V[pi]> and Dq = <dO, O> the same integer: exactly zero; the other keys
    give |dQ|, |dK| <= leak: held to 1e-6.
"""
import math

import pytest
import torch

from oracle import clip_oracle as O
from . import attention_cases as AC
from .test_kernels_gpu import check, ops

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
DEV = "cuda"

FWD_TOL = (2 ** -6, 8e-3)         # test_attention's
BWD_TOL = (2 ** -5, 2e-2)
# log-sum-exp encoded by the statistics: the relative bound of test_fused_similarity_cross_entropy's "loss rows" (1e-4); its
# absolute part (2e-4 there) is needed where a row's log-sum-exp crosses zero and is taken ten times tighter: the statistics are
# fp32 throughout (a few ulps of a scaled logit <= 32, hardware exp2 / log2: ~1e-6 each)
LSE_TOL = (1e-4, 2e-5)


def _oracle(qkv, dout, B, L, H, causal):
    """fp64: (out [B, L, D], dqkv [B, L, 3D], log-sum-exp of the scaled, masked logits [B*H*L] in the statistics' order)."""
    D = qkv.shape[1] // 3
    dh = D // H
    x = qkv.double().reshape(B, L, 3 * D).requires_grad_(True)
    o = O.attention(x, H, causal)
    o.backward(dout.double().reshape(B, L, D))
    q, k, _ = x.detach().split(D, dim=-1)
    q = q.reshape(B, L, H, dh).transpose(1, 2)
    k = k.reshape(B, L, H, dh).transpose(1, 2)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    if causal:
        s = s + torch.full((L, L), float("-inf"), dtype=s.dtype).triu(1)
    return o.detach(), x.grad, torch.logsumexp(s, dim=-1).reshape(-1)


def _lse(stats):
    """The forward's two floats per (batch, head, query) row (AttnArgs::stats, softmax_rows): (c * rowmax, 1 / rowsum) with
    c = scale * log2(e) and the row sum taken of exp2(c * (s - rowmax)) -> log-sum-exp = ln 2 * c rowmax - ln(1 / rowsum)."""
    st = stats.double().cpu()
    return st[:, 0] * math.log(2.0) - torch.log(st[:, 1])


def _run(qkv, dout, B, L, H, causal):
    o = ops()
    q, d = qkv.to(DEV), dout.to(DEV)
    got, stats = o.attention_fwd(q, B, L, H, causal, want_stats=True)
    assert torch.equal(got, o.attention_fwd(q, B, L, H, causal)), "the forward differs with / without statistics"
    dqkv = o.attention_bwd(q, got, d, stats, B, L, H, causal)
    return got, stats, dqkv


def _check_random(dh, H, B, L, causal):
    qkv, dout = AC.random_case(dh, H, B, L, seed=AC.case_seed(dh, L, causal))
    D = dh * H
    ref, dref, lse = _oracle(qkv, dout, B, L, H, causal)
    got, stats, dqkv = _run(qkv, dout, B, L, H, causal)
    check("fwd", got.reshape(B, L, D), ref, *FWD_TOL)
    assert stats.shape == (B * H * L, 2)
    check("log-sum-exp of the statistics", _lse(stats), lse, *LSE_TOL)
    check("dqkv", dqkv.reshape(B, L, 3 * D), dref, *BWD_TOL)


def _where(name, bad, B, L, H, dh):
    """Names the first wrong element as (batch, row, head, column)."""
    i = int(torch.nonzero(bad.reshape(-1))[0])
    row, col = divmod(i, H * dh)
    return f"{name}: {int(bad.sum())} wrong; first at batch {row // L} row {row % L} head {col // dh} column {col % dh}"


def _check_routed(dh, H, B, L, causal):
    r = AC.routed_case(dh, H, B, L, causal, AC.case_seed(dh, L, causal))
    D = dh * H
    got, stats, dqkv = _run(r.qkv, r.dout, B, L, H, causal)
    got, dqkv = got.cpu(), dqkv.cpu()
    dq, dk, dv = (t.double() for t in dqkv.split(D, dim=1))
    bad = got.double() != r.out
    assert not bad.any(), _where("forward != V[pi]", bad, B, L, H, dh) + f" (got {got.double()[bad][0]:g}, want {r.out[bad][0]:g})"
    assert torch.equal(got, r.out.to(bf16))                                   # bitwise (no -0.0 either: V is never zero)
    hit = r.dv != 0
    bad = hit & (dv != r.dv)
    assert not bad.any(), _where("dV != sum of the routed dO rows", bad, B, L, H, dh) + f" (got {dv[bad][0]:g}, want {r.dv[bad][0]:g})"
    assert torch.equal(dqkv[:, 2 * D:][hit], r.dv.to(bf16)[hit])
    hits = torch.stack([torch.stack([torch.bincount(r.pi[b, h], minlength=L) for h in range(H)], 1) for b in range(B)])   # [B, L, H]
    hits = hits[..., None].expand(B, L, H, dh).reshape(B * L, D).double()
    zero_tol = AC.leak_bound(L) + hits * r.dv_abs * 2.0 ** -23               # (module docstring: unrouted keys / cancelling rows)
    bad = ~hit & (dv.abs() > zero_tol)
    assert not bad.any(), _where("dV of an exact zero above its bound", bad, B, L, H, dh) + f" (got {dv[bad][0]:g}, bound {zero_tol[bad][0]:g})"
    assert float(dq.abs().max()) <= 1e-6, f"max |dQ| = {float(dq.abs().max()):g}"
    assert float(dk.abs().max()) <= 1e-6, f"max |dK| = {float(dk.abs().max()):g}"
    ref, dref, lse = _oracle(r.qkv, r.dout, B, L, H, causal)
    check("fwd", got.reshape(B, L, D), ref, *FWD_TOL)
    check("log-sum-exp of the statistics", _lse(stats), lse, *LSE_TOL)
    check("dqkv", dqkv.reshape(B, L, 3 * D), dref, *BWD_TOL)


@pytest.mark.parametrize("case", AC.SHORT_CASES, ids=AC.short_id)
def test_attention_instantiation_random(case):
    inst, L = case
    _check_random(inst.dh, AC.SHORT_H, AC.SHORT_B, L, inst.causal)


@pytest.mark.parametrize("case", AC.SHORT_CASES, ids=AC.short_id)
def test_attention_instantiation_routed(case):
    inst, L = case
    _check_routed(inst.dh, AC.SHORT_H, AC.SHORT_B, L, inst.causal)


@pytest.mark.parametrize("case", AC.LONG_CASES, ids=AC.long_id)
def test_attention_long_random(case):
    dh, L, causal = case
    _check_random(dh, AC.LONG_H, AC.LONG_B, L, causal)


@pytest.mark.parametrize("case", AC.LONG_CASES, ids=AC.long_id)
def test_attention_long_routed(case):
    """Some queries' routed keys lie in the second or third 256-row chunk: the online softmax meets a lesser maximum first and
    its rescale (alpha <= exp(-40)) has to wipe that partial sum and output."""
    dh, L, causal = case
    _check_routed(dh, AC.LONG_H, AC.LONG_B, L, causal)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dh", [64, 80])
def test_attention_varlen_every_class(dh, causal):
    """Packed sequences at both edges of all nine tile classes (1, 32, 33, 64, ..., 257, 288) and five seeded lengths, context
    288: every sequence against the oracle, and BIT FOR BIT against the fixed-length kernels run on that sequence alone
    (B = 1, L = len: the same instantiation, the same L in the kernel's view of the arguments); pad rows zero."""
    o = ops()
    H, ctx = 2, 288
    D = dh * H
    g = torch.Generator().manual_seed(7 + dh + int(causal))
    lens = [L for nkt in range(1, AC.MAX_NKT + 1) for L in AC.edge_lengths(nkt)] + torch.randint(1, ctx + 1, (5,), generator=g).tolist()
    lens = torch.tensor(lens)[torch.randperm(len(lens), generator=g)]         # classes interleaved in the packed matrix
    vl = o.VarLen(lens, ctx, DEV)
    assert sorted(k for k, _, _ in vl.classes) == list(range(1, 10)) and vl.rows > vl.T
    qkv = torch.zeros(vl.rows, 3 * D, dtype=bf16)
    dout = torch.zeros(vl.rows, D, dtype=bf16)
    qkv[:vl.T], dout[:vl.T] = AC.random_case(dh, H, 1, vl.T, seed=500 + dh + int(causal))
    qkv_d, dout_d = qkv.to(DEV), dout.to(DEV)
    got, stats = o.attention_fwd_varlen(qkv_d, vl, H, causal, want_stats=True)
    assert torch.equal(got, o.attention_fwd_varlen(qkv_d, vl, H, causal))
    dq = o.attention_bwd_varlen(qkv_d, got, dout_d, stats, vl, H, causal)
    assert not got[vl.T:].float().abs().any() and not dq[vl.T:].float().abs().any(), "pad rows must be zero"
    starts = (torch.cumsum(lens, 0) - lens).tolist()
    for b, (s0, n) in enumerate(zip(starts, lens.tolist())):
        ref, dref, _ = _oracle(qkv[s0:s0 + n], dout[s0:s0 + n], 1, n, H, causal)
        check(f"fwd seq {b} (len {n})", got[s0:s0 + n].reshape(1, n, D), ref, *FWD_TOL)
        check(f"dqkv seq {b} (len {n})", dq[s0:s0 + n].reshape(1, n, 3 * D), dref, *BWD_TOL)
        one, one_stats = o.attention_fwd(qkv_d[s0:s0 + n], 1, n, H, causal, want_stats=True)
        assert torch.equal(one, got[s0:s0 + n]), f"forward of sequence {b} (len {n}) differs from the fixed-length kernel"
        one_dq = o.attention_bwd(qkv_d[s0:s0 + n], one, dout_d[s0:s0 + n], one_stats, 1, n, H, causal)
        assert torch.equal(one_dq, dq[s0:s0 + n]), f"backward of sequence {b} (len {n}) differs from the fixed-length kernel"


def test_attention_argument_errors():
    o = ops()
    qkv = torch.zeros(64, 3 * 2 * 88, dtype=bf16, device=DEV)
    with pytest.raises(RuntimeError, match="head dim 88 is compiled for image towers only"):
        o.attention_fwd(qkv, 2, 32, 2, True)
    long_qkv = torch.zeros(1025, 3 * 64, dtype=bf16, device=DEV)
    with pytest.raises(RuntimeError, match=r"L=1025 outside \(0, 1024\]"):
        o.attention_fwd(long_qkv, 1, 1025, 1, False)
    vl = o.VarLen(torch.tensor([20, 32]), 32, DEV)
    wide = torch.zeros(vl.rows, 3 * 2 * 88, dtype=bf16, device=DEV)
    with pytest.raises(RuntimeError, match=r"attention \(varlen\): head dim 88 unsupported \(64 and 80\)"):
        o.attention_fwd_varlen(wide, vl, 2, False)
    stats = torch.zeros(vl.rows * 2, 2, device=DEV)
    with pytest.raises(RuntimeError, match=r"attention \(varlen\): head dim 88 unsupported \(64 and 80\)"):
        o.attention_bwd_varlen(wide, wide[:, :2 * 88].contiguous(), wide[:, :2 * 88].contiguous(), stats, vl, 2, False)
