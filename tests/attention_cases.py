"""Cases of the fused attention kernels (csrc/attention.hip, attention_wide.hip), host only: the table of every kernel
instantiation the library compiles, the sequence lengths that reach each of them, and two input generators - the seeded
random inputs of tests/test_kernels_gpu.py::test_attention and "routed" inputs on which every key matters and the result is
known as integers before any kernel runs.

Used by tests/test_attention_cases_cpu.py (the table and the exactness of the routed inputs, checked against the fp64 oracle
on the CPU) and tests/test_attention_gpu.py (the kernels)."""
import math
from collections import namedtuple

import torch

bf16 = torch.bfloat16

SHORT_DH = (64, 80)            # either mask
WIDE_DH = (88, 104, 112)       # image towers only: no causal mask
MAX_NKT = 9                    # one-piece kernels: L <= 288
LONG_CHUNK = 256               # rows per LDS chunk of the long kernels (LONG_CT * 32)
LONG_LMAX = 1024

# ---- traits, restated from the constexpr formulas of csrc/attention_common.h -------------------------------------------------
# HD<DH>::RB / ::WGS / ::KS, WGHeads<NKT>::HPW, attn_waves<NKT, DH>(), Stg<DH>::BYTES, fwd_stages<NKT, DH>(),
# bwd_stages<NKT, DH>() there, and PREFETCH in attn_fwd_kernel (csrc/attention.hip).  A change of those formulas must change
# these lines too: tests/test_attention_cases_cpu.py pins the values the table is expected to hold.


def _rb(dh):
    return 128 if dh == 64 else 256


def _wgs(dh):
    return 2 if dh == 64 else 1


def _hpw(nkt):
    return 4 if nkt == 1 else (2 if nkt == 2 else 1)


def _waves(nkt, dh):
    return 8 if (dh == 80 and nkt >= 5) else 4


def _stg(dh):
    return 4096 if dh == 64 else 2560


def _fwd_staged(nkt, dh):
    return dh in SHORT_DH and (_hpw(nkt) * 2 * nkt * 32 * _rb(dh) + _waves(nkt, dh) * _stg(dh)) * _wgs(dh) <= 160 * 1024


def _bwd_staged(nkt, dh):
    return dh in SHORT_DH and (_hpw(nkt) * (2 * nkt * 32 * _rb(dh) + 3 * nkt * 32 * 4) + _waves(nkt, dh) * _stg(dh)) * _wgs(dh) <= 160 * 1024


def _prefetch(nkt, dh):
    return not (nkt == 9 and dh == 64)


Inst = namedtuple("Inst", "nkt dh causal hpw waves fwd_staged bwd_staged prefetch ragged_k")


def _inst(nkt, dh, causal):
    return Inst(nkt, dh, causal, _hpw(nkt), _waves(nkt, dh), _fwd_staged(nkt, dh), _bwd_staged(nkt, dh), _prefetch(nkt, dh),
                dh % 16 != 0)


INSTANTIATIONS = tuple([_inst(nkt, dh, causal) for dh in SHORT_DH for causal in (False, True) for nkt in range(1, MAX_NKT + 1)]
                       + [_inst(nkt, dh, False) for dh in WIDE_DH for nkt in range(1, MAX_NKT + 1)])


def nkt_of(L):
    """Key tiles of a one-piece launch (ATTN_DISPATCH_DH: (L + 31) / 32)."""
    return (L + 31) // 32


def edge_lengths(nkt):
    """One valid row in the last tile, and a full last tile."""
    return (32 * (nkt - 1) + 1, 32 * nkt)


SHORT_B, SHORT_H = 3, 3        # nine heads: 1 live + 3 empty slots in the last workgroup at NKT = 1, 1 + 1 at NKT = 2
LONG_B, LONG_H = 1, 2
SHORT_CASES = tuple((i, L) for i in INSTANTIATIONS for L in edge_lengths(i.nkt))
LONG_CASES = tuple([(dh, L, causal) for dh in SHORT_DH for causal in (False, True) for L in (289, 512, 513)]
                   + [(dh, L, False) for dh in WIDE_DH for L in (289, 513)])


def short_id(case):
    i, L = case
    return f"nkt{i.nkt}-dh{i.dh}-{'causal' if i.causal else 'full'}-L{L}"


def long_id(case):
    dh, L, causal = case
    return f"long-dh{dh}-{'causal' if causal else 'full'}-L{L}"


def case_seed(dh, L, causal):
    return 1000 * dh + 2 * L + int(causal)


# ---- random inputs -----------------------------------------------------------------------------------------------------------
def random_case(dh, H, B, L, seed):
    """The inputs of test_attention: qkv ~ N(0, 1.2^2) [B*L, 3*H*dh], dO ~ N(0, 1) [B*L, H*dh], both bf16."""
    D = dh * H
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B * L, 3 * D, generator=g) * 1.2).to(bf16)
    g = torch.Generator().manual_seed(seed + 1)
    dout = torch.randn(B * L, D, generator=g).to(bf16)
    return qkv, dout


# ---- routed inputs -----------------------------------------------------------------------------------------------------------
MARGIN = 40.0                  # least scaled-logit distance between a query's routed key and any other admissible key
ROUTE_GAIN = 16.0              # Q row i = ROUTE_GAIN * K[pi(i)]
MAX_HITS = 32                  # queries routed to one key: |dV| <= 8 * 32 = 256, every such integer is a bf16 value

Routed = namedtuple("Routed", "qkv dout pi out dv dv_abs margin")


def leak_bound(L):
    """What the keys a query is NOT routed to may add to an output whose exact value is zero: each carries a probability below
    exp(-MARGIN) (kept, not flushed: bf16 has fp32's exponent range), times |v| <= 8, over at most L keys; the factor 2 covers
    the rounding of the probabilities."""
    return 2.0 * 8.0 * L * math.exp(-MARGIN)


def _pattern(digit_mul, col_mul, h_mul, b_mul, idx, dh, h, b):
    """Integers of {-8..-1, 1..8}, [len(idx), dh]: column d carries base-16 digit (d % 3) of the row index, so two different
    rows differ in a third of the columns at least; never zero, so no output of the forward is an exact zero."""
    d = torch.arange(dh)
    digit = torch.stack([idx % 16, (idx // 16) % 16, idx // 256], 1)[:, d % 3]              # [rows, dh]
    v = (digit_mul * digit + col_mul * d[None, :] + h_mul * h + b_mul * b) % 16 - 8
    return torch.where(v >= 0, v + 1, v)


def _route_full(L, g, repeats):
    """A seeded permutation (every key hit exactly once); `repeats`: a few queries are re-routed to keys that are hit already,
    so that some dV rows sum several dO rows (and, the map being L -> L, as many keys go without a query)."""
    pi = torch.randperm(L, generator=g)
    if repeats and L > 1:
        n = max(1, L // 8)
        rows = torch.randperm(L, generator=g)[:n]
        pi[rows] = pi[torch.randint(0, L, (n,), generator=g)]
    return pi


def _route_causal(L, g):
    """pi(i) <= i, seeded, with the routes a wrong mask bound would lose or gain: the diagonal at the first and last key of every
    tile, the same keys from a query of a later tile where one exists, and key 0 from a few late queries."""
    rows = torch.arange(L)
    pi = torch.minimum((torch.rand(L, generator=g, dtype=torch.float64) * (rows + 1)).long(), rows)
    forced = {}
    tiles = nkt_of(L)
    for t in range(tiles):
        for key in (32 * t, min(32 * t + 31, L - 1)):
            forced[key] = key                                       # the diagonal: the last admissible key of that query
    free = [i for i in range(L) if i not in forced]
    order = [free[j] for j in torch.randperm(len(free), generator=g).tolist()]
    for t in range(tiles):
        for key in (32 * t, min(32 * t + 31, L - 1)):
            row = next((i for i in order if i not in forced and i >= 32 * (t + 1)), None)
            if row is not None:
                forced[row] = key                                   # ... and from a later tile
    for row in [i for i in order if i not in forced and i > 0][:3]:
        forced[row] = 0
    for row, key in forced.items():
        pi[row] = key
    return pi


def routed_case(dh, H, B, L, causal, seed):
    """Inputs on which attention is a table lookup, and the lookup's result.

    Per (batch, head): K rows are seeded +-1 sign codes, Q row i = 16 * K[pi(i)], V and dO small non-zero integers (|v| <= 8)
    that differ between any two rows and between heads and batch rows; everything is exact in bf16.  The scaled logit of the
    routed key is 16 sqrt(dh); the function asserts that every other admissible key lies at least MARGIN = 40 below it, which
    makes the softmax a one-hot row up to exp(-40):
        out[i] = V[pi(i)],  dV[j] = sum of dO[i] over pi(i) = j,  dQ = dK = 0      (delta = <dO, O> = dP at the routed key).
    pi: causal - _route_causal; otherwise a permutation on the even heads (b * H + h) and a permutation with repeats on the odd
    ones (a map L -> L that hits every key is a permutation: repeats and full coverage cannot share one head).
    Returns Routed(qkv [B*L, 3D] bf16, dout [B*L, D] bf16, pi [B, H, L], out [B*L, D] f64, dv [B*L, D] f64, dv_abs [B*L, D] f64
    = the same sums over |dO| (what an fp32 accumulation of dv passes through), least margin)."""
    D = dh * H
    g = torch.Generator().manual_seed(seed)
    qkv = torch.zeros(B, L, 3, H, dh)
    dout = torch.zeros(B, L, H, dh)
    out = torch.zeros(B, L, H, dh, dtype=torch.float64)
    dv = torch.zeros(B, L, H, dh, dtype=torch.float64)
    dv_abs = torch.zeros(B, L, H, dh, dtype=torch.float64)
    pis = torch.zeros(B, H, L, dtype=torch.long)
    idx = torch.arange(L)
    margin = float("inf")
    for b in range(B):
        for h in range(H):
            code = (torch.randint(0, 2, (L, dh), generator=g) * 2 - 1).float()
            pi = _route_causal(L, g) if causal else _route_full(L, g, repeats=(b * H + h) % 2 == 1)
            v = _pattern(7, 3, 5, 11, idx, dh, h, b).float()
            do = _pattern(5, 7, 3, 13, idx, dh, h, b).float()
            qkv[b, :, 0, h], qkv[b, :, 1, h], qkv[b, :, 2, h] = ROUTE_GAIN * code[pi], code, v
            dout[b, :, h] = do
            out[b, :, h] = v[pi].double()
            dv[b, :, h].index_add_(0, pi, do.double())
            dv_abs[b, :, h].index_add_(0, pi, do.double().abs())
            pis[b, h] = pi
            # the condition on the INPUTS that the exact restatement rests on
            s = (ROUTE_GAIN * code[pi].double()) @ code.double().T / math.sqrt(dh)          # [query, key]
            gap = ROUTE_GAIN * math.sqrt(dh) - s
            gap[idx, pi] = float("inf")
            if causal:
                gap.masked_fill_(idx[None, :] > idx[:, None], float("inf"))
            if L > 1:
                margin = min(margin, float(gap.min()))
            assert int(torch.bincount(pi, minlength=L).max()) <= MAX_HITS
            if causal:
                assert bool((pi <= idx).all())
    assert margin >= MARGIN, f"routed_case(dh={dh}, L={L}, causal={causal}, seed={seed}): margin {margin:.1f} < {MARGIN}"
    qkv_b, dout_b = qkv.reshape(B * L, 3 * D).to(bf16), dout.reshape(B * L, D).to(bf16)
    assert torch.equal(qkv_b.float(), qkv.reshape(B * L, 3 * D)) and torch.equal(dout_b.float(), dout.reshape(B * L, D))
    assert torch.equal(dv.to(bf16).double(), dv) and bool((out != 0).all())
    return Routed(qkv_b, dout_b, pis, out.reshape(B * L, D), dv.reshape(B * L, D), dv_abs.reshape(B * L, D), margin)
