"""tests/attention_cases.py checked on the CPU: the instantiation table against the values csrc/attention_common.h is known to
give, the lengths against the tile counts they are meant to reach, and the routed inputs against the fp64 oracle - their
integer restatement is PROVEN here, before a kernel is held to it bit for bit (tests/test_attention_gpu.py)."""
import functools

import torch

from oracle import clip_oracle as O
from . import attention_cases as AC


def _all_routed():
    for inst, L in AC.SHORT_CASES:
        yield AC.short_id((inst, L)), (inst.dh, AC.SHORT_H, AC.SHORT_B, L, inst.causal)
    for dh, L, causal in AC.LONG_CASES:
        yield AC.long_id((dh, L, causal)), (dh, AC.LONG_H, AC.LONG_B, L, causal)


@functools.lru_cache(maxsize=None)
def _routed(dh, H, B, L, causal):
    return AC.routed_case(dh, H, B, L, causal, AC.case_seed(dh, L, causal))


def test_instantiation_table_is_complete():
    T = AC.INSTANTIATIONS
    assert len(T) == 36 + 27 and len({(i.nkt, i.dh, i.causal) for i in T}) == 63
    assert sum(i.dh in (64, 80) for i in T) == 36 and sum(i.dh in (88, 104, 112) for i in T) == 27
    assert not any(i.causal for i in T if i.dh > 80)
    # every trait value occurs ...
    assert {i.hpw for i in T} == {1, 2, 4} and {i.waves for i in T} == {4, 8}
    for trait in ("fwd_staged", "bwd_staged", "prefetch", "ragged_k"):
        assert {getattr(i, trait) for i in T} == {True, False}, trait
    # ... where csrc/attention_common.h puts it
    for i in T:
        assert i.hpw == {1: 4, 2: 2}.get(i.nkt, 1)
        assert i.waves == (8 if i.dh == 80 and i.nkt >= 5 else 4)
        assert i.fwd_staged == (i.dh in (64, 80) and i.nkt <= 8)
        assert i.bwd_staged == ((i.dh == 64 and i.nkt <= 7) or (i.dh == 80 and i.nkt <= 8))
        assert i.prefetch == ((i.nkt, i.dh) != (9, 64))
        assert i.ragged_k == (i.dh in (88, 104))
    # 8 key tiles at head dim 64: the forward's LDS sits exactly at the limit of two workgroups per CU
    assert (2 * 8 * 32 * 128 + 4 * 4096) * 2 == 160 * 1024


def test_lengths_reach_their_instantiation():
    assert len(AC.SHORT_CASES) == 126
    for inst, L in AC.SHORT_CASES:
        assert AC.nkt_of(L) == inst.nkt and 1 <= L <= 288
    for inst in AC.INSTANTIATIONS:
        lo, hi = AC.edge_lengths(inst.nkt)
        assert lo % 32 == 1 and hi % 32 == 0 and AC.nkt_of(lo - 1) == inst.nkt - 1 and AC.nkt_of(hi + 1) == inst.nkt + 1
    assert len(AC.LONG_CASES) == 2 * 2 * 3 + 3 * 2
    for dh, L, causal in AC.LONG_CASES:
        assert 288 < L <= AC.LONG_LMAX and not (causal and dh > 80)
        assert L > AC.LONG_CHUNK                      # more than one chunk: the online softmax rescales
    assert {L % 32 for _, L, _ in AC.LONG_CASES} == {0, 1}
    # nine heads leave empty slots in the last workgroup wherever a workgroup takes more than one head
    assert (AC.SHORT_B * AC.SHORT_H) % 4 == 1 and (AC.SHORT_B * AC.SHORT_H) % 2 == 1 and AC.SHORT_B >= 2 and AC.SHORT_H >= 2


def test_fp64_oracle_reproduces_the_routed_restatement():
    for name, (dh, H, B, L, causal) in _all_routed():
        r = _routed(dh, H, B, L, causal)
        D = dh * H
        x = r.qkv.double().reshape(B, L, 3 * D).requires_grad_(True)
        o = O.attention(x, H, causal)
        o.backward(r.dout.double().reshape(B, L, D))
        dq, dk, dv = x.grad.reshape(B * L, 3 * D).split(D, dim=1)
        assert float((o.detach().reshape(B * L, D) - r.out).abs().max()) <= 1e-12, name
        assert float((dv - r.dv).abs().max()) <= 1e-12, name
        assert float(dq.abs().max()) <= 1e-9 and float(dk.abs().max()) <= 1e-9, name


def test_routed_maps_meet_margin_and_coverage():
    margins = []
    for name, (dh, H, B, L, causal) in _all_routed():
        r = _routed(dh, H, B, L, causal)
        if L > 1:
            assert r.margin >= AC.MARGIN, name
            margins.append(r.margin)
        idx = torch.arange(L)
        for b in range(B):
            for h in range(H):
                pi = r.pi[b, h]
                hits = torch.bincount(pi, minlength=L)
                assert int(hits.max()) <= AC.MAX_HITS, name
                if L > 32 * AC.MAX_NKT:    # long kernels: a routed key in a later chunk than the first one the row meets
                    assert bool((pi >= AC.LONG_CHUNK).any()) and bool((pi < AC.LONG_CHUNK).any()), name
                if not causal:
                    if (b * H + h) % 2 == 0:
                        assert bool((hits == 1).all()), name                  # a permutation: every key hit
                    elif L > 1:
                        assert int(hits.max()) >= 2, name                     # some dV row sums several dO rows
                    continue
                assert bool((pi <= idx).all()), name
                assert int(pi[0]) == 0 and bool((pi == idx).any()), name
                if L > 1:
                    assert bool((pi[1:] == 0).any()), name
                for t in range(AC.nkt_of(L)):
                    for key in (32 * t, min(32 * t + 31, L - 1)):
                        assert int(pi[key]) == key, name                      # the diagonal at the tile's edges
                        if L - 32 * (t + 1) >= 32:
                            assert bool((pi[32 * (t + 1):] == key).any()), (name, key)   # and from a later tile
    assert min(margins) >= AC.MARGIN
