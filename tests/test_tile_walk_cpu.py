"""The restated tile walk of the persistent NT GEMMs (tests/tile_walk.py) at 256 CUs (an MI355X): it visits every tile exactly
once, and the shapes of the multi-tile GPU tests have the properties those tests are built on - a workgroup that runs a second
and a third tile, a ragged last group, a tile count that is no multiple of the 8 XCDs, each branch of nt_group_size.

Second half: the restated slice plan of the weight-gradient GEMM (tests/tn_plan.py) gives the library's own slice counts at 256
CUs, gemm_tna's decode of a workgroup id visits every (tile, slice) pair exactly once in both work orders, and the case shapes of
the "gemm_tna across tiles and slices" GPU tests have the features those tests are there for."""
import ctypes

import pytest

from . import tile_walk as TW
from . import tn_plan as TP

CUS = 256
# name -> tiles, gm, tilesM % gm, ntiles % 8, {tiles per workgroup: workgroups}; the same for bf16 and fp8 operands
TABLE = {
    "S1": (603, 16, 3, 3, {3: 91, 2: 165}),
    "S2": (260, 8, 5, 4, {2: 4, 1: 252}),
    "S3": (260, 8, 1, 4, {2: 4, 1: 252}),
    "S0": (12, 16, 4, 4, {1: 12}),
}


def _all_tiles_once(w):
    seen = [t for tiles in w.workgroups for t in tiles]
    assert len(seen) == w.ntiles
    assert sorted(seen) == [(m, n) for m in range(w.tiles_m) for n in range(w.tiles_n)]


@pytest.mark.parametrize("bpe", [2, 1])
@pytest.mark.parametrize("name", list(TABLE))
def test_walk_is_a_permutation_with_the_stated_properties(name, bpe):
    M, N, K = TW.SHAPES[name]
    tiles, gm, m_mod_gm, mod8, hist = TABLE[name]
    w = TW.walk(M, N, K, bpe, CUS)
    _all_tiles_once(w)
    assert w.ntiles == tiles and w.grid == min(tiles, CUS) and len(w.workgroups) == w.grid
    assert w.gm == gm
    assert w.tiles_m_mod_gm == m_mod_gm
    assert w.ntiles_mod8 == mod8
    assert TW.tiles_per_workgroup(w) == hist
    assert len(TW.later_tiles(w)) == tiles - w.grid
    if name == "S0":
        with pytest.raises(AssertionError, match="no workgroup runs a second tile"):
            TW.require_second_tiles(w, "control")
    else:
        assert TW.require_second_tiles(w, name) == tiles - CUS
        assert m_mod_gm != 0 and mod8 != 0          # ragged last group, uneven split over the XCDs
        panels = TW.panels_to_check(w)
        assert len(panels) >= 8 and panels[0] == 0 and panels[-1] == w.tiles_m - 1
        assert {m for m, _ in TW.later_tiles(w)} <= set(panels)


def test_group_size_branches():
    """The three branches of nt_group_size and which test shape takes which."""
    assert TW.nt_group_size(9, 256 * 512 * 2) == 16 and TW.nt_group_size(9, 256 * 512) == 16          # S1: narrow output
    assert TW.nt_group_size(20, 256 * 1280 * 2) == 8 and TW.nt_group_size(20, 256 * 1280) == 8        # S2: tilesN > 12
    assert TW.nt_group_size(4, 256 * 4096 * 2) == 8 and TW.nt_group_size(4, 256 * 4096) == 8          # S3: tilesN == 4, 1 - 2 MiB panels
    assert TW.nt_group_size(4, 256 * 1024 * 2) == 16                                                 # ... K = 1024 keeps 16
    assert TW.nt_group_size(16, 256 * 4096 * 2) == 4                                                 # the 8 MiB cap
    assert TW.nt_group_size(4, 8 << 20) == 2 and TW.nt_group_size(4, 0) == 16                        # floor of 2; no division by zero


@pytest.mark.parametrize("cus", [8, 64, 104, 228, 256, 304])
@pytest.mark.parametrize("shape", [TW.SHAPES["S1"], TW.SHAPES["S2"], TW.SHAPES["S3"], TW.RAGGED_BF16, TW.RAGGED_F8, (256, 256, 512)])
def test_walk_is_a_permutation_on_other_parts(shape, cus):
    for bpe in (1, 2):
        _all_tiles_once(TW.walk(*shape, bpe, cus))


@pytest.mark.parametrize("gm", [1, 2, 5, 16])
def test_group_override_only_reorders(gm):
    """The tile-group override the GPU test sweeps on S1: another order of the same tiles."""
    w = TW.walk(*TW.SHAPES["S1"], 2, CUS, gm=gm)
    _all_tiles_once(w)
    assert w.gm == gm and TW.tiles_per_workgroup(w) == {3: 91, 2: 165}
    if gm != 16:
        assert w.workgroups != TW.walk(*TW.SHAPES["S1"], 2, CUS).workgroups


# ---- the slice plan of clipa_gemm_tn and the (tile, slice) decode of gemm_tna (tests/tn_plan.py) -------------------------------
# case -> slice order, tiles R x C, S_plan, slices used, rows per slice, rows of the last slice, nloop, nloop of the last slice,
# grid, idle workgroups
TN_TABLE = {
    "A": (True, (3, 3), 56, 32, 256, 256, 0, 0, (288, 1), 0),
    "B": (True, (3, 3), 56, 33, 256, 256, 0, 0, (360, 1), 63),
    "C": (True, (3, 3), 56, 43, 384, 256, 1, 0, (432, 1), 45),
    "D": (False, (2, 6), 64, 48, 256, 256, 0, 0, (12, 48), 0),
    "E": (False, (1, 5), 43, 43, 384, 256, 1, 0, (5, 43), 0),
    "F": (True, (2, 1), 64, 52, 640, 384, 3, 1, (112, 1), 8),
}
TN_OTHER = [(1000, 264, 136), (130, 8, 2304), (8, 16, 16), (64, 256, 256), (4100, 1024, 512), (70000, 520, 264), (70000, 136, 72),
            (806912, 256, 256), (806912, 1024, 3072)]


def _library_slices(M, R, C):
    from clipa_amd import lib
    ns = ctypes.c_int64(-1)
    nbytes = lib.load().clipa_gemm_tn_workspace(M, R, C, ctypes.byref(ns))
    assert nbytes == ns.value * (R * C + R) * 4
    return ns.value


@pytest.mark.parametrize("shape", list(TP.CASES.values()) + TP.NEIGHBOURS + TP.PRODUCTION + TN_OTHER, ids=lambda s: "x".join(map(str, s)))
def test_tn_plan_slice_count_is_the_librarys(shape):
    """Without a device clipa_gemm_tn_workspace prices a shape for 256 CUs: the restated tn_per_xcd / tn_slices give the same
    count, for the case shapes, their non-eligible neighbours, the production weight gradients and the shapes of test_gemm_tn."""
    assert TP.plan(*shape, CUS).S_plan == _library_slices(*shape)


def test_tn_plan_production_shapes_reach_gemm_tna():
    """Every block weight gradient of the production configuration is a gemm_tna launch, in both orders, with a short last slice
    on the square one - what the small cases stand in for."""
    plans = {s: TP.plan(*s, CUS) for s in TP.PRODUCTION}
    assert all(pl.kernel == TP.TNA for pl in plans.values())
    assert {s[1:] for s, pl in plans.items() if not pl.per_xcd} == {(1024, 4096), (768, 3072)}          # c_proj: tile order
    sq = plans[(806912, 1024, 1024)]
    assert (sq.nslices, sq.slice_rows, sq.last_rows) == (48, 16896, 12800)
    one = TP.plan(806912, 256, 256, CUS)                         # test_gemm_tn_production_rows: ONE tile, no idle workgroup
    assert (one.tiles, one.nslices, one.slice_rows, one.last_rows, one.idle) == (1, 64, 12672, 8576, 0)


@pytest.mark.parametrize("case", list(TN_TABLE))
def test_tn_case_table(case):
    """The GPU cases have the features they are there for at 256 CUs (tn_plan.CASES)."""
    M, R, C = TP.CASES[case]
    per_xcd, tiles, s_plan, used, rows, last, nloop, nloop_last, grid, idle = TN_TABLE[case]
    pl = TP.plan(M, R, C, CUS)
    assert pl.kernel == TP.TNA
    assert (pl.per_xcd, (pl.tiles_r, pl.tiles_c), pl.S_plan, pl.nslices, pl.slice_rows, pl.last_rows, pl.nloop, pl.nloop_last,
            pl.grid, pl.idle) == (per_xcd, tiles, s_plan, used, rows, last, nloop, nloop_last, grid, idle)
    assert pl.tiles > 1 and pl.tiles_c > 1 or case == "F"        # a tile with tc != 0: no column sums from it
    assert (M - pl.last_rows) == (pl.nslices - 1) * pl.slice_rows and pl.last_rows % 128 == 0 and pl.last_rows >= 256
    assert 16 * M < 2 ** 20                                      # the exact operands' partial sums stay integers in fp32
    if case in "AB":
        assert pl.nslices < pl.S_plan                            # column-sum partials behind slab S_used, not S_plan
    if case == "D":
        assert pl.tiles & 7 == 4                                 # xcd_remap with a remainder
    if case == "E":
        assert pl.tiles < 8                                      # XCDs without a tile


def test_tn_neighbours_are_not_eligible():
    """One step outside tna_eligible in each direction: the launcher keeps gemm_tn2."""
    for shape in TP.NEIGHBOURS:
        assert TP.plan(*shape, CUS).kernel == TP.TN2, shape
    M, R, C = TP.NEIGHBOURS[0]
    assert M % 256 == 128 and TP.tna_eligible(M - 128, R, C, 256) and not TP.tna_eligible(M, R, C, 256)   # a 128-row last slice
    assert TP.NEIGHBOURS[1][0] % 128 == 64 and TP.NEIGHBOURS[2][2] % 256 != 0
    assert not TP.tna_eligible(4096, 768, 768, 128) and TP.tna_eligible(4096, 768, 768, 256)
    assert TP.plan(4096, 768, 768, CUS).slice_rows == 128       # 64 K steps over 56 slices: 128-row slices


def _decode_covers(pl, M):
    seen, idle = [], 0
    for by in range(pl.grid[1]):
        for bx in range(pl.grid[0]):
            d = TP.decode(pl, bx, by)
            if d is None:
                idle += 1
            else:
                seen.append(d)
    assert sorted(seen) == [(tr, tc, s) for tr in range(pl.tiles_r) for tc in range(pl.tiles_c) for s in range(pl.nslices)]
    assert idle == pl.idle == pl.grid[0] * pl.grid[1] - pl.tiles * pl.nslices
    rows = [TP.slice_rows_of(pl, M, s) for s in range(pl.nslices)]
    assert rows[0][0] == 0 and rows[-1][1] == M and all(a[1] == b[0] for a, b in zip(rows, rows[1:]))
    assert all((e - b) % 128 == 0 and e - b >= 256 for b, e in rows)


@pytest.mark.parametrize("flags", [0, TP.FORCE_SLICE_ORDER, TP.FORCE_TILE_ORDER])
@pytest.mark.parametrize("shape", list(TP.CASES.values()) + TP.PRODUCTION + [(806912, 256, 256)], ids=lambda s: "x".join(map(str, s)))
def test_tna_decode_visits_every_tile_and_slice_once(shape, flags):
    """In both work orders every (tile row, tile column, slice) is computed by exactly one workgroup, every other workgroup of the
    grid is one that returns, and the slices partition the rows of M into whole pairs of K steps."""
    pl = TP.plan(*shape, CUS, flags)
    assert pl.kernel == TP.TNA and pl.per_xcd == (TP.tn_per_xcd(*shape) if not flags else flags == TP.FORCE_SLICE_ORDER)
    _decode_covers(pl, shape[0])


@pytest.mark.parametrize("cus", [8, 64, 104, 228, 304])
def test_tna_decode_on_other_parts(cus):
    for shape in TP.CASES.values():
        for flags in (0, TP.FORCE_SLICE_ORDER, TP.FORCE_TILE_ORDER):
            pl = TP.plan(*shape, cus, flags)
            if pl.kernel == TP.TNA:
                _decode_covers(pl, shape[0])


def test_xcd_remap_is_a_bijection():
    for n in (1, 5, 7, 8, 12, 36, 64, 603):
        assert sorted(TP.xcd_remap(b, n) for b in range(n)) == list(range(n))
