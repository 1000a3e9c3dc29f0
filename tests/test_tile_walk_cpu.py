"""The restated tile walk of the persistent NT GEMMs (tests/tile_walk.py) at 256 CUs (an MI355X): it visits every tile exactly
once, and the shapes of the multi-tile GPU tests have the properties those tests are built on - a workgroup that runs a second
and a third tile, a ragged last group, a tile count that is no multiple of the 8 XCDs, each branch of nt_group_size."""
import pytest

from . import tile_walk as TW

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
