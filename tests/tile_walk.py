"""The tile walk of the persistent NT GEMM kernels (gemm_nta, gemm_f8a, gemm_nt2, gemm_nt_f8_kernel), restated once in plain
Python for the tests that need to know which workgroup runs which tile in which order (tests/test_tile_walk_cpu.py, the
multi-tile tests of tests/test_kernels_gpu.py and tests/test_fp8_gpu.py).  A shared module like tests/glue_cases.py: no
test lives here.  Each piece cites the lines of the library it restates; a change there has to be repeated here, and
test_tile_walk_cpu.py then says which property of the test shapes moved."""
from collections import namedtuple

BM = BN = 256                      # clipa_amd/csrc/gemm_common.h:10

# The whole-tile shapes of the multi-tile tests and what they are there for (the table of test_tile_walk_cpu.py, at 256 CUs):
#   S1  603 tiles: three tiles on 91 workgroups, two on the rest; ragged last group, ntiles % 8 != 0; K = 512 is gemm_f8a's
#       shortest tile (nloop = 0: the prologue and the two cross-tile steps only)
#   S2  260 tiles: four workgroups go on to a second tile, 252 stop after one; tilesN > 12 -> groups of 8; K = 1280 (ViT-H)
#   S3  260 tiles: the tilesN == 4 branch of nt_group_size for both element sizes, long K
#   S0  control: 12 tiles, one per workgroup (what the small-shape tests run)
SHAPES = {"S1": (17152, 2304, 512), "S2": (3328, 5120, 1280), "S3": (16640, 1024, 4096), "S0": (1024, 768, 512)}
# Ragged shapes with more than 256 tiles for the kernels that take any shape (gemm_nt2 / gemm_nt_f8_kernel)
RAGGED_BF16 = (17000, 2296, 520)
RAGGED_F8 = (17000, 2296, 528)


def nt_group_size(tiles_n, panel_bytes):
    """clipa_amd/csrc/gemm_common.h:35-42 (nt_group_size): A panels per tile group."""
    pb = panel_bytes if panel_bytes > 0 else 1
    if tiles_n == 4 and pb >= (1 << 20) and 8 * pb <= (16 << 20):
        return 8
    want = 16 if tiles_n <= 12 else 8
    cap = (8 << 20) // pb
    g = min(want, cap)
    return max(g, 2)


def persistent_grid(tiles, num_cu):
    """clipa_amd/csrc/gemm_4w.h:129-132 (persistent_grid); gemm_nt.hip:398-408 and gemm_f8.hip:305-306 launch the generic kernels
    with the same rule on the rounded-up tile counts."""
    return min(tiles, num_cu)


def tile_origin(t, gm_arg, tiles_m, tiles_n):
    """gemm_nta.hip:170-178 = gemm_f8a.hip:172-180 = gemm_nt.hip:83-91 (tile_origin): position t of the walk -> (M panel, N tile).
    Groups of gm_arg panels, N-tile major inside a group; the last group may hold fewer panels."""
    per = gm_arg * tiles_n
    g, r = divmod(t, per)
    gm = min(gm_arg, tiles_m - g * gm_arg)
    tn, mm = divmod(r, gm)
    return g * gm_arg + mm, tn


Walk = namedtuple("Walk", "tiles_m tiles_n ntiles gm grid workgroups ntiles_mod8 tiles_m_mod_gm")


def walk(M, N, K, bytes_per_element, num_cu, gm=None):
    """-> Walk: for every workgroup (block index order) the (M panel, N tile) pairs it computes, in order, and the figures the
    tests state about a shape.  bytes_per_element: 2 = bf16 (gemm_nt.hip:387), 1 = fp8 (gemm_f8.hip:292).  gm: the tile-group
    override of clipa_internal_debug_set flag bits 20..25 (gemm_nt.hip:388)."""
    tiles_m, tiles_n = -(-M // BM), -(-N // BN)
    ntiles = tiles_m * tiles_n
    if gm is None:
        gm = nt_group_size(tiles_n, 256 * K * bytes_per_element)
    G = persistent_grid(ntiles, num_cu)
    q8, r8 = ntiles >> 3, ntiles & 7
    workgroups = []
    for block in range(G):
        # gemm_nta.hip:165-169 = gemm_f8a.hip:167-171 = gemm_nt.hip:59-63: XCD x owns the range [base, base + len) of the walk, its
        # gx workgroups take every gx-th position of it (gemm_nta.hip:227-229, 242-244, 287-288: it = idx, it += gx while it < len)
        xcd, idx = block & 7, block >> 3
        gx = (G - xcd + 7) >> 3
        base = xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8
        ln = q8 + (1 if xcd < r8 else 0)
        workgroups.append([tile_origin(base + it, gm, tiles_m, tiles_n) for it in range(idx, ln, gx)])
    return Walk(tiles_m, tiles_n, ntiles, gm, G, workgroups, ntiles % 8, tiles_m % gm)


def tile_factors(count, stride, period):
    """Operand magnitudes that depend on the tile: factor i of `count` (an M panel or an N tile) = 10^-(i stride mod period) / (period - 1),
    one decade from 1 down to 0.1, neighbours far apart (stride and period coprime).  A's rows carry the factor of their panel,
    B's rows and the bias that of their N tile: the output tiles span two decades, and a tile computed from another tile's
    operands, bias or scale vectors is wrong by a factor, not within a tolerance."""
    return [10.0 ** (-((i * stride) % period) / (period - 1.0)) for i in range(count)]


def tiles_per_workgroup(w):
    """-> {tiles: number of workgroups that run that many}"""
    hist = {}
    for tiles in w.workgroups:
        hist[len(tiles)] = hist.get(len(tiles), 0) + 1
    return hist


def later_tiles(w):
    """The tiles that are not their workgroup's first: what runs after a tile transition."""
    return [t for tiles in w.workgroups for t in tiles[1:]]


def require_second_tiles(w, what):
    """The GPU tests' guard: loud, not silently empty, on a part with so many CUs that no workgroup gets a second tile."""
    n = len(later_tiles(w))
    assert n > 0, f"{what}: {w.ntiles} tiles on {w.grid} workgroups - no workgroup runs a second tile, the test checks no tile transition"
    return n


def panels_to_check(w, at_least=8):
    """M panels whose full rows an fp64 check of a long shape looks at: the first and the last panel, every panel holding a tile
    that is not its workgroup's first, filled up to `at_least` with evenly spaced ones."""
    panels = {0, w.tiles_m - 1} | {m for m, _ in later_tiles(w)}
    step = max(1, w.tiles_m // at_least)
    for m in range(0, w.tiles_m, step):
        if len(panels) >= at_least:
            break
        panels.add(m)
    return sorted(panels)
