"""The slice plan of the bf16 weight-gradient GEMM (clipa_gemm_tn) and the workgroup decode of its four-wave kernel (gemm_tna),
restated once in plain Python for the tests that need to know how many slices a shape gets, which kernel takes it and which
workgroup computes which (tile, slice): tests/test_tile_walk_cpu.py and the "gemm_tna across tiles and slices" section of
tests/test_kernels_gpu.py.  A shared module like tests/tile_walk.py: no test lives here.  Each piece cites the lines of the
library it restates; a change there has to be repeated here, and test_tile_walk_cpu.py then says which property of the case
shapes moved."""
from collections import namedtuple

TILE = 256                         # clipa_amd/csrc/gemm_common.h:10 (BM = BN)
KSTEP = 64                         # rows of M per K step (gemm_tna.hip:54)

# experiment flags of lib.debug_set(0, flags) that the launcher reads (gemm_tn.hip:392-395, 472, 478, 486)
FORCE_TN3, FORCE_TN2, FORCE_SLICE_ORDER, FORCE_TILE_ORDER, NO_TNA, SCHEDULE_1 = 1024, 2048, 4096, 8192, 16384, 32768
TN2, TN3, TNA = 3, 4, 5            # kernel families of lib.last_gemm() / lib.gemm_counts()

# The smallest whole-tile shapes with each feature of the (tile, slice) decode and of the slice lengths, and what they are
# there for (the table of test_tile_walk_cpu.py, at 256 CUs):
#   A  3 x 3 tiles, slice order; 32 slices of 256 rows = the minimal main loop (nloop = 0); fewer slices (32) than the workspace
#      was sized for (56): the column-sum partials sit behind slab 32, not 56
#   B  33 slices: the grid is rounded up to 40 and 63 workgroups return without writing
#   C  384-row slices (nloop = 1), a SHORT last slice of 256 rows, 43 slices and 45 idle workgroups
#   D  tile order: 2 x 6 tiles through xcd_remap with remainder 4, blockIdx.y is the slice
#   E  tile order: 5 tiles (fewer than the XCDs), 384-row slices with a 256-row last one
#   F  R > C; 640-row slices (nloop = 3), last slice 384 rows (nloop = 1), 52 slices and 8 idle workgroups
CASES = {"A": (8192, 768, 768), "B": (8448, 768, 768), "C": (16384, 768, 768), "D": (12288, 512, 1536),
         "E": (16384, 256, 1280), "F": (33024, 512, 256)}
# Neighbours of case A just outside tna_eligible: a 128-row last slice, M no multiple of 128, a partial tile, 128-row slices
NEIGHBOURS = [(8320, 768, 768), (8256, 768, 768), (8192, 768, 760), (4096, 768, 768)]
# The block weight gradients of the production configurations (ViT-L/16 @ 224 and its 12-layer text tower at local batch 4096:
# 197 x 4096 and 77 x 4096 rows), P x Q widths of in-proj, out-proj, c_fc, c_proj
PRODUCTION = ([(806912, r, c) for r, c in ((3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096))]
              + [(315392, r, c) for r, c in ((2304, 768), (768, 768), (3072, 768), (768, 3072))])


def tn_per_xcd(M, R, C, flags=0):
    """gemm_tn.hip:392-398 (tn_per_xcd): True = slice-per-XCD order, False = tile order."""
    if flags & FORCE_SLICE_ORDER:
        return True
    if flags & FORCE_TILE_ORDER:
        return False
    return not C >= 3 * R


def tn_slices(M, R, C, num_cu, per_xcd):
    """gemm_tn.hip:400-430 (tn_slices): the slice count the workspace is sized for (S_plan)."""
    tiles = -(-R // TILE) * -(-C // TILE)
    mt = -(-M // KSTEP)
    if per_xcd:
        cu_x = max(num_cu // 8, 1)
        best, best_fill = 1, -1.0
        for k in range(1, 9):
            w = k * tiles
            rounds = -(-w // cu_x)
            if 8 * k > mt:
                break
            fill = w / (rounds * cu_x)
            score = fill - (0.15 * (3 - rounds) if rounds < 3 else 0.0) - (0.02 * (rounds - 8) if rounds > 8 else 0.0)
            if score > best_fill + 1e-9:
                best_fill, best = score, k
        return 8 * best
    S = max(min(4 * num_cu // tiles, 64), 1)
    for c in range(S, 0, -1):
        w = tiles * c
        rounds = -(-w // num_cu)
        full = w * 100 >= rounds * num_cu * 97
        if full or c == 1:
            if full:
                S = c
            break
    S = max(min(S, mt), 1)
    if mt > 0:
        per = -(-mt // S)
        S = -(-mt // per)
    return S


def tna_eligible(M, R, C, slice_rows):
    """gemm_tna.hip:126-130 (tna_eligible): whole tiles, slices of an even number (>= 4) of K steps, the last one included."""
    if R % TILE or C % TILE or M % 128 or slice_rows % 128 or slice_rows < 256:
        return False
    last = M % slice_rows
    return last == 0 or last >= 256


Plan = namedtuple("Plan", "per_xcd S_plan kernel slice_rows nslices tiles_r tiles_c tiles grid last_rows nloop nloop_last idle")


def plan(M, R, C, num_cu, flags=0):
    """clipa_gemm_tn (gemm_tn.hip:453-498) -> Plan: S_plan = the slice count clipa_gemm_tn_workspace reports, kernel = the family
    that runs (TNA / TN3 / TN2), slice_rows / nslices = what that kernel is launched with (S_used), grid = (x, y); for gemm_tna
    also last_rows = rows of the last slice, nloop(_last) = main-loop trips of a full (the last) slice (gemm_tna.hip:54, 82) and
    idle = the workgroups of the grid that return at once."""
    per_xcd = tn_per_xcd(M, R, C, flags)
    S_plan = tn_slices(M, R, C, num_cu, per_xcd)
    mt = -(-M // KSTEP)
    slice_rows = -(-mt // S_plan) * KSTEP                                # gemm_tn.hip:458-459
    tiles_r, tiles_c = -(-R // TILE), -(-C // TILE)
    tiles = tiles_r * tiles_c
    if not flags & (NO_TNA | FORCE_TN3 | FORCE_TN2):                      # gemm_tn.hip:478-491
        rows4 = -(-slice_rows // 128) * 128                               # slices rounded up to 128 rows
        S4 = -(-M // rows4)
        if S4 <= S_plan and tna_eligible(M, R, C, rows4):
            grid = (tiles * (-(-S4 // 8) * 8), 1) if per_xcd else (tiles, S4)          # slice order: rounded up to 8 slices
            last = M - (S4 - 1) * rows4
            return Plan(per_xcd, S_plan, TNA, rows4, S4, tiles_r, tiles_c, tiles, grid, last, rows4 // KSTEP // 2 - 2,
                        last // KSTEP // 2 - 2, grid[0] * grid[1] - tiles * S4)
    v3 = bool(flags & FORCE_TN3) or (not flags & FORCE_TN2 and ((R >= 3072 and C >= 1024) or (R == 1024 and C == 1024)))   # gemm_tn.hip:472
    grid = (tiles * S_plan, 1) if per_xcd else (tiles, S_plan)           # gemm_tn.hip:493
    return Plan(per_xcd, S_plan, TN3 if v3 else TN2, slice_rows, S_plan, tiles_r, tiles_c, tiles, grid, None, None, None, 0)


def xcd_remap(bid, nwg):
    """common.h:239-244 (xcd_remap): block b runs on XCD b % 8; every XCD gets a contiguous chunk of the tile sequence."""
    q, r = nwg >> 3, nwg & 7
    xcd, idx = bid & 7, bid >> 3
    base = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return base + idx


def decode(pl, bx, by=0):
    """gemm_tna.hip:38-51: workgroup (blockIdx.x, blockIdx.y) of a gemm_tna launch -> (tile row, tile column, slice), or None for
    a workgroup that returns (slice order: a slice of the rounded-up grid that does not exist)."""
    if pl.per_xcd:                                                        # p.nslices > 0
        xcd, j = bx & 7, bx >> 3
        sl, t = xcd + 8 * (j // pl.tiles), j % pl.tiles
        if sl >= pl.nslices:
            return None
    else:
        t, sl = xcd_remap(bx, pl.tiles), by
    tr = t // pl.tiles_c
    return tr, t - tr * pl.tiles_c, sl


def slice_rows_of(pl, M, sl):
    """gemm_tna.hip:52-53: rows [mbeg, mend) of slice sl."""
    mbeg = sl * pl.slice_rows
    return mbeg, min(M, mbeg + pl.slice_rows)


def require(cond, case, what, pl):
    """The GPU tests' guard: loud, not silently empty, on a part whose CU count gives a case shape another plan."""
    assert cond, f"case {case}: {what} - on this part the plan is {pl}; the test no longer reaches what it is there for"
