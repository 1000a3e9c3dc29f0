"""TEST INFRASTRUCTURE: the case table of the HBM-bound "glue" kernels (clipa_amd/csrc/misc.hip) and of the optimizer /
gradient-exchange kernels (clipa_amd/csrc/runtime.hip), shared by tests/test_glue_kernels_gpu.py (clipa_amd.ops on the
device) and tests/test_glue_standins_cpu.py (tests/cpu_ops, the torch stand-ins the CPU and gloo suites stand on).

For every operation: a list of named cases (each name says which branch of the launch code the case exists for) and a
`check_<op>(o, dev, case, ...)` that builds the seeded inputs on the CPU, runs them through the ops module `o` on `dev`
and compares with a plain-torch CPU reference.  No fixtures, no global state, only seeded torch.Generator inputs.

Two kinds of input carry the work:
  * EXACT-SUM inputs for every reduction: small integers times a power of two, chosen so that every partial sum in any
    order is an integer number of quanta below 2^24 and therefore exact in fp32.  The fp32 result then does not depend
    on the summation order, the reference is the fp64 sum and the comparison is torch.equal: a dropped, duplicated or
    misplaced element moves the result by at least one quantum.  The bound is stated next to each case list.
  * POSITION-CODED inputs for every pure data movement: element (r, c) holds bf16 bit pattern number (131 r + c + salt)
    mod P of an enumeration of P distinct finite bf16 bit patterns (`coded`), compared bit for bit.
One rounding of an fp32 value to bf16 is round-to-nearest-even and `tensor.to(torch.bfloat16)` reproduces it bit for bit.
A tolerance appears only where the device's own sqrt / division enters (l2norm, clip_coef, AdamW); they are the ones
tests/test_kernels_gpu.py already uses (TOL_* below) against fp64 references.
"""
import math

import torch

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
POOL_FIRST, POOL_LAST, POOL_INDEX, POOL_MEAN_ALL, POOL_MEAN_PATCH = 0, 1, 2, 3, 4

TOL_L2_FWD = (1e-6, 1e-6)            # (rtol, atol): test_kernels_gpu "l2norm"
TOL_L2_BWD = (1e-5, 1e-5)            # "l2norm bwd"
TOL_ADAMW = {f32: (2e-6, 1e-6), bf16: (2 ** -7, 1e-6)}      # f32 / bf16 parameters


class Case:
    def __init__(self, name, **kw):
        self.name = name
        self.__dict__.update(kw)

    def __repr__(self):
        return self.name


def names(cases):
    return [c.name for c in cases]


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def _patterns(idx, emin, emax):
    """int64 pattern numbers -> bf16: number p of the P = 2 * (emax - emin + 1) * 128 bit patterns sign | exponent field
    in [emin, emax] | 7 mantissa bits - all finite, normal, non-zero and distinct (a lookup of bit patterns, no float
    arithmetic)."""
    per = (emax - emin + 1) * 128
    p = idx % (2 * per)
    bits = (p // per) * 32768 + (p % per) + emin * 128
    bits -= (bits >= 32768) * 65536
    return bits.to(torch.int16).view(bf16)


def coded(rows, cols, salt=0, emin=1, emax=254):
    """Position-coded bf16 [rows, cols].  131 is prime to P, so two elements hold the same pattern only if
    131 (r - r') + (c - c') = 0 mod P: never within a row shorter than P, never between rows closer than P / 131 apart in
    the same column, which no row- or column-misplacement of these kernels can produce."""
    assert rows * 131 + cols + salt < 2 ** 31
    r = torch.arange(rows, dtype=torch.int32)[:, None]
    c = torch.arange(cols, dtype=torch.int32)[None, :]
    return _patterns(r * 131 + c + salt, emin, emax)


def coded_flat(n, salt=0, emin=1, emax=254):
    """Position-coded flat bf16 [n]: the pattern number advances by one per element and by 7 more per period."""
    i = torch.arange(n, dtype=torch.int32)
    return _patterns(i + (i // (2 * (emax - emin + 1) * 128)) * 7 + salt, emin, emax)


def spread_f32(t, seed):
    """f32 values whose rounding to bf16 matters: the bf16 tensor times (1 + k 2^-9), k in {-1, 0, 1, 3} - exact in fp32
    (8 x 11 significant bits); k = +-1 / 3 land exactly half way between two bf16 values for even / odd mantissas."""
    k = torch.tensor([-1.0, 0.0, 1.0, 3.0])[torch.randint(0, 4, t.shape, generator=gen(seed))]
    return t.float() * (1.0 + k * 2.0 ** -9)


def ints(shape, seed, amax, shift=0, dtype=bf16):
    """Exact-sum input: integers in [-amax, amax] times 2^-shift (exact in bf16 for amax <= 256)."""
    v = torch.randint(-amax, amax + 1, shape, generator=gen(seed), dtype=torch.int8 if amax < 128 else torch.int64)
    return v.to(dtype) * 2.0 ** -shift


def gauss(shape, seed, scale=1.0, dtype=f32):
    return (torch.randn(shape, generator=gen(seed)) * scale).to(dtype)


def token_ids(B, T, V, seed):
    """Realistic captions: SOT = V - 2, a random body, one EOT = V - 1 (the row maximum) at a random position, pad id 0
    after it -> (ids int64 [B, T], eot positions [B])."""
    g = gen(seed)
    ids = torch.randint(1, V - 2, (B, T), generator=g)
    eot = torch.randint(1, T, (B,), generator=g)
    ids[:, 0] = V - 2
    t = torch.arange(T)[None, :]
    ids[t == eot[:, None]] = V - 1
    ids[t > eot[:, None]] = 0
    return ids, eot


# ---- comparisons ----------------------------------------------------------------------------------------------------
def _where(bad, shape):
    i = int(torch.nonzero(bad.reshape(-1))[0])
    idx = []
    for s in reversed(shape):
        idx.append(i % s)
        i //= s
    return tuple(reversed(idx))


def same(name, got, ref):
    """torch.equal over the whole output (same dtype and shape); the first mismatch is named on failure."""
    got = got.detach().cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{name}: {got.dtype} {tuple(got.shape)} vs {ref.dtype} {tuple(ref.shape)}"
    if ref.is_floating_point() and ref.isnan().any():      # NaN where and only where the reference has one, equal elsewhere
        assert torch.equal(got.isnan(), ref.isnan()), f"{name}: NaN pattern differs from the reference"
        got, ref = got.nan_to_num(nan=0.0), ref.nan_to_num(nan=0.0)
    if not torch.equal(got, ref):
        bad = ~((got == ref) | (got.isnan() & ref.isnan())) if got.is_floating_point() else got != ref
        at = _where(bad, got.shape) if bad.any() else ()
        raise AssertionError(f"{name}: {int(bad.sum())}/{got.numel()} elements differ; first at {at}: got "
                             f"{got[at].item()!r} ref {ref[at].item()!r}")


def same_bits(name, got, ref, nan_as_one=False):
    """Bit-for-bit equality (torch.equal of the integer views): -0 != +0, NaN payloads count.  nan_as_one: every NaN
    pattern is first replaced by the canonical one (a conversion may quiet a NaN, it must stay a NaN)."""
    got = got.detach().cpu().contiguous()
    ref = ref.contiguous()
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{name}: {got.dtype} {tuple(got.shape)} vs {ref.dtype} {tuple(ref.shape)}"
    if nan_as_one:
        got = torch.where(got.isnan(), torch.full_like(got, float("nan")), got)
        ref = torch.where(ref.isnan(), torch.full_like(ref, float("nan")), ref)
    it = torch.int16 if got.element_size() == 2 else torch.int32
    same(name + " (bits)", got.view(it), ref.view(it))


def close(name, got, ref, tol):
    """|got - ref| <= atol + rtol |ref| against an fp64 reference; got must be finite wherever ref is."""
    rtol, atol = tol
    got = got.detach().cpu().double()
    ref = ref.double()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    fin = ref.isfinite()
    assert torch.equal(got.isfinite(), fin), f"{name}: finite / non-finite pattern differs from the reference"
    err = torch.where(fin, (got - ref).abs(), torch.zeros_like(ref))
    lim = torch.where(fin, atol + rtol * ref.abs(), torch.ones_like(ref))
    bad = err > lim
    if bad.any():
        at = _where(bad, got.shape)
        raise AssertionError(f"{name}: {int(bad.sum())}/{got.numel()} outside tol; first at {at}: got {got[at].item():.9g} "
                             f"ref {ref[at].item():.9g}")


def poison(shape, dtype, dev):
    """Fill and release a buffer of the size the next output has: a caching allocator hands the same block to the op's
    torch.empty, so an element the kernel forgets to write shows a recognisable value, not a lucky zero."""
    if dev != "cpu":
        t = torch.full(shape, 1.75, dtype=dtype, device=dev)
        del t


def sum64(x, dim=0, chunk=8192):
    """fp64 sum over `dim` (0 or 1) of a big tensor, in slabs so that the fp64 copy stays small."""
    out = None
    for s in range(0, x.shape[dim], chunk):
        part = x.narrow(dim, s, min(chunk, x.shape[dim] - s)).double().sum(dim)
        out = part if out is None else out + part
    return out


# ---- assemble_tokens / assemble_tokens_bwd ---------------------------------------------------------------------------
def assemble_chunks(B, L, D):
    """(nchunk, bchunk) of clipa_assemble_tokens_bwd: misc.hip assemble_bwd_chunks."""
    threads = L * (D // 8)
    nc = max(1, min(B, (4096 * 256 + threads - 1) // threads))
    bc = (B + nc - 1) // nc
    return (B + bc - 1) // bc, bc


_ASM_SHAPES = [(100, 197, 1024, "chunks_of_3_short_last"),     # ViT-L/16 tokens: 34 chunks of 3, the last holds 1
               (64, 257, 1280, "chunks_of_3_short_last_vit_h"),  # ViT-H/14: 22 chunks of 3, the last holds 1
               (37, 50, 768, "one_image_per_chunk"),             # nchunk == B, bchunk == 1
               (1, 197, 1024, "single_image"),                   # one chunk of one
               (5, 10, 128, "toy")]
ASSEMBLE = [Case(f"B{B}_L{L}_D{D}_{why}", B=B, L=L, D=D) for B, L, D, why in _ASM_SHAPES]
# exact: |dtok| <= 8 in quanta of 2^-2 -> |any partial sum| <= 32 B <= 3200 quanta < 2^24
ASSEMBLE_BWD = [Case(f"{c.name}_{'pos' if p else 'nopos'}", B=c.B, L=c.L, D=c.D, need_pos=p, chunked=c.B in (100, 64))
                for c in ASSEMBLE for p in (True, False)]


def check_assemble_tokens(o, dev, c):
    B, L, D = c.B, c.L, c.D
    patch = coded(B * (L - 1), D, salt=3, emin=110, emax=135)            # 2^-17 .. 2^9
    cls, pos = gauss(D, 11), gauss((L, D), 12)
    tok = o.assemble_tokens(patch.to(dev), cls.to(dev), pos.to(dev), B, L)
    x = torch.cat([cls.to(bf16).float().expand(B, 1, D), patch.float().reshape(B, L - 1, D)], 1) + pos.to(bf16).float()
    same_bits("tokens", tok, x.reshape(B * L, D).to(bf16))              # fp32 add of two bf16 values, one rounding


def check_assemble_tokens_bwd(o, dev, c, query=None):
    B, L, D = c.B, c.L, c.D
    nchunk, bchunk = assemble_chunks(B, L, D)
    if query is not None:
        assert query("clipa_assemble_tokens_bwd_workspace", B, L, D) == nchunk * L * D * 4, "chunk heuristic changed: re-derive the cases"
    if c.chunked:       # the in-chunk batch loop runs more than once and the last chunk is short
        assert 1 < nchunk < B and bchunk > 1 and B % bchunk != 0, (nchunk, bchunk)
    else:
        assert nchunk == B and bchunk == 1
    # data movement: position-coded rows (the sums of these are not looked at)
    dtok = coded(B * L, D, salt=5)
    poison((B * (L - 1), D), bf16, dev)
    dpatch, _, _ = o.assemble_tokens_bwd(dtok.to(dev), B, L, need_pos=c.need_pos)
    same_bits("dpatch", dpatch, dtok.reshape(B, L, D)[:, 1:].reshape(-1, D))
    del dpatch
    # reductions: exact-sum input
    dtok = ints((B * L, D), 21, 8, 2)
    d3 = dtok.double().reshape(B, L, D)
    dp, dcls, dpos = o.assemble_tokens_bwd(dtok.to(dev), B, L, need_pos=c.need_pos)
    same("dpatch", dp, dtok.reshape(B, L, D)[:, 1:].reshape(-1, D))
    same("dcls", dcls, d3[:, 0].sum(0).float())
    if c.need_pos:
        same("dpos", dpos, d3.sum(0).float())
    else:
        assert dpos is None
    _, dcls2, dpos2 = o.assemble_tokens_bwd(dtok.to(dev), B, L, need_pos=c.need_pos)
    same("dcls, second call", dcls2, dcls.cpu())
    if c.need_pos:
        same("dpos, second call", dpos2, dpos.cpu())
    # Gaussian data: each output is a chain of at most bchunk additions inside a chunk and nchunk across the chunks, each
    # off by at most 2^-24 of a partial sum <= sum |x|  ->  |error| <= (bchunk + nchunk) 2^-24 sum_b |x|
    dtok = gauss((B * L, D), 22, dtype=bf16)
    d3 = dtok.double().reshape(B, L, D)
    _, dcls, dpos = o.assemble_tokens_bwd(dtok.to(dev), B, L, need_pos=c.need_pos)
    bound = (bchunk + nchunk) * 2.0 ** -24 * d3.abs().sum(0)
    got = dpos.cpu().double() if c.need_pos else dcls.cpu().double()[None]
    ref = d3.sum(0) if c.need_pos else d3[:, 0].sum(0)[None]
    assert ((got - ref).abs() <= bound[:got.shape[0]]).all(), "Gaussian dpos / dcls outside the summation-order bound"


# ---- embed_tokens / embed_tokens_bwd / argmax_tokens ------------------------------------------------------------------
EMBED = [Case(f"B{B}_T{T}_D{D}_V{V}_{'bf16' if tb else 'f32'}_table", B=B, T=T, D=D, V=V, table_bf16=tb)
         for B, T, D, V in [(300, 77, 768, 49408), (64, 32, 384, 1000)] for tb in (False, True)]
EMBED_BWD = [Case(f"B{B}_T{T}_D{D}_V{V}", B=B, T=T, D=D, V=V) for B, T, D, V in [(300, 77, 768, 49408), (64, 32, 384, 1000)]]


def check_embed_tokens(o, dev, c):
    B, T, D, V = c.B, c.T, c.D, c.V
    ids, _ = token_ids(B, T, V, 31)
    table = coded(V, D, salt=7, emin=112, emax=130)                      # rows recognisable, 2^-15 .. 2^4
    if not c.table_bf16:
        table = spread_f32(table, 32)                                    # the table's own rounding to bf16 matters
    pos = gauss((T, D), 33, 0.01)
    out = o.embed_tokens(ids.to(dev), table.to(dev), pos.to(dev))
    ref = (table.to(bf16).float()[ids.reshape(-1)] + pos.to(bf16).float().repeat(B, 1)).to(bf16)
    same_bits("embedding", out, ref)
    if hasattr(o, "check_token_ids"):
        o.check_token_ids(wait=True)


def _dtable_ref(ids, dx, V):
    """fp64 scatter-add of the contract in embed_tokens_bwd_kernel, rounded once to fp32: finite elements beyond 2^17
    saturate, a table row that receives a non-finite element is NaN."""
    d = dx.double()
    ok = d.isfinite()
    d = torch.where(ok, d.clamp(-131072.0, 131072.0), torch.zeros_like(d))
    ref = torch.zeros(V, dx.shape[1], dtype=f64).index_add_(0, ids.reshape(-1), d).float()
    ref[ids.reshape(-1)[~ok.all(1)]] = float("nan")
    return ref


def check_embed_tokens_bwd(o, dev, c, query=None):
    B, T, D, V = c.B, c.T, c.D, c.V
    ids, eot = token_ids(B, T, V, 41)
    live = (torch.arange(T)[None, :] <= eot[:, None]).reshape(-1, 1)     # the rows after EOT carry no gradient
    nchunk, bchunk = assemble_chunks(B, T, D)
    if query is not None:
        assert query("clipa_embed_tokens_bwd_workspace", B, T, D, V, 0, 1) == nchunk * T * D * 4
    if B == 300:
        assert 1 < nchunk < B and bchunk > 1                             # dpos takes the chunked batch loop
    # (a) exact-sum rows: |dx| <= 8 quanta of 2^-2; at most B T rows meet in one table row / B in one position:
    #     |sum| <= 32 * 23100 quanta < 2^24, and < 2^19 in value as the fixed-point accumulator needs
    dx = ints((B * T, D), 42, 8, 2) * live
    dtable, dpos = o.embed_tokens_bwd(ids.to(dev), dx.to(dev), V)
    same("dtable (exact-sum rows)", dtable, _dtable_ref(ids, dx, V))
    same("dpos", dpos, dx.double().reshape(B, T, D).sum(0).float())
    dt2, dp2 = o.embed_tokens_bwd(ids.to(dev), dx.to(dev), V)
    same("dtable, second call", dt2, dtable.cpu())
    del dtable, dt2, dp2
    none_t, dpos = o.embed_tokens_bwd(ids.to(dev), dx.to(dev), V, need_table=False)
    assert none_t is None
    same("dpos without dtable", dpos, dx.double().reshape(B, T, D).sum(0).float())
    # (b) magnitudes 2^-12 .. 16 with full 8-bit mantissas: every value is a multiple of 2^-19 below 2^4, B T < 2^15
    #     of them sum to a multiple of 2^-19 below 2^19: 38 bits, exact in fp64 and in the 2^-44 fixed point, so dtable
    #     is the fp64 index_add_ rounded once to fp32
    g = gen(43)
    mag = 2.0 ** torch.randint(-12, 4, (B * T, D), generator=g).float() * (1.0 + torch.randint(0, 128, (B * T, D), generator=g).float() / 128.0)
    dx = (mag * (torch.randint(0, 2, (B * T, D), generator=g).float() * 2 - 1)).to(bf16) * live
    assert (dx.float().abs().max() < 16) and (dx.float().abs()[dx != 0].min() >= 2.0 ** -12)
    if c.B == 64:
        # saturation and non-finite rows: a body token of three different captions gets a reserved id
        rows = [1 * T + 1, 2 * T + 1, 3 * T + 1]
        ids = ids.clone()
        ids[(ids == 10) | (ids == 20) | (ids == 30)] = 11
        ids.view(-1)[rows] = torch.tensor([10, 20, 30])
        dx[rows[0], 5] = 2.0 ** 18                                       # lands as exactly 2^17 in table row 10
        dx[rows[1], 9] = float("inf")                                    # table rows 20 and 30 come out as NaN,
        dx[rows[2], 0] = float("nan")                                    # every other row is untouched
    dtable, none_p = o.embed_tokens_bwd(ids.to(dev), dx.to(dev), V, need_pos=False)
    assert none_p is None
    ref = _dtable_ref(ids, dx, V)
    same("dtable (fp64 index_add_, one rounding)", dtable, ref)
    if c.B == 64:
        nan_rows = set(torch.nonzero(dtable.cpu().isnan().any(1)).flatten().tolist())
        assert nan_rows == {20, 30} and bool(dtable.cpu()[[20, 30]].isnan().all())
        sat = dx[rows[0]].float()
        sat[5] = 131072.0
        same("the saturated row", dtable[10], sat)
    if hasattr(o, "check_token_ids"):
        o.check_token_ids(wait=True)


ARGMAX = [Case("B1_one_block_one_row", B=1), Case("B257_second_block_of_one", B=257), Case("B5000_many_blocks", B=5000)]


def check_argmax_tokens(o, dev, c):
    T, V = 77, 49408
    ids, eot = token_ids(c.B, T, V, 51)
    kind = (torch.arange(c.B) + 1) % 4               # row 0 (the only row of B = 1) gets repeated maxima
    for b in range(c.B):
        if kind[b] == 1 and eot[b] < T - 2:          # the maximum again after its first occurrence: the first wins
            ids[b, eot[b] + 2:] = V - 1
        elif kind[b] == 2:                           # maximum at t = 0 (and once more later)
            ids[b, 0] = V - 1
        elif kind[b] == 3:                           # strictly increasing: maximum at t = T - 1
            ids[b] = torch.arange(T) + 5
    if c.B == 1:
        ids[0, 3], ids[0, 40], ids[0, 76] = V - 1, V - 1, V - 1
        ids[0, :3] = 17
    top = ids.max(-1, keepdim=True).values
    first = torch.where(ids == top, torch.arange(T)[None, :], T).min(-1).values
    assert c.B == 1 or ((first == 0).any() and (first == T - 1).any() and ((ids == top).sum(-1) > 1).any())
    same("argmax", o.argmax_tokens(ids.to(dev)), first.to(torch.int32))


# ---- pooling --------------------------------------------------------------------------------------------------------
_POOL_MODES = {POOL_FIRST: "first", POOL_LAST: "last", POOL_INDEX: "index", POOL_MEAN_ALL: "mean_all", POOL_MEAN_PATCH: "mean_patch"}
# (300, 197, 1024): B D / 8 = 38400 work items = 150 blocks; (33, 257, 1280) ViT-H; (500, 77, 768) the text tower; toy.
# exact: |x| <= 8 quanta of 2^-3 -> |sum over L <= 257| <= 2056 quanta < 2^24; the mean is fp32(sum) * fp32(1.0f / n)
POOL = [Case(f"{nm}_B{B}_L{L}_D{D}", mode=m, B=B, L=L, D=D) for B, L, D in [(300, 197, 1024), (33, 257, 1280), (500, 77, 768), (5, 10, 128)]
        for m, nm in _POOL_MODES.items()]


def _pool_span(mode, L):
    return {POOL_FIRST: (0, 1), POOL_LAST: (L - 1, L), POOL_MEAN_ALL: (0, L), POOL_MEAN_PATCH: (1, L)}.get(mode)


def check_pool(o, dev, c):
    B, L, D, mode = c.B, c.L, c.D, c.mode
    idx = torch.randint(0, L, (B,), generator=gen(61)).to(torch.int32)
    idx[0], idx[1], idx[2] = 0, L - 1, L - 1                             # both ends of the sequence
    ii = idx.to(dev) if mode == POOL_INDEX else None
    x = ints((B * L, D), 62, 8, 3)
    x3 = x.reshape(B, L, D)
    span = _pool_span(mode, L)
    if mode == POOL_INDEX:
        ref, n = x3[torch.arange(B), idx.long()].float(), 1
    else:
        ref, n = x3[:, span[0]:span[1]].double().sum(1).float(), span[1] - span[0]
    sc = torch.ones((), dtype=f32) / torch.tensor(float(n), dtype=f32)   # 1.0f / (float)n
    same("pool_fwd", o.pool_fwd(x.to(dev), B, L, mode, ii), ref * sc)
    dout = gauss((B, D), 63)
    row = (dout * sc).to(bf16)                                           # dout * fp32(1 / n), one rounding
    ref = torch.zeros(B, L, D, dtype=bf16)
    if mode == POOL_INDEX:
        ref[torch.arange(B), idx.long()] = row
    else:
        ref[:, span[0]:span[1]] = row[:, None]
    poison((B * L, D), bf16, dev)
    same_bits("pool_bwd", o.pool_bwd(dout.to(dev), B, L, mode, ii), ref.reshape(B * L, D))


# ---- gather_rows / scatter_rows ----------------------------------------------------------------------------------------
_ROW_LISTS = ["keep_half_sorted", "permutation", "with_minus_one", "beyond_n_src", "empty", "single"]
# (12288, 1024): 4096 images of 3 tokens at ViT-L width; (1000, 1280): ViT-H width; (64, 8): one 16-byte piece per row
ROWS = [Case(f"{kind}_n{n}_D{D}", n=n, D=D, kind=kind, img=img) for n, D, img in [(4096 * 3, 1024, 3), (1000, 1280, 50), (64, 8, 16)]
        for kind in _ROW_LISTS]


def _row_list(c):
    g = gen(71)
    n, img = c.n, c.img
    if c.kind == "permutation":
        return torch.randperm(n, generator=g)
    if c.kind == "empty":
        return torch.zeros(0, dtype=torch.int64)
    if c.kind == "single":
        return torch.tensor([n - 1])
    keep = max(1, img // 2)                                              # the engine's keep plan: half the rows of each image, sorted
    order = torch.rand(n // img, img, generator=g).argsort(1)[:, :keep].sort(1).values
    rows = (order + torch.arange(n // img)[:, None] * img).reshape(-1)
    if c.kind == "with_minus_one":
        rows[torch.rand(rows.numel(), generator=g) < 0.2] = -1
        rows[0] = -1
    elif c.kind == "beyond_n_src":
        m = rows.numel()
        rows[0], rows[m // 2], rows[m - 1] = n, n + 5, 2 ** 40
    return rows


def check_rows(o, dev, c):
    n, D = c.n, c.D
    rows = _row_list(c)
    ok = (rows >= 0) & (rows < n)
    x = coded(n, D, salt=9)
    ref = torch.zeros(rows.numel(), D, dtype=bf16)
    ref[ok] = x[rows[ok]]
    poison((rows.numel(), D), bf16, dev)
    got = o.gather_rows(x.to(dev), rows.to(dev))
    same_bits("gather_rows", got, ref)                                   # a row index outside [0, n) gathers zeros
    dy = coded(rows.numel(), D, salt=1234)
    ref = torch.zeros(n, D, dtype=bf16)
    ref[rows[ok]] = dy[ok]
    poison((n, D), bf16, dev)
    same_bits("scatter_rows", o.scatter_rows(dy.to(dev), rows.to(dev), n), ref)    # ... and is skipped on scatter
    back = torch.zeros(n, D, dtype=bf16)
    back[rows[ok]] = x[rows[ok]]
    poison((n, D), bf16, dev)
    same_bits("scatter of the gather", o.scatter_rows(got, rows.to(dev), n), back)


# ---- l2norm -----------------------------------------------------------------------------------------------------------
L2NORM = [Case("r37_E96_toy", rows=37, E=96), Case("r4099_E1024_rows_not_multiple_of_4", rows=4099, E=1024),
          Case("r513_E1280", rows=513, E=1280), Case("r6_E40_shorter_than_a_wave", rows=6, E=40), Case("r1_E512_one_row", rows=1, E=512)]


def _l2_ref(x, eps):
    xd = x.double()
    n = xd.norm(dim=-1).clamp_min(eps)                                   # F.normalize: x / max(||x||, eps)
    return xd / n[:, None], 1.0 / n


def check_l2norm(o, dev, c):
    rows, E, eps = c.rows, c.E, 1e-12
    x = gauss((rows, E), 81)
    if rows >= 6:
        x[0] = 0                                                         # y = 0, inv = 1 / eps
        x[1] = x[3] * 1e-20                                              # ||x|| < eps: the clamp decides, y = x / eps
        x[2] = x[3] * 1e18                                               # fp32 squares overflow
    yr, ir = _l2_ref(x, eps)
    y, ybf, inv = o.l2norm_fwd(x.to(dev), eps, want_bf16=True)
    close("y", y, yr, TOL_L2_FWD)
    close("inv_norm", inv, ir, (TOL_L2_FWD[0], 0.0))
    same_bits("y as bf16: one rounding of the f32 result", ybf, y.cpu().to(bf16))
    dy = gauss((rows, E), 82)
    # d/dx of x / max(||x||, eps): (dy - y <y, dy>) / ||x|| above the clamp, dy / eps below it
    dxr = torch.where((x.double().norm(dim=-1) > eps)[:, None], ir[:, None] * (dy.double() - yr * (yr * dy.double()).sum(-1, keepdim=True)),
                      dy.double() / eps)
    dx = o.l2norm_bwd(y, inv, dy.to(dev))
    assert bool(dx.cpu().isfinite().all())
    close("dx", dx, dxr, TOL_L2_BWD)
    if rows >= 6:
        assert not y.cpu()[0].any() and inv.cpu()[0].item() == (torch.ones((), dtype=f32) / torch.tensor(eps, dtype=f32)).item()
        # with eps out of the way the tiny, the huge and the plain copy of one row normalise to the same unit vector
        y3, _, inv3 = o.l2norm_fwd(x[1:4].contiguous().to(dev), 1e-30)
        yr3, ir3 = _l2_ref(x[1:4], 1e-30)
        close("y, rows scaled by 1e-20 / 1e18 / 1", y3, yr3, TOL_L2_FWD)
        close("inv_norm, scaled rows", inv3, ir3, (TOL_L2_FWD[0], 0.0))
        close("tiny row == plain row", y3[0], y3.cpu()[2].double(), (0.0, 2 * TOL_L2_FWD[1]))
        close("huge row == plain row", y3[1], y3.cpu()[2].double(), (0.0, 2 * TOL_L2_FWD[1]))


# ---- colsum -----------------------------------------------------------------------------------------------------------
def colsum_geometry(M):
    """(blocks the workspace is sized for, rows per block, partial blocks launched): misc.hip colsum_blocks / clipa_colsum."""
    nb = max(1, min(1024, (M + 511) // 512))
    rpb = (M + nb - 1) // nb
    return nb, rpb, (M + rpb - 1) // rpb


# exact: |dy| <= 4 -> |any partial sum| <= 4 M <= 2 400 004 < 2^24.   nblk8 = partial blocks mod 8: which of the 8- and
# 4-stride loops of colsum_final_kernel the last partials fall into
COLSUM = [Case("M5000_N1032_toy", M=5000, N=1032, nblk8=2),
          Case("M3_N8_fewer_rows_than_waves", M=3, N=8, nblk8=1),
          Case("M1_N64", M=1, N=64, nblk8=1),
          Case("M513_N520_ragged_last_512_columns_rpb257", M=513, N=520, nblk8=2),
          Case("M4097_N1024_9_blocks", M=4097, N=1024, nblk8=1),
          Case("M600001_N64_block_cap_1024_rpb586", M=600001, N=64, nblk8=0),
          Case("M40000_N4096_79_blocks_rpb507", M=40000, N=4096, nblk8=7),
          Case("M2000_N72_4_blocks_tail_loop_only", M=2000, N=72, nblk8=4),
          Case("M2500_N264_5_blocks", M=2500, N=264, nblk8=5),
          Case("M5000_N1032_column_slice_ld_2N", M=5000, N=1032, nblk8=2, sliced=True),
          Case("M513_N64_column_slice_ld_2N", M=513, N=64, nblk8=2, sliced=True)]


def check_colsum(o, dev, c, query=None):
    M, N = c.M, c.N
    nb, rpb, nblk = colsum_geometry(M)
    if query is not None:
        assert query("clipa_colsum_workspace", M, N) == nb * N * 4, "block heuristic changed: re-derive the cases"
    assert nblk % 8 == c.nblk8, (nb, rpb, nblk)
    if "block_cap" in c.name:
        assert nb == 1024 and M > 1024 * 512
    if "rpb" in c.name:
        assert rpb % 4 != 0
    sliced = getattr(c, "sliced", False)
    wide = ints((M, 2 * N if sliced else N), 91, 4)
    dy = wide[:, 8:8 + N] if sliced else wide                            # a 16-byte aligned column slice: ld = 2 N
    ref = sum64(dy).float()
    d = wide.to(dev)
    d = d[:, 8:8 + N] if sliced else d
    out = o.colsum(d)
    same("colsum", out, ref)
    same("colsum, second call", o.colsum(d), out.cpu())
    if c.name == "M5000_N1032_toy":
        # Gaussian data: a wave adds ceil(rpb / 4) rows, the block 4 waves, colsum_final ceil(nblk / 8) partials per
        # accumulator, the two accumulators, 4 groups  ->  depth = ceil(rpb/4) + 3 + ceil(nblk/8) + 1 + 3 additions
        dy = gauss((M, N), 92, dtype=bf16)
        depth = (rpb + 3) // 4 + 3 + (nblk + 7) // 8 + 1 + 3
        err = (o.colsum(dy.to(dev)).cpu().double() - sum64(dy)).abs()
        assert (err <= depth * 2.0 ** -24 * sum64(dy.abs())).all(), "Gaussian colsum outside the summation-order bound"


# ---- casts and transposes ---------------------------------------------------------------------------------------------
CAST_N = [1, 7, 8, 9, 2047 * 8 + 3, 4 * 2 ** 20 + 5]
CAST = [Case(f"n{n}_{'f32' if d == f32 else 'bf16'}_in", n=n, dt=d) for n in CAST_N for d in (f32, bf16)]


def _f32_bits(words):
    return torch.tensor([w - 2 ** 32 if w >= 2 ** 31 else w for w in words], dtype=torch.int32).view(f32)


# ties to even in both directions (+-), the largest finite values (0x7f7fffff and the tie 0x7f7f8000 round to inf,
# 0x7f7f7fff stays the largest bf16), +-inf, quiet and signalling NaN (low payload bits only: truncation would make
# inf of it), +-0, fp32 denormals, the smallest normal
SPECIAL_F32 = _f32_bits([0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x3f808001, 0x3f807fff, 0x7f7fffff, 0x7f7f8000,
                         0x7f7f7fff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0x7f800001, 0xffc00001, 0x00000000,
                         0x80000000, 0x00000001, 0x00008000, 0x00018000, 0x807fffff, 0x00800000])


def _cast_input(n, dt, shift):
    """Position-coded values with the special ones (rotated by `shift`) at the front - the 16-byte body - and at the end -
    the scalar tail when n % 8 != 0."""
    x = coded_flat(n, salt=shift)
    if dt == bf16:
        sp = torch.cat([SPECIAL_F32[[10, 11, 12, 15, 16, 19, 21]].to(bf16),          # +-inf, NaN, +-0, a denormal, the smallest normal
                        torch.tensor([0x7fa5, 0x7f81], dtype=torch.int16).view(bf16)])     # NaNs with a payload
    else:
        x, sp = spread_f32(x, shift), SPECIAL_F32
    sp = sp.roll(shift)
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    x[n - k:] = sp[sp.numel() - k:]
    return x


def check_cast(o, dev, c):
    shifts = (0, 5, 10, 15, 20) if c.n < 100000 else (0, 10)            # a tail of 7 sees every special value
    for s in shifts if c.dt == f32 else shifts[:2]:
        x = _cast_input(c.n, c.dt, s)
        poison((c.n,), bf16, dev)
        # f32 -> bf16 may quiet a NaN but must keep it a NaN; a bf16 -> bf16 copy keeps every bit
        same_bits("to_bf16", o.to_bf16(x.to(dev)), x.to(bf16), nan_as_one=c.dt == f32)
        if c.dt == bf16:
            poison((c.n,), f32, dev)
            same_bits("to_f32", o.to_f32(x.to(dev)), x.float())


TRANSPOSE = [Case(f"R{R}_C{C}_{'f32' if d == f32 else 'bf16'}{'_column_slice' if s else ''}_{why}", R=R, C=C, dt=d, sliced=s)
             for R, C, why in [(200, 136, "toy"), (64, 64, "one_whole_tile"), (1, 1000, "one_row"), (1024, 4096, "mlp_weight_whole_tiles"),
                               (65, 63, "one_past_and_one_short_of_a_tile")]
             for d in (f32, bf16) for s in (False, True) if not s or (R, C) in ((200, 136), (64, 64), (65, 63))]


def check_transpose(o, dev, c):
    R, C = c.R, c.C
    wide = coded(R, 2 * C + 5 if c.sliced else C, salt=13)
    if c.dt == f32:
        wide = spread_f32(wide, 14)
    t = wide[:, 5:5 + C] if c.sliced else wide                           # ldi = 2 C + 5 != C
    d = wide.to(dev)
    d = d[:, 5:5 + C] if c.sliced else d
    poison((C, R), bf16, dev)
    same_bits("transpose_bf16", o.transpose_bf16(d), t.to(bf16).T.contiguous())


# ---- sum_scale --------------------------------------------------------------------------------------------------------
# exact: |x| <= 16 quanta of 2^-4 -> |sum| <= 1.6e6 quanta < 2^24; then one multiply (one rounding) and, with
# accumulate, one addition (one rounding) - both reproduced in fp32 torch
SUM_SCALE = [Case(f"n{n}_{why}", n=n) for n, why in [(1, "one_lane"), (255, "last_lane_idle"), (256, "one_pass"), (257, "second_pass_of_one"),
                                                     (4096 + 3, "ragged"), (100000, "many_passes")]]


def check_sum_scale(o, dev, c):
    x = ints((c.n,), 101, 16, 4, dtype=f32)
    s = x.double().sum().float()
    for scale in (0.25, 1.0 / 3.0, 1.0):
        want = s * torch.tensor(scale, dtype=f32)
        same(f"sum_scale * {scale:.3g}", o.sum_scale(x.to(dev), scale), want)
        out = torch.tensor(5.5, dtype=f32).to(dev)
        if scale != 1.0 / 3.0:      # a power-of-two scale: the product is exact, so out + sum * scale has one rounding whether
            r = o.sum_scale(x.to(dev), scale, out=out, accumulate=True)      # or not the multiply and the add are fused
            same("accumulate into a preset value", r, torch.tensor(5.5, dtype=f32) + want)
        r = o.sum_scale(x.to(dev), scale, out=out, accumulate=False)
        same("overwrite a preset value", r, want)
    # the two-call pattern of clipa_amd/loss.py: loss = sum_scale(li, gs); sum_scale(lt, gs, out=loss, accumulate=True)
    x2 = ints((c.n,), 102, 16, 4, dtype=f32)
    loss = o.sum_scale(x.to(dev), 0.5)
    o.sum_scale(x2.to(dev), 0.5, out=loss, accumulate=True)
    same("two-call sum", loss, s * 0.5 + x2.double().sum().float() * 0.5)


# ---- reduce_shards ----------------------------------------------------------------------------------------------------
_DT = {f32: "f32", bf16: "bf16"}
# n / 8 work items, 256 per block: 8 -> one thread; 2040 / 2048 / 2056 -> 255 / 256 / 257 threads (the last block holds
# one); 8 (2^20 + 1) -> 4097 blocks, the last holds one thread
REDUCE_SMALL = [Case(f"W{W}_{_DT[i]}_to_{_DT[t]}_small_n", W=W, i=i, t=t, ns=(8, 2040, 2048, 2056))
                for W in (1, 2, 3, 8) for i in (f32, bf16) for t in (f32, bf16)]
REDUCE_BIG = [Case(f"W{W}_{_DT[i]}_to_{_DT[t]}_n8M", W=W, i=i, t=t, ns=(8 * (2 ** 20 + 1),))
              for W, i, t in [(3, f32, f32), (3, f32, bf16), (3, bf16, f32), (3, bf16, bf16), (8, f32, f32), (1, bf16, bf16), (2, bf16, f32)]]


def check_reduce_shards(o, dev, c):
    W = c.W
    for n in c.ns:
        pieces = coded(W, n, salt=17, emin=117, emax=137)                # piece w, element i recognisable; 2^-10 .. 2^11
        pieces = spread_f32(pieces, 18) if c.i == f32 else pieces
        for scale in (None, 0.37):
            a = torch.zeros(n, dtype=f32)
            for w in range(W):                                           # sequential fp32 additions in rank order,
                a = a + pieces[w].float()
            a = a * torch.tensor(1.0 / W if scale is None else scale, dtype=f32)        # one multiply,
            poison((n,), c.t, dev)
            got = o.reduce_shards(pieces.reshape(-1).to(dev), W, scale=scale, out_dtype=c.t)
            same_bits(f"reduce_shards n={n} scale={scale}", got, a.to(c.t))              # one rounding
        out = torch.empty(n, dtype=c.t, device=dev)
        r = o.reduce_shards(pieces.reshape(-1).to(dev), W, out=out, scale=0.37)
        same_bits("reduce_shards into out=", r, a.to(c.t))


def check_reduce_shards_errors(o, dev):
    import pytest
    with pytest.raises(RuntimeError, match="multiple of world"):
        o.reduce_shards(torch.zeros(50, dtype=f32).to(dev), 3)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        o.reduce_shards(torch.zeros(36, dtype=f32).to(dev), 3)          # n = 12


# ---- AdamW ------------------------------------------------------------------------------------------------------------
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-6, weight_decay=0.2)
_PAIRS = [(f32, f32), (bf16, bf16), (f32, bf16), (bf16, f32)]
# the launch caps the grid at 4096 blocks of 256: only n > 4096 * 256 makes the grid-stride loop iterate
ADAMW = [Case(f"n{n}_p{_DT[p]}_g{_DT[g]}_{why}", n=n, p=p, g=g) for n, why in [(4096 * 256 + 4099, "grid_stride_second_pass"), (1, "one_element")]
         for p, g in _PAIRS]


def adamw_ref(p, g, m, v, step, gscale, h=HYPER):
    """One fp64 torch.optim.AdamW step (decoupled decay, bias correction) on fp64 tensors, in place."""
    g = g * gscale
    p.mul_(1 - h["lr"] * h["weight_decay"])
    m.mul_(h["beta1"]).add_(g, alpha=1 - h["beta1"])
    v.mul_(h["beta2"]).addcmul_(g, g, value=1 - h["beta2"])
    denom = v.sqrt() / math.sqrt(1 - h["beta2"] ** step) + h["eps"]
    p.addcdiv_(m, denom, value=-h["lr"] / (1 - h["beta1"] ** step))


def check_adamw(o, dev, c):
    n = c.n
    p0, g0 = gauss(n, 111).to(c.p), gauss(n, 112, 0.1)
    ref = torch.nn.Parameter(p0.double())
    opt = torch.optim.AdamW([ref], lr=HYPER["lr"], betas=(HYPER["beta1"], HYPER["beta2"]), eps=HYPER["eps"], weight_decay=HYPER["weight_decay"])
    p = p0.to(dev)
    m, v = torch.zeros(n, dtype=f32).to(dev), torch.zeros(n, dtype=f32).to(dev)
    gscale = 0.37
    for step in (1, 2, 3):
        g = (g0 * step).to(c.g)
        ref.grad = g.double() * gscale
        opt.step()
        if c.p == bf16:
            ref.data = ref.data.to(bf16).double()
        o.adamw_(p, g.to(dev), m, v, step=step, grad_scale=gscale, **HYPER)
    close("adamw_ parameters after 3 steps", p.float(), ref.data, TOL_ADAMW[c.p])


# 120 tensors, 17 of them empty (i % 7 == 3): 103 non-empty = launches of 48 + 48 + 7 (MT_MAX = 48)
MT_SIZES = [0 if i % 7 == 3 else (1 if i == 5 else 4096 if i == 9 else 4097 if i == 11 else 2 ** 20 + 7 if i == 60 else 33 + 17 * i)
            for i in range(120)]
_MT_LIVE = [i for i, n in enumerate(MT_SIZES) if n > 0]
# the clamped tensor: non-empty tensor number 20 / 70 / 100 -> launch 0 / 1 / 2; empty tensors precede each, so its slot
# in the launch differs from its list index
_MT_CLAMP = {"first_launch": _MT_LIVE[20], "second_launch": _MT_LIVE[70], "third_launch": _MT_LIVE[100], "none": -1}
ADAMW_MULTI = [Case(f"clamp_{k}_p{_DT[p]}_g{_DT[g]}", p=p, g=g, clamp_index=ci, launch={"first_launch": 0, "second_launch": 1, "third_launch": 2}.get(k))
               for k, ci in _MT_CLAMP.items() for p, g in _PAIRS]


def check_adamw_multi(o, dev, c):
    ci = c.clamp_index
    if ci >= 0:
        k = _MT_LIVE.index(ci)               # its slot in the launch is k % 48, not its list index: empty tensors precede it
        assert k // 48 == c.launch and k % 48 != ci and 0 in MT_SIZES[:ci]
    lo, hi = 0.25, 0.5                    # N(0, 1) parameters: nearly every value of every tensor lies outside [lo, hi]
    ps = [gauss(n, 200 + i).to(c.p) for i, n in enumerate(MT_SIZES)]
    g0 = [gauss(n, 400 + i, 0.1) for i, n in enumerate(MT_SIZES)]
    refs = [(p.double(), torch.zeros(p.numel(), dtype=f64), torch.zeros(p.numel(), dtype=f64)) for p in ps]
    dps = [p.to(dev) for p in ps]
    ms = [torch.zeros(n, dtype=f32).to(dev) for n in MT_SIZES]
    vs = [torch.zeros(n, dtype=f32).to(dev) for n in MT_SIZES]
    coef = torch.tensor([0.61], dtype=f32)
    for step in (1, 2):
        gs = [(g * step).to(c.g) for g in g0]
        o.adamw_multi_(dps, [g.to(dev) for g in gs], ms, vs, step=step, grad_scale=0.5, grad_scale_dev=coef.to(dev),
                       clamp_index=ci, clamp=(lo, hi), **HYPER)
        for i, ((p, m, v), g) in enumerate(zip(refs, gs)):
            adamw_ref(p, g.double(), m, v, step, 0.5 * float(coef[0]))
            if i == ci:
                p.clamp_(lo, hi)                                         # exactly that tensor, no other
            if c.p == bf16:
                p.copy_(p.to(bf16).double())
    for i, (d, (p, _, _)) in enumerate(zip(dps, refs)):
        close(f"adamw_multi_ tensor {i} ({MT_SIZES[i]} elements)", d.float(), p, TOL_ADAMW[c.p])
        if i == ci:
            assert bool(((d.float() >= lo) & (d.float() <= hi)).all())
        elif d.numel() > 8:      # the close() above against the unclamped reference is the guard; this only makes sure that
            assert bool(((d.float() < lo) | (d.float() > hi)).sum() > d.numel() // 2)      # a stray clamp would have shown


# ---- grad_sqnorm / clip_coef ------------------------------------------------------------------------------------------
def _sq_sizes(live, empty_at):
    """`live` non-empty tensors - 1, 4095, 4096, 4097 elements (one short of, exactly and one past a 4096-element block),
    then ragged sizes - with empty tensors inserted at the list positions `empty_at`: they use no slot of a launch."""
    sizes = [[1, 4095, 4096, 4097][i] if i < 4 else 100 + 37 * i for i in range(live)]
    for at in sorted(empty_at):
        sizes.insert(at, 0)
    return sizes


# launches: per dtype call of ops.grad_sqnorm (f32 tensors first, then bf16) the (launches, tensors in the last launch)
# that MT_MAX = 48 non-empty tensors per launch gives; check_grad_sqnorm asserts it from the sizes
_T130 = [2 * 2 ** 20 if i == 5 else 0 if i % 9 == 4 else [1, 4095, 4096, 4097][i] if i < 4 else 64 + 29 * i for i in range(130)]
SQNORM = [Case("t1_one_f32_element", sizes=[1], dts=[f32], launches={f32: (1, 1)}),
          Case("t48_bf16_exactly_one_launch", sizes=_sq_sizes(48, (4, 30)), dts=[bf16] * 50, launches={bf16: (1, 48)}),
          Case("t49_f32_second_launch_of_one", sizes=_sq_sizes(49, (4, 30, 50)), dts=[f32] * 52, launches={f32: (2, 1)}),
          Case("t130_mixed_with_empties_and_2M", sizes=_T130, dts=[f32 if i % 2 == 0 else bf16 for i in range(130)],
               launches={f32: (2, 10), bf16: (2, 10)})]


def check_grad_sqnorm(o, dev, c):
    for dt in (f32, bf16):       # the launch geometry the case is named for: empty tensors take no slot
        live = sum(1 for n, d in zip(c.sizes, c.dts) if d == dt and n > 0)
        if live or dt in c.launches:
            assert ((live + 47) // 48, live - 48 * ((live + 47) // 48 - 1)) == c.launches[dt], (dt, live)
    assert 0 in c.sizes or len(c.sizes) == 1
    # exact: g in {-2 .. 2}: squares and every partial sum of them are integers <= 2 * total (both calls) < 2^24
    grads = [ints((n,), 500 + i, 2, dtype=d) for i, (n, d) in enumerate(zip(c.sizes, c.dts))]
    for g in grads:
        if g.numel():
            g[-1] = 2                                                    # the last partial of every launch is not zero
    total = sum(float((g.double() ** 2).sum()) for g in grads)
    assert 2 * total < 2 ** 24
    dg = [g.to(dev) for g in grads]
    buf = o.grad_sqnorm(dg)
    same("sum of squares", buf[0], torch.tensor(total, dtype=f32))
    buf = o.grad_sqnorm(dg, buf=buf)                                     # a second call accumulates into a non-zero buffer
    same("accumulated sum of squares", buf[0], torch.tensor(2 * total, dtype=f32))
    norm, coef = o.clip_coef(buf, 1.0)
    close("norm", norm, torch.tensor(math.sqrt(2 * total), dtype=f64), (TOL_L2_FWD[0], 0.0))
    close("coef", coef, torch.tensor(1.0 / (math.sqrt(2 * total) + 1e-6), dtype=f64).clamp(max=1.0), (TOL_L2_FWD[0], 0.0))
    norm, coef = o.grad_clip_coef(dg, 1e9)
    same("coef below the threshold", coef, torch.tensor(1.0, dtype=f32))
    close("norm", norm, torch.tensor(math.sqrt(total), dtype=f64), (TOL_L2_FWD[0], 0.0))


CLIP_COEF = [Case("norm_above_max", sq=400.0, max_norm=1.0, coef=1.0 / (20.0 + 1e-6)),
             Case("norm_below_max_coef_exactly_1", sq=0.25, max_norm=1.0, coef=1.0),
             Case("norm_zero_coef_exactly_1", sq=0.0, max_norm=1.0, coef=1.0),
             Case("norm_inf_coef_0", sq=float("inf"), max_norm=1.0, coef=0.0),
             Case("norm_nan_coef_nan", sq=float("nan"), max_norm=1.0, coef=float("nan"))]


def check_clip_coef(o, dev, c):
    buf = torch.tensor([c.sq, -1.0, -1.0], dtype=f32).to(dev)
    norm, coef = o.clip_coef(buf, c.max_norm)
    norm, coef = norm.cpu(), coef.cpu()
    if math.isnan(c.sq):
        assert bool(norm.isnan()) and bool(coef.isnan()), f"NaN norm -> NaN coefficient (torch.clamp(coef, max=1.0)), got {coef.item()}"
    elif math.isinf(c.sq) or c.coef == 1.0:
        assert norm.item() == math.sqrt(c.sq) and coef.item() == c.coef
    else:
        close("norm", norm, torch.tensor(math.sqrt(c.sq), dtype=f64), (TOL_L2_FWD[0], 0.0))
        close("coef", coef, torch.tensor(c.coef, dtype=f64), (TOL_L2_FWD[0], 0.0))


def check_grad_clip_coef_nonfinite(o, dev):
    """One NaN gradient element poisons the coefficient (and through it every update), one inf element zeroes it."""
    sizes = [5000, 0, 33, 4097]
    for bad, dt in ((float("nan"), f32), (float("nan"), bf16), (float("inf"), f32)):
        grads = [ints((n,), 600 + i, 2, dtype=dt if i == 2 else f32) for i, n in enumerate(sizes)]
        grads[2][17] = bad
        norm, coef = o.grad_clip_coef([g.to(dev) for g in grads], 1.0)
        if math.isnan(bad):
            assert bool(norm.cpu().isnan()) and bool(coef.cpu().isnan()), f"NaN gradient -> coef {coef.item()}"
        else:
            assert norm.item() == float("inf") and coef.item() == 0.0
