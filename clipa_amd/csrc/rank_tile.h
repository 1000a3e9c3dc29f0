// The 128 x 128 fp32 similarity tile of the evaluation kernels (retrieval.hip, retrieval_multi.hip, fewshot.hip, zeroshot.hip,
// topk.hip, logreg.hip) and what every consumer of it needs: one copy, so every x_ij = A_i . B_j comes out of the same instruction sequence
// whichever kernel, launch or tile computes it.  That is what lets a positive compare with itself exactly (retrieval.hip) and
// what tests/test_retrieval_multi_gpu.py and tests/test_topk_gpu.py check between the kernels bit for bit.
//   RankLane        a lane's place in the tile: the only copy of the D-fragment map (row(q), col(ni))
//   rank_rows       buffer resource and valid rows of a 128-row block of an operand
//   rank_tile       the main loop
//   halve32, rank_row_meet   per-row reduction over the 64 lanes that share a tile row: 32 lanes of a wave, then the two column waves
//   rank_count      the count epilogue of the two retrieval kernels
//   RankBest, rank_better    a row's running (logit, class) best and its order-free meeting
//   f32_key / f32_unkey      order-preserving float <-> unsigned map (integer atomicMax, sort keys)
//   rank_check_args, rank_launch   host side: argument checks and the launch on the 2 x R_STAGE ring
//
// Arithmetic: v_mfma_f32_32x32x2_f32, one accumulator chain per output in ascending k (bit for bit a chain of fp32 fmaf),
// no split-K.
//
// Tile 128 x 128, 4 waves as 2 x 2, each wave 2 x 2 accumulators of 32 x 32; k-chunks of 32 fp32 staged by 4-byte LDS-DMA
// into a double-buffered ring (2 x 32 KiB: two workgroups per CU).  The per-dword DMA lets the LDS image put, for each row,
// the pair {k = 4q + h, 4q + 2 + h} of lane half h in one 8-byte slot: one ds_read_b64 feeds two consecutive MFMA k-steps,
// and the slot index is XOR-swizzled with the row (swz below) so 16 consecutive rows hit 16 distinct slots and the 32 rows of a
// lane half 32 distinct bank pairs: conflict-free as ds_read_b64 and as the ds_read2st64_b64 hipcc pairs them into.
#pragma once
#include "gemm_common.h"

namespace clipa_gemm {
namespace {

constexpr int RT = 128;                       // output tile (rows of A and of B)
constexpr int RK = 32;                        // k per stage
constexpr int RTHREADS = 256;
constexpr int R_IMG = RT * RK * 4;            // one operand image: 16 KiB
constexpr int R_STAGE = 2 * R_IMG;

// 8-byte slot swizzle of image row r: a bijection of 0..15 over any 16 consecutive rows that also differs between r and r + 16
__device__ __forceinline__ int swz(int r) { return (r & 15) ^ ((r >> 4) & 1); }

// A lane's place in the tile.  4 waves as 2 (wm: rows) x 2 (wn: columns) of 64 x 64; lane = hi * 32 + L.  The D fragment of
// v_mfma_f32_32x32x2_f32 puts accumulator acc[mi][ni][r], value index q = mi * 16 + r, at tile row row(q) and column col(ni);
// with the tile's origin (m0, n0) as second argument, at that row and column of the whole matrix.
struct RankLane {
  int tid, lane, wave, L, hi, wm, wn;
  __device__ __forceinline__ int row(int q, int m0 = 0) const { return m0 + wm * 64 + (q >> 4) * 32 + (q & 3) + 8 * ((q & 15) >> 2) + 4 * hi; }
  __device__ __forceinline__ int col(int ni, int n0 = 0) const { return n0 + wn * 64 + ni * 32 + L; }
};
__device__ __forceinline__ RankLane rank_lane() {
  RankLane t;
  t.tid = threadIdx.x;
  t.lane = t.tid & 63;
  t.wave = __builtin_amdgcn_readfirstlane(t.tid >> 6);
  t.L = t.lane & 31, t.hi = t.lane >> 5;
  t.wm = t.wave >> 1, t.wn = t.wave & 1;
  return t;
}

// Buffer resource of the row block [r0, r0 + RT) of the fp32 matrix X [N, ld]: rows past N read 0.  *rows = its valid rows.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rank_rows(const char* X, int r0, int N, long ld, int* rows) {
  *rows = min(RT, N - r0);
  return make_rsrc(X + (size_t)r0 * ld * 4, (unsigned)(*rows * ld * 4));
}

// order-preserving map float -> unsigned (a < b  <=>  key(a) < key(b) for non-NaN a, b; -0 < +0) and its inverse
__device__ __forceinline__ unsigned f32_key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float f32_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? k & 0x7fffffffu : ~k); }

// acc[mi][ni] = the 32 x 32 block (mi, ni) of this wave's 64 x 64 quarter of the 128 x 128 tile of A rows (rsA) times B
// rows (rsB), rows past a resource's range and k >= E reading 0.  Uses the first 2 * R_STAGE bytes of smem; the caller
// synchronises before reusing them.
// D fragment: acc[mi][ni][r] is the tile's entry (RankLane::row(mi * 16 + r), RankLane::col(ni)).
__device__ __forceinline__ void rank_tile(char* smem, __amdgpu_buffer_rsrc_t rsA, __amdgpu_buffer_rsrc_t rsB, long lda,
                                          long ldb, int E, f32x16 (&acc)[2][2]) {
  const RankLane t = rank_lane();
  // derived again from lane and wave, not read from t.L ... t.wn: with the latter hipcc moves the wave's share of the
  // fragment addresses into scalar adds inside the k loop (the loop below is then not the instruction stream it was)
  const int wave = t.wave;
  const int L = t.lane & 31, hi = t.lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;   // wave tile: 64 (i) x 64 (j)

  // DMA piece pc (256 B = two rows of the image) = 16 j-steps x 4 waves; lane -> row 2 pc + hi, dword L of the row:
  // 8-byte slot L / 2 holds pair (slot ^ swz(row)) = (q, h), element L & 1 is k = 4q + h + 2 (L & 1).
  int kel[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int pr = (L >> 1) ^ swz(8 * j + 2 * wave + hi);
    kel[j] = 4 * (pr >> 1) + (pr & 1) + 2 * (L & 1);
  }
  const unsigned rowA0 = (unsigned)((2 * wave + hi) * lda * 4), rowB0 = (unsigned)((2 * wave + hi) * ldb * 4);
  const unsigned stepA = (unsigned)(8 * lda * 4), stepB = (unsigned)(8 * ldb * 4);

#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  auto stage = [&](int buf, int k0) {
    char* sA = smem + buf * R_STAGE;
    char* sB = sA + R_IMG;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int pc = 4 * j + wave;
      const int k = k0 + kel[j & 3];
      const unsigned oob = k >= E ? 0x80000000u : 0u;   // ragged E: the buffer range check returns 0
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, LDS_PTR(sA + pc * 256), 4, (rowA0 + j * stepA + k * 4) | oob, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, LDS_PTR(sB + pc * 256), 4, (rowB0 + j * stepB + k * 4) | oob, 0, 0, 0);
    }
  };

  const int sw = swz(L);                      // fragment rows start at multiples of 32
  const int rowoffA = (wm * 64 + L) * 128;
  const int rowoffB = (wn * 64 + L) * 128;
  const int nkt = (E + RK - 1) / RK;
  stage(0, 0);
  for (int kt = 0; kt < nkt; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nkt) stage((kt + 1) & 1, (kt + 1) * RK);
    const char* sA = smem + (kt & 1) * R_STAGE;
    const char* sB = sA + R_IMG;
#pragma unroll
    for (int q = 0; q < RK / 4; ++q) {
      const int off = ((2 * q + hi) ^ sw) * 8;
      f32x2 fa[2], fb[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) fa[mi] = *(const f32x2*)(sA + rowoffA + mi * 32 * 128 + off);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) fb[ni] = *(const f32x2*)(sB + rowoffB + ni * 32 * 128 + off);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[mi].x, fb[ni].x, acc[mi][ni], 0, 0, 0);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[mi].y, fb[ni].y, acc[mi][ni], 0, 0, 0);
    }
  }
}

// Recursive halving over the 32 lanes of a lane half: x[q] holds this lane's value for value index q = mi * 16 + r; afterwards
// lane L holds in x[0] the combination of all 32 lanes' values for value index L, tile row RankLane::row(L).  The steps are
// template constants: written as a loop over b >>= 1 the 32-entry array can stay dynamically indexed.  A T that is not one
// register brings its own lane_xor (fewshot.hip).
template <class T>
__device__ __forceinline__ T lane_xor(T x, int b) { return __shfl_xor(x, b, 64); }
template <int b, class T, class F>
__device__ __forceinline__ void halve_step(T (&x)[32], int L, F combine) {
  const bool up = (L & b) != 0;
#pragma unroll
  for (int c = 0; c < b; ++c) {
    const T lo = x[c], hi = x[c + b];
    x[c] = combine(up ? hi : lo, lane_xor(up ? lo : hi, b));
  }
  if constexpr (b > 1) halve_step<b / 2>(x, L, combine);
}
template <class T, class F>
__device__ __forceinline__ void halve32(T (&x)[32], int L, F combine) { halve_step<16>(x, L, combine); }

// The step after halve32: the two column waves' halves of a per-row result meet in buf [2 wn][128] (LDS the caller owns; nobody
// may still be reading it).  x: this lane's x[0] of halve32.  -> the combination for tile row tid & 127.  One barrier, which
// also publishes whatever else the caller stored before the call.
template <class T, class F>
__device__ __forceinline__ T rank_row_meet(const RankLane& t, T* buf, T x, F combine) {
  buf[t.wn * RT + t.row(t.L)] = x;
  __syncthreads();
  const int i = t.tid & (RT - 1);
  return combine(buf[i], buf[RT + i]);
}

// A row's running best of the argmax kernels (fewshot.hip, logreg.hip): the logit and its class (c = 0x7fffffff: no class seen
// yet).  rank_better picks by a strict total order on finite logits - the larger value, equal values by the lower class - so the
// best of a set does not depend on the order of the meeting.
struct RankBest { float v; int c; };
__device__ __forceinline__ RankBest lane_xor(RankBest x, int b) { return {__shfl_xor(x.v, b, 64), __shfl_xor(x.c, b, 64)}; }
__device__ __forceinline__ RankBest rank_better(RankBest a, RankBest o) { return o.v > a.v || (o.v == a.v && o.c < a.c) ? o : a; }

// Count epilogue of the tile at (m0, n0) with rowsA x rowsB valid entries, v = fl(s * acc): per row i the entries that beat
// (gt) or tie (eq) the row's positive, per column j those against the column's positive, added atomically to
// row_gt / row_eq [m0 + i] and col_gt / col_eq [n0 + j].  dpos: the positive of row tid (tid < 128) or of column tid - 128,
// loaded by the caller before the main loop.  cj[ni]: the row index (of the whole matrix) that is the positive of this
// lane's column col(ni); only ever compared.  eq leaves the entry (cj, j) itself out; gt needs no such mask, as
// v > v is false and the positive was computed by the same code (the header of this file).  Reduces within the wave and
// across waves in LDS: one int per row and per column of the tile reaches memory.
__device__ __forceinline__ void rank_count(char* smem, int m0, int n0, int rowsA, int rowsB, float dpos, float s,
                                           const int (&cj)[2], const f32x16 (&acc)[2][2], int* row_gt, int* row_eq,
                                           int* col_gt, int* col_eq) {
  const RankLane t = rank_lane();
  const int tid = t.tid;

  __syncthreads();                            // the ring is dead: reuse its first bytes
  float* dpl = (float*)smem;                  // [256]: positives of the tile's rows, then of its columns
  int* rowp = (int*)(smem + 1024);            // [2 wn][128]  packed gt | eq << 16 per row
  int* colp = rowp + 2 * RT;                  // [2 wm][128]  per column
  dpl[tid] = dpos;
  __syncthreads();

  float dcol[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) dcol[ni] = dpl[RT + t.col(ni)];
  int rc[32];                                 // per (mi, r): this lane's packed row counts over its two columns
  int cc[2] = {0, 0};                         // per ni: packed column counts over this lane's 32 rows
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int il = t.row(mi * 16 + r);
      const float drow = dpl[il];
      int c = 0;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int jl = t.col(ni);
        const float v = s * acc[mi][ni][r];
        const bool ok = jl < rowsB && il < rowsA;
        const bool other = cj[ni] != m0 + il;  // eq counts entries that are not the column's own positive
        c += ok ? (int)(v > drow) + ((int)(other && v == drow) << 16) : 0;
        cc[ni] += ok ? (int)(v > dcol[ni]) + ((int)(other && v == dcol[ni]) << 16) : 0;
      }
      rc[mi * 16 + r] = c;
    }
  // columns: add the other lane half
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) cc[ni] += __shfl_xor(cc[ni], 32, 64);
  colp[t.wm * RT + t.wn * 64 + t.lane] = t.hi ? cc[1] : cc[0];
  // rows: sum over the 32 lanes of each half, then over the two column waves
  auto add = [](int a, int b) { return a + b; };
  halve32(rc, t.L, add);
  const int v = rank_row_meet(t, rowp, rc[0], add);
  if (tid < RT) {
    if (tid < rowsA) {
      if (v & 0xffff) atomicAdd(row_gt + m0 + tid, v & 0xffff);
      if (v >> 16) atomicAdd(row_eq + m0 + tid, v >> 16);
    }
  } else {
    const int j = tid - RT;
    const int w = colp[j] + colp[RT + j];
    if (j < rowsB) {
      if (w & 0xffff) atomicAdd(col_gt + n0 + j, w & 0xffff);
      if (w >> 16) atomicAdd(col_eq + n0 + j, w >> 16);
    }
  }
}

// Argument checks the entry points share (`name` = the entry point, for the message).  big_n: the caller's own row
// counts are out of range; what: how the message names them.
inline int rank_check_args(const char* name, int64_t E, int64_t lda, int64_t ldb, bool big_n, const char* what,
                           std::initializer_list<const void*> ptrs, const float* scale) {
  if (lda < E || ldb < E || lda % 4 != 0 || ldb % 4 != 0) {
    clipa_set_error("%s: lda = %ld and ldb = %ld must be >= E = %ld and multiples of 4", name, (long)lda, (long)ldb, (long)E);
    return CLIPA_ERR_ARG;
  }
  if ((int64_t)RT * lda * 4 >= (1L << 30) || (int64_t)RT * ldb * 4 >= (1L << 30) || big_n) {
    clipa_set_error("%s: %s or leading dimension too large", name, what);
    return CLIPA_ERR_ARG;
  }
  if (int rc = clipa_check_ptrs16(name, ptrs)) return rc;
  if (((uintptr_t)scale & 3)) { clipa_set_error("%s: scale is not 4-byte aligned", name); return CLIPA_ERR_ARG; }
  return 0;
}

// Launch of `kernel`, one of the kernel set `set` (opted in once per device through `optin` to optin_bytes of dynamic LDS, named
// set_name in that error), on `grid` workgroups of RTHREADS threads with lds_bytes of dynamic LDS; name: the launch, for the error.
template <class K, class... A>
inline int rank_launch(LdsOptIn& optin, std::initializer_list<const void*> set, int optin_bytes, const char* set_name, K kernel,
                       int64_t grid, int lds_bytes, void* stream, const char* name, A... args) {
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (int rc = optin.ensure(dev, set, optin_bytes, set_name)) return rc;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(RTHREADS), lds_bytes, (hipStream_t)stream, args...);
  return clipa_check_launch(name);
}

}  // namespace
}  // namespace clipa_gemm
