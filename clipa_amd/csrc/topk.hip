// Top-k similarity search (the `output.topk` of clipa_torch/training/zero_shot.py:47-50 and the top-k lists of
// clipa_jax/evaluators/proj/image_text/image_text_retrieval.py:77-82) without the [Nq, Ng] similarity matrix: per query row i
// the first k entries (v_ij, g) of the gallery under the strict total order
//   (v, g) precedes (v', g')  iff  v > v', or v == v' and g < g'          g = index_base + j, int64
// with v_ij = fl(s * x_ij), x_ij = Q_i . G_j out of rank_tile (rank_tile.h: one ascending-k fp32 MFMA chain per output, no
// split-K), `==` IEEE equality (-0 and +0 tie: zeros are canonicalised to +0 and reported as +0), and a NaN preceding every
// number (torch.topk's convention; NaNs order among themselves by index and are reported as one canonical NaN).  The order is
// strict, so the result is a function of the set of entries alone: not of the tile order, the number of splits, lane timing or
// how the gallery is cut into shards.  No float atomics; maxima, ballots and integer compares only.
//
// Sort key.  ord(v) maps a canonicalised float to 32 bits whose unsigned order is the order of the values: NaN -> 0xffffffff,
// v >= 0 -> bits | 0x80000000, v < 0 -> ~bits.  The smallest real key is ord(-inf) = 0x007fffff, so 0 marks an empty slot and
// sorts after everything.  Within one call a candidate is the 64-bit key ord(v) << 32 | ~j (j the gallery row of this call,
// below 2^31): one unsigned compare is the whole order.
//
// Main kernel, grid = (128-row query tiles) x splits, 256 threads.  A split owns a contiguous range of gallery tiles and sweeps
// it in ascending order.  Per tile: rank_tile; then the 64 KiB ring is dead (as rank_count exploits) and takes the 128 x 128
// values fl(s * x).  Each wave owns 32 rows.  For a row the 64 lanes read two values each (columns lane and lane + 64), turn
// them into ord, and compare with the ord of the row's current k-th entry (a broadcast LDS read); a ballot says whether anything
// survives.  Tiles arrive in ascending j, so a newcomer that only ties the k-th entry loses and the test is ord > ord_k.
// Survivors enter in descending order: a DPP maximum over the wave finds the largest ord, a ballot and a find-first-set the
// lowest column that holds it, and one compare-and-shift step across lanes 0..k-1 (which hold the row's sorted list) inserts it;
// the loop ends when the largest survivor no longer beats the new k-th entry, after at most k rounds.  After the first few
// tiles almost nothing survives and the epilogue is the LDS round trip.  The lists (128 x k keys) stay in LDS behind the ring
// for the whole sweep and go to the workspace at the end: ws[split][row][k].
// LDS: 64 KiB ring + 128 * k * 8 bytes of lists, no static arrays: 80 KiB at k = 16, 96 KiB at k = 32.  Of the 160 KiB of a CU
// that is two workgroups per CU for k <= 16 and one above.
//
// Merge kernel, one wave per query row: the candidates are the splits' lists and the carry (the running lists of earlier
// calls over other shards, (value, int64 index) pairs with index -1 = empty).  k rounds; in each, every lane scans its
// candidates (c = lane, lane + 64, ...) for the first in the order that comes strictly after the previous round's winner, and a
// butterfly over the wave picks the first of those.  Indices are distinct, so the winner is unique.  A row reads all of its
// carry before it writes its output, and no other row touches either: out may alias carry.
#include "rank_tile.h"

namespace clipa_gemm {
namespace {

constexpr int TK_MAX = 32;
constexpr int TK_RING = 2 * R_STAGE;          // the 64 KiB of rank_tile, then of the value tile

__device__ __forceinline__ unsigned tk_ord(float v) {
  if (v != v) return 0xffffffffu;
  return f32_key(v == 0.f ? 0.f : v);         // -0 -> +0
}
__device__ __forceinline__ float tk_unord(unsigned o) { return f32_unkey(o); }   // 0xffffffff -> 0x7fffffff, a NaN

// maximum over the 64 lanes, returned uniform.  Inclusive scan within each row of 16 lanes (row_shr 1, 2, 4, 8; a lane without
// a source takes 0, the identity), then row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3: lane 63 holds it.
__device__ __forceinline__ unsigned tk_wave_max(unsigned x) {
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false));
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false));
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false));
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false));
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false));
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false));
  return (unsigned)__builtin_amdgcn_readlane((int)x, 63);
}

__global__ __launch_bounds__(RTHREADS, 2) void topk_tile_kernel(const char* __restrict__ Q, const char* __restrict__ G, int Nq,
                                                                 int Ng, int E, long ldq, long ldg,
                                                                 const float* __restrict__ scale, int k, int splits,
                                                                 unsigned long long* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* val = (float*)smem;                                              // [128][128] after rank_tile
  unsigned long long* lst = (unsigned long long*)(smem + TK_RING);        // [128][k], sorted, 0 = empty
  const RankLane t = rank_lane();
  const int tid = t.tid, lane = t.lane, wave = t.wave;
  const int tq = blockIdx.x / splits, sp = blockIdx.x - tq * splits;
  const int m0 = tq * RT;
  int rowsA, rowsB;
  const int Tg = (Ng + RT - 1) / RT;
  const int t_lo = (int)((long)sp * Tg / splits), t_hi = (int)((long)(sp + 1) * Tg / splits);
  const __amdgpu_buffer_rsrc_t rsA = rank_rows(Q, m0, Nq, ldq, &rowsA);
  const float s = scale ? scale[0] : 1.0f;

  for (int i = tid; i < RT * k; i += RTHREADS) lst[i] = 0ull;             // published by the first barrier of the sweep
  f32x16 acc[2][2];
  for (int tn = t_lo; tn < t_hi; ++tn) {
    const int n0 = tn * RT;
    const __amdgpu_buffer_rsrc_t rsB = rank_rows(G, n0, Ng, ldg, &rowsB);
    __syncthreads();                          // the previous tile's readers are done with the ring
    if (E > 0) {
      rank_tile(smem, rsA, rsB, ldq, ldg, E, acc);
    } else {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
    }
    __syncthreads();                          // the ring is dead
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          val[t.row(mi * 16 + r) * RT + t.col(ni)] = s * acc[mi][ni][r];
    __syncthreads();

    const int rows = min(32, rowsA - wave * 32);                           // uniform; <= 0: nothing
    for (int rr = 0; rr < rows; ++rr) {
      const int row = wave * 32 + rr;
      unsigned o0 = lane < rowsB ? tk_ord(val[row * RT + lane]) : 0u;
      unsigned o1 = lane + 64 < rowsB ? tk_ord(val[row * RT + 64 + lane]) : 0u;
      unsigned tho = (unsigned)(lst[row * k + k - 1] >> 32);
      unsigned mx = max(o0, o1);
      if (!__ballot(mx > tho)) continue;
      unsigned long long e = lane < k ? lst[row * k + lane] : 0ull;
      do {
        const unsigned w = tk_wave_max(mx);
        const unsigned long long b0 = __ballot(o0 == w), b1 = __ballot(o1 == w);
        int col;
        if (b0) {
          col = __builtin_ctzll(b0);
          if (lane == col) o0 = 0u;
        } else {
          col = __builtin_ctzll(b1);
          if (lane == col) o1 = 0u;
          col += 64;
        }
        const unsigned long long c = ((unsigned long long)w << 32) | (unsigned)~(unsigned)(n0 + col);
        const unsigned long long up = __shfl_up(e, 1, 64);
        e = e > c ? e : ((lane == 0 || up > c) ? c : up);
        tho = (unsigned)__builtin_amdgcn_readlane((int)(e >> 32), k - 1);
        mx = max(o0, o1);
      } while (__ballot(mx > tho));
      if (lane < k) lst[row * k + lane] = e;
    }
  }
  __syncthreads();
  for (int i = tid; i < rowsA * k; i += RTHREADS) ws[((size_t)sp * Nq + m0) * k + i] = lst[i];
}

struct TkCand { unsigned o; long g; };        // o == 0: none
__device__ __forceinline__ bool tk_before(const TkCand& a, const TkCand& b) { return a.o > b.o || (a.o == b.o && a.g < b.g); }

__global__ __launch_bounds__(256) void topk_merge_kernel(const unsigned long long* __restrict__ ws, int Nq, int k, int splits,
                                                          long index_base, const float* carry_val, const long* carry_idx,
                                                          float* out_val, long* out_idx) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= Nq) return;                      // whole waves
  const long nws = (long)splits * k;
  const long n = nws + (carry_idx ? k : 0);
  auto cand = [&](long c) {
    TkCand x;
    if (c < nws) {
      const unsigned long long key = ws[((size_t)(c / k) * Nq + row) * k + c % k];
      x.o = (unsigned)(key >> 32);
      x.g = index_base + (long)(~(unsigned)key);
    } else {
      x.g = carry_idx[(size_t)row * k + (c - nws)];
      x.o = x.g < 0 ? 0u : tk_ord(carry_val[(size_t)row * k + (c - nws)]);
    }
    return x;
  };
  // this lane's slot of the result (lane < k), filled as the rounds go: nothing is written before the last read of the carry
  float rv = -__builtin_huge_valf();
  long rg = -1;
  TkCand prev = {0u, 0};
  for (int t = 0; t < k; ++t) {
    TkCand best = {0u, 0};
    for (long c = lane; c < n; c += 64) {
      const TkCand x = cand(c);
      if (x.o && (t == 0 || tk_before(prev, x)) && (!best.o || tk_before(x, best))) best = x;
    }
#pragma unroll
    for (int b = 32; b >= 1; b >>= 1) {
      TkCand y;
      y.o = __shfl_xor(best.o, b, 64);
      y.g = __shfl_xor(best.g, b, 64);
      if (y.o && (!best.o || tk_before(y, best))) best = y;
    }
    if (!best.o) break;                       // uniform: fewer than k entries exist
    if (lane == t) { rv = tk_unord(best.o); rg = best.g; }
    prev = best;
  }
  if (lane < k) {
    out_val[(size_t)row * k + lane] = rv;
    out_idx[(size_t)row * k + lane] = rg;
  }
}

LdsOptIn g_tk_lds;

constexpr int64_t TK_NMAX = (1L << 31) - RT;  // rows of one call; a larger gallery goes through shards
constexpr int64_t TK_SLOTS = 512;             // workgroups that 256 CUs hold at two per CU

inline int64_t tk_tiles(int64_t n) { return (n + RT - 1) / RT; }

// splits = 0: enough workgroups to fill TK_SLOTS when the query tiles alone do not, never more than there are gallery tiles.
// -> the number of splits of the launch (0 with an empty gallery), or -1: out of range
inline int64_t tk_splits(int64_t Nq, int64_t Ng, int64_t splits) {
  const int64_t Tq = tk_tiles(Nq), Tg = tk_tiles(Ng);
  if (splits < 0 || splits > (Tg > 0 ? Tg : 1)) return -1;
  if (Tg == 0 || Tq == 0) return 0;
  if (splits == 0) splits = std::min(Tg, std::max<int64_t>(1, TK_SLOTS / Tq));
  return splits;
}

inline bool tk_sizes_ok(int64_t Nq, int64_t Ng, int64_t k) {
  return Nq >= 0 && Ng >= 0 && Nq < TK_NMAX && Ng < TK_NMAX && k >= 1 && k <= TK_MAX;
}

}  // namespace
}  // namespace clipa_gemm

using namespace clipa_gemm;

extern "C" int64_t clipa_topk_workspace(int64_t Nq, int64_t Ng, int64_t k, int64_t splits) {
  if (!tk_sizes_ok(Nq, Ng, k)) return 16;
  const int64_t S = tk_splits(Nq, Ng, splits);
  if (S < 0 || S * tk_tiles(Nq) >= (1L << 31)) return 16;
  return std::max<int64_t>(16, S * Nq * k * 8);
}

extern "C" int clipa_topk(const float* Q, const float* G, int64_t Nq, int64_t Ng, int64_t E, int64_t ldq, int64_t ldg,
                          const float* scale, int64_t k, int64_t index_base, int64_t splits, const float* carry_val,
                          const int64_t* carry_idx, float* out_val, int64_t* out_idx, void* workspace, int64_t workspace_bytes,
                          void* stream) {
  if (k < 1 || k > TK_MAX) { clipa_set_error("topk: k = %ld must lie in [1, %d]", (long)k, TK_MAX); return CLIPA_ERR_ARG; }
  if (Nq < 0 || Ng < 0 || E < 0) { clipa_set_error("topk: Nq = %ld, Ng = %ld, E = %ld must be >= 0", (long)Nq, (long)Ng, (long)E); return CLIPA_ERR_ARG; }
  if (index_base < 0 || index_base >= (1L << 62)) { clipa_set_error("topk: index_base = %ld must lie in [0, 2^62)", (long)index_base); return CLIPA_ERR_ARG; }
  if ((carry_val == nullptr) != (carry_idx == nullptr)) { clipa_set_error("topk: carry_val and carry_idx come together or not at all"); return CLIPA_ERR_ARG; }
  if (Nq == 0) return CLIPA_OK;
  const bool reads = Ng > 0 && E > 0;         // otherwise Q and G are never read and may be the null pointers of empty tensors
  if (int rc = rank_check_args("topk", E, ldq, ldg, !tk_sizes_ok(Nq, Ng, k), "Nq, Ng (below 2^31 - 128; a larger gallery goes through shards)",
                               {reads ? (const void*)Q : out_val, reads ? (const void*)G : out_val, out_val, out_idx, workspace}, scale)) return rc;
  if (((uintptr_t)carry_val & 15) || ((uintptr_t)carry_idx & 15)) { clipa_set_error("topk: carry pointers are not 16-byte aligned"); return CLIPA_ERR_ARG; }
  const int64_t S = tk_splits(Nq, Ng, splits);
  if (S < 0) { clipa_set_error("topk: splits = %ld must lie in [0, %ld] (0 = chosen here; at most one per gallery tile)", (long)splits, (long)std::max<int64_t>(1, tk_tiles(Ng))); return CLIPA_ERR_ARG; }
  if (S * tk_tiles(Nq) >= (1L << 31)) { clipa_set_error("topk: %ld query tiles x %ld splits: too many workgroups", (long)tk_tiles(Nq), (long)S); return CLIPA_ERR_ARG; }
  if (workspace_bytes < clipa_topk_workspace(Nq, Ng, k, splits)) { clipa_set_error("topk: workspace too small"); return CLIPA_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  if (S > 0) {
    if (int rc = rank_launch(g_tk_lds, {(const void*)topk_tile_kernel}, TK_RING + RT * TK_MAX * 8, "topk", topk_tile_kernel,
                             tk_tiles(Nq) * S, TK_RING + RT * (int)k * 8, stream, "topk_tiles", (const char*)Q, (const char*)G,
                             (int)Nq, (int)Ng, (int)E, (long)ldq, (long)ldg, scale, (int)k, (int)S, (unsigned long long*)workspace)) return rc;
  }
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((Nq + 3) / 4)), dim3(256), 0, st, (const unsigned long long*)workspace,
                     (int)Nq, (int)k, (int)S, (long)index_base, carry_val, (const long*)carry_idx, out_val, (long*)out_idx);
  return clipa_check_launch("topk_merge");
}
