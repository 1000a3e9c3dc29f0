// Zero-shot classification (clipa_torch/training/zero_shot.py:29-90, clipa_jax/evaluators/proj/image_text/
// discriminative_classifier.py:152-171, 302-312) with the features kept on the GPU.  fp32 throughout.  Two kernels:
//   class mean  W_c = m_c / (eps + ||m_c||), m_c the mean of the prompt embeddings of class c (rows sorted by class)
//   ranks       per image i with labels L_i (up to 32, -1 = none), v_ic = A_i . W_c:
//                 t_i = max over c in L_i of v_ic (-inf: no label)      pred_i = argmax_c v_ic, lowest c on ties
//                 gt_i = #{c : v_ic > t_i}                              eq_i = #{c not in L_i : v_ic == t_i}
//               without the [B, C] logits.  gt_i is the 0-based rank of image i's best label (another label cannot beat t_i),
//               ties resolve in the label's favour as in retrieval.hip; an image without labels gets gt = C, eq = 0.
//
// Class mean, one workgroup of CM_THREADS threads per class.  Every step is one correctly rounded IEEE operation - `+`, `/`,
// sqrtf (correctly rounded in hipcc's default mode) and an explicit fmaf, so nothing depends on the build's -ffp-contract; the
// __f*_rn intrinsics are not used, as this toolchain maps __fsqrt_rn to the approximate native square root - and the order
// below is the whole definition of the result:
//   s[d]  = the rows of the class added in ascending row order into one accumulator, starting from 0
//   m[d]  = s[d] / n
//   q[t]  = fma(m[d], m[d], q[t]) over d = t, t + CM_THREADS, ... in ascending order, starting from 0 (thread t)
//   ss    = q[0] + q[1] + ... + q[CM_THREADS - 1] in ascending t into one accumulator, starting from 0
//   W[d]  = m[d] / (eps + sqrt(ss)); columns E..ldw-1 = 0
// An empty class has no mean: its row comes out NaN (0 / 0).  Callers reject it before the launch (ops.zeroshot_class_mean).
//
// Ranks, one workgroup per 128 images that sweeps the class tiles twice in ascending order.  Every v_ic of both sweeps comes out
// of rank_tile (rank_tile.h: one ascending-k fp32 MFMA chain per output, no split-K, no scale), so the t_i that sweep 1 finds
// compares with its own entry in sweep 2 exactly, and so does the row maximum.  Sweep 1 keeps, per lane and row, the running
// maximum and the running label maximum; the 64 candidates of a row meet once at the end.  Sweep 2 counts against t_i and takes
// the lowest class whose value equals the row maximum (both held in LDS).  Which entries of a tile are labels is a 128-bit mask
// per row, rebuilt from the label list for every tile.  Maxima, minima and integer sums only: no atomics, no workspace, plain
// stores, and the result does not depend on the order in which lanes meet.
// LDS: the 64 KiB ring of rank_tile plus 3 KiB of static arrays: two workgroups per CU.
#include "rank_tile.h"

namespace clipa_gemm {
namespace {

constexpr int CM_THREADS = 256;
constexpr int ZS_MAX_LABELS = 32;

__global__ __launch_bounds__(CM_THREADS) void zeroshot_class_mean_kernel(const float* __restrict__ emb,
                                                                         const int* __restrict__ offsets, int N, int E, long lde,
                                                                         float eps, float* __restrict__ W, long ldw) {
  __shared__ float part[CM_THREADS];
  __shared__ float snorm;
  const int t = threadIdx.x, c = blockIdx.x;
  const int lo = max(offsets[c], 0), hi = min(offsets[c + 1], N);
  const float n = (float)(hi - lo);
  float* w = W + (long)c * ldw;
  float q = 0.f;
  for (int d = t; d < E; d += CM_THREADS) {
    float s = 0.f;
    for (int r = lo; r < hi; ++r) s += emb[(long)r * lde + d];
    const float m = s / n;                     // hipcc's float division and sqrtf are correctly rounded (its default)
    w[d] = m;
    q = fmaf(m, m, q);
  }
  part[t] = q;
  __syncthreads();
  if (t == 0) {
    float ss = 0.f;
    for (int k = 0; k < CM_THREADS; ++k) ss += part[k];
    snorm = eps + sqrtf(ss);
  }
  __syncthreads();
  const float den = snorm;
  for (int d = t; d < ldw; d += CM_THREADS) w[d] = d < E ? w[d] / den : 0.f;   // w[d]: this thread's own store
}

// what the two column waves of a tile row combine at the end of sweep 1 and of sweep 2 (rank_row_meet)
struct ZsMax { float best, t; };
struct ZsOut { int gt, eq, pred; };

__global__ __launch_bounds__(RTHREADS, 2) void zeroshot_ranks_kernel(const char* __restrict__ A, const char* __restrict__ W,
                                                                     const int* __restrict__ labels, int B, int C, int E,
                                                                     int Lmax, long lda, long ldw, int* __restrict__ gt,
                                                                     int* __restrict__ eq, int* __restrict__ pred) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ unsigned smask[RT * 4];            // [row][wn][ni]: bit L = class n0 + wn * 64 + ni * 32 + L is a label of the row
  __shared__ float st[RT], sbest[RT];           // t_i and max_c v_ic
  const RankLane t = rank_lane();
  const int tid = t.tid, L = t.L, wn = t.wn;
  const int m0 = blockIdx.x * RT;
  int rowsA, rowsB;
  const __amdgpu_buffer_rsrc_t rsA = rank_rows(A, m0, B, lda, &rowsA);
  const int Tc = (C + RT - 1) / RT;
  constexpr int NONE = 0x7fffffff;
  const float ninf = -__builtin_huge_valf();
  // this thread's half (64 classes from n0 + 64 * (tid & 1)) of the label mask of row tid / 2; a label outside [0, C) sets nothing
  auto build_mask = [&](int n0) {
    const int row = m0 + (tid >> 1);
    const int base = n0 + 64 * (tid & 1);
    unsigned long long m = 0;
    if (row < B) {
      const int* lab = labels + (long)row * Lmax;
      for (int l = 0; l < Lmax; ++l) {
        const int c = lab[l];
        const unsigned d = (unsigned)(c - base);
        if (d < 64u && c < C) m |= 1ull << d;
      }
    }
    smask[2 * tid] = (unsigned)m;
    smask[2 * tid + 1] = (unsigned)(m >> 32);
  };
  f32x16 acc[2][2];

  // ---- sweep 1: t_i and the row maximum
  {
    float bv[32], tv[32];
#pragma unroll
    for (int q = 0; q < 32; ++q) { bv[q] = ninf; tv[q] = ninf; }
    for (int tn = 0; tn < Tc; ++tn) {
      const int n0 = tn * RT;
      const __amdgpu_buffer_rsrc_t rsB = rank_rows(W, n0, C, ldw, &rowsB);
      __syncthreads();                        // the previous tile's readers are done with the ring and with the mask
      build_mask(n0);
      rank_tile(smem, rsA, rsB, lda, ldw, E, acc);      // its first barrier (E >= 1) publishes the mask
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        if (t.col(ni, n0) < C) {
#pragma unroll
          for (int q = 0; q < 32; ++q) {
            const unsigned mw = smask[(t.row(q) * 2 + wn) * 2 + ni];
            const float v = acc[q >> 4][ni][q & 15];
            bv[q] = v > bv[q] ? v : bv[q];
            tv[q] = ((mw >> L) & 1u) && v > tv[q] ? v : tv[q];
          }
        }
      }
    }
    auto fmax2 = [](float a, float b) { return b > a ? b : a; };
    halve32(bv, L, fmax2);
    halve32(tv, L, fmax2);
    __syncthreads();                          // the ring is dead: its first bytes take the two column waves' halves
    const ZsMax m = rank_row_meet(t, (ZsMax*)smem, ZsMax{bv[0], tv[0]},
                                  [&](ZsMax a, ZsMax b) { return ZsMax{fmax2(a.best, b.best), fmax2(a.t, b.t)}; });
    if (tid < RT) { sbest[tid] = m.best; st[tid] = m.t; }
  }

  // ---- sweep 2: counts against t_i (gt | eq << 16 per lane and row: at most 2 entries a tile, and the entry point keeps C below 2^20) and the lowest
  // class that reaches the row maximum
  int cnt[32], pc[32];
#pragma unroll
  for (int q = 0; q < 32; ++q) { cnt[q] = 0; pc[q] = NONE; }
  for (int tn = 0; tn < Tc; ++tn) {
    const int n0 = tn * RT;
    const __amdgpu_buffer_rsrc_t rsB = rank_rows(W, n0, C, ldw, &rowsB);
    __syncthreads();                          // tn = 0: also publishes st and sbest
    build_mask(n0);
    rank_tile(smem, rsA, rsB, lda, ldw, E, acc);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int cls = t.col(ni, n0);
      if (cls < C) {
#pragma unroll
        for (int q = 0; q < 32; ++q) {
          const unsigned mw = smask[(t.row(q) * 2 + wn) * 2 + ni];
          const float tq = st[t.row(q)], best = sbest[t.row(q)];
          const float v = acc[q >> 4][ni][q & 15];
          const bool lab = (mw >> L) & 1u;
          cnt[q] += (int)(v > tq) + ((int)(!lab && v == tq) << 16);
          pc[q] = v == best && cls < pc[q] ? cls : pc[q];
        }
      }
    }
  }
  int cg[32];
#pragma unroll
  for (int q = 0; q < 32; ++q) { cg[q] = cnt[q] & 0xffff; cnt[q] >>= 16; }
  auto add2 = [](int a, int b) { return a + b; };
  halve32(cg, L, add2);
  halve32(cnt, L, add2);
  halve32(pc, L, [](int a, int b) { return b < a ? b : a; });
  __syncthreads();                            // the ring is dead
  const ZsOut o = rank_row_meet(t, (ZsOut*)smem, ZsOut{cg[0], cnt[0], pc[0]},
                                [](ZsOut a, ZsOut b) { return ZsOut{a.gt + b.gt, a.eq + b.eq, min(a.pred, b.pred)}; });
  if (tid < rowsA) { gt[m0 + tid] = o.gt; eq[m0 + tid] = o.eq; pred[m0 + tid] = o.pred; }
}

LdsOptIn g_zs_lds;

}  // namespace
}  // namespace clipa_gemm

using namespace clipa_gemm;

extern "C" int clipa_zeroshot_class_mean(const float* emb, const int32_t* offsets, int64_t N, int64_t C, int64_t E, int64_t lde,
                                         float eps, float* W, int64_t ldw, void* stream) {
  if (N < 0 || C < 0 || E < 0 || lde < E || ldw < E || N >= (1L << 31) || C >= (1L << 31) || E >= (1L << 31) - CM_THREADS ||
      ldw >= (1L << 31) - CM_THREADS) {
    clipa_set_error("zeroshot_class_mean: N = %ld, C = %ld, E = %ld, lde = %ld, ldw = %ld out of range (lde, ldw >= E)", (long)N,
                    (long)C, (long)E, (long)lde, (long)ldw);
    return CLIPA_ERR_ARG;
  }
  if (!(eps >= 0.f)) { clipa_set_error("zeroshot_class_mean: eps = %g must be >= 0", (double)eps); return CLIPA_ERR_ARG; }
  if (C == 0) return CLIPA_OK;
  if (N < C) { clipa_set_error("zeroshot_class_mean: N = %ld rows cannot fill C = %ld classes (an empty class has no mean)", (long)N, (long)C); return CLIPA_ERR_ARG; }
  if (int rc = clipa_check_ptrs16("zeroshot_class_mean", {emb, offsets, W})) return rc;
  hipLaunchKernelGGL(zeroshot_class_mean_kernel, dim3((unsigned)C), dim3(CM_THREADS), 0, (hipStream_t)stream, emb, offsets, (int)N,
                     (int)E, (long)lde, eps, W, (long)ldw);
  return clipa_check_launch("zeroshot_class_mean");
}

extern "C" int clipa_zeroshot_ranks(const float* A, const float* W, const int32_t* labels, int64_t B, int64_t C, int64_t E,
                                    int64_t Lmax, int64_t lda, int64_t ldw, int32_t* gt, int32_t* eq, int32_t* pred, void* stream) {
  if (B < 0 || C < 0 || E < 0) { clipa_set_error("zeroshot_ranks: B = %ld, C = %ld, E = %ld must be >= 0", (long)B, (long)C, (long)E); return CLIPA_ERR_ARG; }
  if (Lmax < 1 || Lmax > ZS_MAX_LABELS) { clipa_set_error("zeroshot_ranks: Lmax = %ld must lie in [1, %d]", (long)Lmax, ZS_MAX_LABELS); return CLIPA_ERR_ARG; }
  if (B == 0) return CLIPA_OK;
  if (C < 1 || E < 1) { clipa_set_error("zeroshot_ranks: C = %ld classes of E = %ld columns for B = %ld rows (nothing to rank)", (long)C, (long)E, (long)B); return CLIPA_ERR_ARG; }
  if (int rc = rank_check_args("zeroshot_ranks", E, lda, ldw, B >= (1L << 31) - RT || C >= (1L << 20) || B * Lmax >= (1L << 31), "B, C (below 2^20)",
                               {A, W, labels, gt, eq, pred}, nullptr)) return rc;
  return rank_launch(g_zs_lds, {(const void*)zeroshot_ranks_kernel}, 2 * R_STAGE, "zeroshot_ranks", zeroshot_ranks_kernel,
                     (B + RT - 1) / RT, 2 * R_STAGE, stream, "zeroshot_ranks", (const char*)A, (const char*)W, labels, (int)B, (int)C,
                     (int)E, (int)Lmax, (long)lda, (long)ldw, gt, eq, pred);
}
