// Retrieval ranks of the validation metrics (get_clip_metrics, clipa_torch/training/train.py:432-449) without the
// [N, N] logit matrix: v_ij = fl(s * x_ij), x_ij = A_i . B_j in fp32, and per image row i / text column j the number of
// OTHER entries of that row / column that beat (gt) or tie (eq) the positive v_ii / v_jj.  The reference's 0-based rank
// of the positive from an unstable descending argsort lies in [gt, gt + eq]; the engine reports gt (ties resolved in the
// positive's favour, deterministically).
//
// Arithmetic: v_mfma_f32_32x32x2_f32, one accumulator chain per output in ascending k (bit for bit a chain of fp32 fmaf),
// no split-K.  Every x_ij - the diagonal included - comes out of the same code, so v_ii compares with itself exactly:
//   launch 1 (DIAG): the diagonal tiles only; writes v_ii to the workspace and zeroes the four count arrays of its rows;
//   launch 2: every tile; the epilogue counts v_ij > / == v_ii (row i) and v_jj (column j), i != j excluded, reduces
//             within the wave and across waves in LDS and adds one int per row and per column of the tile atomically.
// Memory: O(N) (the workspace is N floats).
//
// Main loop, LDS image and count epilogue: rank_tile.h, shared with retrieval_multi.hip.  Its epilogue excludes the positive
// itself from eq only; from gt it needs no exclusion, since v_ii > v_ii is false and v_ii compares with itself exactly.
#include "rank_tile.h"

namespace clipa_gemm {
namespace {

struct RankArgs {
  const char* A; const char* B;
  int N, E;
  long lda, ldb;                              // elements
  const float* scale;
  float* diag;                                // [N] v_ii
  int* i2t_gt; int* i2t_eq; int* t2i_gt; int* t2i_eq;
};

template <bool DIAG>
__global__ __launch_bounds__(RTHREADS, 2) void retrieval_kernel(RankArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const RankLane t = rank_lane();
  const int tid = t.tid;
  const int T = (p.N + RT - 1) / RT;
  int tm, tn;
  if (DIAG) {
    tm = tn = blockIdx.x;
  } else {
    tm = blockIdx.x / T;
    tn = blockIdx.x - tm * T;
  }
  const int m0 = tm * RT, n0 = tn * RT;
  int rowsA, rowsB;
  const __amdgpu_buffer_rsrc_t rsA = rank_rows(p.A, m0, p.N, p.lda, &rowsA);
  const __amdgpu_buffer_rsrc_t rsB = rank_rows(p.B, n0, p.N, p.ldb, &rowsB);

  // the positives of this tile's rows (tid < 128) and columns: loaded now, used in the epilogue
  float dpos = 0.f;
  if (!DIAG) {
    const int g = tid < RT ? m0 + tid : n0 + tid - RT;
    if (g < p.N) dpos = p.diag[g];
  }

  f32x16 acc[2][2];
  rank_tile(smem, rsA, rsB, p.lda, p.ldb, p.E, acc);

  const float s = p.scale ? p.scale[0] : 1.0f;
  if (DIAG) {
    // zero the counts of this tile's rows, write v_ii
    if (tid < RT && m0 + tid < p.N) {
      p.i2t_gt[m0 + tid] = 0; p.i2t_eq[m0 + tid] = 0; p.t2i_gt[m0 + tid] = 0; p.t2i_eq[m0 + tid] = 0;
    }
    if (t.wm == t.wn) {                       // the waves that hold the tile's diagonal: in acc[mi][mi], where row == column
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int il = t.row(mi * 16 + r);
          if (il == t.col(mi) && m0 + il < p.N) p.diag[m0 + il] = s * acc[mi][mi][r];
        }
    }
    return;
  }

  // the positive of column j is row j: the identity correspondence of retrieval_multi.hip
  const int cj[2] = {t.col(0, n0), t.col(1, n0)};
  rank_count(smem, m0, n0, rowsA, rowsB, dpos, s, cj, acc, p.i2t_gt, p.i2t_eq, p.t2i_gt, p.t2i_eq);
}

LdsOptIn g_rk_lds;

}  // namespace
}  // namespace clipa_gemm

using namespace clipa_gemm;

extern "C" int64_t clipa_retrieval_ranks_workspace(int64_t N) {
  return (N > 0 ? N : 1) * (int64_t)sizeof(float);          // v_ii
}

extern "C" int clipa_retrieval_ranks(const float* A, const float* B, int64_t N, int64_t E, int64_t lda, int64_t ldb,
                                     const float* scale, int32_t* i2t_gt, int32_t* i2t_eq, int32_t* t2i_gt,
                                     int32_t* t2i_eq, void* workspace, int64_t workspace_bytes, void* stream) {
  if (N < 1 || E < 1) { clipa_set_error("retrieval_ranks: N = %ld and E = %ld must be >= 1", (long)N, (long)E); return CLIPA_ERR_ARG; }
  if (int rc = rank_check_args("retrieval_ranks", E, lda, ldb, N >= (1L << 30), "N",
                               {A, B, i2t_gt, i2t_eq, t2i_gt, t2i_eq, workspace}, scale)) return rc;
  if (workspace_bytes < clipa_retrieval_ranks_workspace(N)) { clipa_set_error("retrieval_ranks: workspace too small"); return CLIPA_ERR_ARG; }
  const int64_t T = (N + RT - 1) / RT;
  RankArgs a = {};
  a.A = (const char*)A; a.B = (const char*)B; a.N = (int)N; a.E = (int)E; a.lda = lda; a.ldb = ldb; a.scale = scale;
  a.diag = (float*)workspace; a.i2t_gt = i2t_gt; a.i2t_eq = i2t_eq; a.t2i_gt = t2i_gt; a.t2i_eq = t2i_eq;
  auto launch = [&](auto kernel, int64_t grid, const char* name) {
    return rank_launch(g_rk_lds, {(const void*)retrieval_kernel<true>, (const void*)retrieval_kernel<false>}, 2 * R_STAGE,
                       "retrieval", kernel, grid, 2 * R_STAGE, stream, name, a);
  };
  if (int rc = launch(retrieval_kernel<true>, T, "retrieval_diag")) return rc;
  return launch(retrieval_kernel<false>, T * T, "retrieval_ranks");
}
