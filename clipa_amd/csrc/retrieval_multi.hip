// Multi-caption image-text retrieval ranks (clipa_jax/evaluators/proj/image_text/image_text_retrieval.py,
// image_to_text_retrieval_eval / text_to_image_retrieval_eval) without the [Ni, Nt] similarity matrix.  Image features
// A [Ni, E], text features B [Nt, E], text t describes image c(t); v_it = fl(s * x_it), x_it = A_i . B_t in fp32:
//   p_t = v_{c(t), t}   m_i = max over {t : c(t) = i} of p_t (-inf: image i has no caption)
//   t2i_gt[t] = #{i : v_it > p_t}   t2i_eq[t] = #{i != c(t) : v_it == p_t}          (column t, text -> image)
//   i2t_gt[i] = #{t : v_it > m_i}   i2t_eq[i] = #{t : c(t) != i, v_it == m_i}       (row i, image -> text)
// i2t_gt is the 0-based position of image i's best caption (its other captions cannot beat m_i), t2i_gt that of text
// t's image; ties resolve in the positive's favour, as in retrieval.hip.
//
// Arithmetic: rank_tile (rank_tile.h), the main loop retrieval.hip's kernel runs too (one ascending-k fp32 MFMA chain per
// output, no split-K; tests/test_retrieval_multi_gpu.py checks the two agree bit for bit), so every x_it - the positives
// included - comes out of the same code whichever launch or tile computes it.  Three launches:
//   init: counts = 0, p_t = NaN, m_i = key(-inf);
//   POS:  one workgroup per 128-text tile, over the image tiles [min c, max c] of its texts (tiles that hold none of their
//         images skipped): writes p_t and takes m_i by an integer atomicMax on an order-preserving key of the float.
//         Sorted c (the captions of an image adjacent) makes this about Ti + Tt tiles;
//   count: every Ti x Tt tile; the epilogue counts against m_i (rows) and p_t (columns), c of the tile's columns gives the
//         eq exclusions (rank_count, rank_tile.h, shared with retrieval.hip) and adds one int per row and per column of the tile atomically.
// Memory: O(Ni + Nt) (the workspace is p_t and the keys of m_i).
#include "rank_tile.h"

namespace clipa_gemm {
namespace {

struct MultiArgs {
  const char* A; const char* B; const int* c;
  int Ni, Nt, E;
  long lda, ldb;                              // elements
  const float* scale;
  float* pos;                                 // [Nt] p_t
  unsigned* mkey;                             // [Ni] key(m_i)
  int* i2t_gt; int* i2t_eq; int* t2i_gt; int* t2i_eq;
};

__global__ __launch_bounds__(RTHREADS) void multi_init_kernel(MultiArgs p) {
  const int g = blockIdx.x * RTHREADS + threadIdx.x;
  if (g < p.Ni) { p.mkey[g] = f32_key(-__builtin_huge_valf()); p.i2t_gt[g] = 0; p.i2t_eq[g] = 0; }
  if (g < p.Nt) { p.pos[g] = __builtin_nanf(""); p.t2i_gt[g] = 0; p.t2i_eq[g] = 0; }
}

template <bool POS>
__global__ __launch_bounds__(RTHREADS, 2) void retrieval_multi_kernel(MultiArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const RankLane t = rank_lane();
  const int tid = t.tid;
  const int Tt = (p.Nt + RT - 1) / RT;
  const int tm0 = POS ? 0 : blockIdx.x / Tt;
  const int tn = POS ? blockIdx.x : blockIdx.x - tm0 * Tt;
  const int n0 = tn * RT;
  int rowsA, rowsB;
  const __amdgpu_buffer_rsrc_t rsB = rank_rows(p.B, n0, p.Nt, p.ldb, &rowsB);
  const float s = p.scale ? p.scale[0] : 1.0f;
  // c of this lane's two accumulator columns (-1 past Nt); only ever compared, never used as an index
  int cj[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    cj[ni] = t.col(ni) < rowsB ? p.c[t.col(ni, n0)] : -1;
  }
  f32x16 acc[2][2];

  if (POS) {
    // image-tile range of this tile's texts; values outside [0, Ni) are ignored (their p_t stays NaN)
    __shared__ int srange[2];
    const int ct = tid < rowsB ? p.c[n0 + tid] : -1;
    const bool valid = ct >= 0 && ct < p.Ni;
    if (tid == 0) { srange[0] = 0x7fffffff; srange[1] = -1; }
    __syncthreads();
    if (valid) { atomicMin(&srange[0], ct / RT); atomicMax(&srange[1], ct / RT); }
    __syncthreads();
    const int lo = srange[0], hi_t = srange[1];
    for (int tm = lo; tm <= hi_t; ++tm) {
      // doubles as the barrier before the ring is staged again
      if (!__syncthreads_or(valid && ct / RT == tm)) continue;
      const int m0 = tm * RT;
      const __amdgpu_buffer_rsrc_t rsA = rank_rows(p.A, m0, p.Ni, p.lda, &rowsA);
      rank_tile(smem, rsA, rsB, p.lda, p.ldb, p.E, acc);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = t.row(mi * 16 + r, m0);
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
            if (cj[ni] == i && i < p.Ni) {      // rows past Ni: a bad c must not reach them
              const float v = s * acc[mi][ni][r];
              p.pos[t.col(ni, n0)] = v;
              atomicMax(p.mkey + i, f32_key(v));
            }
        }
    }
    return;
  }

  const int m0 = tm0 * RT;
  const __amdgpu_buffer_rsrc_t rsA = rank_rows(p.A, m0, p.Ni, p.lda, &rowsA);
  // the positives of this tile's rows (tid < 128: m_i) and columns (p_t): loaded now, used in the epilogue
  float dpos = 0.f;
  if (tid < RT) {
    if (tid < rowsA) dpos = f32_unkey(p.mkey[m0 + tid]);
  } else if (tid - RT < rowsB) {
    dpos = p.pos[n0 + tid - RT];
  }
  rank_tile(smem, rsA, rsB, p.lda, p.ldb, p.E, acc);

  rank_count(smem, m0, n0, rowsA, rowsB, dpos, s, cj, acc, p.i2t_gt, p.i2t_eq, p.t2i_gt, p.t2i_eq);
}

LdsOptIn g_rkm_lds;

}  // namespace
}  // namespace clipa_gemm

using namespace clipa_gemm;

static int64_t round4(int64_t n) { return ((n > 0 ? n : 1) + 3) / 4 * 4; }

extern "C" int64_t clipa_retrieval_ranks_multi_workspace(int64_t Ni, int64_t Nt) {
  return (round4(Nt) + round4(Ni)) * (int64_t)sizeof(float);          // p_t, key(m_i)
}

extern "C" int clipa_retrieval_ranks_multi(const float* A, const float* B, const int32_t* txt2img, int64_t Ni, int64_t Nt,
                                           int64_t E, int64_t lda, int64_t ldb, const float* scale, int32_t* i2t_gt,
                                           int32_t* i2t_eq, int32_t* t2i_gt, int32_t* t2i_eq, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
  if (Ni < 1 || Nt < 1 || E < 1) {
    clipa_set_error("retrieval_ranks_multi: Ni = %ld, Nt = %ld and E = %ld must be >= 1", (long)Ni, (long)Nt, (long)E);
    return CLIPA_ERR_ARG;
  }
  const int64_t Ti = (Ni + RT - 1) / RT, Tt = (Nt + RT - 1) / RT;
  if (int rc = rank_check_args("retrieval_ranks_multi", E, lda, ldb, Ni >= (1L << 30) || Nt >= (1L << 30) || Ti * Tt >= (1L << 31),
                               "Ni, Nt", {A, B, txt2img, i2t_gt, i2t_eq, t2i_gt, t2i_eq, workspace}, scale)) return rc;
  if (workspace_bytes < clipa_retrieval_ranks_multi_workspace(Ni, Nt)) { clipa_set_error("retrieval_ranks_multi: workspace too small"); return CLIPA_ERR_ARG; }
  MultiArgs a = {};
  a.A = (const char*)A; a.B = (const char*)B; a.c = txt2img; a.Ni = (int)Ni; a.Nt = (int)Nt; a.E = (int)E;
  a.lda = lda; a.ldb = ldb; a.scale = scale;
  a.pos = (float*)workspace; a.mkey = (unsigned*)((char*)workspace + round4(Nt) * sizeof(float));
  a.i2t_gt = i2t_gt; a.i2t_eq = i2t_eq; a.t2i_gt = t2i_gt; a.t2i_eq = t2i_eq;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nmax = Ni > Nt ? Ni : Nt;
  hipLaunchKernelGGL(multi_init_kernel, dim3((unsigned)((nmax + RTHREADS - 1) / RTHREADS)), dim3(RTHREADS), 0, st, a);
  if (int rc = clipa_check_launch("retrieval_multi_init")) return rc;
  auto launch = [&](auto kernel, int64_t grid, const char* name) {
    return rank_launch(g_rkm_lds, {(const void*)retrieval_multi_kernel<true>, (const void*)retrieval_multi_kernel<false>},
                       2 * R_STAGE, "retrieval_multi", kernel, grid, 2 * R_STAGE, stream, name, a);
  };
  if (int rc = launch(retrieval_multi_kernel<true>, Tt, "retrieval_multi_positives")) return rc;
  return launch(retrieval_multi_kernel<false>, Ti * Tt, "retrieval_ranks_multi");
}
