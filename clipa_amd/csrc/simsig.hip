// Fused similarity + pairwise sigmoid loss of SigLIP (the element maths of clipa_jax/losses/common.py:25-32, sigmoid_xent):
//   l = s * A . B^T + b   (A = this rank's image embeddings [R, E], B = all gathered text embeddings [N, E], bf16; s, b on
//   the device),  y = +1 at column label0 + r and -1 elsewhere,  t = y * l
//   loss_r = sum_j softplus(-t_rj)          d loss / d l_rj = -y_rj * sigmoid(-t_rj)
// Every element of the loss and of its gradient depends on its own logit only (no row-wise log-sum-exp), so ONE pass over
// the similarity GEMM yields both: the epilogue turns each 256 x 256 tile into the bf16 gradient matrix
// s * gscale * d loss / d l  that the two gradient GEMMs consume, plus per-row partials (loss, d loss / d s, d loss / d b)
// that a second tiny kernel sums over the tile columns.  The [R, N] fp32 logits never reach HBM.
//
// Numerics: with a = |t| and e = exp(-a) <= 1,  softplus(-t) = max(-t, 0) + log1p(e)  and  sigmoid(-t) = (t > 0 ? e : 1) /
// (1 + e): one exp, one log and one reciprocal per element, nothing overflows at |l| ~ 110 (logit_scale is clamped at
// log 100).  log1p(e) is the series e - e^2/2 + e^3/3 - e^4/4 below e = 1/64 (truncation < 2e-9 relative), where
// fl(1 + e) would round e itself away, and log(1 + e) above it (rounding of 1 + e < 4e-6 relative there).
//
// Tile / ring / fragments: sim_tile<4>, exactly as simce.hip uses it.
#include "sim_tile.h"

namespace clipa_gemm {
namespace {

struct SigArgs {
  const char* A; const char* B;
  int R, N, K;
  long lda, ldb;
  const float* scale; const float* bias;
  long label0;
  float gscale;
  float* part;          // [tilesN][R][3] per-tile partial (loss, d loss / d s, d loss / d b); GRAD = false fills [0] only
  unsigned short* dl;   // GRAD: bf16 [R, ldd] = s * gscale * d loss / d l, columns >= N zero
  long ldd;
};

template <bool GRAD>
__global__ __launch_bounds__(NTHREADS) void simsig_kernel(SigArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const int wm = wave >> 2, wn = wave & 3;   // wave tile: 128 (m) x 64 (n)
  const int tilesN = (p.N + BN - 1) / BN;
  const int tm = blockIdx.x / tilesN, tn = blockIdx.x - tm * tilesN;
  const int m0 = tm * BM, n0 = tn * BN;
  const int rowsA = min(BM, p.R - m0), rowsB = min(BN, p.N - n0);

  f32x16 acc[2][4];
  sim_tile<4>(smem, p.A + (size_t)m0 * p.lda * 2, p.B + (size_t)n0 * p.ldb * 2, p.lda, p.ldb, p.K, rowsA, rowsB, acc);
  __syncthreads();                                   // the ring is dead: its first bytes become the cross-wave scratch
  float* red = (float*)smem;                         // [4 wn][256 rows][3]

  // D[n][m] fragment: lane holds row m = wm*128 + mi*32 + l31 and columns n = wn*64 + ni*32 + 8*(r>>2) + 4*hi + (r&3)
  const float s = p.scale[0], b = p.bias[0];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int rl = wm * 128 + mi * 32 + l31;          // row within the tile
    const int m = m0 + rl;
    const int label = (int)p.label0 + m;           // label0 + R <= N: fits an int
    float ls = 0.f, ds = 0.f, db = 0.f;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n0 + wn * 64 + ni * 32 + 8 * q + 4 * hi;
        float g[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x = acc[ni][mi][4 * q + e];
          const bool valid = n + e < p.N;
          const bool pos = n + e == label;
          // the loss term is spelled in explicit fma / add steps: both instantiations round it identically
          const float l = __builtin_fmaf(s, x, b);
          const float mt = pos ? -l : l;              // -t
          const float ex = __expf(-__builtin_fabsf(l));
          const float u = 1.0f + ex;
          float ser = __builtin_fmaf(ex, -0.25f, 1.0f / 3.0f);
          ser = __builtin_fmaf(ex, -ser, 0.5f);
          ser = __builtin_fmaf(ex, -ser, 1.0f);
          const float relu = fmaxf(mt, 0.f);
          const float term = ex < 0.015625f ? __builtin_fmaf(ex, ser, relu) : relu + __logf(u);
          ls += valid ? term : 0.f;
          if (GRAD) {
            const float sg = (mt >= 0.f ? 1.0f : ex) * __builtin_amdgcn_rcpf(u);     // sigmoid(-t)
            float gg = p.gscale * sg;                 // d loss / d l = -y * sigmoid(-t)
            gg = pos ? -gg : gg;
            gg = valid ? gg : 0.f;
            ds += gg * x;                             // d loss / d s
            db += gg;                                 // d loss / d b
            g[e] = gg * s;                            // d loss / d raw
          }
        }
        if (GRAD) {
          if (m < p.R && n < p.ldd) {
            u32x2 w;
            w[0] = pack2bf(g[0], g[1]);
            w[1] = pack2bf(g[2], g[3]);
            *(u32x2*)(p.dl + (size_t)m * p.ldd + n) = w;
          }
        }
        // one group of four elements at a time: interleaving the 32 unrolled groups of a row for latency costs more live
        // registers than the 128 left beside acc
        __builtin_amdgcn_sched_barrier(0);
      }
    ls += __shfl_xor(ls, 32, 64);
    if (GRAD) {
      ds += __shfl_xor(ds, 32, 64);
      db += __shfl_xor(db, 32, 64);
    }
    if (hi == 0) {
      float* o = red + (wn * 256 + rl) * 3;
      o[0] = ls;
      if (GRAD) { o[1] = ds; o[2] = db; }
    }
  }
  __syncthreads();
  if (tid < 256 && m0 + tid < p.R) {
    float* o = p.part + ((size_t)tn * p.R + m0 + tid) * 3;
#pragma unroll
    for (int c = 0; c < (GRAD ? 3 : 1); ++c)
      o[c] = (red[tid * 3 + c] + red[(256 + tid) * 3 + c]) + (red[(512 + tid) * 3 + c] + red[(768 + tid) * 3 + c]);
  }
}

// Instantiated explicitly, as in simce.hip: hipcc's host pass leaves the second implicit instantiation of a kernel whose
// body calls sim_tile (a device function template that holds a lambda) undefined.
template __global__ void simsig_kernel<false>(SigArgs);
template __global__ void simsig_kernel<true>(SigArgs);

// sum the per-tile partials per row; dscale_rows / dbias_rows null = forward only
__global__ void simsig_merge_kernel(const float* __restrict__ part, int tilesN, long R, float* __restrict__ loss_rows,
                                    float* __restrict__ dscale_rows, float* __restrict__ dbias_rows) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  float a = 0.f;
  for (int t = 0; t < tilesN; ++t) a += part[((size_t)t * R + r) * 3];
  loss_rows[r] = a;
  if (dscale_rows) {
    float c = 0.f, d = 0.f;
    for (int t = 0; t < tilesN; ++t) {
      c += part[((size_t)t * R + r) * 3 + 1];
      d += part[((size_t)t * R + r) * 3 + 2];
    }
    dscale_rows[r] = c;
    dbias_rows[r] = d;
  }
}

LdsOptIn g_sig_lds;
int ensure_sig_attrs(int dev) {
  return g_sig_lds.ensure(dev, {(const void*)simsig_kernel<false>, (const void*)simsig_kernel<true>}, 2 * STAGE_BYTES, "simsig");
}

}  // namespace
}  // namespace clipa_gemm

using namespace clipa_gemm;

extern "C" int64_t clipa_simsig_workspace(int64_t R, int64_t N) {
  const int64_t tilesN = (N + BN - 1) / BN;
  return tilesN * R * 3 * (int64_t)sizeof(float);
}

extern "C" int clipa_simsig(const void* rows, const void* cols, int64_t R, int64_t N, int64_t E, int64_t lda, int64_t ldb,
                            const float* scale, const float* bias, int64_t label0, float gscale, float* loss_rows,
                            void* dlogits_bf16, int64_t ldd, float* dscale_rows, float* dbias_rows, void* workspace,
                            int64_t workspace_bytes, void* stream) {
  if (R <= 0) return CLIPA_OK;
  if (E <= 0 || E % 8 != 0 || lda % 8 != 0 || ldb % 8 != 0) { clipa_set_error("simsig: E, lda, ldb must be multiples of 8"); return CLIPA_ERR_ARG; }
  if (N <= 0 || label0 < 0 || label0 + R > N) { clipa_set_error("simsig: labels [%ld, %ld) outside [0, %ld)", (long)label0, (long)(label0 + R), (long)N); return CLIPA_ERR_ARG; }
  if (256 * lda * 2 >= (1L << 30) || 256 * ldb * 2 >= (1L << 30)) { clipa_set_error("simsig: leading dimension too large"); return CLIPA_ERR_ARG; }
  if (!rows || !cols || !scale || !bias || !loss_rows) { clipa_set_error("simsig: rows, cols, scale, bias, loss_rows must not be null"); return CLIPA_ERR_ARG; }
  const bool grad = dlogits_bf16 || dscale_rows || dbias_rows;
  const int64_t tilesN = (N + BN - 1) / BN, tilesM = (R + BM - 1) / BM;
  if (grad) {
    if (!dlogits_bf16 || !dscale_rows || !dbias_rows) { clipa_set_error("simsig: the three gradient outputs come together (all null = forward only)"); return CLIPA_ERR_ARG; }
    const int64_t N8 = (N + 7) & ~(int64_t)7;
    if (ldd % 8 != 0 || ldd < N8 || ldd > tilesN * BN) { clipa_set_error("simsig: dlogits needs ldd %% 8 == 0 and N rounded up to 8 <= ldd <= N rounded up to 256"); return CLIPA_ERR_ARG; }
  }
  if (!workspace || workspace_bytes < clipa_simsig_workspace(R, N)) { clipa_set_error("simsig: workspace too small"); return CLIPA_ERR_ARG; }
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (int rc = ensure_sig_attrs(dev)) return rc;
  SigArgs a = {};
  a.A = (const char*)rows; a.B = (const char*)cols; a.R = (int)R; a.N = (int)N; a.K = (int)E; a.lda = lda; a.ldb = ldb;
  a.scale = scale; a.bias = bias; a.label0 = label0; a.gscale = gscale; a.part = (float*)workspace;
  a.dl = (unsigned short*)dlogits_bf16; a.ldd = ldd;    // columns [N, ldd) are written as zeros
  hipStream_t st = (hipStream_t)stream;
  if (grad) hipLaunchKernelGGL(simsig_kernel<true>, dim3((unsigned)(tilesM * tilesN)), dim3(NTHREADS), 2 * STAGE_BYTES, st, a);
  else hipLaunchKernelGGL(simsig_kernel<false>, dim3((unsigned)(tilesM * tilesN)), dim3(NTHREADS), 2 * STAGE_BYTES, st, a);
  if (int rc = clipa_check_launch("simsig")) return rc;
  hipLaunchKernelGGL(simsig_merge_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, a.part, (int)tilesN, (long)R,
                     loss_rows, dscale_rows, dbias_rows);
  return clipa_check_launch("simsig_merge");
}
