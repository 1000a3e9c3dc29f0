// Fused similarity + cross-entropy + distillation loss for one direction of DistillClipLoss
// (clipa_torch/open_clip/loss.py:202-238): student logits z = s * A_s . B_s^T (K = E_s), teacher logits
// y = u * A_t . B_t^T (K = E_t, may differ from E_s), s and u read from DEVICE memory, labels label0 + r:
//   ce_r   = lse_j z_rj - z_r,label
//   dist_r = -sum_j softmax_j(y_rj) log_softmax_j(z_rj) = lse_j z_rj - sum_j p^t_rj z_rj
// Neither [R, N] fp32 logit matrix reaches HBM.  The forward runs both GEMMs per output tile and reduces the pair to
// per-row partials (max z, sum exp z, max y, sum exp y, sum exp(y - max y) z: 20 bytes per row and tile); a merge kernel
// turns them into lse_s, lse_t, ce_rows and dist_rows.  The backward re-runs both GEMMs and writes the bf16
//   dl = s * (g_c gscale (p^s - onehot) + g_d gscale (p^s - p^t))
// plus per-row partials of d loss / d s; g_c, g_d (the upstream gradients of the two loss outputs) are device scalars.
// The teacher gets no gradient.
//
// Tile choice: 128 rows x 256 columns per workgroup (not simce's 256 x 256).  Both fp32 accumulator tiles are live in the
// epilogue; at 256 x 256 that is 2 x 128 accumulator registers per lane, and with 8 waves (2 per SIMD) a wave may hold at
// most 256 VGPR + AGPR, so the ring addresses and fragments would spill.  At 128 x 256 each wave owns 64 x 64 of both
// tiles (2 x 64 registers).  The two GEMMs run one after the other through the same two-stage LDS ring (sim_tile.h:
// simce's main loop with an A image of 128 rows), teacher first.  The loss is a small share of a step: one tile per
// workgroup, no persistence.
#include "sim_tile.h"

namespace clipa_gemm {
namespace {

constexpr int DBM = 128;                                  // rows per tile (BN = 256 columns)
constexpr int D_STAGE = sim_stage_bytes<DBM / 64>();      // A image 16 KiB + B image 32 KiB
constexpr int D_NPART = 5;                                // forward partials per row and tile

struct DArgs {
  const char* As; const char* Bs; const char* At; const char* Bt;
  int R, N, Ks, Kt;
  long ldas, ldbs, ldat, ldbt;
  const float* scale_s; const float* scale_t;
  long label0;
  float gscale;
  const float* gc; const float* gd;   // bwd: upstream gradients of (ce, dist) mean losses, device scalars (NULL = 1)
  float* part;          // fwd: [tilesN][R][5] partials.   bwd: [tilesN][R] partial d loss / d s
  float* lab;           // fwd: [R] raw student similarity at the label column
  const float* lse_s; const float* lse_t;   // bwd
  unsigned short* dl;   // bwd: bf16 [R, ldd], columns >= N zero
  long ldd;
};

template <bool BWD>
__global__ __launch_bounds__(NTHREADS) void simce_distill_kernel(DArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const int wm = wave >> 2, wn = wave & 3;
  const int tilesN = (p.N + BN - 1) / BN;
  const int tm = blockIdx.x / tilesN, tn = blockIdx.x - tm * tilesN;
  const int m0 = tm * DBM, n0 = tn * BN;
  const int rowsA = min(DBM, p.R - m0), rowsB = min(BN, p.N - n0);

  f32x16 acc_t[2][2], acc_s[2][2];
  sim_tile<2>(smem, p.At + (size_t)m0 * p.ldat * 2, p.Bt + (size_t)n0 * p.ldbt * 2, p.ldat, p.ldbt, p.Kt, rowsA, rowsB, acc_t);
  __syncthreads();                                   // the teacher's last step may still read the ring slot staged next
  sim_tile<2>(smem, p.As + (size_t)m0 * p.ldas * 2, p.Bs + (size_t)n0 * p.ldbs * 2, p.ldas, p.ldbs, p.Ks, rowsA, rowsB, acc_s);
  __syncthreads();                                   // the ring is dead: its first bytes become the cross-wave scratch
  float* red = (float*)smem;                         // fwd [4 wn][128 rows][5], bwd [4 wn][128 rows]

  // lane holds row m = wm*64 + mi*32 + l31 and columns n = wn*64 + ni*32 + 8*(r>>2) + 4*hi + (r&3)
  const float s = p.scale_s ? p.scale_s[0] : 1.0f;
  const float u = p.scale_t ? p.scale_t[0] : 1.0f;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int rl = wm * 64 + mi * 32 + l31;
    const int m = m0 + rl;
    const long label = p.label0 + m;
    if (!BWD) {
      float mz = -3.0e38f, my = -3.0e38f;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int n = n0 + wn * 64 + ni * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);
          if (n < p.N) { mz = fmaxf(mz, acc_s[ni][mi][r] * s); my = fmaxf(my, acc_t[ni][mi][r] * u); }
          if ((long)n == label && m < p.R) p.lab[m] = acc_s[ni][mi][r];
        }
      mz = fmaxf(mz, __shfl_xor(mz, 32, 64));
      my = fmaxf(my, __shfl_xor(my, 32, 64));
      float sz = 0.f, sy = 0.f, syz = 0.f;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int n = n0 + wn * 64 + ni * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);
          if (n < p.N) {
            const float z = acc_s[ni][mi][r] * s;
            const float e = __expf(acc_t[ni][mi][r] * u - my);
            sz += __expf(z - mz);
            sy += e;
            syz += e * z;
          }
        }
      sz += __shfl_xor(sz, 32, 64);
      sy += __shfl_xor(sy, 32, 64);
      syz += __shfl_xor(syz, 32, 64);
      if (hi == 0) {
        float* o = red + (wn * DBM + rl) * D_NPART;
        o[0] = mz; o[1] = sz; o[2] = my; o[3] = sy; o[4] = syz;
      }
    } else {
      const float ls = m < p.R ? p.lse_s[m] : 0.f;
      const float lt = m < p.R ? p.lse_t[m] : 0.f;
      const float gcs = (p.gc ? p.gc[0] : 1.0f) * p.gscale;
      const float gds = (p.gd ? p.gd[0] : 1.0f) * p.gscale;
      float ds = 0.f;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = n0 + wn * 64 + ni * 32 + 8 * q + 4 * hi;
          float g[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float x = acc_s[ni][mi][4 * q + e];
            const bool ok = n + e < p.N;
            const float ps = ok ? __expf(x * s - ls) : 0.f;
            const float pt = ok ? __expf(acc_t[ni][mi][4 * q + e] * u - lt) : 0.f;
            const float oh = ((long)(n + e) == label) ? 1.0f : 0.0f;
            const float gg = gcs * (ps - oh) + gds * (ps - pt);   // d loss / d logit
            ds += gg * x;                                         // d loss / d s
            g[e] = gg * s;                                        // d loss / d raw
          }
          if (m < p.R && n < p.ldd) {
            u32x2 w;
            w[0] = pack2bf(g[0], g[1]);
            w[1] = pack2bf(g[2], g[3]);
            *(u32x2*)(p.dl + (size_t)m * p.ldd + n) = w;
          }
        }
      ds += __shfl_xor(ds, 32, 64);
      if (hi == 0) red[wn * DBM + rl] = ds;
    }
  }
  __syncthreads();
  if (tid < DBM && m0 + tid < p.R) {
    if (!BWD) {
      float mz = -3.0e38f, my = -3.0e38f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        mz = fmaxf(mz, red[(w * DBM + tid) * D_NPART]);
        my = fmaxf(my, red[(w * DBM + tid) * D_NPART + 2]);
      }
      float sz = 0.f, sy = 0.f, syz = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float* q = red + (w * DBM + tid) * D_NPART;
        sz += q[1] * __expf(q[0] - mz);
        const float f = __expf(q[2] - my);
        sy += q[3] * f;
        syz += q[4] * f;
      }
      float* o = p.part + ((size_t)tn * p.R + m0 + tid) * D_NPART;
      o[0] = mz; o[1] = sz; o[2] = my; o[3] = sy; o[4] = syz;
    } else {
      p.part[(size_t)tn * p.R + m0 + tid] = red[tid] + red[DBM + tid] + red[2 * DBM + tid] + red[3 * DBM + tid];
    }
  }
}

// Instantiated explicitly: hipcc's host pass leaves the second implicit instantiation of a kernel undefined (the library
// then fails to load) when the kernel's body calls a device function template that holds a lambda, as sim_tile does.
template __global__ void simce_distill_kernel<false>(DArgs);
template __global__ void simce_distill_kernel<true>(DArgs);

// fwd: merge the per-tile partials -> lse_s, lse_t, ce_rows, dist_rows.   bwd: sum the per-tile partials of d loss / d s
// into ce_rows (the caller's dscale_rows).
template <bool BWD>
__global__ void simce_distill_merge_kernel(const float* __restrict__ part, int tilesN, long R, const float* __restrict__ lab,
                                           const float* __restrict__ scale, float* __restrict__ lse_s,
                                           float* __restrict__ lse_t, float* __restrict__ ce_rows,
                                           float* __restrict__ dist_rows) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  if (!BWD) {
    float mz = -3.0e38f, my = -3.0e38f;
    for (int t = 0; t < tilesN; ++t) {
      mz = fmaxf(mz, part[((size_t)t * R + r) * D_NPART]);
      my = fmaxf(my, part[((size_t)t * R + r) * D_NPART + 2]);
    }
    float sz = 0.f, sy = 0.f, syz = 0.f;
    for (int t = 0; t < tilesN; ++t) {
      const float* q = part + ((size_t)t * R + r) * D_NPART;
      sz += q[1] * __expf(q[0] - mz);
      const float f = __expf(q[2] - my);
      sy += q[3] * f;
      syz += q[4] * f;
    }
    const float ls = mz + logf(sz);
    lse_s[r] = ls;
    lse_t[r] = my + logf(sy);
    ce_rows[r] = ls - lab[r] * (scale ? scale[0] : 1.0f);
    dist_rows[r] = ls - syz / sy;
  } else {
    float a = 0.f;
    for (int t = 0; t < tilesN; ++t) a += part[(size_t)t * R + r];
    ce_rows[r] = a;
  }
}

LdsOptIn g_dce_lds;
int ensure_dce_attrs(int dev) {
  return g_dce_lds.ensure(dev, {(const void*)simce_distill_kernel<false>, (const void*)simce_distill_kernel<true>}, 2 * D_STAGE, "simce_distill");
}

int dce_check(int64_t R, int64_t N, int64_t Es, int64_t Et, int64_t ldas, int64_t ldbs, int64_t ldat, int64_t ldbt,
              int64_t label0) {
  if (Es <= 0 || Et <= 0 || Es % 8 != 0 || Et % 8 != 0 || ldas % 8 != 0 || ldbs % 8 != 0 || ldat % 8 != 0 || ldbt % 8 != 0) {
    clipa_set_error("simce_distill: E_s, E_t and every leading dimension must be positive multiples of 8");
    return CLIPA_ERR_ARG;
  }
  if (ldas < Es || ldbs < Es || ldat < Et || ldbt < Et) { clipa_set_error("simce_distill: leading dimension below E"); return CLIPA_ERR_ARG; }
  if (label0 < 0 || label0 + R > N) { clipa_set_error("simce_distill: labels [%ld, %ld) outside [0, %ld)", (long)label0, (long)(label0 + R), (long)N); return CLIPA_ERR_ARG; }
  const int64_t ldmax = std::max(std::max(ldas, ldbs), std::max(ldat, ldbt));
  if (256 * ldmax * 2 >= (1L << 30)) { clipa_set_error("simce_distill: leading dimension too large"); return CLIPA_ERR_ARG; }
  if (R >= (1L << 30) || N >= (1L << 30)) { clipa_set_error("simce_distill: R or N too large"); return CLIPA_ERR_ARG; }
  return 0;
}

// the fields the forward and the backward share; part = the workspace
DArgs make_args(const void* rows_s, const void* cols_s, const void* rows_t, const void* cols_t, int64_t R, int64_t N,
                int64_t Es, int64_t Et, int64_t ldas, int64_t ldbs, int64_t ldat, int64_t ldbt, const float* scale_s,
                const float* scale_t, int64_t label0, void* workspace) {
  DArgs a = {};
  a.As = (const char*)rows_s; a.Bs = (const char*)cols_s; a.At = (const char*)rows_t; a.Bt = (const char*)cols_t;
  a.R = (int)R; a.N = (int)N; a.Ks = (int)Es; a.Kt = (int)Et; a.ldas = ldas; a.ldbs = ldbs; a.ldat = ldat; a.ldbt = ldbt;
  a.scale_s = scale_s; a.scale_t = scale_t; a.label0 = label0; a.part = (float*)workspace;
  return a;
}

}  // namespace
}  // namespace clipa_gemm

using namespace clipa_gemm;

extern "C" int64_t clipa_simce_distill_workspace(int64_t R, int64_t N) {
  const int64_t tilesN = (N + BN - 1) / BN;
  return (tilesN * R * D_NPART + R) * (int64_t)sizeof(float);   // per-tile partials + the label similarities
}

extern "C" int clipa_simce_distill_fwd(const void* rows_s, const void* cols_s, const void* rows_t, const void* cols_t,
                                       int64_t R, int64_t N, int64_t Es, int64_t Et, int64_t ldas, int64_t ldbs,
                                       int64_t ldat, int64_t ldbt, const float* scale_s, const float* scale_t,
                                       int64_t label0, float* lse_s, float* lse_t, float* ce_rows, float* dist_rows,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
  if (R <= 0) return CLIPA_OK;
  if (int rc = dce_check(R, N, Es, Et, ldas, ldbs, ldat, ldbt, label0)) return rc;
  if (!workspace || workspace_bytes < clipa_simce_distill_workspace(R, N)) { clipa_set_error("simce_distill_fwd: workspace too small"); return CLIPA_ERR_ARG; }
  if (!lse_s || !lse_t || !ce_rows || !dist_rows) { clipa_set_error("simce_distill_fwd: null output"); return CLIPA_ERR_ARG; }
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (int rc = ensure_dce_attrs(dev)) return rc;
  const int64_t tilesN = (N + BN - 1) / BN, tilesM = (R + DBM - 1) / DBM;
  DArgs a = make_args(rows_s, cols_s, rows_t, cols_t, R, N, Es, Et, ldas, ldbs, ldat, ldbt, scale_s, scale_t, label0, workspace);
  a.lab = (float*)workspace + tilesN * R * D_NPART;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(simce_distill_kernel<false>, dim3((unsigned)(tilesM * tilesN)), dim3(NTHREADS), 2 * D_STAGE, st, a);
  if (int rc = clipa_check_launch("simce_distill_fwd")) return rc;
  hipLaunchKernelGGL(simce_distill_merge_kernel<false>, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, a.part,
                     (int)tilesN, (long)R, a.lab, scale_s, lse_s, lse_t, ce_rows, dist_rows);
  return clipa_check_launch("simce_distill_merge");
}

extern "C" int clipa_simce_distill_bwd(const void* rows_s, const void* cols_s, const void* rows_t, const void* cols_t,
                                       int64_t R, int64_t N, int64_t Es, int64_t Et, int64_t ldas, int64_t ldbs,
                                       int64_t ldat, int64_t ldbt, const float* scale_s, const float* scale_t,
                                       int64_t label0, float gscale, const float* g_c, const float* g_d,
                                       const float* lse_s, const float* lse_t, void* dlogits_bf16, int64_t ldd,
                                       float* dscale_rows, void* workspace, int64_t workspace_bytes, void* stream) {
  if (R <= 0) return CLIPA_OK;
  if (int rc = dce_check(R, N, Es, Et, ldas, ldbs, ldat, ldbt, label0)) return rc;
  const int64_t N8 = (N + 7) & ~(int64_t)7;
  if (!dlogits_bf16 || ldd % 8 != 0 || ldd < N8) { clipa_set_error("simce_distill_bwd: dlogits needs ldd %% 8 == 0 and ldd >= N rounded up to 8"); return CLIPA_ERR_ARG; }
  if (!workspace || workspace_bytes < clipa_simce_distill_workspace(R, N)) { clipa_set_error("simce_distill_bwd: workspace too small"); return CLIPA_ERR_ARG; }
  if (!lse_s || !lse_t || !dscale_rows) { clipa_set_error("simce_distill_bwd: null lse / dscale_rows"); return CLIPA_ERR_ARG; }
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (int rc = ensure_dce_attrs(dev)) return rc;
  const int64_t tilesN = (N + BN - 1) / BN, tilesM = (R + DBM - 1) / DBM;
  DArgs a = make_args(rows_s, cols_s, rows_t, cols_t, R, N, Es, Et, ldas, ldbs, ldat, ldbt, scale_s, scale_t, label0, workspace);
  a.gscale = gscale; a.gc = g_c; a.gd = g_d; a.lse_s = lse_s; a.lse_t = lse_t;
  a.dl = (unsigned short*)dlogits_bf16; a.ldd = ldd;    // columns [N, ldd) inside the last tile are written as zeros
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(simce_distill_kernel<true>, dim3((unsigned)(tilesM * tilesN)), dim3(NTHREADS), 2 * D_STAGE, st, a);
  if (int rc = clipa_check_launch("simce_distill_bwd")) return rc;
  hipLaunchKernelGGL(simce_distill_merge_kernel<true>, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, a.part,
                     (int)tilesN, (long)R, (const float*)nullptr, scale_s, (float*)nullptr, (float*)nullptr,
                     dscale_rows, (float*)nullptr);
  return clipa_check_launch("simce_distill_merge");
}
