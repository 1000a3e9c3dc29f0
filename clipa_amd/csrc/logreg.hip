// Logistic-regression linear probe (Radford et al. 2021, section 3.2 and appendix A.3: an L2-regularised multinomial logistic
// regression on frozen image features, fitted with L-BFGS) with the features kept on the GPU.  fp32 throughout.  One objective-
// and-gradient evaluation at the weights theta [C, dim] (class-major, dim = D + 1, the last column the bias) is four launches:
//   logits      Zt[c, n] = theta_c . x~_n (x~ = [x, 1]), lse[n] = log sum_c exp Zt[c, n], and the argmax over classes
//   residual    ce[n] = lse[n] - Zt[y_n, n], then in place Zt[c, n] <- exp(Zt[c, n] - lse[n]) - [c == y_n]
//   grad        dtheta[c, d] = sum_n Gt[c, n] X~t[d, n] (Gt: the residual), n in slices of LR_SLICE samples, one partial each
//   grad reduce the partials added in ascending slice order
// and once per fit
//   prepare     X~ [N, ld] and X~t [dim, ldn] from x [N, D]: the ones column / row, zero padding.
// The data term of the objective is (1 / N) sum_n ce[n]; that sum, the 1 / N and the L2 term are the caller's, in fp64.
// The two products run on rank_tile (rank_tile.h): one ascending-k fp32 MFMA chain per output.  Every other reduction has a
// fixed order that is part of the algorithm (the constants and the comments below), not of the launch: no float atomics, so every
// result is bit-reproducible whatever the grid.
#include "rank_tile.h"

namespace clipa_gemm {
namespace {

constexpr int LR_SLICE = 4096;                // grad: samples per partial product (the default of the entry point's `slice`)
constexpr int LR_RES_CLASSES = 64;            // residual: classes per workgroup (elementwise: no effect on any value)
constexpr int LR_PT = 32;                     // prepare: tile edge (256 threads as 32 x 8)
constexpr long LR_MAX_N = 1L << 21;           // N * 128 * 4 bytes, the row block of Zt that grad reads, stays below 1 GiB
constexpr int LR_NONE = 0x7fffffff;

// Tile (blockIdx.x: rows n, blockIdx.y: columns c) of X~ [N, ld]; the tile goes through LDS and comes out transposed into
// X~t [D + 1, ldn].  The grid covers rows up to max(N, ldn) so that the padding of X~t is written too.
__global__ __launch_bounds__(256) void logreg_prepare_kernel(const float* __restrict__ x, int N, int D, long ldx,
                                                             float* __restrict__ Xp, long ld, float* __restrict__ Xt, long ldn) {
  __shared__ float tile[LR_PT][LR_PT + 1];
  const int tx = threadIdx.x % LR_PT, ty = threadIdx.x / LR_PT;
  const int c0 = blockIdx.y * LR_PT, n0 = blockIdx.x * LR_PT;
  const int c = c0 + tx;
#pragma unroll
  for (int j = 0; j < LR_PT / 8; ++j) {
    const int n = n0 + ty + 8 * j;
    float v = 0.f;
    if (n < N) {
      if (c < D) v = x[(long)n * ldx + c];
      else if (c == D) v = 1.0f;
      if (c < ld) Xp[(long)n * ld + c] = v;
    }
    tile[ty + 8 * j][tx] = v;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < LR_PT / 8; ++j) {
    const int d = c0 + ty + 8 * j, n = n0 + tx;
    if (d <= D && n < ldn) Xt[(long)d * ldn + n] = tile[tx][ty + 8 * j];
  }
}

// A running log-sum-exp: sum = s * exp(m); m = -inf, s = 0 is the empty sum.  lr_meet(a, b) is not symmetric in the last bit
// (a's term is the addend the compiler may fuse), so every meeting below names which side is a.
struct LrLse { float m, s; };
__device__ __forceinline__ LrLse lr_meet(LrLse a, LrLse b) {
  const float M = fmaxf(a.m, b.m);
  if (M == -__builtin_huge_valf()) return {M, 0.f};
  return {M, a.s * expf(a.m - M) + b.s * expf(b.m - M)};
}

// One workgroup per 128 samples, over the class tiles in ascending order.  theta is the tile's row operand, X~ its column
// operand: a lane's two accumulator columns are samples n0 + col(ni) (consecutive lanes, consecutive n: the Zt stores are
// coalesced), its 32 values per column the classes m0 + row(q), ascending in q.  Per lane and column a running (m, s) and
// best: each tile folds in as m' = max(m, max_q v_q), s = s exp(m - m') + sum_q exp(v_q - m') with q ascending; classes >= C
// contribute nothing.  "Replace only on strictly greater" in ascending (tile, q) keeps the lowest class of the lane's maxima.
// Then the two lane halves meet (hi = 0 first), then the two row waves through LDS (wm = 0 first).
__global__ __launch_bounds__(RTHREADS, 2) void logreg_logits_kernel(const char* __restrict__ Th, const char* __restrict__ X,
                                                                    int C, int N, int dim, long ldt, long ldx,
                                                                    float* __restrict__ Zt, long ldz, float* __restrict__ lse,
                                                                    int* __restrict__ pred, float* __restrict__ best) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const RankLane t = rank_lane();
  const float ninf = -__builtin_huge_valf();
  const int n0 = blockIdx.x * RT;
  int rowsA, rowsB;
  const __amdgpu_buffer_rsrc_t rsB = rank_rows(X, n0, N, ldx, &rowsB);
  LrLse run[2] = {{ninf, 0.f}, {ninf, 0.f}};
  RankBest top[2] = {{ninf, LR_NONE}, {ninf, LR_NONE}};

  const int Tc = (C + RT - 1) / RT;
  f32x16 acc[2][2];
  for (int tm = 0; tm < Tc; ++tm) {
    const int m0 = tm * RT;
    const __amdgpu_buffer_rsrc_t rsA = rank_rows(Th, m0, C, ldt, &rowsA);
    __syncthreads();                          // the previous tile's readers are done with the ring
    rank_tile(smem, rsA, rsB, ldt, ldx, dim, acc);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int nl = t.col(ni);
      const bool live = nl < rowsB;
      float* zcol = Zt + n0 + nl;
      float tmax = ninf;
#pragma unroll
      for (int q = 0; q < 32; ++q) {
        const int cls = t.row(q, m0);
        const float v = acc[q >> 4][ni][q & 15];
        if (cls < C) {
          tmax = fmaxf(tmax, v);
          const bool take = v > top[ni].v || top[ni].c == LR_NONE;
          top[ni] = take ? RankBest{v, cls} : top[ni];
          if (live) zcol[(long)cls * ldz] = v;
        }
      }
      if (tmax > ninf) {                      // this lane holds a class of this tile
        const float mn = fmaxf(run[ni].m, tmax);
        float sum = 0.f;
#pragma unroll
        for (int q = 0; q < 32; ++q)
          if (t.row(q, m0) < C) sum += expf(acc[q >> 4][ni][q & 15] - mn);
        run[ni].s = run[ni].s * expf(run[ni].m - mn) + sum;      // first fold: 0 * exp(-inf) = 0
        run[ni].m = mn;
      }
    }
  }
  // the lane halves: both lanes of a pair compute the same meeting, hi = 0's values first
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const LrLse o = {__shfl_xor(run[ni].m, 32, 64), __shfl_xor(run[ni].s, 32, 64)};
    run[ni] = t.hi ? lr_meet(o, run[ni]) : lr_meet(run[ni], o);
    top[ni] = rank_better(top[ni], lane_xor(top[ni], 32));
  }
  __syncthreads();                            // the ring is dead: its first 4 KiB take the two row waves' results
  LrLse* lrun = (LrLse*)smem;                 // [2 wm][128]
  RankBest* ltop = (RankBest*)(smem + 2 * RT * sizeof(LrLse));      // [2 wm][128]
  if (t.hi == 0) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      lrun[t.wm * RT + t.col(ni)] = run[ni];
      ltop[t.wm * RT + t.col(ni)] = top[ni];
    }
  }
  __syncthreads();
  if (t.tid < rowsB) {
    const LrLse r = lr_meet(lrun[t.tid], lrun[RT + t.tid]);
    const RankBest b = rank_better(ltop[t.tid], ltop[RT + t.tid]);
    lse[n0 + t.tid] = r.m + logf(r.s);
    pred[n0 + t.tid] = b.c;
    best[n0 + t.tid] = b.v;
  }
}

// Threads along n, blockIdx.y over blocks of LR_RES_CLASSES classes.  The thread that overwrites Zt[y_n, n] is the one that
// read it for ce[n], before the overwrite.  overwrite = 0 (the line search: the objective alone) touches only Zt[y_n, n].
// A label outside [0, C) (callers validate) gives ce = NaN and is never used as an index.
__global__ __launch_bounds__(256) void logreg_residual_kernel(float* __restrict__ Zt, const float* __restrict__ lse,
                                                              const int* __restrict__ y, int C, int N, long ldz,
                                                              float* __restrict__ ce, int overwrite) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float l = lse[n];
  const int yn = y[n];
  const bool bad = (unsigned)yn >= (unsigned)C;
  if (!overwrite) {
    ce[n] = bad ? __builtin_nanf("") : l - Zt[(long)yn * ldz + n];
    return;
  }
  if (bad && blockIdx.y == 0) ce[n] = __builtin_nanf("");
  const int c0 = blockIdx.y * LR_RES_CLASSES, c1 = min(C, c0 + LR_RES_CLASSES);
  for (int c = c0; c < c1; ++c) {
    float* z = Zt + (long)c * ldz + n;
    const float v = *z;
    const bool hit = c == yn;
    if (hit) ce[n] = l - v;
    *z = expf(v - l) - (hit ? 1.0f : 0.0f);
  }
}

// Work item w = (slice, class tile, dim tile), slices outermost; a workgroup takes items blockIdx.x, + gridDim.x, ...  The
// item's 128 x 128 product over its slice's samples goes to the slice's partial P + slice * pstride, [C, ldp].
__global__ __launch_bounds__(RTHREADS, 2) void logreg_grad_kernel(const char* __restrict__ Gt, const char* __restrict__ Xt,
                                                                  int C, int dim, int N, long ldz, long ldn, int S,
                                                                  float* __restrict__ P, long ldp, long pstride, int nwork) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const RankLane t = rank_lane();
  const int Tc = (C + RT - 1) / RT, Td = (dim + RT - 1) / RT;
  f32x16 acc[2][2];
  for (int w = blockIdx.x; w < nwork; w += gridDim.x) {
    const int sl = w / (Tc * Td), rem = w % (Tc * Td);
    const int m0 = (rem / Td) * RT, d0 = (rem % Td) * RT;
    const long s0 = (long)sl * S;
    const int E = (int)min((long)S, (long)N - s0);
    const int rowsA = min(RT, C - m0), rowsB = min(RT, dim - d0);
    // rows [m0, m0 + rowsA) of Gt from column s0 on: the range ends with the last row (k < E <= ldz - s0 stays inside it)
    const __amdgpu_buffer_rsrc_t rsA = make_rsrc(Gt + ((size_t)m0 * ldz + s0) * 4, (unsigned)((rowsA * ldz - s0) * 4));
    const __amdgpu_buffer_rsrc_t rsB = make_rsrc(Xt + ((size_t)d0 * ldn + s0) * 4, (unsigned)((rowsB * ldn - s0) * 4));
    __syncthreads();                          // the previous item's readers are done with the ring
    rank_tile(smem, rsA, rsB, ldz, ldn, E, acc);
    float* out = P + (long)sl * pstride;
#pragma unroll
    for (int q = 0; q < 32; ++q) {
      const int c = t.row(q, m0);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int d = t.col(ni, d0);
        if (c < C && d < dim) out[(long)c * ldp + d] = acc[q >> 4][ni][q & 15];
      }
    }
  }
}

// dtheta[c, d] = the nsl partials added in ascending slice order
__global__ __launch_bounds__(256) void logreg_grad_reduce_kernel(const float* __restrict__ P, long ldp, long pstride, int nsl,
                                                                 int C, int dim, float* __restrict__ G, long ldg) {
  const int d = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
  if (d >= dim) return;
  const float* p = P + (long)c * ldp + d;
  float s = p[0];
  for (int k = 1; k < nsl; ++k) s += p[(long)k * pstride];
  G[(long)c * ldg + d] = s;
}

LdsOptIn g_lr_lds;

template <class K, class... A>
int lr_launch(K kernel, int64_t grid, void* stream, const char* name, A... args) {
  return rank_launch(g_lr_lds, {(const void*)logreg_logits_kernel, (const void*)logreg_grad_kernel}, 2 * R_STAGE, "logreg", kernel,
                     grid, 2 * R_STAGE, stream, name, args...);
}
// the sizes every entry point takes; N >= 2^21 says so
int lr_sizes(const char* name, int64_t C, int64_t N, int64_t dim) {
  if (C < 0 || N < 0 || dim < 0 || C > 65535 || dim >= (1L << 21)) {
    clipa_set_error("%s: C = %ld, N = %ld, dim = %ld out of range (C <= 65535, dim < 2^21)", name, (long)C, (long)N, (long)dim);
    return CLIPA_ERR_ARG;
  }
  if (N >= LR_MAX_N) {
    clipa_set_error("%s: N = %ld must be below 2^21 = %ld (a 128-class block of the [C, N] logits must stay below 1 GiB; features "
                    "that do not fit one such problem are not supported)", name, (long)N, LR_MAX_N);
    return CLIPA_ERR_ARG;
  }
  return 0;
}
int64_t lr_slice(int64_t slice) { return slice == 0 ? LR_SLICE : slice; }

}  // namespace
}  // namespace clipa_gemm

using namespace clipa_gemm;

extern "C" int clipa_logreg_prepare(const float* x, int64_t N, int64_t D, int64_t ldx, float* Xp, int64_t ld, float* Xt,
                                    int64_t ldn, void* stream) {
  if (D < 0 || ldx < D) { clipa_set_error("logreg_prepare: D = %ld, ldx = %ld out of range (ldx >= D >= 0)", (long)D, (long)ldx); return CLIPA_ERR_ARG; }
  if (int rc = lr_sizes("logreg_prepare", 0, N, D + 1)) return rc;
  if (ld < D + 1 || ldn < N || ld % 4 || ldn % 4 || ld >= (1L << 21) || ldn >= LR_MAX_N + 4) {
    clipa_set_error("logreg_prepare: ld = %ld must be >= D + 1 = %ld, ldn = %ld >= N = %ld, both multiples of 4 below 2^21", (long)ld,
                    (long)(D + 1), (long)ldn, (long)N);
    return CLIPA_ERR_ARG;
  }
  if (N == 0) return CLIPA_OK;
  if (int rc = clipa_check_ptrs16("logreg_prepare", {Xp, Xt})) return rc;
  if (D > 0) if (int rc = clipa_check_ptrs16("logreg_prepare", {x})) return rc;
  const int64_t gx = (ldn + LR_PT - 1) / LR_PT, gy = (ld + LR_PT - 1) / LR_PT;      // ldn >= N
  if (gy > 65535) { clipa_set_error("logreg_prepare: ld = %ld is more than 65535 tiles of %d columns", (long)ld, LR_PT); return CLIPA_ERR_ARG; }
  hipLaunchKernelGGL(logreg_prepare_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, x, (int)N, (int)D,
                     (long)ldx, Xp, (long)ld, Xt, (long)ldn);
  return clipa_check_launch("logreg_prepare");
}

extern "C" int clipa_logreg_logits(const float* theta, const float* Xp, int64_t C, int64_t N, int64_t dim, int64_t ldt, int64_t ld,
                                   float* Zt, int64_t ldz, float* lse, int32_t* pred, float* best, void* stream) {
  if (int rc = lr_sizes("logreg_logits", C, N, dim)) return rc;
  if (N == 0) return CLIPA_OK;
  if (C == 0) { clipa_set_error("logreg_logits: C = 0 classes for N = %ld rows (a softmax over nothing)", (long)N); return CLIPA_ERR_ARG; }
  if (dim == 0) { clipa_set_error("logreg_logits: dim = 0 (the bias column alone makes dim >= 1)"); return CLIPA_ERR_ARG; }
  if (ldz < N || ldz % 4 || ldz >= LR_MAX_N + 4) {
    clipa_set_error("logreg_logits: ldz = %ld must be >= N = %ld and a multiple of 4", (long)ldz, (long)N);
    return CLIPA_ERR_ARG;
  }
  if (int rc = rank_check_args("logreg_logits", dim, ldt, ld, false, "C, N", {theta, Xp, Zt, lse, pred, best}, nullptr)) return rc;
  return lr_launch(logreg_logits_kernel, (N + RT - 1) / RT, stream, "logreg_logits", (const char*)theta, (const char*)Xp, (int)C,
                   (int)N, (int)dim, (long)ldt, (long)ld, Zt, (long)ldz, lse, pred, best);
}

extern "C" int clipa_logreg_residual(float* Zt, const float* lse, const int32_t* y, int64_t C, int64_t N, int64_t ldz, float* ce,
                                     int32_t overwrite, void* stream) {
  if (int rc = lr_sizes("logreg_residual", C, N, 0)) return rc;
  if (N == 0) return CLIPA_OK;
  if (C == 0) { clipa_set_error("logreg_residual: C = 0 classes for N = %ld rows (no label exists)", (long)N); return CLIPA_ERR_ARG; }
  if (ldz < N) { clipa_set_error("logreg_residual: ldz = %ld must be >= N = %ld", (long)ldz, (long)N); return CLIPA_ERR_ARG; }
  if (int rc = clipa_check_ptrs16("logreg_residual", {Zt, lse, y, ce})) return rc;
  const unsigned gy = overwrite ? (unsigned)((C + LR_RES_CLASSES - 1) / LR_RES_CLASSES) : 1u;
  hipLaunchKernelGGL(logreg_residual_kernel, dim3((unsigned)((N + 255) / 256), gy), dim3(256), 0, (hipStream_t)stream, Zt, lse, y,
                     (int)C, (int)N, (long)ldz, ce, (int)overwrite);
  return clipa_check_launch("logreg_residual");
}

extern "C" int64_t clipa_logreg_grad_workspace(int64_t C, int64_t dim, int64_t N, int64_t slice) {
  const int64_t S = lr_slice(slice);
  if (C <= 0 || dim <= 0 || N <= 0 || S <= 0) return 0;
  const int64_t nsl = (N + S - 1) / S;
  return nsl > 1 ? nsl * C * ((dim + 3) / 4 * 4) * 4 : 0;      // a single slice is written in place
}

extern "C" int clipa_logreg_grad(const float* Gt, const float* Xt, int64_t C, int64_t dim, int64_t N, int64_t ldz, int64_t ldn,
                                 float* dtheta, int64_t ldg, int64_t slice, int64_t max_workgroups, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
  if (int rc = lr_sizes("logreg_grad", C, N, dim)) return rc;
  const int64_t S = lr_slice(slice);
  if (S < 4 || S % 4 || S > (1L << 30) || max_workgroups < 0 || ldg < dim) {
    clipa_set_error("logreg_grad: slice = %ld must be a positive multiple of 4 (0: the default %d), max_workgroups = %ld >= 0, ldg = "
                    "%ld >= dim = %ld", (long)slice, LR_SLICE, (long)max_workgroups, (long)ldg, (long)dim);
    return CLIPA_ERR_ARG;
  }
  if (C == 0 || dim == 0) return CLIPA_OK;
  if (N == 0) {                               // the empty sum: dtheta = 0
    if (int rc = clipa_check_ptrs16("logreg_grad", {dtheta})) return rc;
    const hipError_t e = hipMemset2DAsync(dtheta, (size_t)ldg * 4, 0, (size_t)dim * 4, (size_t)C, (hipStream_t)stream);
    if (e != hipSuccess) { clipa_set_error("logreg_grad: hipMemset2DAsync: %s", hipGetErrorString(e)); return CLIPA_ERR_LAUNCH; }
    return CLIPA_OK;
  }
  if (int rc = rank_check_args("logreg_grad", N, ldz, ldn, ldz >= LR_MAX_N + 4 || ldn >= LR_MAX_N + 4, "N", {Gt, Xt, dtheta}, nullptr)) return rc;
  const int64_t nsl = (N + S - 1) / S, ldp = (dim + 3) / 4 * 4;
  const int64_t need = clipa_logreg_grad_workspace(C, dim, N, slice);
  const int64_t nwork = nsl * ((C + RT - 1) / RT) * ((dim + RT - 1) / RT);
  if (nwork >= (1L << 31)) { clipa_set_error("logreg_grad: %ld tile products are too many for one launch", (long)nwork); return CLIPA_ERR_ARG; }
  if (nsl > 1) {
    if (workspace_bytes < need) { clipa_set_error("logreg_grad: workspace of %ld bytes, needs %ld", (long)workspace_bytes, (long)need); return CLIPA_ERR_ARG; }
    if (int rc = clipa_check_ptrs16("logreg_grad", {workspace})) return rc;
  }
  float* P = nsl > 1 ? (float*)workspace : dtheta;
  const int64_t grid = max_workgroups ? std::min(max_workgroups, nwork) : nwork;
  if (int rc = lr_launch(logreg_grad_kernel, grid, stream, "logreg_grad", (const char*)Gt, (const char*)Xt, (int)C, (int)dim, (int)N,
                         (long)ldz, (long)ldn, (int)S, P, (long)(nsl > 1 ? ldp : ldg), (long)(C * ldp), (int)nwork)) return rc;
  if (nsl == 1) return CLIPA_OK;
  hipLaunchKernelGGL(logreg_grad_reduce_kernel, dim3((unsigned)((dim + 255) / 256), (unsigned)C), dim3(256), 0, (hipStream_t)stream,
                     (const float*)P, (long)ldp, (long)(C * ldp), (int)nsl, (int)C, (int)dim, dtheta, (long)ldg);
  return clipa_check_launch("logreg_grad (reduce)");
}
