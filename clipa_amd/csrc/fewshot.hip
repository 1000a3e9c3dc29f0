// Few-shot linear probe (clipa_jax/evaluators/fewshot_lsr.py:31-108, big_vision's closed-form L2-regularised least squares on
// frozen features) with the features kept on the GPU.  fp32 throughout.  Five kernels:
//   moments     mean / std of the selected rows of x (two passes; std = sqrt(mean((x - mean)^2)) + 1e-5, fewshot_lsr.py:39-40)
//   whiten      Z = (x - mean) / std with the constant 100.0 column appended (fewshot_lsr.py:41-44, 95-96), optionally also Z^T
//   gram        S = A A^T (x^T x of route A on Z^T, x x^T of route B on Z; fewshot_lsr.py:72-79), upper tiles mirrored
//   class sums  R = Z^T Y for Y = +1 at the label, -1 elsewhere (fewshot_lsr.py:47, 74) from class-contiguous rows, Y never formed
//   predict     argmax over classes of Z_test W^T (fewshot_lsr.py:107) without the [Nt, C] logits
// The two products run on rank_tile (rank_tile.h): one ascending-k fp32 MFMA chain per output, no split-K.  Every other
// reduction has a fixed order that is part of the algorithm (the constants below), not of the launch: no float atomics, so every
// result is bit-reproducible.  The ridge system itself (dim x dim or N x N) is solved by the caller on the host, as the reference
// does on its CPU backend.
#include "rank_tile.h"

namespace clipa_gemm {
namespace {

constexpr int MOM_COLS = 32;                  // moments: columns per workgroup
constexpr int MOM_SLICES = 32;                // and row slices: slice s sums rows s, s + 32, ... in order, the slices add in order
constexpr int WT = 32;                        // whiten: tile edge (256 threads as 32 x 8)

// row of x that output row n reads: -1 when the index list names a row outside [0, Ntot) (callers validate; never dereferenced)
__device__ __forceinline__ long src_row(const int* index, int n, int Ntot) {
  const int r = index ? index[n] : n;
  return (unsigned)r < (unsigned)Ntot ? (long)r : -1L;
}

__global__ __launch_bounds__(MOM_COLS * MOM_SLICES) void fewshot_moments_kernel(const float* __restrict__ x,
                                                                                const int* __restrict__ index, int N, int Ntot,
                                                                                int D, long ldx, float* __restrict__ mean,
                                                                                float* __restrict__ stdv) {
  __shared__ float part[MOM_SLICES][MOM_COLS];
  __shared__ float smean[MOM_COLS];
  const int tx = threadIdx.x % MOM_COLS, ty = threadIdx.x / MOM_COLS;
  const int d = blockIdx.x * MOM_COLS + tx;
  const bool live = d < D;
  const float nan = __builtin_nanf("");
  float mu = 0.f;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    float acc = 0.f;
    if (live) {
#pragma unroll 4
      for (int n = ty; n < N; n += MOM_SLICES) {
        const long r = src_row(index, n, Ntot);
        const float v = r >= 0 ? x[r * ldx + d] : nan;
        const float c = v - mu;                // pass 0: mu = 0
        acc += pass ? c * c : v;
      }
    }
    part[ty][tx] = acc;
    __syncthreads();
    if (ty == 0) {
      float s = part[0][tx];
#pragma unroll
      for (int k = 1; k < MOM_SLICES; ++k) s += part[k][tx];
      const float m = s / (float)N;
      if (pass == 0) {
        smean[tx] = m;
        if (live) mean[d] = m;
      } else if (live) {
        stdv[d] = sqrtf(m) + 1e-5f;
      }
    }
    __syncthreads();
    mu = smean[tx];
  }
}

// Tile (blockIdx.x: rows n, blockIdx.y: columns c) of Z [N, ldz]; with Zt the tile goes through LDS and comes out transposed
// into Zt [D + 1, ldt].  The grid covers rows up to max(N, ldt) so that the padding of Zt is written too.
__global__ __launch_bounds__(256) void fewshot_whiten_kernel(const float* __restrict__ x, const int* __restrict__ index, int N,
                                                             int Ntot, int D, long ldx, const float* __restrict__ mean,
                                                             const float* __restrict__ stdv, float* __restrict__ Z, long ldz,
                                                             float* __restrict__ Zt, long ldt) {
  __shared__ float tile[WT][WT + 1];
  const int tx = threadIdx.x % WT, ty = threadIdx.x / WT;
  const int c0 = blockIdx.y * WT, n0 = blockIdx.x * WT;
  const int c = c0 + tx;
  const float mu = c < D ? mean[c] : 0.f, sd = c < D ? stdv[c] : 1.f;
#pragma unroll
  for (int j = 0; j < WT / 8; ++j) {
    const int n = n0 + ty + 8 * j;
    float v = 0.f;
    if (n < N) {
      if (c < D) {
        const long r = src_row(index, n, Ntot);
        const float xv = r >= 0 ? x[r * ldx + c] : __builtin_nanf("");
        v = (xv - mu) / sd;                    // true subtraction, then true division: the reference's rounding
      } else if (c == D) {
        v = 100.0f;                            // BIAS_CONSTANT
      }
      if (c < ldz) Z[(long)n * ldz + c] = v;
    }
    tile[ty + 8 * j][tx] = v;
  }
  if (!Zt) return;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < WT / 8; ++j) {
    const int d = c0 + ty + 8 * j, n = n0 + tx;
    if (d <= D && n < ldt) Zt[(long)d * ldt + n] = tile[tx][ty + 8 * j];
  }
}

// S = A A^T, A [M, E]: workgroup b takes the b-th upper tile (tm <= tn, row by row) and writes it and its mirror image.  Inside a
// diagonal tile only i <= j is taken, so S[i][j] and S[j][i] are always one value.
__global__ __launch_bounds__(RTHREADS, 2) void fewshot_gram_kernel(const char* __restrict__ A, int M, int E, long lda,
                                                                   float* __restrict__ S, long lds) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const RankLane t = rank_lane();
  const int T = (M + RT - 1) / RT;
  int tm = 0, b = blockIdx.x;
  while (b >= T - tm) { b -= T - tm; ++tm; }  // row tm of the upper triangle holds T - tm tiles
  const int tn = tm + b;
  const int m0 = tm * RT, n0 = tn * RT;
  int rowsA, rowsB;
  const __amdgpu_buffer_rsrc_t rsA = rank_rows(A, m0, M, lda, &rowsA);
  const __amdgpu_buffer_rsrc_t rsB = rank_rows(A, n0, M, lda, &rowsB);
  f32x16 acc[2][2];
  rank_tile(smem, rsA, rsB, lda, lda, E, acc);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = t.row(mi * 16 + r, m0);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int j = t.col(ni, n0);
        if (i <= j && j < M) {                 // i <= j < M
          const float v = acc[mi][ni][r];
          S[(long)i * lds + j] = v;
          S[(long)j * lds + i] = v;
        }
      }
    }
}

// seg[d, c] = sum of Z[n, d] over the rows of class c, in row order: one workgroup per (64 columns, class)
__global__ __launch_bounds__(64) void fewshot_segsum_kernel(const float* __restrict__ Z, const int* __restrict__ offsets, int N,
                                                            int dim, long ldz, float* __restrict__ R, long ldr) {
  const int d = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y;
  if (d >= dim) return;
  const int lo = max(offsets[c], 0), hi = min(offsets[c + 1], N);
  float s = 0.f;
  for (int n = lo; n < hi; ++n) s += Z[(long)n * ldz + d];
  R[(long)d * ldr + c] = s;
}
// total[d] = the segment sums added in class order; R[d, c] = 2 seg - total (an empty class: -total)
__global__ __launch_bounds__(64) void fewshot_signsum_kernel(int dim, int C, float* __restrict__ R, long ldr) {
  const int d = blockIdx.x * 64 + threadIdx.x;
  if (d >= dim) return;
  float* row = R + (long)d * ldr;
  float total = 0.f;
  for (int c = 0; c < C; ++c) total += row[c];
  for (int c = 0; c < C; ++c) row[c] = 2.0f * row[c] - total;
}

// One workgroup per 128 test rows, over the class tiles in ascending order.  A lane's accumulator columns are classes
// tn * 128 + col(ni): ascending in (tn, ni), so per row "replace only on strictly greater" keeps the lowest class of the lane's
// maxima.  The 64 candidates of a row (32 lanes of each of the two column waves) meet once, at the end (halve32, rank_row_meet);
// there equal values resolve to the lower class.
__global__ __launch_bounds__(RTHREADS, 2) void fewshot_predict_kernel(const char* __restrict__ Zs, const char* __restrict__ W,
                                                                      int Nt, int C, int dim, long ldz, long ldw,
                                                                      int* __restrict__ pred, float* __restrict__ best) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const RankLane t = rank_lane();
  const int m0 = blockIdx.x * RT;
  int rowsA, rowsB;
  const __amdgpu_buffer_rsrc_t rsA = rank_rows(Zs, m0, Nt, ldz, &rowsA);
  constexpr int NONE = 0x7fffffff;
  RankBest best_q[32];
#pragma unroll
  for (int q = 0; q < 32; ++q) best_q[q] = {-__builtin_huge_valf(), NONE};

  const int Tc = (C + RT - 1) / RT;
  f32x16 acc[2][2];
  for (int tn = 0; tn < Tc; ++tn) {
    const int n0 = tn * RT;
    const __amdgpu_buffer_rsrc_t rsB = rank_rows(W, n0, C, ldw, &rowsB);
    __syncthreads();                          // the previous tile's readers are done with the ring
    rank_tile(smem, rsA, rsB, ldz, ldw, dim, acc);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int cls = t.col(ni, n0);
      if (cls < C) {
#pragma unroll
        for (int q = 0; q < 32; ++q) {
          const float v = acc[q >> 4][ni][q & 15];
          const bool take = v > best_q[q].v || best_q[q].c == NONE;
          best_q[q] = take ? RankBest{v, cls} : best_q[q];
        }
      }
    }
  }
  halve32(best_q, t.L, rank_better);
  __syncthreads();                            // the ring is dead: its first 2 KiB take the two column waves' results
  const RankBest b = rank_row_meet(t, (RankBest*)smem, best_q[0], rank_better);
  if (t.tid < rowsA) {
    pred[m0 + t.tid] = b.c;
    best[m0 + t.tid] = b.v;
  }
}

LdsOptIn g_fs_lds;

template <class K, class... A>
int fs_launch(K kernel, int64_t grid, void* stream, const char* name, A... args) {
  return rank_launch(g_fs_lds, {(const void*)fewshot_gram_kernel, (const void*)fewshot_predict_kernel}, 2 * R_STAGE, "fewshot", kernel,
                     grid, 2 * R_STAGE, stream, name, args...);
}
int fs_rows(const char* name, const void* index, int64_t N, int64_t Ntot, int64_t D, int64_t ldx) {
  if (N < 0 || Ntot < 0 || D < 0 || ldx < D || N >= (1L << 31) || Ntot >= (1L << 31) || D >= (1L << 31) - 64) {
    clipa_set_error("%s: N = %ld, Ntot = %ld, D = %ld, ldx = %ld out of range (ldx >= D)", name, (long)N, (long)Ntot, (long)D, (long)ldx);
    return CLIPA_ERR_ARG;
  }
  if (!index && N > Ntot) { clipa_set_error("%s: N = %ld rows of a matrix of %ld without an index list", name, (long)N, (long)Ntot); return CLIPA_ERR_ARG; }
  if (index && ((uintptr_t)index & 3)) { clipa_set_error("%s: index is not 4-byte aligned", name); return CLIPA_ERR_ARG; }
  return 0;
}

}  // namespace
}  // namespace clipa_gemm

using namespace clipa_gemm;

extern "C" int clipa_fewshot_moments(const float* x, const int32_t* index, int64_t N, int64_t Ntot, int64_t D, int64_t ldx,
                                     float* mean, float* std, void* stream) {
  if (int rc = fs_rows("fewshot_moments", index, N, Ntot, D, ldx)) return rc;
  if (D == 0) return CLIPA_OK;
  if (int rc = clipa_check_ptrs16("fewshot_moments", {mean, std})) return rc;
  if (N > 0) if (int rc = clipa_check_ptrs16("fewshot_moments", {x})) return rc;       // N = 0: x is never read, mean = std = 0 / 0 = NaN
  hipLaunchKernelGGL(fewshot_moments_kernel, dim3((unsigned)((D + MOM_COLS - 1) / MOM_COLS)), dim3(MOM_COLS * MOM_SLICES), 0,
                     (hipStream_t)stream, x, index, (int)N, (int)Ntot, (int)D, (long)ldx, mean, std);
  return clipa_check_launch("fewshot_moments");
}

extern "C" int clipa_fewshot_whiten(const float* x, const int32_t* index, int64_t N, int64_t Ntot, int64_t D, int64_t ldx,
                                    const float* mean, const float* std, float* Z, int64_t ldz, float* Zt, int64_t ldt,
                                    void* stream) {
  if (int rc = fs_rows("fewshot_whiten", index, N, Ntot, D, ldx)) return rc;
  if (ldz < D + 1 || ldz >= (1L << 31) - 64 || (Zt && (ldt < N || ldt >= (1L << 31) - 64))) {
    clipa_set_error("fewshot_whiten: ldz = %ld must be >= D + 1 = %ld and ldt = %ld >= N = %ld", (long)ldz, (long)(D + 1), (long)ldt, (long)N);
    return CLIPA_ERR_ARG;
  }
  if (N == 0) return CLIPA_OK;
  if (int rc = clipa_check_ptrs16("fewshot_whiten", {Z})) return rc;
  if (D > 0) if (int rc = clipa_check_ptrs16("fewshot_whiten", {x, mean, std})) return rc;
  if (Zt && ((uintptr_t)Zt & 15)) { clipa_set_error("fewshot_whiten: Zt is not 16-byte aligned"); return CLIPA_ERR_ARG; }
  const int64_t rows = Zt && ldt > N ? ldt : N;
  const int64_t gx = (rows + WT - 1) / WT, gy = (ldz + WT - 1) / WT;
  if (gy > 65535) { clipa_set_error("fewshot_whiten: ldz = %ld is more than 65535 tiles of %d columns", (long)ldz, WT); return CLIPA_ERR_ARG; }
  hipLaunchKernelGGL(fewshot_whiten_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, x, index, (int)N,
                     (int)Ntot, (int)D, (long)ldx, mean, std, Z, (long)ldz, Zt, (long)ldt);
  return clipa_check_launch("fewshot_whiten");
}

extern "C" int clipa_fewshot_gram(const float* A, int64_t M, int64_t E, int64_t lda, float* S, int64_t lds, void* stream) {
  if (M < 0 || E < 0 || lds < M) { clipa_set_error("fewshot_gram: M = %ld, E = %ld, lds = %ld out of range (lds >= M)", (long)M, (long)E, (long)lds); return CLIPA_ERR_ARG; }
  if (M == 0) return CLIPA_OK;
  if (E == 0) {                               // the empty sum: S = 0
    if (int rc = clipa_check_ptrs16("fewshot_gram", {S})) return rc;
    const hipError_t e = hipMemset2DAsync(S, (size_t)lds * 4, 0, (size_t)M * 4, (size_t)M, (hipStream_t)stream);
    if (e != hipSuccess) { clipa_set_error("fewshot_gram: hipMemset2DAsync: %s", hipGetErrorString(e)); return CLIPA_ERR_LAUNCH; }
    return CLIPA_OK;
  }
  const int64_t T = (M + RT - 1) / RT;
  if (int rc = rank_check_args("fewshot_gram", E, lda, lda, M >= (1L << 30) || T * (T + 1) / 2 >= (1L << 31), "M", {A, S}, nullptr)) return rc;
  return fs_launch(fewshot_gram_kernel, T * (T + 1) / 2, stream, "fewshot_gram", (const char*)A, (int)M, (int)E, (long)lda, S, (long)lds);
}

extern "C" int clipa_fewshot_class_sums(const float* Z, const int32_t* offsets, int64_t N, int64_t dim, int64_t C, int64_t ldz,
                                        float* R, int64_t ldr, void* stream) {
  if (N < 0 || dim < 0 || C < 0 || ldz < dim || ldr < C || N >= (1L << 31) || dim >= (1L << 31) - 64 || C > 65535) {
    clipa_set_error("fewshot_class_sums: N = %ld, dim = %ld, C = %ld (at most 65535), ldz = %ld, ldr = %ld out of range", (long)N, (long)dim,
                    (long)C, (long)ldz, (long)ldr);
    return CLIPA_ERR_ARG;
  }
  if (dim == 0 || C == 0) return CLIPA_OK;
  if (int rc = clipa_check_ptrs16("fewshot_class_sums", {offsets, R})) return rc;
  if (N > 0) if (int rc = clipa_check_ptrs16("fewshot_class_sums", {Z})) return rc;
  const unsigned gx = (unsigned)((dim + 63) / 64);
  hipLaunchKernelGGL(fewshot_segsum_kernel, dim3(gx, (unsigned)C), dim3(64), 0, (hipStream_t)stream, Z, offsets, (int)N, (int)dim,
                     (long)ldz, R, (long)ldr);
  if (int rc = clipa_check_launch("fewshot_class_sums (segments)")) return rc;
  hipLaunchKernelGGL(fewshot_signsum_kernel, dim3(gx), dim3(64), 0, (hipStream_t)stream, (int)dim, (int)C, R, (long)ldr);
  return clipa_check_launch("fewshot_class_sums");
}

extern "C" int clipa_fewshot_predict(const float* Z, const float* W, int64_t Nt, int64_t C, int64_t dim, int64_t ldz, int64_t ldw,
                                     int32_t* pred, float* best, void* stream) {
  if (Nt < 0 || C < 0 || dim < 0) { clipa_set_error("fewshot_predict: Nt = %ld, C = %ld, dim = %ld must be >= 0", (long)Nt, (long)C, (long)dim); return CLIPA_ERR_ARG; }
  if (Nt == 0) return CLIPA_OK;
  if (C == 0) { clipa_set_error("fewshot_predict: C = 0 classes for Nt = %ld rows (an argmax over nothing)", (long)Nt); return CLIPA_ERR_ARG; }
  if (dim == 0) {                             // every logit is the empty sum 0: class 0 wins with 0
    if (int rc = clipa_check_ptrs16("fewshot_predict", {pred, best})) return rc;
    hipError_t e = hipMemsetAsync(pred, 0, (size_t)Nt * 4, (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(best, 0, (size_t)Nt * 4, (hipStream_t)stream);
    if (e != hipSuccess) { clipa_set_error("fewshot_predict: hipMemsetAsync: %s", hipGetErrorString(e)); return CLIPA_ERR_LAUNCH; }
    return CLIPA_OK;
  }
  if (int rc = rank_check_args("fewshot_predict", dim, ldz, ldw, Nt >= (1L << 31) - RT || C >= (1L << 31) - RT, "Nt, C", {Z, W, pred, best}, nullptr)) return rc;
  return fs_launch(fewshot_predict_kernel, (Nt + RT - 1) / RT, stream, "fewshot_predict", (const char*)Z, (const char*)W, (int)Nt,
                   (int)C, (int)dim, (long)ldz, (long)ldw, pred, best);
}
