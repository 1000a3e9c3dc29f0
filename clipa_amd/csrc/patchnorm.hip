// Dual PatchNorm stem (input_patchnorm, arXiv 2302.01327) of the image tower on gfx950.
// open_clip/transformer.py:362-371,483-489: x = rearrange(img, 'b c (h p1) (w p2) -> b (h w) (c p1 p2)');
// x = patchnorm_pre_ln(x) (LayerNorm over K = 3 P P, eps 1e-5); x = conv1(x) (nn.Linear(K, width)).
// The engine splits LayerNorm_K(x) W^T + b into xhat W'^T + b' with xhat = (x - mean) * rstd (patchify_ln_kernel, the only
// pass over the images), W' = W diag(gamma) and b' = b + W beta (patchnorm_fold_kernel, once per optimizer step), so the
// stem GEMM and its weight-gradient GEMM run unchanged; patchnorm_unfold_kernel turns the folded layer's gradients into
// those of conv1.weight, patchnorm_pre_ln.weight and patchnorm_pre_ln.bias.
#include "row_wave.h"
#include "clipa_hip.h"

namespace {

// 8 consecutive elements k0 .. k0 + 7 of a patch row in (ph, pw, c) order as floats, with the optional (x / 255 - mean) / std
// of train.py:191-197; elements >= K are zero.  The element order, the index arithmetic and the uint8 channels_last fast path
// (8 consecutive bytes of an image row) are those of misc.hip's patchify_kernel.
struct PatchSrc {
  const void* img;
  size_t b;
  int S, P, K, py, px, nhwc, normalize, fast8;
  float m[3], is[3];
};
template <int DT>
__device__ __forceinline__ void patch_load8(const PatchSrc& p, int k0, float* f) {
  if (DT == 0 && p.fast8) {
    if (k0 < p.K) {       // 3 P % 8 == 0: K is a multiple of 8 and a chunk never straddles two image rows
      const int ph = k0 / (3 * p.P), off = k0 - ph * 3 * p.P;
      const size_t src = ((p.b * p.S + (p.py * p.P + ph)) * p.S + p.px * p.P) * 3 + off;
      const uint2 raw = *(const uint2*)((const unsigned char*)p.img + src);
      int c = off % 3;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float v = (float)(((i < 4 ? raw.x : raw.y) >> (8 * (i & 3))) & 0xffu);
        if (p.normalize) v = (v * (1.0f / 255.0f) - p.m[c]) * p.is[c];
        f[i] = v;
        c = c == 2 ? 0 : c + 1;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) f[i] = 0.f;
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = k0 + i;
    float v = 0.f;
    if (k < p.K) {
      const int c = k % 3, pw = (k / 3) % p.P, ph = k / (3 * p.P);
      const int y = p.py * p.P + ph, x = p.px * p.P + pw;
      const size_t src = p.nhwc ? ((p.b * p.S + y) * p.S + x) * 3 + c : ((p.b * 3 + c) * p.S + y) * p.S + x;
      if (DT == 0) v = (float)((const unsigned char*)p.img)[src];
      else if (DT == 1) v = bf2f(((const unsigned short*)p.img)[src]);
      else v = ((const float*)p.img)[src];
      if (p.normalize) v = (v * (1.0f / 255.0f) - p.m[c]) * p.is[c];
    }
    f[i] = v;
  }
}

// One wave per patch row, four rows per workgroup; lane l holds the 8-element chunks l + 64 c of the Kp-wide row (row_wave.h).
// K = 192 (P = 8) fills 24 lanes, K = 588 (P = 14) ends inside chunk 73 of Kp = 592, K = 3072 (P = 32) is 6 chunks per lane.
// The statistics are row_wave.h's LayerNorm arithmetic - the lane's sum over c, then i, ascending; wave_sum; mean; the centred
// sum of squares in fused multiply-adds; wave_sum; rsqrtf - over the K real elements: the pad columns hold zeros, which add
// nothing to the sum, and are left out of the squares.  They are taken on x - x[0]: (x - mean) is the same number, a constant
// patch becomes exact zeros (mean 0, every deviation 0, whatever K equal terms sum to in fp32), and uint8 values up to 255
// lose nothing to cancellation.
template <int DT, int NCH>
__global__ __launch_bounds__(256) void patchify_ln_kernel(const void* __restrict__ img, unsigned short* __restrict__ out, long rows,
                                                          int S, int P, int g, int Kp, int nhwc, int normalize, float m0,
                                                          float m1, float m2, float is0, float is1, float is2, float eps) {
  const RowWave<NCH> w(Kp);
  const long patch = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (patch >= rows) return;                  // (a whole wave: the shuffles below see 64 lanes)
  PatchSrc p;
  p.img = img;
  p.S = S; p.P = P; p.K = 3 * P * P;
  p.px = (int)(patch % g);
  p.py = (int)((patch / g) % g);
  p.b = (size_t)(patch / ((long)g * g));
  p.nhwc = nhwc; p.normalize = normalize;
  p.fast8 = nhwc && (3 * P) % 8 == 0 && (3 * S) % 8 == 0 && ((size_t)img & 7) == 0;
  p.m[0] = m0; p.m[1] = m1; p.m[2] = m2; p.is[0] = is0; p.is[1] = is1; p.is[2] = is2;
  const int K = p.K;
  float v[NCH][8] = {};
  w.each([&](int c, size_t col) { patch_load8<DT>(p, (int)col, v[c]); });
  const float pivot = __shfl(v[0][0], 0, 64);          // element 0 of the row: chunk 0 of lane 0 (Kp >= 8)
  w.each([&](int c, size_t col) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[c][i] = (int)col + i < K ? v[c][i] - pivot : 0.f;
  });
  float s = 0.f;
  ln_row_sum(w, v, s);
  const float invK = 1.0f / (float)K;
  const float mean = wave_sum(s) * invK;
  float ss = 0.f;
  w.each([&](int c, size_t col) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if ((int)col + i < K) { const float d = v[c][i] - mean; ss = __builtin_fmaf(d, d, ss); }
  });
  const float rstd = rsqrtf(__builtin_fmaf(wave_sum(ss), invK, eps));
  unsigned short* orow = out + (size_t)patch * Kp;
  w.each([&](int c, size_t col) {
    float y[8];
    ln_xhat8(v[c], mean, rstd, y);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if ((int)col + i >= K) y[i] = 0.f;
    *(u32x4*)(orow + col) = pack8(y);
  });
}

__device__ __forceinline__ float pn_load1(const void* __restrict__ w, int w_f32, size_t i) {
  return w_f32 ? ((const float*)w)[i] : bf2f(((const unsigned short*)w)[i]);
}
// column j of the engine's (ph, pw, c) order -> column of the parameters' (c, p1, p2) order
__device__ __forceinline__ int pn_src_col(int j, int P2) { return (j % 3) * P2 + j / 3; }

// One wave per row n of W: lane l takes the output columns j = l, l + 64, ... (ascending), so the stores are contiguous and the
// reads gather within the row (the matrix is small and built once per optimizer step).  b' adds the lane's products in that
// order with fused multiply-adds, then the fixed butterfly of wave_sum.
__global__ __launch_bounds__(256) void patchnorm_fold_kernel(const void* __restrict__ w, int w_f32, const float* __restrict__ b,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             unsigned short* __restrict__ wf, float* __restrict__ bf, long N,
                                                             int P2, int Kp) {
  const int lane = threadIdx.x & 63;
  const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const int K = 3 * P2;
  float acc = 0.f;
  for (int j = lane; j < Kp; j += 64) {
    float o = 0.f;
    if (j < K) {
      const int k = pn_src_col(j, P2);
      const float x = pn_load1(w, w_f32, (size_t)n * K + k);
      o = x * gamma[k];
      acc = __builtin_fmaf(x, beta[k], acc);
    }
    wf[(size_t)n * Kp + j] = f2bf(o);
  }
  acc = wave_sum(acc);
  if (lane == 0) bf[n] = b[n] + acc;
}

// A workgroup of 16 waves owns 64 columns k of the parameters' order (lane = column); wave v walks the rows n = v, v + 16, ...
// (ascending) with the reads of W and the stores of dW contiguous along k, and the 16 partial sums of a column meet in LDS in
// wave order: no atomics, the same bits on every run.
constexpr int PN_WAVES = 16;
template <bool DW_F32>
__global__ __launch_bounds__(64 * PN_WAVES) void patchnorm_unfold_kernel(const float* __restrict__ g, const float* __restrict__ s,
                                                                         const void* __restrict__ w, int w_f32,
                                                                         const float* __restrict__ gamma,
                                                                         const float* __restrict__ beta, void* __restrict__ dw,
                                                                         float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                         int N, int P2, int Kp) {
  __shared__ float red[2][PN_WAVES][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int K = 3 * P2;
  const int k = blockIdx.x * 64 + lane;
  const bool live = k < K;
  const int j = live ? (k % P2) * 3 + k / P2 : 0;      // this column in g's (ph, pw, c) order
  const float gm = live ? gamma[k] : 0.f, bt = live ? beta[k] : 0.f;
  const bool need_w = dgamma || dbeta;
  float ag = 0.f, ab = 0.f;
  if (live) {
    for (int n = wv; n < N; n += PN_WAVES) {
      const float gv = g[(size_t)n * Kp + j], sv = s[n];
      if (need_w) {
        const float x = pn_load1(w, w_f32, (size_t)n * K + k);
        ag = __builtin_fmaf(x, gv, ag);
        ab = __builtin_fmaf(x, sv, ab);
      }
      if (dw) {
        const float d = __builtin_fmaf(bt, sv, gm * gv);
        if (DW_F32) ((float*)dw)[(size_t)n * K + k] = d;
        else ((unsigned short*)dw)[(size_t)n * K + k] = f2bf(d);
      }
    }
  }
  if (!need_w) return;                         // (uniform over the workgroup)
  red[0][wv][lane] = ag;
  red[1][wv][lane] = ab;
  __syncthreads();
  if (wv == 0 && live) {
    float a = 0.f, c = 0.f;
#pragma unroll
    for (int i = 0; i < PN_WAVES; ++i) { a += red[0][i][lane]; c += red[1][i][lane]; }
    if (dgamma) dgamma[k] = a;
    if (dbeta) dbeta[k] = c;
  }
}

int pn_geometry(const char* who, int64_t P, int64_t Kp) {
  if (P <= 0 || Kp % 8 != 0 || Kp < 3 * P * P || Kp > 3072) {
    clipa_set_error("%s: bad geometry P=%ld Kp=%ld (Kp %% 8 == 0, 3*P*P <= Kp <= 3072)", who, (long)P, (long)Kp);
    return CLIPA_ERR_ARG;
  }
  return CLIPA_OK;
}

}  // namespace

extern "C" int clipa_patchify_ln(const void* img, void* out, int64_t B, int64_t S, int64_t P, int64_t Kp, int in_dtype, int nhwc,
                                 int normalize, const float* mean3, const float* std3, float eps, void* stream) {
  if (int rc = pn_geometry("patchify_ln", P, Kp)) return rc;
  const int64_t g = S / P;
  if (g <= 0) { clipa_set_error("patchify_ln: bad geometry S=%ld P=%ld", (long)S, (long)P); return CLIPA_ERR_ARG; }
  if (in_dtype != CLIPA_DT_U8 && in_dtype != CLIPA_DT_BF16 && in_dtype != CLIPA_DT_F32) { clipa_set_error("patchify_ln: unsupported input dtype %d", in_dtype); return CLIPA_ERR_ARG; }
  if (B <= 0) return CLIPA_OK;
  if (!img || !out) { clipa_set_error("patchify_ln: null operand"); return CLIPA_ERR_ARG; }
  float m[3] = {0, 0, 0}, is[3] = {1, 1, 1};
  if (normalize) {
    if (!mean3 || !std3) { clipa_set_error("patchify_ln: normalize needs mean/std"); return CLIPA_ERR_ARG; }
    for (int i = 0; i < 3; ++i) { m[i] = mean3[i]; is[i] = 1.0f / std3[i]; }
  }
  const int64_t rows = B * g * g;
  if ((rows + 3) / 4 > 0x7fffffffL) { clipa_set_error("patchify_ln: %ld patches exceed one grid", (long)rows); return CLIPA_ERR_ARG; }
  const dim3 grid((unsigned)((rows + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
  dispatch_nch<1, 2, 6>(Kp, [&](auto nch) {
    constexpr int NCH = decltype(nch)::value;
#define CLIPA_PATCHIFY_LN(DT) hipLaunchKernelGGL((patchify_ln_kernel<DT, NCH>), grid, dim3(256), 0, st, img, (unsigned short*)out, (long)rows, (int)S, (int)P, (int)g, (int)Kp, nhwc, normalize, m[0], m[1], m[2], is[0], is[1], is[2], eps)
    if (in_dtype == CLIPA_DT_U8) CLIPA_PATCHIFY_LN(0);
    else if (in_dtype == CLIPA_DT_BF16) CLIPA_PATCHIFY_LN(1);
    else CLIPA_PATCHIFY_LN(2);
#undef CLIPA_PATCHIFY_LN
  });
  return clipa_check_launch("patchify_ln");
}

extern "C" int clipa_patchnorm_fold(const void* w, int w_f32, const float* b, const float* gamma, const float* beta,
                                    void* w_folded, float* b_folded, int64_t N, int64_t P, int64_t Kp, void* stream) {
  if (!w || !b || !gamma || !beta || !w_folded || !b_folded) { clipa_set_error("patchnorm_fold: null operand"); return CLIPA_ERR_ARG; }
  if (int rc = pn_geometry("patchnorm_fold", P, Kp)) return rc;
  if (N <= 0) return CLIPA_OK;
  if ((N + 3) / 4 > 0x7fffffffL) { clipa_set_error("patchnorm_fold: N=%ld exceeds one grid", (long)N); return CLIPA_ERR_ARG; }
  hipLaunchKernelGGL(patchnorm_fold_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, w, w_f32, b, gamma,
                     beta, (unsigned short*)w_folded, b_folded, (long)N, (int)(P * P), (int)Kp);
  return clipa_check_launch("patchnorm_fold");
}

extern "C" int clipa_patchnorm_unfold(const float* g, const float* s, const void* w, int w_f32, const float* gamma,
                                      const float* beta, void* dw, int dw_f32, float* dgamma, float* dbeta, int64_t N, int64_t P,
                                      int64_t Kp, void* stream) {
  if (!g || !s || !w || !gamma || !beta) { clipa_set_error("patchnorm_unfold: null operand (only the outputs dw, dgamma, dbeta may be null)"); return CLIPA_ERR_ARG; }
  if (int rc = pn_geometry("patchnorm_unfold", P, Kp)) return rc;
  if (N <= 0 || (!dw && !dgamma && !dbeta)) return CLIPA_OK;
  if (N > 0x7fffffffL) { clipa_set_error("patchnorm_unfold: N=%ld outside [1, 2^31)", (long)N); return CLIPA_ERR_ARG; }
  const int K = (int)(3 * P * P);
  const dim3 grid((unsigned)((K + 63) / 64));
  hipStream_t st = (hipStream_t)stream;
  if (dw_f32) hipLaunchKernelGGL(patchnorm_unfold_kernel<true>, grid, dim3(64 * PN_WAVES), 0, st, g, s, w, w_f32, gamma, beta, dw, dgamma, dbeta, (int)N, (int)(P * P), (int)Kp);
  else hipLaunchKernelGGL(patchnorm_unfold_kernel<false>, grid, dim3(64 * PN_WAVES), 0, st, g, s, w, w_f32, gamma, beta, dw, dgamma, dbeta, (int)N, (int)(P * P), (int)Kp);
  return clipa_check_launch("patchnorm_unfold");
}
