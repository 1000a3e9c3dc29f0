// Multihead attention pooling (the "map" head of clipa_jax/models/vit.py:187-207), the part that touches all B * L tokens.
//
// The head has ONE query per sample and that query is the same for every sample (a learned probe), so the K and V
// projections fold out of the token-level work (clipa_amd/engine.py: MapHeadFn):
//   s[b,l,h] = x[b,l,:] . U[h,:]                U[h,:] = dh^-0.5 Wk_h^T q_h          ([H, D], built once per weight version)
//   p[b,:,h] = softmax_l s[b,:,h]               (the bk_h . q_h term is constant over l and cancels)
//   z[b,h,:] = sum_l p[b,l,h] x[b,l,:]          head_h = Wv_h z[b,h,:] + bv_h follows on B rows, outside this file
// forward:  x is read once; per chunk of MP_CH = 32 rows S = X U^T and Z += P^T X run on v_mfma_f32_16x16x32_bf16 (H <= 16
//           heads fill one 16-wide tile), online softmax over the chunks with the z accumulators in registers
//           ([16, D] fp32 over 256 lanes = D / 16 registers per lane).  P is rounded to bf16 for the second product, the
//           softmax sum is taken over the unrounded fp32 values (as the attention kernels do).
// backward: delta[b,h] = z[b,h,:] . dz[b,h,:] (= sum_l p dp, the flash-attention identity); per chunk
//           s = X U^T, dp = X dZ^T, p = exp(s - m) / sum (saved statistics), ds = p (dp - delta),
//           dX = [P | dS] . [dZ ; U] (ONE product with K = 32: 16 heads of P and 16 heads of dS), dU += dS^T X.
//           x is read once, dx written once.  dZ, P and dS are rounded to bf16 as MFMA operands.  dU leaves each workgroup
//           as an fp32 partial and is summed over the workgroups in index order by a second kernel: no atomics, the result
//           is a function of the launch shape (B, max_workgroups) alone.
// A workgroup (4 waves) owns a sample at a time: b = blockIdx.x, blockIdx.x + gridDim.x, ...
// LDS: the chunk as a row-major image [32][D] bf16 with 16 pad bytes per row - read row-wise (ds_read_b128) as the A operand
// of S / dP and column-wise (ds_read_b64_tr_b16) as the B operand of Z / dU - plus the cross-wave score tiles.
#include "common.h"
#include <algorithm>

namespace clipa_gemm {
namespace {

constexpr int MP_CH = 32;                      // rows per chunk = the K of one Z / dU MFMA
constexpr int MP_THREADS = 256;
constexpr int MP_DMAX = 2048;
constexpr int MP_RED_BYTES = 2 * 2 * MP_CH * 16 * 4;   // [k half][S | dP][row][head] fp32
constexpr int MP_SM_BYTES = 3 * 16 * 4;                // max, 1 / sum, delta per head
constexpr int MP_DEFAULT_WG = 768;

__host__ __device__ constexpr int mp_pitch(int D) { return 2 * D + 16; }
constexpr int mp_lds_bytes(int D) { return MP_CH * mp_pitch(D) + MP_RED_BYTES + MP_SM_BYTES; }

struct MPArgs {
  const unsigned short* x; long ldx;      // bf16 [B * L, ldx]
  const unsigned short* U;                // bf16 [H, D]
  float* z; float* stats;                 // f32 [B, H, D], [B, H, 2]
  const float* dz;                        // f32 [B, H, D]
  unsigned short* dx; long lddx;          // bf16 [B * L, lddx]
  const unsigned short* UT;               // bf16 [D, 16]      (bwd: head-minor copies, the B operand of dX)
  const unsigned short* dzT;              // bf16 [B, D, 16]
  float* part;                            // f32 [workgroups, H, D]
  int B, L, D, H;
};

typedef __attribute__((address_space(3))) bf16x4* lds_bf16x4;

// the chunk's rows l0 .. l0 + 31 of sample b into the image; rows past L are zeros
__device__ __forceinline__ void mp_stage(char* img, const MPArgs& p, int b, int l0, int tid) {
  const int cpr = p.D >> 3;                               // 16-byte pieces per row
  const int PB = mp_pitch(p.D);
  const unsigned short* xb = p.x + ((size_t)b * p.L + l0) * p.ldx;
#pragma unroll 4
  for (int q = tid; q < MP_CH * cpr; q += MP_THREADS) {
    const int row = q / cpr, c = q - row * cpr;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (l0 + row < p.L) v = *(const u32x4*)(xb + (size_t)row * p.ldx + c * 8);
    *(u32x4*)(img + row * PB + c * 16) = v;
  }
}

// B operand of a product that sums over the chunk's rows: lane (g, i) gets X[8g + j][d0 + i], j = 0..7
__device__ __forceinline__ bf16x8 mp_colfrag(const char* img, int PB, int d0, int g, int i) {
  bf16x8 f;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int row = 8 * g + 4 * half + (i >> 2);
    const bf16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4)(img + row * PB + (d0 + 4 * (i & 3)) * 2));
    f[4 * half + 0] = v[0]; f[4 * half + 1] = v[1]; f[4 * half + 2] = v[2]; f[4 * half + 3] = v[3];
  }
  return f;
}

__device__ __forceinline__ bf16x8 mp_pack(const float* f) { return __builtin_bit_cast(bf16x8, pack8(f)); }

template <int NB>
__global__ __launch_bounds__(MP_THREADS) void mappool_fwd_kernel(MPArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, i = lane & 15;
  const int D = p.D, H = p.H, L = p.L, PB = mp_pitch(D);
  char* img = smem;
  float* red = (float*)(smem + MP_CH * PB);               // [k half][32 rows][16 heads]
  const int nb = D >> 6;                                  // 16-column blocks per wave: block cb * 4 + wave
  const int rb = wave & 1, kh = wave >> 1;                // scores: row block, half of the K range
  const int khalf = D >> 6, k0 = kh * khalf;              // K steps of 32 per half
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
    f32x4 acc[NB];
#pragma unroll
    for (int cb = 0; cb < NB; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -3.0e38f, sum = 0.f;                        // of head i (every 16-lane group holds the same)
    for (int l0 = 0; l0 < L; l0 += MP_CH) {
      __syncthreads();                                    // the previous chunk's readers are done
      mp_stage(img, p, b, l0, tid);
      __syncthreads();
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      for (int ks = k0; ks < k0 + khalf; ++ks) {
        const bf16x8 a = *(const bf16x8*)(img + (rb * 16 + i) * PB + (ks * 32 + 8 * g) * 2);
        const bf16x8 u = i < H ? *(const bf16x8*)(p.U + (size_t)i * D + ks * 32 + 8 * g) : zero8;
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, u, s, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(kh * MP_CH + rb * 16 + 4 * g + r) * 16 + i] = s[r];   // col = head i, row = 4g + r
      __syncthreads();
      // the P^T fragment of this chunk: head i, rows 8g + j
      float sv[8];
      float cmax = -3.0e38f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int l = 8 * g + j;
        sv[j] = l0 + l < L ? red[l * 16 + i] + red[(MP_CH + l) * 16 + i] : -3.0e38f;
        cmax = fmaxf(cmax, sv[j]);
      }
      cmax = fmaxf(cmax, __shfl_xor(cmax, 16, 64));
      cmax = fmaxf(cmax, __shfl_xor(cmax, 32, 64));
      const float mnew = fmaxf(m, cmax);
      const float scale = __expf(m - mnew);
      float psum = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) { sv[j] = __expf(sv[j] - mnew); psum += sv[j]; }
      psum += __shfl_xor(psum, 16, 64);
      psum += __shfl_xor(psum, 32, 64);
      sum = sum * scale + psum;
      m = mnew;
      const bf16x8 pf = mp_pack(sv);
      float sc[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) sc[r] = __shfl(scale, 4 * g + r, 64);      // accumulator row = head 4g + r
#pragma unroll
      for (int cb = 0; cb < NB; ++cb)
        if (cb < nb) {
          const bf16x8 xf = mp_colfrag(img, PB, (cb * 4 + wave) * 16, g, i);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[cb][r] *= sc[r];
          acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, xf, acc[cb], 0, 0, 0);
        }
    }
    const float inv = 1.0f / sum;
    float ir[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ir[r] = __shfl(inv, 4 * g + r, 64);
#pragma unroll
    for (int cb = 0; cb < NB; ++cb)
      if (cb < nb) {
        const int d = (cb * 4 + wave) * 16 + i;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * g + r < H) p.z[((size_t)b * H + 4 * g + r) * D + d] = acc[cb][r] * ir[r];
      }
    if (wave == 0 && g == 0 && i < H) {
      p.stats[((size_t)b * H + i) * 2] = m;
      p.stats[((size_t)b * H + i) * 2 + 1] = sum;
    }
  }
}

template <int NB>
__global__ __launch_bounds__(MP_THREADS) void mappool_bwd_kernel(MPArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, i = lane & 15;
  const int D = p.D, H = p.H, L = p.L, PB = mp_pitch(D);
  char* img = smem;
  float* red = (float*)(smem + MP_CH * PB);               // [k half][S | dP][32 rows][16 heads]
  float* sm_m = red + 2 * 2 * MP_CH * 16;
  float* sm_inv = sm_m + 16;
  float* sm_delta = sm_inv + 16;
  const int nb = D >> 6;
  const int rb = wave & 1, kh = wave >> 1;
  const int khalf = D >> 6, k0 = kh * khalf;
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const int hb = 8 * (g & 1);                             // the dX operand: lanes g < 2 carry P, g >= 2 dS, heads hb + j

  f32x4 du[NB];
#pragma unroll
  for (int cb = 0; cb < NB; ++cb) du[cb] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
    __syncthreads();                                      // the previous sample's readers of sm_* are done
    for (int h = wave; h < 16; h += 4) {
      float a = 0.f;
      if (h < H) {
        const float* zr = p.z + ((size_t)b * H + h) * D;
        const float* dr = p.dz + ((size_t)b * H + h) * D;
        for (int d = lane; d < D; d += 64) a += zr[d] * dr[d];
      }
      a = wave_sum(a);
      if (lane == 0) {
        sm_delta[h] = a;
        sm_m[h] = h < H ? p.stats[((size_t)b * H + h) * 2] : 0.f;
        sm_inv[h] = h < H ? 1.0f / p.stats[((size_t)b * H + h) * 2 + 1] : 0.f;
      }
    }
    for (int l0 = 0; l0 < L; l0 += MP_CH) {
      __syncthreads();
      mp_stage(img, p, b, l0, tid);
      __syncthreads();
      f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
      for (int ks = k0; ks < k0 + khalf; ++ks) {
        const bf16x8 a = *(const bf16x8*)(img + (rb * 16 + i) * PB + (ks * 32 + 8 * g) * 2);
        bf16x8 u = zero8, dzf = zero8;
        if (i < H) {
          u = *(const bf16x8*)(p.U + (size_t)i * D + ks * 32 + 8 * g);
          const float* src = p.dz + ((size_t)b * H + i) * D + ks * 32 + 8 * g;
          float f[8];
          *(f32x4*)f = *(const f32x4*)src;
          *(f32x4*)(f + 4) = *(const f32x4*)(src + 4);
          dzf = mp_pack(f);
        }
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, u, s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, dzf, dp, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        red[((kh * 2 + 0) * MP_CH + rb * 16 + 4 * g + r) * 16 + i] = s[r];
        red[((kh * 2 + 1) * MP_CH + rb * 16 + 4 * g + r) * 16 + i] = dp[r];
      }
      __syncthreads();
      // dX^T[d][l] = sum_k W^T[d][k] A^T[k][l], A = [P | dS]: lane (g, i) holds A[row l = 16 rb2 + i][k = 8g + j]
      bf16x8 af[2];
#pragma unroll
      for (int rb2 = 0; rb2 < 2; ++rb2) {
        const int l = rb2 * 16 + i;
        const bool ok = l0 + l < L;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int h = hb + j;
          const float sj = red[(0 * MP_CH + l) * 16 + h] + red[(2 * MP_CH + l) * 16 + h];
          const float dj = red[(1 * MP_CH + l) * 16 + h] + red[(3 * MP_CH + l) * 16 + h];
          const float pj = ok ? __expf(sj - sm_m[h]) * sm_inv[h] : 0.f;
          v[j] = g < 2 ? pj : pj * (dj - sm_delta[h]);
        }
        af[rb2] = mp_pack(v);
      }
      const unsigned short* wsrc = g < 2 ? p.dzT + (size_t)b * D * 16 : p.UT;
#pragma unroll
      for (int cb = 0; cb < NB; ++cb)
        if (cb < nb) {
          const int d0 = (cb * 4 + wave) * 16;
          const bf16x8 wf = *(const bf16x8*)(wsrc + (size_t)(d0 + i) * 16 + hb);
#pragma unroll
          for (int rb2 = 0; rb2 < 2; ++rb2) {
            const f32x4 c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af[rb2], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            const int l = l0 + rb2 * 16 + i;              // col = row of x, rows = columns d0 + 4g .. + 3
            if (l < L) {
              u32x2 w;
              w[0] = pack2bf(c[0], c[1]);
              w[1] = pack2bf(c[2], c[3]);
              *(u32x2*)(p.dx + ((size_t)b * L + l) * p.lddx + d0 + 4 * g) = w;
            }
          }
        }
      // dU[h][d] += sum_l dS[l][h] X[l][d]: lane (g, i) holds dS of head i, rows 8g + j
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int l = 8 * g + j;
        const float sj = red[(0 * MP_CH + l) * 16 + i] + red[(2 * MP_CH + l) * 16 + i];
        const float dj = red[(1 * MP_CH + l) * 16 + i] + red[(3 * MP_CH + l) * 16 + i];
        const float pj = l0 + l < L ? __expf(sj - sm_m[i]) * sm_inv[i] : 0.f;
        v[j] = pj * (dj - sm_delta[i]);
      }
      const bf16x8 dsf = mp_pack(v);
#pragma unroll
      for (int cb = 0; cb < NB; ++cb)
        if (cb < nb) {
          const bf16x8 xf = mp_colfrag(img, PB, (cb * 4 + wave) * 16, g, i);
          du[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf, xf, du[cb], 0, 0, 0);
        }
    }
  }
#pragma unroll
  for (int cb = 0; cb < NB; ++cb)
    if (cb < nb) {
      const int d = (cb * 4 + wave) * 16 + i;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * g + r < H) p.part[((size_t)blockIdx.x * H + 4 * g + r) * D + d] = du[cb][r];
    }
}

// head-minor bf16 copies for the dX product: dzT[b][d][16] = dz[b][0..H)[d] (zero padded), UT[d][16] = U[0..H)[d]; b == B: U
__global__ void mappool_prep_kernel(MPArgs p, unsigned short* dzT, unsigned short* UT) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)(p.B + 1) * p.D) return;
  const int b = (int)(idx / p.D), d = (int)(idx - (size_t)b * p.D);
  float v[16];
#pragma unroll
  for (int h = 0; h < 16; ++h)
    v[h] = h >= p.H ? 0.f : b < p.B ? p.dz[((size_t)b * p.H + h) * p.D + d] : bf2f(p.U[(size_t)h * p.D + d]);
  unsigned short* dst = b < p.B ? dzT + ((size_t)b * p.D + d) * 16 : UT + (size_t)d * 16;
  *(u32x4*)dst = pack8(v);
  *(u32x4*)(dst + 8) = pack8(v + 8);
}

// dU[h][d] = the workgroups' partials summed in index order
__global__ void mappool_reduce_kernel(const float* __restrict__ part, float* __restrict__ dU, int nwg, int HD) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= HD) return;
  float a = 0.f;
  for (int w = 0; w < nwg; ++w) a += part[(size_t)w * HD + e];
  dU[e] = a;
}

LdsOptIn g_mp_lds;
#define MP_KERNELS(NB) (const void*)mappool_fwd_kernel<NB>, (const void*)mappool_bwd_kernel<NB>
int ensure_mp_attrs(int dev) {
  return g_mp_lds.ensure(dev, {MP_KERNELS(4), MP_KERNELS(12), MP_KERNELS(16), MP_KERNELS(22), MP_KERNELS(32)},
                         mp_lds_bytes(MP_DMAX), "mappool");
}

int mp_check(const char* who, int64_t B, int64_t L, int64_t D, int64_t H, int64_t ldx) {
  if (H < 1 || H > 16) { clipa_set_error("%s: H = %ld outside 1..16 (one 16-wide MFMA tile of heads)", who, (long)H); return CLIPA_ERR_ARG; }
  if (D < 64 || D % 64 != 0 || D > MP_DMAX) { clipa_set_error("%s: D = %ld must be a multiple of 64 in 64..%d", who, (long)D, MP_DMAX); return CLIPA_ERR_ARG; }
  if (L < 1 || L >= (1L << 31) || B >= (1L << 31)) { clipa_set_error("%s: L = %ld, B = %ld outside int32 indexing", who, (long)L, (long)B); return CLIPA_ERR_ARG; }
  if (ldx < D || ldx % 8 != 0) { clipa_set_error("%s: row stride %ld must be a multiple of 8 and >= D", who, (long)ldx); return CLIPA_ERR_ARG; }
  return CLIPA_OK;
}

int mp_grid(int64_t B, int64_t max_wg) { return (int)std::min<int64_t>(B, max_wg > 0 ? max_wg : MP_DEFAULT_WG); }

template <bool BWD>
int mp_launch(const MPArgs& a, int grid, hipStream_t st, const char* what) {
  const int nb = a.D / 64, lds = mp_lds_bytes(a.D);
#define MP_GO(NB)                                                                                              \
  do {                                                                                                         \
    if (BWD) hipLaunchKernelGGL(mappool_bwd_kernel<NB>, dim3((unsigned)grid), dim3(MP_THREADS), lds, st, a);   \
    else hipLaunchKernelGGL(mappool_fwd_kernel<NB>, dim3((unsigned)grid), dim3(MP_THREADS), lds, st, a);       \
  } while (0)
  if (nb <= 4) MP_GO(4);
  else if (nb <= 12) MP_GO(12);
  else if (nb <= 16) MP_GO(16);
  else if (nb <= 22) MP_GO(22);
  else MP_GO(32);
#undef MP_GO
  return clipa_check_launch(what);
}

}  // namespace
}  // namespace clipa_gemm

using namespace clipa_gemm;

extern "C" int64_t clipa_mappool_bwd_workspace(int64_t B, int64_t H, int64_t D, int64_t max_workgroups) {
  if (B <= 0 || H <= 0 || D <= 0) return 0;
  return D * 32 + B * D * 32 + (int64_t)mp_grid(B, max_workgroups) * H * D * (int64_t)sizeof(float);   // UT, dzT, partials
}

extern "C" int clipa_mappool_fwd(const void* x, const void* U, float* z, float* stats, int64_t B, int64_t L, int64_t D,
                                 int64_t H, int64_t ldx, int64_t max_workgroups, void* stream) {
  if (B <= 0) return CLIPA_OK;
  if (int rc = mp_check("mappool_fwd", B, L, D, H, ldx)) return rc;
  if (int rc = clipa_check_ptrs16("mappool_fwd", {x, U, z})) return rc;
  if (!stats) { clipa_set_error("mappool_fwd: null stats"); return CLIPA_ERR_ARG; }
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (int rc = ensure_mp_attrs(dev)) return rc;
  MPArgs a = {};
  a.x = (const unsigned short*)x; a.ldx = ldx; a.U = (const unsigned short*)U; a.z = z; a.stats = stats;
  a.B = (int)B; a.L = (int)L; a.D = (int)D; a.H = (int)H;
  return mp_launch<false>(a, mp_grid(B, max_workgroups), (hipStream_t)stream, "mappool_fwd");
}

extern "C" int clipa_mappool_bwd(const void* x, const void* U, const float* z, const float* stats, const float* dz, void* dx,
                                 float* dU, int64_t B, int64_t L, int64_t D, int64_t H, int64_t ldx, int64_t lddx,
                                 int64_t max_workgroups, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = mp_check("mappool_bwd", B > 0 ? B : 1, L, D, H, ldx)) return rc;
  if (!dU) { clipa_set_error("mappool_bwd: null dU"); return CLIPA_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  if (B <= 0) {      // no sample: dU = 0
    if (hipMemsetAsync(dU, 0, (size_t)(H * D) * sizeof(float), st) != hipSuccess) { clipa_set_error("mappool_bwd: memset failed"); return CLIPA_ERR_LAUNCH; }
    return CLIPA_OK;
  }
  if (lddx < D || lddx % 4 != 0) { clipa_set_error("mappool_bwd: dx row stride %ld must be a multiple of 4 and >= D", (long)lddx); return CLIPA_ERR_ARG; }
  if (int rc = clipa_check_ptrs16("mappool_bwd", {x, U, z, dz, dx, workspace})) return rc;
  if (!stats) { clipa_set_error("mappool_bwd: null stats"); return CLIPA_ERR_ARG; }
  if (workspace_bytes < clipa_mappool_bwd_workspace(B, H, D, max_workgroups)) { clipa_set_error("mappool_bwd: workspace too small"); return CLIPA_ERR_ARG; }
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (int rc = ensure_mp_attrs(dev)) return rc;
  const int grid = mp_grid(B, max_workgroups);
  MPArgs a = {};
  a.x = (const unsigned short*)x; a.ldx = ldx; a.U = (const unsigned short*)U; a.z = const_cast<float*>(z);
  a.stats = const_cast<float*>(stats); a.dz = dz; a.dx = (unsigned short*)dx; a.lddx = lddx;
  a.B = (int)B; a.L = (int)L; a.D = (int)D; a.H = (int)H;
  unsigned short* UT = (unsigned short*)workspace;
  unsigned short* dzT = UT + D * 16;
  a.UT = UT; a.dzT = dzT; a.part = (float*)(dzT + B * D * 16);
  const size_t nprep = (size_t)(B + 1) * D;
  hipLaunchKernelGGL(mappool_prep_kernel, dim3((unsigned)((nprep + 255) / 256)), dim3(256), 0, st, a, dzT, UT);
  if (int rc = clipa_check_launch("mappool_prep")) return rc;
  if (int rc = mp_launch<true>(a, grid, st, "mappool_bwd")) return rc;
  hipLaunchKernelGGL(mappool_reduce_kernel, dim3((unsigned)((H * D + 255) / 256)), dim3(256), 0, st, a.part, dU, grid, (int)(H * D));
  return clipa_check_launch("mappool_reduce");
}
