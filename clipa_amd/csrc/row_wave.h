// The row-per-wave scheme of the HBM-bound LayerNorm / row-quantise kernels (layernorm.hip, quant.hip) for gfx950: one 64-lane
// wave owns a row, lane l holds the 16-byte chunks l + 64 c (c < NCH) of 8 elements each, and the row stays in registers
// between the reductions and the stores.  One copy of the chunk geometry, the 8-element loads / stores, the LayerNorm
// statistics and affine output, the LayerNorm + quantise row loop, the row-quantise sweep and the host-side dispatch from a
// row width / runtime flags to template arguments.
// NOT shared, on purpose - they add in different orders, and merging them would change bits: the three fixed-order partial
// reducers (colsum_reduce_kernel, ln_bwd_reduce_kernel, misc.hip's colsum_final_kernel) and the two block column-sum epilogues
// (((r0 + r1) + r2) + r3 per chunk in quantize_rows_colsum_kernel, (s0 + s1) + (s2 + s3) in ln_bwd_kernel).
#pragma once
#include <type_traits>
#include "common.h"
#include "stream.h"

namespace {

// ---- geometry: chunk c of the lane is chunk lane + 64 c of the row: in(c) where that lies inside the row, col(c) = its first
// element; each(f) calls f(c, col(c)) for the chunks that are in ----
template <int NCH>
struct RowWave {
  int lane, nchunks;
  bool live = true;      // false: an empty row (ln_fwd_kernel's second row past the end)
  __device__ __forceinline__ RowWave(int width) : lane(threadIdx.x & 63), nchunks(width >> 3) {}
  __device__ __forceinline__ RowWave(const RowWave& w, bool live) : lane(w.lane), nchunks(w.nchunks), live(live) {}
  __device__ __forceinline__ bool in(int c) const { return lane + c * 64 < nchunks && live; }
  __device__ __forceinline__ size_t col(int c) const { return (size_t)(lane + c * 64) * 8; }
  template <class F>
  __device__ __forceinline__ void each(F&& f) const {
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (in(c)) f(c, col(c));
  }
};

// ---- load / store 8 consecutive elements as float ----
// STREAM: the operand is a row stream that the kernel touches once (non-temporal); gamma / beta are not
template <bool F32, bool STREAM = true>
__device__ __forceinline__ void ld8(const void* base, size_t elem, float* f) {
  if (F32) {
    const f32x4* p = (const f32x4*)((const float*)base + elem);
    const f32x4 a = STREAM ? ld_stream<f32x4>(p) : p[0];
    const f32x4 b = STREAM ? ld_stream<f32x4>(p + 1) : p[1];
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  } else {
    const u32x4* p = (const u32x4*)((const unsigned short*)base + elem);
    unpack8(STREAM ? ld_stream<u32x4>(p) : *p, f);
  }
}
template <bool F32>
__device__ __forceinline__ void st8(void* base, size_t elem, const float* f) {
  if (F32) {
    st_stream((float*)base + elem, f32x4{f[0], f[1], f[2], f[3]});
    st_stream((float*)base + elem + 4, f32x4{f[4], f[5], f[6], f[7]});
  } else {
    st_stream((unsigned short*)base + elem, pack8(f));
  }
}
// 8 bf16 of a byte-addressed row stream, still packed
__device__ __forceinline__ u32x4 ld_row8(const char* x, size_t elem) { return ld_stream<u32x4>(x + elem * 2); }

// ---- LayerNorm of a row held in v[NCH][8] ----
// THE bit-exactness contract of the LayerNorm family: ln_fwd_kernel, ln_bwd_kernel (plain, EMIT, QFMT), ln_fwd_q8_kernel and
// ln_fwd_q8s_kernel must agree bit for bit on rstd, y, dx, dgamma, dbeta - a block's gradients may not depend on which of its
// tensors were kept - so all of them take mean, rstd, xhat and y from the functions below and nowhere else.  Every multiply-add
// is WRITTEN as __builtin_fmaf, here and in the kernels' own sums: which products hipcc contracts under -ffp-contract=fast
// depends on use counts that differ between instantiations (and `#pragma clang fp contract(off)` is ignored under that flag).
// What is left to the compiler are single multiplications and additions.  Sums run over c, then i, ascending.
// s = the lane's sum of its chunks' elements: ln_sum8 adds a chunk, ln_row_sum all of them.  ln_q8_rows (below) is the one
// caller that walks the chunks itself, with ln_sum8 between its loads; everybody else calls ln_row_sum.
// ln_stats takes R rows at once (ln_fwd_kernel keeps two per wave): each step runs over all of them before the next one
// starts, so that their wave reductions are independent neighbours and their shuffles interleave.  w, v, s, mean, rstd point
// at R of each.
__device__ __forceinline__ void ln_sum8(const float* v, float& s) {
#pragma unroll
  for (int i = 0; i < 8; ++i) s += v[i];
}
template <int NCH>
__device__ __forceinline__ void ln_row_sum(const RowWave<NCH>& w, const float (&v)[NCH][8], float& s) {
  w.each([&](int c, size_t) { ln_sum8(v[c], s); });
}
template <int R = 1, int NCH>
__device__ __forceinline__ void ln_stats(const RowWave<NCH>* w, const float (*v)[NCH][8], const float* s, float invD, float eps,
                                         float* mean, float* rstd) {
  float ss[R] = {};
#pragma unroll
  for (int k = 0; k < R; ++k) mean[k] = wave_sum(s[k]) * invD;
#pragma unroll
  for (int k = 0; k < R; ++k)
    w[k].each([&](int c, size_t) {
#pragma unroll
      for (int i = 0; i < 8; ++i) { const float d = v[k][c][i] - mean[k]; ss[k] = __builtin_fmaf(d, d, ss[k]); }
    });
#pragma unroll
  for (int k = 0; k < R; ++k) rstd[k] = rsqrtf(__builtin_fmaf(wave_sum(ss[k]), invD, eps));
}
// of one chunk: xhat = (x - mean) * rstd, y = xhat * gamma + beta from xhat (the backward keeps xhat) and y from x
__device__ __forceinline__ void ln_xhat8(const float* v, float mean, float rstd, float* xhat) {
#pragma unroll
  for (int i = 0; i < 8; ++i) xhat[i] = (v[i] - mean) * rstd;
}
__device__ __forceinline__ void ln_affine8(const float* xhat, const float* g, const float* b, float* y) {
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = __builtin_fmaf(xhat[i], g[i], b[i]);
}
__device__ __forceinline__ void ln_y8(const float* v, float mean, float rstd, const float* g, const float* b, float* y) {
  ln_xhat8(v, mean, rstd, y);
  ln_affine8(y, g, b, y);
}

// ---- the row loop of the LayerNorm + quantise kernels (bf16 rows) ----
// gamma / beta in registers, a grid of waves striding the rows, tail(w, r, at, y8) per row r, which starts at element
// `at` = r D; y8(c, o) puts the eight values of LayerNorm(x[r]) of the lane's chunk c into o - fp32, not yet rounded.
// LN_Q8_PREFETCH: the next row's loads are issued before this row's arithmetic (a wave keeps two rows in flight - these
// kernels are latency-bound at one row per wave and ~100 registers, tools/stream8_bench.py).
// The loop walks the chunks itself (in / col, not each) because a chunk outside the row still unpacks its zeros, and adds the
// lane's sum between a chunk's unpack and the load of its successor instead of calling ln_row_sum afterwards: with the load
// alone in its block hipcc issues it ahead of the unpack, into registers of its own, and ln_fwd_q8s_kernel<2> loses 15 %
// (0.436 -> 0.501 ms at 806912 x 1024, profiles/row_wave_refactor_ab.md).
#ifndef LN_Q8_PREFETCH
#define LN_Q8_PREFETCH 1                          // A/B knob (tools/stream8_bench.py --lib)
#endif
template <int NCH, class Tail>
__device__ __forceinline__ void ln_q8_rows(const char* __restrict__ x, const float* __restrict__ gamma,
                                           const float* __restrict__ beta, long rows, int D, float eps, Tail&& tail) {
  const RowWave<NCH> w(D);
  const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long nw = (long)gridDim.x * 4;
  float g[NCH][8] = {}, bt[NCH][8] = {};
  w.each([&](int c, size_t col) { ld8<true, false>(gamma, col, g[c]); ld8<true, false>(beta, col, bt[c]); });
  const float invD = 1.0f / (float)D;
  const size_t step = (size_t)nw * D;
  size_t at = (size_t)wid * D;           // row r starts at element `at`
  u32x4 nxt[NCH] = {};
  if (wid < rows) w.each([&](int c, size_t col) { nxt[c] = ld_row8(x, at + col); });
  for (long r = wid; r < rows; r += nw, at += step) {
    float v[NCH][8], s = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (!LN_Q8_PREFETCH && w.in(c) && r != wid) nxt[c] = ld_row8(x, at + w.col(c));
      unpack8(nxt[c], v[c]);
      if (w.in(c)) {
        ln_sum8(v[c], s);
        if (LN_Q8_PREFETCH && r + nw < rows) nxt[c] = ld_row8(x, at + step + w.col(c));
      }
    }
    float mean, rstd;
    ln_stats(&w, &v, &s, invD, eps, &mean, &rstd);
    tail(w, r, at, [&](int c, float* y) { ln_y8(v[c], mean, rstd, g[c], bt[c], y); });
  }
}

// ---- row-scaled fp8 quantisation: FMT 0 = OCP e4m3 (max 448), 1 = e5m2 (max 57344) ----
template <int FMT>
__device__ __forceinline__ u32x2 cvt8(const float* f, float s) {
  int w0 = 0, w1 = 0;
  if (FMT == 0) {
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0] * s, f[1] * s, w0, false);
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2] * s, f[3] * s, w0, true);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4] * s, f[5] * s, w1, false);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6] * s, f[7] * s, w1, true);
  } else {
    w0 = __builtin_amdgcn_cvt_pk_bf8_f32(f[0] * s, f[1] * s, w0, false);
    w0 = __builtin_amdgcn_cvt_pk_bf8_f32(f[2] * s, f[3] * s, w0, true);
    w1 = __builtin_amdgcn_cvt_pk_bf8_f32(f[4] * s, f[5] * s, w1, false);
    w1 = __builtin_amdgcn_cvt_pk_bf8_f32(f[6] * s, f[7] * s, w1, true);
  }
  u32x2 r;
  r[0] = (unsigned)w0;
  r[1] = (unsigned)w1;
  return r;
}
template <int FMT>
__device__ __forceinline__ void row_scales(float amax, float& s, float& dq) {
  const float FMAX = FMT == 0 ? 448.0f : 57344.0f;
  s = amax > 0.f ? FMAX / amax : 1.0f;
  // an all-zero row (padding tokens): zero bytes, zero scale - the fp8 weight gradient's tensor scale is a maximum over these
  dq = amax > 0.f ? amax / FMAX : 0.0f;
}
// a chunk of the row to quantise is held as 8 packed bf16 or as the 8 floats they unpack to
__device__ __forceinline__ void chunk8(const u32x4& v, float* f) { unpack8(v, f); }
__device__ __forceinline__ void chunk8(const float (&v)[8], float* f) {
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = v[i];
}
// a lane's share of max|v| and sum v^2, gathered (c, then i, ascending) where the kernel has each chunk's values in hand
struct RowMag {
  float amax = 0.f, ssq = 0.f;
  __device__ __forceinline__ void add8(const float* f) {
#pragma unroll
    for (int i = 0; i < 8; ++i) { amax = fmaxf(amax, fabsf(f[i])); ssq = __builtin_fmaf(f[i], f[i], ssq); }
  }
};
// The sweep: q[row] = fp8(v * s) with s = FMAX / max|v|, dq[row] = 1 / s, and - where rnorm is given - rnorm[row] = ||v||_2
// (engine._row_bound: a Cauchy-Schwarz bound of what the next layer makes of this row).  One copy, so that the stand-alone
// quantisers and the kernels that quantise a row they produced (ln_fwd_q8_kernel, ln_bwd_kernel<., QFMT>) write the same bytes.
template <int FMT, int NCH, class Chunk>
__device__ __forceinline__ void quantize_row(const RowWave<NCH>& w, const Chunk (&v)[NCH], RowMag m, char* __restrict__ qrow,
                                             float* __restrict__ dq, float* __restrict__ rnorm, long row) {
  float s, d;
  row_scales<FMT>(wave_max(m.amax), s, d);
  if (w.lane == 0) dq[row] = d;
  if (rnorm) {
    const float n2 = wave_sum(m.ssq);
    if (w.lane == 0) rnorm[row] = sqrtf(n2);
  }
  w.each([&](int c, size_t col) {
    float f[8];
    chunk8(v[c], f);
    st_stream(qrow + col, cvt8<FMT>(f, s));
  });
}

// ---- host: runtime row width / flags -> template arguments ----
// f(integral_constant<int, N>) for the first N of the list with width <= 512 N (the last one takes what is left): a call site
// instantiates exactly the chunk counts it names
template <int N, int... REST, class F>
void dispatch_nch(long width, F&& f) {
  if constexpr (sizeof...(REST) > 0) {
    if (width > 512L * N) return dispatch_nch<REST...>(width, f);
  }
  f(std::integral_constant<int, N>{});
}
// f(bool_constant...) for the runtime flags: a call site instantiates the 2^n combinations of the flags it passes and no other
template <class F>
void dispatch_flags(F&& f) { f(); }
template <class F, class... R>
void dispatch_flags(F&& f, bool flag, R... rest) {
  if (flag) dispatch_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else dispatch_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

}  // namespace
