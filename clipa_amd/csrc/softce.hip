// Fused soft-target cross-entropy for gfx950: loss, log-sum-exp and the logit gradient of a classifier row in one pass.
//
// Replaces softmax_xent (clipa_jax/losses/common.py:104-109) on the mixed, smoothed labels of MixupAndCutmix
// (clipa_jax/transforms/mixup.py:203-211 with MixupAndCutmix.label_smoothing) without the [B, C] target matrix: the targets stay
// compact - ya, optional yb with lam, a scalar smoothing eps -
//     t_c = (1 - eps) (lam [c = ya] + (1 - lam) [c = yb]) + eps / C          (ya == yb: the two terms add; no yb: lam = 1)
// logits z fp32 [B, ld] with C <= ld real columns; columns >= C are padding and are NEVER read (NaN there is harmless).
//     lse_i   = m + log sum_c exp(z_c - m),  m = max_c z_c
//     loss_i  = lse_i - sum_c t_c z_c = log sum_c exp(z_c - m) - sum_c t_c (z_c - m)          (sum_c t_c = 1: the second form is
//               the one computed - |z| near 100 cancels inside z_c - m, not in the loss)
//     dlogits = g (softmax(z) - t) in bf16 [B, ldd], pad columns written as zero          (g: a scalar, 1 / B for the mean)
// One 64-lane wave per row, the row_wave.h scheme on 16-byte chunks of 4 floats: lane l owns chunks l + 64 j.  Up to 4096
// columns the row stays in registers between the sweeps (NCH = 4 or 16 chunks per lane); a longer row (up to 32768, ImageNet-21k)
// is re-read from cache for the second and third sweep.  The sweeps: the maximum; sum exp(z - m) and sum (z - m); the write.
// THE order of every sum, the same for every NCH: a lane adds its elements in ascending column order, then the xor butterfly of
// wave_sum (offsets 32, 16, ..., 1).  t_c = base + [c = ya] wa + [c = yb] wb with base = eps / C, wa = (1 - eps) lam,
// wb = (1 - eps) (1 - lam), added in that order.  A row's result depends on nothing but the row: no float atomics, and every
// output is bit-identical whatever the grid.  The scalar mean is the caller's fixed-order reduction of the row losses.
// A label outside [0, C), or lam outside [0, 1] or NaN, is counted in err_count and never used as an index: that row's loss and
// lse come out NaN and its gradient row zero.
#include "common.h"
#include "clipa_hip.h"

namespace {

constexpr int SCE_MAX_C = 32768;

// 4 floats at columns col .. col + 3 of a row; columns >= C are not read and come back as `fill`
__device__ __forceinline__ void sce_load4(const float* __restrict__ z, int col, int C, float fill, float* v) {
  if (col + 4 <= C) {
    const f32x4 t = *(const f32x4*)(z + col);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = col + i < C ? z[col + i] : fill;
  }
}

// f(col, v[4]) over the lane's chunks in ascending order; NCH > 0: the row in registers, NCH == 0: re-read
template <int NCH, class F>
__device__ __forceinline__ void sce_each(const float* __restrict__ z, int C, int lane, const float (*reg)[4], F&& f) {
  if constexpr (NCH > 0) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const int col = (lane + 64 * j) * 4;
      if (col < C) f(col, reg[j]);
    }
  } else {
    for (int col = lane * 4; col < C; col += 256) {
      float v[4];
      sce_load4(z, col, C, 0.f, v);
      f(col, v);
    }
  }
}

template <int NCH>
__global__ __launch_bounds__(256) void softce_kernel(const float* __restrict__ logits, int B, int C, long ld,
                                                     const int* __restrict__ ya, const int* __restrict__ yb,
                                                     const float* __restrict__ lam, float eps, float g,
                                                     float* __restrict__ loss, float* __restrict__ lse,
                                                     unsigned short* __restrict__ dl, long ldd, int* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const float ninf = -__builtin_huge_valf();
  const float base = eps / (float)C;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < B; r += (long)gridDim.x * 4) {
    const float* z = logits + r * ld;
    const int a = ya[r], b = yb ? yb[r] : a;
    const float l = (yb && lam) ? lam[r] : 1.0f;
    const bool bad = (unsigned)a >= (unsigned)C || (unsigned)b >= (unsigned)C || !(l >= 0.f && l <= 1.f);
    unsigned short* drow = dl ? dl + r * ldd : nullptr;
    if (bad) {
      if (lane == 0) {
        if (err) atomicAdd(err, 1);
        loss[r] = __builtin_nanf("");
        lse[r] = __builtin_nanf("");
      }
      if (drow)
        for (long col = lane * 4; col < ldd; col += 256) *(u32x2*)(drow + col) = u32x2{0u, 0u};
      continue;
    }
    float reg[NCH > 0 ? NCH : 1][4];
    if constexpr (NCH > 0) {
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const int col = (lane + 64 * j) * 4;
        if (col < C) sce_load4(z, col, C, 0.f, reg[j]);
      }
    }
    // sweep 1: the maximum
    float m = ninf;
    sce_each<NCH>(z, C, lane, reg, [&](int col, const float* v) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (col + i < C) m = fmaxf(m, v[i]);
    });
    m = wave_max(m);
    // sweep 2: sum exp(z - m) and sum (z - m)
    float s = 0.f, q = 0.f;
    sce_each<NCH>(z, C, lane, reg, [&](int col, const float* v) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (col + i < C) { const float d = v[i] - m; s += expf(d); q += d; }
    });
    s = wave_sum(s);
    q = wave_sum(q);
    const float wa = (1.0f - eps) * l, wb = (1.0f - eps) * (1.0f - l);
    const float logs = logf(s);
    if (lane == 0) {
      const float tz = wa * (z[a] - m) + wb * (z[b] - m) + base * q;
      loss[r] = logs - tz;
      lse[r] = m + logs;
    }
    if (!drow) continue;
    // sweep 3: g (softmax - t) as bf16, then the zero padding
    const float inv = 1.0f / s;
    sce_each<NCH>(z, C, lane, reg, [&](int col, const float* v) {
      float d[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = col + i;
        float t = base;
        if (c == a) t += wa;
        if (c == b) t += wb;
        d[i] = c < C ? g * (expf(v[i] - m) * inv - t) : 0.f;
      }
      *(u32x2*)(drow + col) = u32x2{pack2bf(d[0], d[1]), pack2bf(d[2], d[3])};
    });
    for (long col = ((long)(C + 3) / 4 + lane) * 4; col < ldd; col += 256) *(u32x2*)(drow + col) = u32x2{0u, 0u};
  }
}

}  // namespace

extern "C" int clipa_softce(const float* logits, int64_t B, int64_t C, int64_t ld, const int32_t* ya, const int32_t* yb,
                            const float* lam, float smoothing, float gscale, float* loss, float* lse, void* dlogits,
                            int64_t ldd, int64_t max_workgroups, int32_t* err_count, void* stream) {
  if (B <= 0) return CLIPA_OK;
  if (C < 2 || C > SCE_MAX_C) { clipa_set_error("softce: C = %ld classes out of range (2..%d)", (long)C, SCE_MAX_C); return CLIPA_ERR_ARG; }
  if (B >= (1L << 31)) { clipa_set_error("softce: B = %ld rows are too many for one launch", (long)B); return CLIPA_ERR_ARG; }
  if (ld < C || ld % 4) { clipa_set_error("softce: ld = %ld must be >= C = %ld and a multiple of 4", (long)ld, (long)C); return CLIPA_ERR_ARG; }
  if (!(smoothing >= 0.f && smoothing <= 1.f)) { clipa_set_error("softce: smoothing = %g outside [0, 1]", (double)smoothing); return CLIPA_ERR_ARG; }
  if (max_workgroups < 0) { clipa_set_error("softce: max_workgroups = %ld must be >= 0", (long)max_workgroups); return CLIPA_ERR_ARG; }
  if (yb && !lam) { clipa_set_error("softce: yb comes with lam"); return CLIPA_ERR_ARG; }
  if (int rc = clipa_check_ptrs16("softce", {logits, ya, loss, lse})) return rc;
  if (dlogits) {
    if (ldd < C || ldd % 8) { clipa_set_error("softce: ldd = %ld must be >= C = %ld and a multiple of 8", (long)ldd, (long)C); return CLIPA_ERR_ARG; }
    if (int rc = clipa_check_ptrs16("softce (dlogits)", {dlogits})) return rc;
  }
  int64_t grid = (B + 3) / 4;
  if (max_workgroups && grid > max_workgroups) grid = max_workgroups;
  if (grid > 0x7fffffffL) grid = 0x7fffffffL;
  hipStream_t st = (hipStream_t)stream;
  unsigned short* dl = (unsigned short*)dlogits;
#define SCE_LAUNCH(N)                                                                                                          \
  hipLaunchKernelGGL(softce_kernel<N>, dim3((unsigned)grid), dim3(256), 0, st, logits, (int)B, (int)C, (long)ld, ya, yb, lam, \
                     smoothing, gscale, loss, lse, dl, (long)ldd, err_count)
  if (C <= 1024) SCE_LAUNCH(4);
  else if (C <= 4096) SCE_LAUNCH(16);
  else SCE_LAUNCH(0);
#undef SCE_LAUNCH
  return clipa_check_launch("softce");
}
