// Batch Mixup / CutMix on the uint8 image batch for gfx950, IN PLACE, after the device augmentation (augment.hip).
//
// Replaces the image half of MixupAndCutmix of the JAX tree (clipa_jax/transforms/mixup.py:141-201; the box of _fill_rectangle,
// transforms/random_erasing.py:25-61): sample b is mixed with its mirror B-1-b (tf.reverse(images, [0]), mixup.py:179,199).
// The label half is the soft target of softce.hip.  lam and the boxes are sampled on the host (clipa_amd/finetune.py:
// sample_mixcut) - a few bytes per sample, like crop boxes and jitter factors.
//
// img is [B,3,S,S] uint8 in NCHW or channels_last memory: either way image b is the n = 3 S S contiguous bytes at b n.
//   mixup   out_b = lam_b x_b + (1 - lam_b) x_{B-1-b}; output b uses lam_b and output B-1-b uses lam_{B-1-b} (mixup.py:189-201).
//           THE uint8 arithmetic, per byte a of x_b and b' of x_{B-1-b}, in fp32 with no contraction:
//               d = a - b';  t = lam * d;  v = t + b';  out = (uint8)(int)(v + 0.5f)
//           (a - b' and every intermediate are exact or rounded once; for lam in [0, 1] v stays inside [min(a, b'), max(a, b')],
//           so nothing is clamped; lam = 1 gives a, lam = 0 gives b').  A numpy float32 restatement reproduces it bit for bit.
//   cutmix  inside box_b = (y0, y1, x0, x1), half-open, out_b = x_{B-1-b}; outside it out_b = x_b.  A pure copy.
// One thread owns the same 16 bytes of both images of a pair: it reads both, then writes both, so the exchange is safe in place
// (2 reads + 2 writes per byte pair, and none at all where a cutmix chunk lies outside both boxes, or where both lam are 1).
// With odd B the middle sample pairs with itself and is never touched.  The image's n % 16 last bytes are a scalar tail of one
// thread.  The 16-byte accesses are declared unaligned (n = 972 at S = 18 puts image 1 at byte 972): gfx950 global accesses take
// any alignment, and at the production sizes (n % 16 == 0) they are aligned.  HBM-bound byte work, no LDS.
// Descriptors are validated before anything is written: lam outside [0, 1] or NaN (mixup), a box outside the image or with
// y0 > y1 or x0 > x1 (cutmix) - a pair with a bad descriptor is left as it was and counted in err_count.
#include "common.h"
#include "clipa_hip.h"

namespace {

typedef u32x4 u32x4_u __attribute__((aligned(1)));      // 16 bytes at any address

// mixup.py:199 on one byte pair.  The product must be rounded before the sum: the library is built with -ffp-contract=fast,
// under which the backend fuses a multiply into a dependent add whatever the pragma says, so the product additionally passes
// through an empty asm that the optimiser cannot see through (no instruction is emitted for it).
#pragma clang fp contract(off)
__device__ __forceinline__ unsigned mix_byte(unsigned a, unsigned b, float lam) {
  const float fb = (float)b;
  const float d = (float)a - fb;
  float t = lam * d;
  asm("" : "+v"(t));
  const float v = t + fb;
  return (unsigned)(int)(v + 0.5f);
}
// four byte pairs of a word: -> lam_a a + (1 - lam_a) b and lam_b b + (1 - lam_b) a
__device__ __forceinline__ void mix_word(unsigned a, unsigned b, float lam_a, float lam_b, unsigned& oa, unsigned& ob) {
  oa = 0; ob = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned x = (a >> (8 * j)) & 0xffu, y = (b >> (8 * j)) & 0xffu;
    oa |= mix_byte(x, y, lam_a) << (8 * j);
    ob |= mix_byte(y, x, lam_b) << (8 * j);
  }
}

struct Box { int y0, y1, x0, x1; };
__device__ __forceinline__ bool box_ok(const Box& b, int S) {
  return b.y0 >= 0 && b.y0 <= b.y1 && b.y1 <= S && b.x0 >= 0 && b.x0 <= b.x1 && b.x1 <= S;
}
__device__ __forceinline__ bool box_empty(const Box& b) { return b.y0 == b.y1 || b.x0 == b.x1; }

// The pixel (y, x) of byte i of an image, walked byte by byte: NCHW i = (c S + y) S + x, channels_last i = (y S + x) 3 + c
template <bool NHWC>
struct PixelWalk {
  int y, x, c, S;
  __device__ __forceinline__ PixelWalk(unsigned i, int S) : S(S) {
    if (NHWC) {
      const unsigned pix = i / 3u;
      c = (int)(i - pix * 3u);
      y = (int)(pix / (unsigned)S);
      x = (int)(pix - (unsigned)y * (unsigned)S);
    } else {
      const unsigned row = i / (unsigned)S;       // c S + y
      c = 0;
      x = (int)(i - row * (unsigned)S);
      y = (int)(row % (unsigned)S);
    }
  }
  __device__ __forceinline__ void next() {
    if (NHWC && ++c < 3) return;
    c = 0;
    if (++x == S) { x = 0; if (++y == S) y = 0; }
  }
  __device__ __forceinline__ bool in(const Box& b) const { return y >= b.y0 && y < b.y1 && x >= b.x0 && x < b.x1; }
};

// blockIdx.y = pair p: samples p and B-1-p.  blockIdx.x * 256 + threadIdx.x = 16-byte chunk k of the image; k == n / 16 is the
// scalar tail.  MODE 0 mixup, 1 cutmix.
template <int MODE, bool NHWC>
__global__ __launch_bounds__(256) void mixcut_kernel(unsigned char* __restrict__ img, const float* __restrict__ lam,
                                                     const int* __restrict__ box, int B, int S, unsigned n,
                                                     int* __restrict__ err) {
  const int p = blockIdx.y, q = B - 1 - p;
  float la = 1.f, lb = 1.f;
  Box ba = {0, 0, 0, 0}, bb = {0, 0, 0, 0};
  int bad = 0;
  if (MODE == 0) {
    la = lam[p]; lb = lam[q];
    bad = !(la >= 0.f && la <= 1.f) + (p != q && !(lb >= 0.f && lb <= 1.f));
  } else {
    ba = {box[p * 4], box[p * 4 + 1], box[p * 4 + 2], box[p * 4 + 3]};
    bb = {box[q * 4], box[q * 4 + 1], box[q * 4 + 2], box[q * 4 + 3]};
    bad = !box_ok(ba, S) + (p != q && !box_ok(bb, S));
  }
  if (bad) {                                   // the whole pair stays as it was
    if (err && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(err, bad);
    return;
  }
  if (p == q) return;                          // odd B: the middle sample is its own mirror
  if (MODE == 0 ? (la == 1.f && lb == 1.f) : (box_empty(ba) && box_empty(bb))) return;
  const unsigned k = blockIdx.x * 256u + threadIdx.x, full = n >> 4;
  if (k > full || (k == full && (n & 15u) == 0)) return;
  unsigned char* pa = img + (size_t)p * n + (size_t)k * 16;
  unsigned char* pb = img + (size_t)q * n + (size_t)k * 16;
  if (k < full) {
    u32x4 ma = {0, 0, 0, 0}, mb = {0, 0, 0, 0};       // cutmix: byte masks "takes the other image's byte"
    if (MODE == 1) {
      PixelWalk<NHWC> w(k * 16u, S);
      unsigned any = 0;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const unsigned bit = 0xffu << (8 * (j & 3));
        if (w.in(ba)) ma[j >> 2] |= bit;
        if (w.in(bb)) mb[j >> 2] |= bit;
        w.next();
      }
      any = ma[0] | ma[1] | ma[2] | ma[3] | mb[0] | mb[1] | mb[2] | mb[3];
      if (!any) return;                        // outside both boxes: nothing moves
    }
    const u32x4 a = *(const u32x4_u*)pa, b = *(const u32x4_u*)pb;
    u32x4 oa, ob;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (MODE == 0) {
        unsigned ra, rb;
        mix_word(a[j], b[j], la, lb, ra, rb);
        oa[j] = ra; ob[j] = rb;
      } else {
        oa[j] = (a[j] & ~ma[j]) | (b[j] & ma[j]);
        ob[j] = (b[j] & ~mb[j]) | (a[j] & mb[j]);
      }
    }
    *(u32x4_u*)pa = oa;
    *(u32x4_u*)pb = ob;
  } else {                                     // the n % 16 last bytes
    PixelWalk<NHWC> w(k * 16u, S);
    const int rest = (int)(n & 15u);
    for (int j = 0; j < rest; ++j) {
      const unsigned a = pa[j], b = pb[j];
      if (MODE == 0) {
        pa[j] = (unsigned char)mix_byte(a, b, la);
        pb[j] = (unsigned char)mix_byte(b, a, lb);
      } else {
        if (w.in(ba)) pa[j] = (unsigned char)b;
        if (w.in(bb)) pb[j] = (unsigned char)a;
        w.next();
      }
    }
  }
}

}  // namespace

extern "C" int clipa_mixcut_u8(void* img, const float* lam, const int32_t* box, int64_t B, int64_t S, int nhwc, int mode,
                               int32_t* err_count, void* stream) {
  if (B <= 0) return CLIPA_OK;
  if (S <= 0 || S > 4096) { clipa_set_error("mixcut_u8: S = %ld out of range (1..4096)", (long)S); return CLIPA_ERR_ARG; }
  if (mode != 0 && mode != 1) { clipa_set_error("mixcut_u8: mode = %d (0 mixup, 1 cutmix)", mode); return CLIPA_ERR_ARG; }
  if (!img || (mode == 0 && !lam) || (mode == 1 && !box)) {
    clipa_set_error("mixcut_u8: null image, or no %s for mode %d", mode == 0 ? "lam" : "box", mode);
    return CLIPA_ERR_ARG;
  }
  const int64_t pairs = (B + 1) / 2;
  if (pairs > 65535) { clipa_set_error("mixcut_u8: B = %ld, at most 131070 samples per call", (long)B); return CLIPA_ERR_ARG; }
  const unsigned n = (unsigned)(3 * S * S);
  const unsigned chunks = (n >> 4) + ((n & 15u) ? 1u : 0u);
  const dim3 grid((chunks + 255u) / 256u, (unsigned)pairs), block(256);
  hipStream_t st = (hipStream_t)stream;
  unsigned char* p = (unsigned char*)img;
  if (mode == 0) hipLaunchKernelGGL((mixcut_kernel<0, false>), grid, block, 0, st, p, lam, box, (int)B, (int)S, n, err_count);
  else if (nhwc) hipLaunchKernelGGL((mixcut_kernel<1, true>), grid, block, 0, st, p, lam, box, (int)B, (int)S, n, err_count);
  else hipLaunchKernelGGL((mixcut_kernel<1, false>), grid, block, 0, st, p, lam, box, (int)B, (int)S, n, err_count);
  return clipa_check_launch("mixcut_u8");
}
