// Device-side image resampling of a RAGGED batch for gfx950: every sample has its own source size, crop box, resize target
// and S x S output window.
//
//   out[b][y][x] = resize(crop(img_b, box_b), (out_h_b, out_w_b), filter)[oy_b + y][ox_b + x],   0 <= y, x < S
//
// One definition for the three geometries of the reference's transforms (clipa_torch/open_clip/transform.py):
//   train  RandomResizedCrop(S, BICUBIC)              :152-157  box sampled per image, (out_h, out_w) = (S, S), window (0, 0)
//   eval   Resize(S, interpolation) + CenterCrop(S)   :197-201  whole image, short side S, window centred
//   eval   Resize((S, S)) with --square-resize-only   :191-196  whole image, (S, S), window (0, 0)
// (--interpolation bicubic | bilinear and --square-resize-only of training/params.py:445-454).  After Resize(S) the long side is
// >= S, so CenterCrop's zero-padding branch never occurs and the window always lies inside the resized image; a window that
// does not is a rejected sample, not padding.
// `resize` is Pillow's ImagingResample for 8-bit channels, bit for bit, as in augment.hip: coefficient windows normalised in
// double and rounded to 22-bit fixed point, a horizontal pass into a uint8 intermediate, a vertical pass, out =
// clip8((2^21 + sum p * k) >> 22).  A pass at scale 1 has the single coefficient 2^22 and returns its input, which is what
// Pillow's skipping of that pass gives.  Only the window is computed: S columns in the horizontal pass, and of the box's
// rows only those that the window's vertical taps read.
// Storage is ragged as well: sample b's intermediate rows and its two coefficient tables live at offsets of the workspace that
// the host derives from the size table (the descriptor below), so one large photograph costs its own rows only.
// The descriptors are not trusted: rr_validate_kernel checks each one against the packed buffer and the workspace before any
// other kernel dereferences it, and writes a plan the later kernels read; a failing sample is counted in err_count and comes
// back as zeros, the rest of the batch is untouched by it.
// HBM-bound byte work: one thread per output pixel, neighbouring threads read neighbouring source pixels; blockIdx.y is the
// sample and blockIdx.x is sized by the largest sample (surplus blocks return at once).
#include "common.h"
#include "clipa_hip.h"

namespace {

constexpr int RR_PREC = 22;              // Resample.c PRECISION_BITS for 8-bit channels
constexpr int RR_DESC = 16;              // int64 words per sample descriptor
constexpr int RR_MAX_SIDE = 16384;
constexpr int RR_MAX_DOWN = 64;          // down-scale per axis: 2 * ceil(2 * 64) + 1 = 257 bicubic taps
// descriptor words
enum { D_OFF, D_H, D_W, D_TOP, D_LEFT, D_BH, D_BW, D_OH, D_OW, D_OY, D_OX, D_TMP, D_COEF, D_KH, D_KV, D_ROWS };
// plan words (int32, written by rr_validate_kernel): ok, first box row the window's vertical taps read, number of such rows
constexpr int RR_PLAN = 4;

// Pillow's filters and coefficient code in the same double operations, in the same order: no FMA contraction here
#pragma clang fp contract(off)
__device__ double rr_filter(double x, int filter) {
  if (x < 0.0) x = -x;
  if (filter == 1) return x < 1.0 ? 1.0 - x : 0.0;            // bilinear_filter (triangle)
  const double a = -0.5;                                      // bicubic_filter
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

struct RRWindow { double scale, support, ss, center; int ksize, xmin, n; };

// precompute_coeffs for output coordinate o of a resize in_size -> out_size (box offset 0: the crop is its own image)
__device__ RRWindow rr_window(int in_size, int out_size, int o, int filter) {
#pragma clang fp contract(off)
  RRWindow w;
  w.scale = (double)(float)in_size / out_size;
  const double filterscale = w.scale < 1.0 ? 1.0 : w.scale;
  w.support = (filter == 1 ? 1.0 : 2.0) * filterscale;
  w.ksize = (int)ceil(w.support) * 2 + 1;
  w.ss = 1.0 / filterscale;
  w.center = 0.0 + (o + 0.5) * w.scale;
  int xmin = (int)(w.center - w.support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(w.center + w.support + 0.5);
  if (xmax > in_size) xmax = in_size;
  w.xmin = xmin;
  w.n = xmax - xmin;
  return w;
}

// thread = sample: every check that keeps the later kernels inside [packed, packed + packed_bytes) and inside the workspace
__global__ void rr_validate_kernel(const long* __restrict__ desc, int* __restrict__ plan, int B, int S, int filter,
                                   long packed_bytes, long tmp_bytes, long coef_ints, int max_rows, int* __restrict__ err) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const long* d = desc + (long)b * RR_DESC;
  const long off = d[D_OFF], H = d[D_H], W = d[D_W], top = d[D_TOP], left = d[D_LEFT], bh = d[D_BH], bw = d[D_BW];
  const long oh = d[D_OH], ow = d[D_OW], oy = d[D_OY], ox = d[D_OX], tmp = d[D_TMP], coef = d[D_COEF], kh = d[D_KH], kv = d[D_KV];
  const long rows = d[D_ROWS];
  bool ok = H > 0 && W > 0 && H <= RR_MAX_SIDE && W <= RR_MAX_SIDE && off >= 0 && off <= packed_bytes &&
            H * W * 3 <= packed_bytes - off;                                        // the image inside the packed buffer
  ok = ok && top >= 0 && left >= 0 && bh > 0 && bw > 0 && bh <= H - top && bw <= W - left;      // the box inside the image
  ok = ok && oh > 0 && ow > 0 && oh <= RR_MAX_SIDE && ow <= RR_MAX_SIDE && oy >= 0 && ox >= 0 && S <= oh - oy && S <= ow - ox;
  ok = ok && bh <= oh * RR_MAX_DOWN && bw <= ow * RR_MAX_DOWN;
  int row0 = 0, nrows = 0;
  if (ok) {
    const RRWindow wh = rr_window((int)bw, (int)ow, (int)ox, filter), wv = rr_window((int)bh, (int)oh, (int)oy, filter);
    const RRWindow wl = rr_window((int)bh, (int)oh, (int)oy + S - 1, filter);
    row0 = wv.xmin;
    nrows = wl.xmin + wl.n - row0;                                                  // windows move monotonically with the coordinate
    ok = kh >= wh.ksize && kv >= wv.ksize && kh <= 4 * RR_MAX_DOWN + 1 && kv <= 4 * RR_MAX_DOWN + 1;  // taps within the tables
    ok = ok && coef >= 0 && coef <= coef_ints && (long)S * (kh + kv) <= coef_ints - coef;
    ok = ok && nrows > 0 && nrows <= rows && rows <= max_rows && tmp >= 0 && tmp <= tmp_bytes && rows * S * 3 <= tmp_bytes - tmp;
  }
  int* p = plan + (long)b * RR_PLAN;
  p[0] = ok ? 1 : 0; p[1] = row0; p[2] = ok ? nrows : 0; p[3] = 0;
  if (!ok && err) atomicAdd(err, 1);              // reported to the host; the sample's output is zeros
}

// thread = (sample blockIdx.y, axis, window coordinate j); axis 0 = horizontal (source extent = box width), 1 = vertical
__global__ void rr_coeffs_kernel(const long* __restrict__ desc, const int* __restrict__ plan, int* __restrict__ bounds,
                                 int* __restrict__ coef, int S, int filter) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * S) return;
  const int axis = t >= S ? 1 : 0, j = t - axis * S;
  int* bo = bounds + ((long)b * 2 * S + t) * 2;
  if (!plan[(long)b * RR_PLAN]) { bo[0] = 0; bo[1] = 0; return; }
  const long* d = desc + (long)b * RR_DESC;
  const int in_size = (int)(axis ? d[D_BH] : d[D_BW]), out_size = (int)(axis ? d[D_OH] : d[D_OW]);
  const int kstride = (int)(axis ? d[D_KV] : d[D_KH]);
  const RRWindow w = rr_window(in_size, out_size, (int)(axis ? d[D_OY] : d[D_OX]) + j, filter);
  int* ko = coef + d[D_COEF] + (axis ? (long)S * d[D_KH] : 0) + (long)j * kstride;
  const int n = w.n < kstride ? w.n : kstride;                // n <= ksize <= kstride by construction; never write past the row
  // the weights are evaluated twice (sum, then normalise) instead of being kept: the same operands give the same doubles,
  // and 257 of them per thread would live in scratch memory
  double ww = 0.0;
  for (int x = 0; x < n; ++x) ww += rr_filter((x + w.xmin - w.center + 0.5) * w.ss, filter);
  for (int x = 0; x < n; ++x) {
    double k = rr_filter((x + w.xmin - w.center + 0.5) * w.ss, filter);
    if (ww != 0.0) k /= ww;
    ko[x] = k < 0 ? (int)(-0.5 + k * (1 << RR_PREC)) : (int)(0.5 + k * (1 << RR_PREC));
  }
  bo[0] = w.xmin;
  bo[1] = n;
}

__device__ __forceinline__ unsigned char rr_clip8(int v) {
  v >>= RR_PREC;
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// horizontal pass: tmp_b[r][j][c], r < nrows (the box rows row0 .. row0 + nrows); thread = (sample blockIdx.y, r, j)
__global__ void rr_horizontal_kernel(const unsigned char* __restrict__ packed, const long* __restrict__ desc,
                                     const int* __restrict__ plan, const int* __restrict__ bounds, const int* __restrict__ coef,
                                     unsigned char* __restrict__ tmp, int S) {
  const int b = blockIdx.y;
  const int* pl = plan + (long)b * RR_PLAN;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (!pl[0] || t >= (long)pl[2] * S) return;
  const int j = (int)(t % S), r = (int)(t / S);
  const long* d = desc + (long)b * RR_DESC;
  const int* bo = bounds + ((long)b * 2 * S + j) * 2;
  const int xmin = bo[0], n = bo[1];
  const int* k = coef + d[D_COEF] + (long)j * d[D_KH];
  const unsigned char* p = packed + d[D_OFF] + ((d[D_TOP] + pl[1] + r) * d[D_W] + d[D_LEFT] + xmin) * 3;
  int s0 = 1 << (RR_PREC - 1), s1 = s0, s2 = s0;
  for (int x = 0; x < n; ++x) {
    const int kx = k[x];
    s0 += p[3 * x + 0] * kx;
    s1 += p[3 * x + 1] * kx;
    s2 += p[3 * x + 2] * kx;
  }
  unsigned char* o = tmp + d[D_TMP] + t * 3;
  o[0] = rr_clip8(s0); o[1] = rr_clip8(s1); o[2] = rr_clip8(s2);
}

// vertical pass (+ optional rgb2l grayscale of flagged samples): out[b][y][x][c]; thread = (sample blockIdx.y, y, x)
__global__ void rr_vertical_kernel(const unsigned char* __restrict__ tmp, const long* __restrict__ desc,
                                   const int* __restrict__ plan, const int* __restrict__ bounds, const int* __restrict__ coef,
                                   const unsigned char* __restrict__ gray, unsigned char* __restrict__ out, int S) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= S * S) return;
  unsigned char* o = out + ((long)b * S * S + t) * 3;
  const int* pl = plan + (long)b * RR_PLAN;
  if (!pl[0]) { o[0] = o[1] = o[2] = 0; return; }          // rejected sample: zeros, error counted
  const int xx = t % S, yy = t / S;
  const long* d = desc + (long)b * RR_DESC;
  const int* bo = bounds + ((long)b * 2 * S + S + yy) * 2;
  const int ymin = bo[0] - pl[1], n = bo[1];
  const int* k = coef + d[D_COEF] + (long)S * d[D_KH] + (long)yy * d[D_KV];
  unsigned char c0 = 0, c1 = 0, c2 = 0;
  if (ymin >= 0 && ymin + n <= pl[2]) {                    // always true for a plan rr_validate_kernel accepted
    const unsigned char* p = tmp + d[D_TMP] + ((long)ymin * S + xx) * 3;
    int s0 = 1 << (RR_PREC - 1), s1 = s0, s2 = s0;
    for (int y = 0; y < n; ++y) {
      const int ky = k[y];
      const unsigned char* q = p + (long)y * S * 3;
      s0 += q[0] * ky;
      s1 += q[1] * ky;
      s2 += q[2] * ky;
    }
    c0 = rr_clip8(s0); c1 = rr_clip8(s1); c2 = rr_clip8(s2);
  }
  if (gray && gray[b]) {                                   // Pillow Convert.c rgb2l, replicated (Grayscale(num_output_channels=3))
    const unsigned char l = (unsigned char)((c0 * 19595 + c1 * 38470 + c2 * 7471 + 0x8000) >> 16);
    c0 = c1 = c2 = l;
  }
  o[0] = c0; o[1] = c1; o[2] = c2;
}

inline int64_t rr_align(int64_t v) { return (v + 255) / 256 * 256; }

}  // namespace

// workspace = [intermediate rows: tmp_bytes][plan: B x 4 int32][bounds: B x 2 x S x 2 int32][coefficients: coef_ints int32]
extern "C" int64_t clipa_resample_ragged_workspace(int64_t B, int64_t S, int64_t tmp_bytes, int64_t coef_ints) {
  if (B < 0 || S < 0 || tmp_bytes < 0 || coef_ints < 0) return 0;
  return rr_align(tmp_bytes) + rr_align(B * RR_PLAN * 4) + rr_align(B * 2 * S * 2 * 4) + coef_ints * 4;
}

extern "C" int clipa_resample_ragged_u8(const void* packed, int64_t packed_bytes, const int64_t* desc, const uint8_t* gray_flags,
                                        void* out, int64_t B, int64_t S, int filter, int64_t max_rows, int64_t tmp_bytes,
                                        int64_t coef_ints, void* workspace, int64_t workspace_bytes, int32_t* err_count,
                                        void* stream) {
  if (B <= 0) return CLIPA_OK;
  if (S <= 0 || S > 4096 || B > 65535 || packed_bytes < 0 || !packed || !desc || !out) { clipa_set_error("resample_ragged: bad sizes (1 <= S <= 4096, B <= 65535)"); return CLIPA_ERR_ARG; }
  if (filter != 0 && filter != 1) { clipa_set_error("resample_ragged: filter is 0 (bicubic) or 1 (bilinear)"); return CLIPA_ERR_ARG; }
  if (max_rows <= 0 || max_rows > RR_MAX_SIDE || tmp_bytes < 0 || coef_ints < 0) { clipa_set_error("resample_ragged: bad storage sizes"); return CLIPA_ERR_ARG; }
  if (!workspace || workspace_bytes < clipa_resample_ragged_workspace(B, S, tmp_bytes, coef_ints)) { clipa_set_error("resample_ragged: workspace too small"); return CLIPA_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  unsigned char* tmp = (unsigned char*)workspace;
  int* plan = (int*)(tmp + rr_align(tmp_bytes));
  int* bounds = (int*)((unsigned char*)plan + rr_align(B * RR_PLAN * 4));
  int* coef = (int*)((unsigned char*)bounds + rr_align(B * 2 * S * 2 * 4));
  const long* d = (const long*)desc;
  hipLaunchKernelGGL(rr_validate_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, d, plan, (int)B, (int)S, filter,
                     (long)packed_bytes, (long)tmp_bytes, (long)coef_ints, (int)max_rows, err_count);
  if (int rc = clipa_check_launch("resample_ragged_validate")) return rc;
  hipLaunchKernelGGL(rr_coeffs_kernel, dim3((unsigned)((2 * S + 255) / 256), (unsigned)B), dim3(256), 0, st, d, plan, bounds, coef,
                     (int)S, filter);
  if (int rc = clipa_check_launch("resample_ragged_coeffs")) return rc;
  hipLaunchKernelGGL(rr_horizontal_kernel, dim3((unsigned)((max_rows * S + 255) / 256), (unsigned)B), dim3(256), 0, st,
                     (const unsigned char*)packed, d, plan, bounds, coef, tmp, (int)S);
  if (int rc = clipa_check_launch("resample_ragged_horizontal")) return rc;
  hipLaunchKernelGGL(rr_vertical_kernel, dim3((unsigned)((S * S + 255) / 256), (unsigned)B), dim3(256), 0, st, tmp, d, plan, bounds,
                     coef, gray_flags, (unsigned char*)out, (int)S);
  return clipa_check_launch("resample_ragged_vertical");
}
