// Shared pieces of the fused attention kernels (attention.hip, attention_wide.hip): argument block, LDS image geometry per head
// dim and the LDS layout of a workgroup, the chunk swizzle that serves direct and transposed fragment reads, LDS-DMA of a head's
// rows, MFMA fragment loads, the mask bound of a score fragment, output stores (whole rows through a per-wave LDS window, or
// scattered), the in-register row softmax, the tile arithmetic of the four kernels (ATTN_* macros: score products, <dO, O>,
// accumulation through transposed fragments, scattered tile output), the head prologue of the short kernels.
// (The single-sweep persistent kernels of round 5 that once shared this header were measured slower and are gone from the tree:
// profiles/r05_attention_persistent_single_sweep.md, sources in the git history.)
#pragma once
#include "common.h"

namespace {

struct AttnArgs {
  const char* q; const char* k; const char* v; long ld_qkv;   // bf16 rows, stride in elements
  char* o; const char* o_in; const char* d_o; long ld_o;
  char* dq; char* dk; char* dv; long ld_dqkv;
  float* stats;   // [B*H*L][2] = (c*rowmax, 1/rowsum), written by fwd, read by bwd
  int B, H, L;
  float scale;
  int causal;
  // packed variable-length sequences (short kernels only; clipa_attention_*_varlen): sequence i of this launch is
  // seq_ids[i] (or i), its rows are [seq_start[s], seq_start[s] + seq_len[s]) of the token matrix, B = sequences of the launch
  const int* seq_start; const int* seq_len; const int* seq_ids;
};

// Geometry per head dim.  dh = 64 (ViT-S/B/L, every text tower): 128-byte LDS rows, 4 k-steps, 2 output tiles.
// dh = 80 (ViT-H/14, transformer.py:126 with head_width 80): 256-byte LDS rows of which 160 B carry data
// (power-of-two row stride keeps the XOR swizzle), 5 k-steps, 3 output tiles whose last 16 columns are
// never stored; one workgroup per CU instead of two.
template <int DH>
struct HD {
  static constexpr int RB = DH == 64 ? 128 : 256;   // LDS row bytes
  static constexpr int NCH = RB / 16;               // 16-byte chunk positions per row
  static constexpr int KS = (DH + 15) / 16;         // 16-wide reduction steps over the head dim (a ragged last step sees zeros)
  static constexpr int DT = (DH + 31) / 32;         // 32-wide output tiles over the head dim
  static constexpr int WGS = DH == 64 ? 2 : 1;      // workgroups per CU the LDS image allows
};
// Short sequences (CLIPA's 84-112 px images = 26-50 tokens, 8-32 token captions) fit one or two 32-row tiles: a
// workgroup then takes 4 or 2 heads (one or two waves each) instead of idling three or two of its waves.
template <int NKT>
struct WGHeads {
  static constexpr int HPW = NKT == 1 ? 4 : (NKT == 2 ? 2 : 1);   // heads per workgroup
  static constexpr int WPH = 4 / HPW;                             // waves per head
};
// Waves per workgroup.  Head dim 80 with five or more key tiles (ViT-H/14: 257 tokens = 9 tiles) has LDS for ONE workgroup per
// CU; four waves there leave every SIMD a single wave and nothing to overlap its MFMA -> softmax -> MFMA chain with, so those
// instantiations run eight waves (two per SIMD, one 32-row tile each for all but one wave).
template <int NKT, int DH>
// (Round 6, "one tile per wave": 7 or 8 waves for the 7 tiles of 197 tokens need 154-165 registers each, which leaves ONE
// workgroup per CU - forward 1.63 -> 2.03 ms, backward 4.76 -> 5.61 ms; 9 waves for the 9 tiles of 257 tokens at head dim 80 cap a
// wave at 168 registers: 53-57 spills.  profiles/r06_attention_waves_per_workgroup_ab.jsonl)
__host__ __device__ constexpr int attn_waves() { return (DH == 80 && NKT >= 5) ? 8 : 4; }   // (wider heads spill at 256 registers per wave)

// chunk permutation of an LDS row: conflict-free for both the direct ds_read_b128 operand reads and the
// transposed ds_read_b64_tr_b16 reads (tools/lds_bank_sim.py) - 8 chunks per 128-B row, 16 per 256-B row
template <int DH>
__device__ __forceinline__ int swz_u(int row) {
  if (DH == 64) return (((row >> 1) & 1) << 2) | ((row >> 2) & 1) | (((row >> 3) & 1) << 1);
  return ((row & 3) << 2) | ((row >> 2) & 3);
}

// DMA rows [0, LP) of one head into a swizzled LDS image; rows >= L and chunks >= dh read zeros
template <int DH>
__device__ __forceinline__ void dma_image(const __amdgpu_buffer_rsrc_t rs, char* img, int LP, long ld,
                                          int wave, int lane, int nwaves = 4) {
  constexpr int NCH = HD<DH>::NCH, RPP = 1024 / HD<DH>::RB;
  for (int pc = wave; pc < LP / RPP; pc += nwaves) {
    const int row = pc * RPP + lane / NCH;
    const int chunk = (lane & (NCH - 1)) ^ swz_u<DH>(row);
    const unsigned oob = (chunk * 8 >= DH) ? 0x80000000u : 0u;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, LDS_PTR(img + pc * 1024), 16,
                                             (unsigned)(row * ld * 2 + chunk * 16) | oob, 0, 0, 0);
  }
}

// direct operand fragment: lane -> image row (rowbase + l31), k-chunk 2*ks+hi
template <int DH>
__device__ __forceinline__ bf16x8 frag_direct(const char* img, int rowbase, int l31, int hi, int ks) {
  return *(const bf16x8*)(img + (rowbase + l31) * HD<DH>::RB + (((2 * ks + hi) ^ swz_u<DH>(l31)) << 4));
}

// transposed operand fragment for a 16-wide reduction step: rows rowbase16 + {4hi+0..3, 8+4hi+0..3},
// column (colbase + 16*q16 + i16) -> 8 k-slots matching the register order of a 32x32 C fragment
template <int DH>
__device__ __forceinline__ bf16x8 frag_trans(const char* img, int rowbase16, int colbase, int hi, int q16, int i16) {
  constexpr int RB = HD<DH>::RB;
  const int col = colbase + 16 * q16 + 4 * (i16 & 3);
  const int r0 = rowbase16 + 4 * hi + (i16 >> 2);
  const int r1 = r0 + 8;
  const bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) bf16x4*)(img + r0 * RB + (((col >> 3) ^ swz_u<DH>(r0)) << 4) + (col & 7) * 2));
  const bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) bf16x4*)(img + r1 * RB + (((col >> 3) ^ swz_u<DH>(r1)) << 4) + (col & 7) * 2));
  bf16x8 f;
  f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3];
  f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
  return f;
}

__device__ __forceinline__ bf16x8 pack_frag(const float* v) {
  u32x4 w;
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = pack2bf(v[2 * i], v[2 * i + 1]);
  return __builtin_bit_cast(bf16x8, w);
}

// store a 32x32 fragment held as X^T[d][row] (lane: row = l31, d = 8*(r>>2)+4*hi+(r&3)) into a
// row-major bf16 matrix: 4 consecutive d per store
__device__ __forceinline__ void store_frag_T(char* base, long ld, long row, int col0, int hi, const f32x16& a, float mul,
                                             int ncols = 32) {
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    if (8 * qd >= ncols) continue;     // partial last tile of a head dim that is not a multiple of 32
    u32x2 w;
    w[0] = pack2bf(a[4 * qd + 0] * mul, a[4 * qd + 1] * mul);
    w[1] = pack2bf(a[4 * qd + 2] * mul, a[4 * qd + 3] * mul);
    *(u32x2*)(base + (row * ld + col0 + 8 * qd + 4 * hi) * 2) = w;
  }
}

// The same tile (head dim 64: both 32-column fragments of a 32-row tile = 32 rows of 128 B) stored as WHOLE 128-byte rows:
// store_frag_T writes 8 bytes per lane to 32 different rows per instruction (16 instructions, every one touching 32 cache
// lines); here the tile passes through 4 KB of LDS private to the wave (16-byte chunks XOR-swizzled by the row, conflict-free
// both ways) and leaves as 4 instructions of 8 full rows each.  The global stores of the backward cost 21 % of its time
// in the scattered form (profiles/r03_attention_bwd_ablations.jsonl).
__device__ __forceinline__ void store_tile64(char* stage, char* base, long ld, long row0, int rows_valid, int col0, int lane,
                                             const f32x16& a0, const f32x16& a1, float mul) {
  const int l31 = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    const f32x16& a = dt ? a1 : a0;
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      u32x2 w;
      w[0] = pack2bf(a[4 * qd + 0] * mul, a[4 * qd + 1] * mul);
      w[1] = pack2bf(a[4 * qd + 2] * mul, a[4 * qd + 3] * mul);
      *(u32x2*)(stage + l31 * 128 + (((4 * dt + qd) ^ (l31 & 7)) << 4) + 8 * hi) = w;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // one wave: LDS operations retire in order, only the compiler needs telling
  const int chunk = lane & 7;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = 8 * j + (lane >> 3);
    const u32x4 v = *(const u32x4*)(stage + row * 128 + ((chunk ^ (row & 7)) << 4));
    if (row < rows_valid) *(u32x4*)(base + ((row0 + row) * ld + col0) * 2 + chunk * 16) = v;
  }
  asm volatile("" ::: "memory");
}

// Head dim 80 (ViT-H/14): rows of 160 bytes = 10 chunks, three 32-column fragments of which the last 16 columns do not exist.
// Its 256-byte-row images leave 10-13 KB of LDS per workgroup, so the tile goes through the window in two halves of 16 rows
// (2560 B per wave); 160 = 10 x 16 makes the read side linear in the lane index.
__device__ __forceinline__ void store_tile80(char* stage, char* base, long ld, long row0, int rows_valid, int col0, int lane,
                                             const f32x16& a0, const f32x16& a1, const f32x16& a2, float mul) {
  const int l31 = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if ((l31 >> 4) == h) {
#pragma unroll
      for (int dt = 0; dt < 3; ++dt) {
        const f32x16& a = dt == 0 ? a0 : (dt == 1 ? a1 : a2);
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
          if (4 * dt + qd >= 10) continue;
          u32x2 w;
          w[0] = pack2bf(a[4 * qd + 0] * mul, a[4 * qd + 1] * mul);
          w[1] = pack2bf(a[4 * qd + 2] * mul, a[4 * qd + 3] * mul);
          *(u32x2*)(stage + (l31 & 15) * 160 + (4 * dt + qd) * 16 + 8 * hi) = w;
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int task = 64 * j + lane;               // 16 rows x 10 chunks
      if (task < 160) {
        const u32x4 v = *(const u32x4*)(stage + task * 16);
        const int row = task / 10, chunk = task - 10 * row;
        if (16 * h + row < rows_valid) *(u32x4*)(base + ((row0 + 16 * h + row) * ld + col0) * 2 + chunk * 16) = v;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
}
template <int DH>
struct Stg { static constexpr int BYTES = DH == 64 ? 4096 : 2560; };      // LDS window per wave
template <int DH>
__device__ __forceinline__ void store_tile(char* stage, char* base, long ld, long row0, int rows_valid, int col0, int lane,
                                           const f32x16* a, float mul) {
  if constexpr (DH == 64) store_tile64(stage, base, ld, row0, rows_valid, col0, lane, a[0], a[1], mul);
  else store_tile80(stage, base, ld, row0, rows_valid, col0, lane, a[0], a[1], a[2], mul);
}

// Mask bound of a query row: register r of the score fragment of key tile T holds key 32 T + 8 (r >> 2) + (r & 3) + 4 hi, valid
// iff it lies below the sequence length and, under the causal mask, at or below the query qg (the 4 hi is folded into the bound).
template <bool CAUSAL>
__device__ __forceinline__ int key_limit(int L, int qg, int hi) { return (CAUSAL ? min(L, qg + 1) : L) - 4 * hi; }
__device__ __forceinline__ bool key_valid(int T, int r, int lim2) { return 32 * T + 8 * (r >> 2) + (r & 3) < lim2; }

// Row softmax over the transposed score fragments of one 32-query tile.  In: raw q.k scores.  Out: s =
// exp2(c*(s - rowmax)) (un-normalised, c = scale*log2 e folded into one FMA), inv = 1/rowsum, m2 = c*rowmax.
// key(kt, r) = 32kt + 8(r>>2) + (r&3) + 4hi is valid iff < lim (padding / causal bound); tiles valid for
// every lane skip the compare/select: without a causal mask only the last key tile can be partial (NKT =
// ceil(L / 32) exactly), so the image tower pays 16 compares per row instead of 16 * NKT.
template <int NKT, bool CAUSAL>
__device__ __forceinline__ void softmax_rows(f32x16 (&s)[NKT], const AttnArgs& p, int qt, int qg, int hi,
                                             float& inv, float& m2) {
  const float c = p.scale * 1.4426950408889634f;
  const int lim2 = key_limit<CAUSAL>(p.L, qg, hi);
  float mx = -1e30f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    const bool full = CAUSAL ? ((32 * kt + 32 <= p.L) && kt < qt) : (kt < NKT - 1);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = s[kt][r];
      if (!full) v = key_valid(kt, r, lim2) ? v : -1e30f;
      s[kt][r] = v;
      mx = fmaxf(mx, v);
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  m2 = mx * c;
  float sum = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e = __builtin_amdgcn_exp2f(fmaf(s[kt][r], c, -m2));
      s[kt][r] = e;
      sum += e;
    }
  sum += __shfl_xor(sum, 32, 64);
  inv = 1.0f / sum;
}

// load the k-step fragments of one 32-row tile straight from global memory (rows >= L read zeros)
// (chunks at or beyond the head dim - the ragged last k-step of head dims 88 / 104 - would be the NEXT head's columns: their
// offset is pushed out of the descriptor's range, which returns zeros, as dma_image does for the LDS images)
template <int KS, int DH>
__device__ __forceinline__ void load_frags(const __amdgpu_buffer_rsrc_t rs, long ld, int row, int hi, bf16x8 (&f)[KS]) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const unsigned oob = ((2 * ks + hi) * 8 >= DH) ? 0x80000000u : 0u;
    f[ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, (unsigned)(row * ld * 2 + (2 * ks + hi) * 16) | oob, 0, 0));
  }
}

// half s2 of the 16 probabilities a lane holds per 32-key tile, as an MFMA operand
__device__ __forceinline__ bf16x8 pack_frag(const f32x16& v, int s2) {
  float pv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) pv[e] = v[8 * s2 + e];
  return pack_frag(pv);
}

// ---- The tile arithmetic of the four kernels, one copy each.  Macros over the kernels' own names (DH, KS, DT, l31, hi, q16, i16; h
// for the stores), not functions: every function form tried - by value, by reference, over one or two accumulators - moves the
// compiler's schedule of the short backward, and helpers that take an accumulator array even move kernels that do not call them
// (profiles/attention_shared_isa.md).  A macro expands to the statements the kernels had.
// Raw scores of the image tile at `rowbase` against the wave's own 32 rows (k-step fragments f): acc += S^T[image row][own row].
#define ATTN_SCORE_TILE(acc, img, rowbase, f)                                                                                   \
  _Pragma("unroll") for (int ks = 0; ks < KS; ++ks)                                                                             \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_direct<DH>(img, rowbase, l31, hi, ks), f[ks], acc, 0, 0, 0);
// The two products of a backward pair, k-steps interleaved: s from image 0 and fa (q.k), dp from image 1 and fb (dO.v).
#define ATTN_SCORE_PAIR(s, dp, rowbase, fa, fb)                                                                                 \
  _Pragma("unroll") for (int ks = 0; ks < KS; ++ks) {                                                                           \
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_direct<DH>(img0, rowbase, l31, hi, ks), fa[ks], s, 0, 0, 0);               \
    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_direct<DH>(img1, rowbase, l31, hi, ks), fb[ks], dp, 0, 0, 0);             \
  }
// float D = <dO, O> of the lane's row, from the k-step fragments of the two (each half-wave holds half of the row)
#define ATTN_ROW_DOT(D, fdo, fo)                                                                                                \
  float D = 0.f;                                                                                                                \
  _Pragma("unroll") for (int ks = 0; ks < KS; ++ks) {                                                                           \
    float a[8], o8[8];                                                                                                          \
    unpack8(__builtin_bit_cast(u32x4, fdo[ks]), a);                                                                             \
    unpack8(__builtin_bit_cast(u32x4, fo[ks]), o8);                                                                             \
    _Pragma("unroll") for (int i = 0; i < 8; ++i) D += a[i] * o8[i];                                                            \
  }                                                                                                                             \
  D += __shfl_xor(D, 32, 64);
// acc^T[d][own row] += image^T[d][tile row] . P[tile row][own row] over the 32-row tile at `rowbase`: the 16 values a lane holds go
// in as two packed halves (FRAG: the bf16x8 of half s2), the image as transposed fragments.  The second form runs two
// accumulators interleaved (dV and dK).
#define ATTN_TRANS_MFMA(acc, img, rowbase16, f)                                                                                 \
  acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_trans<DH>(img, rowbase16, 32 * dt, hi, q16, i16), f, acc[dt], 0, 0, 0);
#define ATTN_ACC_TRANS(acc, img, rowbase, FRAG)                                                                                 \
  _Pragma("unroll") for (int s2 = 0; s2 < 2; ++s2) {                                                                            \
    const bf16x8 fa_ = FRAG;                                                                                                    \
    _Pragma("unroll") for (int dt = 0; dt < DT; ++dt) ATTN_TRANS_MFMA(acc, img, rowbase + 16 * s2, fa_)                         \
  }
#define ATTN_ACC_TRANS2(acca, imga, FRAGA, accb, imgb, FRAGB, rowbase)                                                          \
  _Pragma("unroll") for (int s2 = 0; s2 < 2; ++s2) {                                                                            \
    const bf16x8 fa_ = FRAGA;                                                                                                   \
    const bf16x8 fb_ = FRAGB;                                                                                                   \
    _Pragma("unroll") for (int dt = 0; dt < DT; ++dt) {                                                                         \
      ATTN_TRANS_MFMA(acca, imga, rowbase + 16 * s2, fa_)                                                                       \
      ATTN_TRANS_MFMA(accb, imgb, rowbase + 16 * s2, fb_)                                                                       \
    }                                                                                                                           \
  }
// The scattered output of the lane's row `row` of a tile (two tiles interleaved in the second form): DT fragments, the last one
// partial where the head dim is no multiple of 32.
#define ATTN_STORE_ROWS(base, ld, row, acc, mul)                                                                                \
  _Pragma("unroll") for (int dt = 0; dt < DT; ++dt) store_frag_T(base, ld, row, h * DH + 32 * dt, hi, acc[dt], mul, DH - 32 * dt);
#define ATTN_STORE_ROWS2(basea, acca, mula, baseb, accb, mulb, ld, row)                                                         \
  _Pragma("unroll") for (int dt = 0; dt < DT; ++dt) {                                                                           \
    store_frag_T(basea, ld, row, h * DH + 32 * dt, hi, acca[dt], mula, DH - 32 * dt);                                           \
    store_frag_T(baseb, ld, row, h * DH + 32 * dt, hi, accb[dt], mulb, DH - 32 * dt);                                           \
  }

// LDS layout of a short-kernel workgroup, stated once for the kernels' pointers, the launchers' sizes and the staging decision:
// HPW head slots of two [LP, RB] images each (the backward appends 3 LP floats of per-query statistics to a slot), then one
// store_tile window per wave where the instantiation stages.
// whole-row stores (store_tile) need 16 / 10 KB of LDS more per workgroup: taken where the workgroups per CU stay what they are
// (STAGE; tests/attention_cases.py restates it as fwd_stages / bwd_stages, the names it had as two functions)
template <int NKT, int DH, bool BWD>
struct ShortLds {
  static constexpr int IMG = NKT * 32 * HD<DH>::RB, SLOT = 2 * IMG + (BWD ? 3 * NKT * 32 * 4 : 0), SLOTS = WGHeads<NKT>::HPW * SLOT;
  static constexpr int WINDOWS = attn_waves<NKT, DH>() * Stg<DH>::BYTES;
  static constexpr bool STAGE = (DH == 64 || DH == 80) && (SLOTS + WINDOWS) * HD<DH>::WGS <= 160 * 1024;
  static constexpr int BYTES = SLOTS + (STAGE ? WINDOWS : 0);
  static __device__ __forceinline__ char* image(char* smem, int slot, int i) { return smem + slot * SLOT + i * IMG; }
  static __device__ __forceinline__ float* stats(char* smem, int slot) { return (float*)(smem + slot * SLOT + 2 * IMG); }
  static __device__ __forceinline__ char* stage(char* smem, int wave_wg) { return smem + SLOTS + wave_wg * Stg<DH>::BYTES; }
};
// The long kernels: two images of LONG_CT tiles; the backward appends three rows of LONG_LMAX per-query statistics.
constexpr int LONG_CT = 8;          // 256 rows per chunk
constexpr int LONG_LMAX = 1024;
template <int DH, bool BWD>
struct LongLds {
  static constexpr int IMG = LONG_CT * 32 * HD<DH>::RB, BYTES = 2 * IMG + (BWD ? 3 * LONG_LMAX * 4 : 0);
  static __device__ __forceinline__ float* stats(char* smem) { return (float*)(smem + 2 * IMG); }
};

// The head prologue of the short kernels.  A workgroup serves HPW heads with WPH waves each; the last workgroup may have empty
// head slots (live = false: they run on the last head and store nothing).  Declares, for both kernels, the wave's place in the
// workgroup, the LDS pointers, the lane split, the head's (b, h), `p`, row0 / stat0 and the descriptors of the five operand
// matrices; the forward leaves the backward's (sM, sD, rsDO, rsO) unused.  (A macro in the backward's statement order, not a
// function that returns these values in a struct: that form, and already another order of these statements, changes the
// scalar prologue of every short kernel - profiles/attention_shared_isa.md.)
// Where the (batch, head) pair of this workgroup slot lives: fixed-length batches have sequence b at rows b * L; packed
// variable-length launches (the text tower on the tokens up to each caption's EOT) look the sequence up.  `p` is the kernel's
// view of the arguments with L = THIS sequence's length; statistics sit at [row0 * H + h * L + query].
#define ATTN_HEAD_PROLOGUE(NKT, DH, BWD)                                                                              \
  constexpr int HPW = WGHeads<NKT>::HPW, WPH = attn_waves<NKT, DH>() / HPW;                                           \
  const int tid = threadIdx.x, lane = tid & 63;                                                                       \
  const int wave_wg = __builtin_amdgcn_readfirstlane(tid >> 6);                                                       \
  const int slot = wave_wg / WPH, wave = wave_wg % WPH; /* head slot of this wave, wave index within the head */      \
  using Lds = ShortLds<NKT, DH, BWD>;                                                                                 \
  char* img0 = Lds::image(smem, slot, 0);                                                                             \
  char* img1 = Lds::image(smem, slot, 1);                                                                             \
  float* sM = Lds::stats(smem, slot);                   /* the backward's per-query statistics */                     \
  float* sD = sM + 2 * NKT * 32;                                                                                      \
  char* stage = Lds::stage(smem, wave_wg);              /* the wave's store_tile window, where Lds::STAGE */          \
  const int l31 = lane & 31, hi = lane >> 5, q16 = (lane >> 4) & 1, i16 = lane & 15;                                  \
  const long nheads = (long)pin.B * pin.H;                                                                            \
  const long head_raw = (long)blockIdx.x * HPW + slot;                                                                \
  const bool live = head_raw < nheads;                                                                                \
  const long head = live ? head_raw : nheads - 1;                                                                     \
  const int b = (int)(head / pin.H), h = (int)(head - (long)b * pin.H);                                               \
  AttnArgs p = pin;                                                                                                   \
  long row0 = (long)b * pin.L;                                                                                        \
  size_t stat0 = (size_t)head * pin.L;                                                                                \
  if (pin.seq_len) {                                                                                                  \
    const int sid = pin.seq_ids ? pin.seq_ids[b] : b;                                                                 \
    p.L = pin.seq_len[sid];                                                                                           \
    row0 = pin.seq_start[sid];                                                                                        \
    stat0 = (size_t)row0 * pin.H + (size_t)h * p.L;                                                                   \
  }                                                                                                                   \
  /* the head's rows in the [*, ld_qkv] matrices (q, k, v) and in the [*, ld_o] ones (dO and O: the backward's) */    \
  const size_t hoff = ((size_t)row0 * p.ld_qkv + (size_t)h * DH) * 2;                                                 \
  const size_t ooff = ((size_t)row0 * p.ld_o + (size_t)h * DH) * 2;                                                   \
  const unsigned nrec = (unsigned)((long)(p.L - 1) * p.ld_qkv * 2 + DH * 2);                                          \
  const unsigned nrec_o = (unsigned)((long)(p.L - 1) * p.ld_o * 2 + DH * 2);                                          \
  const __amdgpu_buffer_rsrc_t rsQ = make_rsrc(p.q + hoff, nrec), rsK = make_rsrc(p.k + hoff, nrec),                  \
                               rsV = make_rsrc(p.v + hoff, nrec), rsDO = make_rsrc(p.d_o + ooff, nrec_o),             \
                               rsO = make_rsrc(p.o_in + ooff, nrec_o);

}  // namespace
