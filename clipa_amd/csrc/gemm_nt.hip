// bf16 MFMA GEMM for gfx950 (MI355X):  C[M,N] = epi(alpha * A[M,K] . B[N,K]^T + bias[N])   (forward, dgrad with W^T)
//
// Reference call sites these replace (clipa_torch/open_clip/transformer.py): nn.MultiheadAttention in/out
// projection :209,:234, mlp.c_fc/c_proj :217-219, conv1 as a patch GEMM :371,:491, the final projections
// :528-529 and model.py:254, and the logits GEMMs of loss.py:135-142 - plus the input-gradient transposes of each.
//
// Operand tiles are DMA'd HBM->LDS with `buffer_load_dwordx4 ... lds` (bounds-checked SRD, so ragged edges read
// zeros); the LDS image is lane-linear (DMA constraint), so bank conflicts are removed by permuting the 16-byte
// chunks on the *source* address and applying the same XOR on the fragment read (tools/lds_bank_sim.py).  Tile
// ids are remapped so each XCD's L2 sees a contiguous run of tiles.  Kernels in this file:
//   gemm_nt2_kernel  256x256x64 tile, 8 waves, one persistent workgroup per CU, 2-slot ring, epilogue through an
//                    LDS window.  <f32> serves the f32-output GEMMs (head projections, loss gradients); <bf16, M16>
//                    every bf16-output GEMM.
// The round-1 generations (one tile per workgroup, loader/storer wave roles, ping-pong main loops) are in the git
// history only; the round-2 experiments (direct MFMA-fragment epilogue, two workgroups per CU, five-slot K-32 ring,
// deferred stores: none beat this kernel by more than its run-to-run noise except on one epilogue) are in
// the git history (tools/experiments/gemm_nt_round2.hip up to round 4: outside the package and libclipa_hip.so); measurements in
// profiles/r02_gemm_epilogue_experiments.md.
#include "gemm_common.h"
#include "internal_hooks.h"
#include <cstdlib>
#include <type_traits>

namespace clipa_gemm {
namespace {

// ------------------------------------------------------------------------------------------------
// gemm_nt v2: PERSISTENT tiles.  One workgroup per CU walks its share of the output tiles; the DMA
// ring never drains (the first K tile of the next output tile is fetched while the last K tile of
// the current one computes), MFMA operand fragments are register-prefetched one k-step ahead, and
// the epilogue goes through a dedicated 32 KiB LDS window (4 passes of 64 rows) placed after the
// 128 KiB ring, so its global stores retire underneath the next tile's main loop.
constexpr int CBUF_OFF = 2 * STAGE_BYTES;            // 131072
constexpr int LDS2_BYTES = CBUF_OFF + 64 * 512;      // 163840 = all 160 KiB of the CU

// M16 = true (bf16 output, non-STAG only): the main loop issues v_mfma_f32_16x16x32_bf16 (wave tile = 8 x 4
// blocks of 16 x 16, fragment = 16 rows x 32 k: lane -> row l&15, chunk 4*kk + (l>>4); the image and its
// (row>>1)&7 swizzle are unchanged and stay conflict-free for that read).  A quarter of the accumulator registers
// are read and written per instruction: less register-file energy per FLOP, which is what counts under the power cap.
// EPI / PRE (bf16 output): the epilogue and "also store the pre-activation" are compile-time, so that an epilogue without aux
// operand holds no aux registers and the compiler's vmcnt bookkeeping sees one straight-line sequence of loads and stores:
// with a run-time epilogue selector it has to place `s_waitcnt vmcnt(0)` in front of every chunk (the aux registers are
// written on one path and overwritten on another), which drains the chunk's predecessor store before the next one issues.
template <bool OUT_F32, bool SETPRIO, bool M16 = false, int EPI = CLIPA_EPI_NONE, bool PRE = false>
__global__ __launch_bounds__(NTHREADS) void gemm_nt2_kernel(NTArgs p) {
  static_assert(!M16 || !OUT_F32, "16x16x32 variant: bf16 output");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const int wm = wave >> 2, wn = wave & 3;

  const int tilesN = (p.N + BN - 1) / BN;
  const int tilesM = (p.M + BM - 1) / BM;
  const unsigned ntiles = (unsigned)(tilesM * tilesN);
  // XCD x (blocks with bid%8 == x) owns the contiguous tile range [base, base+len); its workgroups
  // take consecutive tiles, so the N-tiles of one A panel run side by side under one L2.
  const unsigned G = gridDim.x, xcd = blockIdx.x & 7u, idx = blockIdx.x >> 3;
  const unsigned gx = (G - xcd + 7u) >> 3;            // workgroups on this XCD
  const unsigned q8 = ntiles >> 3, r8 = ntiles & 7u;
  const unsigned base = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
  const unsigned len = q8 + (xcd < r8 ? 1u : 0u);

  unsigned voffA[4], voffB[4];
  int kel[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = (j * 8 + wave) * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ ((row >> 1) & 7);
    voffA[j] = (unsigned)(row * p.lda * 2 + chunk * 16);
    voffB[j] = (unsigned)(row * p.ldb * 2 + chunk * 16);
    kel[j] = chunk * 8;
  }
  const int sw = (l31 >> 1) & 7;
  const int rowoffA = (wm * 128 + l31) * 128;
  const int rowoffB = (wn * 64 + l31) * 128;
  const int nkt = (p.K + BK - 1) / BK;

  // Tile order inside an XCD's range: groups of GM = p.gm A-panels (nt_group_size), N-tile major inside a group, so the
  // ~32 tiles an XCD runs concurrently touch GM A-panels x (32/GM) B-tiles instead of 2 x 16 (fewer distinct operand tiles
  // per L2) and the weight matrix passes through the fabric once per group.  p.abl bit 3: plain row-major order (A/B).
  auto tile_origin = [&](unsigned t, int& m0, int& n0) {
    const int GM = (p.abl & 8) ? 1 : p.gm;
    const int per = GM * tilesN;
    const int g = (int)t / per, r = (int)t - g * per;
    const int gm = min(GM, tilesM - g * GM);
    const int tn = r / gm, mm = r - tn * gm;
    m0 = (g * GM + mm) * BM;
    n0 = tn * BN;
  };
  auto stage = [&](int buf, int m0, int n0, int k0) {
    const __amdgpu_buffer_rsrc_t rsA = make_rsrc(p.A + (size_t)m0 * p.lda * 2, (unsigned)(min(BM, p.M - m0) * p.lda * 2));
    const __amdgpu_buffer_rsrc_t rsB = make_rsrc(p.B + (size_t)n0 * p.ldb * 2, (unsigned)(min(BN, p.N - n0) * p.ldb * 2));
    char* sA = smem + buf * STAGE_BYTES;
    char* sB = sA + IMG_BYTES;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int pc = j * 8 + wave;
      const unsigned oob = (k0 + kel[j] >= p.K) ? 0x80000000u : 0u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, LDS_PTR(sA + pc * 1024), 16, voffA[j] | oob, k0 * 2, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, LDS_PTR(sB + pc * 1024), 16, voffB[j] | oob, k0 * 2, 0, 0);
    }
  };

  if (idx >= len) return;
  unsigned it = idx;
  int m0, n0;
  tile_origin(base + it, m0, n0);
  stage(0, m0, n0, 0);
  unsigned gk = 0;   // global K-tile counter: ring slot = gk & 1
  RING_WAIT_ALL();
  for (;;) {
    const bool has_next = it + gx < len;
    int m1 = 0, n1 = 0;
    if (has_next) tile_origin(base + it + gx, m1, n1);

    f32x16 acc[2][4];
    f32x4v acc16[4][8];      // M16: [n block of 16][m block of 16]
    if constexpr (M16) {
#pragma unroll
      for (int bj = 0; bj < 4; ++bj)
#pragma unroll
        for (int ai = 0; ai < 8; ++ai) acc16[bj][ai] = f32x4v{0.f, 0.f, 0.f, 0.f};
    } else {
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[ni][mi][r] = 0.f;
    }

    for (int kt = 0; kt < nkt; ++kt, ++gk) {
      if (kt + 1 < nkt) stage((gk + 1) & 1, m0, n0, (kt + 1) * BK);
      else {
        // the tile's 256 bias values ride the last K step as ONE 1 KiB LDS-DMA into the (idle) epilogue window
        if (!OUT_F32 && p.bias && wave == 0) {
          const __amdgpu_buffer_rsrc_t rsBias = make_rsrc(p.bias + n0, (unsigned)(max(0, min(BN, p.N - n0)) * 4));
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsBias, LDS_PTR(smem + CBUF_OFF), 16, (unsigned)(lane * 16), 0, 0, 0);
        }
        if (has_next) stage((gk + 1) & 1, m1, n1, 0);
      }
      const char* sA = smem + (gk & 1) * STAGE_BYTES;
      const char* sB = sA + IMG_BYTES;
      if constexpr (M16) {
        // 8 sub-steps per K tile: (kk, s) = 32-wide k-step kk, A blocks 2s and 2s+1 against the four B blocks of
        // kk (8 MFMAs); A fragments double-buffered per sub-step, B fragments per k-step
        const int l15 = lane & 15, g4 = lane >> 4, sw16 = (l15 >> 1) & 7;
        const char* pa = sA + (wm * 128 + l15) * 128;
        const char* pb = sB + (wn * 64 + l15) * 128;
        bf16x8 ga[2][2], gb[2][4];
#pragma unroll
        for (int bj = 0; bj < 4; ++bj) gb[0][bj] = *(const bf16x8*)(pb + bj * 2048 + ((g4 ^ sw16) << 4));
#pragma unroll
        for (int a = 0; a < 2; ++a) ga[0][a] = *(const bf16x8*)(pa + a * 2048 + ((g4 ^ sw16) << 4));
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int kk = u >> 2, sb = u & 3;
          if (u < 7) {
            const int k1 = (u + 1) >> 2, s1 = (u + 1) & 3;
#pragma unroll
            for (int a = 0; a < 2; ++a) ga[(u + 1) & 1][a] = *(const bf16x8*)(pa + (2 * s1 + a) * 2048 + (((4 * k1 + g4) ^ sw16) << 4));
          }
          if (u == 1) {
#pragma unroll
            for (int bj = 0; bj < 4; ++bj) gb[1][bj] = *(const bf16x8*)(pb + bj * 2048 + (((4 + g4) ^ sw16) << 4));
          }
          if (SETPRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int bj = 0; bj < 4; ++bj)
#pragma unroll
            for (int a = 0; a < 2; ++a)
              acc16[bj][2 * sb + a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gb[kk][bj], ga[u & 1][a], acc16[bj][2 * sb + a], 0, 0, 0);
          if (SETPRIO) __builtin_amdgcn_s_setprio(0);
        }
        if (kt + 1 < nkt) RING_WAIT_ALL();
        continue;
      }
      bf16x8 fa[2][4], fb[2][2];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) fa[0][mi] = *(const bf16x8*)(sA + rowoffA + mi * 4096 + ((hi ^ sw) << 4));
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) fb[0][ni] = *(const bf16x8*)(sB + rowoffB + ni * 4096 + ((hi ^ sw) << 4));
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int cur = ks & 1, nxt = cur ^ 1;
        if (ks < 3) {
          const int coff = ((2 * (ks + 1) + hi) ^ sw) << 4;
#pragma unroll
          for (int mi = 0; mi < 4; ++mi) fa[nxt][mi] = *(const bf16x8*)(sA + rowoffA + mi * 4096 + coff);
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) fb[nxt][ni] = *(const bf16x8*)(sB + rowoffB + ni * 4096 + coff);
        }
        if (SETPRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
            acc[ni][mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[cur][ni], fa[cur][mi], acc[ni][mi], 0, 0, 0);
        if (SETPRIO) __builtin_amdgcn_s_setprio(0);
      }
      if (kt + 1 < nkt) RING_WAIT_ALL();
    }

    // ---- epilogue of tile (m0, n0); the ring keeps filling for the next tile meanwhile ----
    if (p.abl & 2) {   // ablation: keep the accumulators live, write nothing
      float t = 0.f;
      if constexpr (M16) {
#pragma unroll
        for (int bj = 0; bj < 4; ++bj)
#pragma unroll
          for (int ai = 0; ai < 8; ++ai) t += acc16[bj][ai][0] + acc16[bj][ai][1] + acc16[bj][ai][2] + acc16[bj][ai][3];
      } else {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) t += acc[ni][mi][r];
      }
      if (t == 1.2345e-30f) ((float*)p.C)[tid] = t;
    } else if constexpr (OUT_F32) {
      float* C = (float*)p.C;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
          const int m = m0 + wm * 128 + mi * 32 + l31;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int n = n0 + wn * 64 + ni * 32 + 8 * q + 4 * hi;
            if (m < p.M && n < p.N) {
              float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
              if (p.bias) b4 = *(const float4*)(p.bias + n);
              float4 o;
              o.x = acc[ni][mi][4 * q + 0] * p.alpha + b4.x;
              o.y = acc[ni][mi][4 * q + 1] * p.alpha + b4.y;
              o.z = acc[ni][mi][4 * q + 2] * p.alpha + b4.z;
              o.w = acc[ni][mi][4 * q + 3] * p.alpha + b4.w;
              *(float4*)(C + (size_t)m * p.ldc + n) = o;
            }
          }
        }
    } else {
      static_assert(M16 || OUT_F32, "bf16 output: 16x16x32 main loop only");
      char* cb = smem + CBUF_OFF;
      // bias of this tile's 256 columns: landed in the window with the last K step (see the main loop), parked in the ring
      // slot that step has finished with, read back by the packing waves of each pass
      const bool use_bias = p.bias && !(p.abl & 4);
      char* park = smem + ((gk + 1) & 1) * STAGE_BYTES;   // gk & 1 holds the next tile's first K step
      if (use_bias) {
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        park_vectors(cb, park, tid, 1024);
      }
      float4 bias4[4];
      WinOut o;
      o.C = p.C; o.C2 = p.C2; o.aux = p.aux; o.ldc = p.ldc; o.ldaux = p.ldaux;
      o.M = p.M; o.N = p.N; o.m0 = m0; o.n0 = n0; o.act = p.act; o.abl = p.abl;
      window_epilogue<EPI, PRE, false>(cb, o, tid, wm, wn,
        [&](int) {
          if (use_bias) lds_read4_f4(bias4, park + (wn * 64 + 4 * (lane >> 4)) * 4);
          else {
#pragma unroll
            for (int bj = 0; bj < 4; ++bj) bias4[bj] = make_float4(0.f, 0.f, 0.f, 0.f);
          }
        },
        [&](int ai, int bj) {
          const float4 b4 = bias4[bj];
          u32x2 w;
          w[0] = pack2bf(acc16[bj][ai][0] * p.alpha + b4.x, acc16[bj][ai][1] * p.alpha + b4.y);
          w[1] = pack2bf(acc16[bj][ai][2] * p.alpha + b4.z, acc16[bj][ai][3] * p.alpha + b4.w);
          return w;
        });
    }
    if (!has_next) break;
    // the next tile's first K step (issued before the epilogue) has landed; the epilogue's stores need not have
    if constexpr (OUT_F32) RING_WAIT_ALL();
    else RING_WAIT_AFTER_EPILOGUE(win_stores(PRE));
    it += gx;
    m0 = m1;
    n0 = n1;
  }
}


LdsOptIn g_nt_lds;
int ensure_nt_attrs(int dev) {
  return g_nt_lds.ensure(dev, {(const void*)gemm_nt2_kernel<true, false>,
                               (const void*)gemm_nt2_kernel<false, true, true, CLIPA_EPI_NONE, false>,
                               (const void*)gemm_nt2_kernel<false, true, true, CLIPA_EPI_ACT, false>,
                               (const void*)gemm_nt2_kernel<false, true, true, CLIPA_EPI_ACT, true>,
                               (const void*)gemm_nt2_kernel<false, true, true, CLIPA_EPI_ADD, false>,
                               (const void*)gemm_nt2_kernel<false, true, true, CLIPA_EPI_DACT, false>},
                         LDS2_BYTES, "gemm_nt2");
}

}  // namespace

std::atomic<int> g_nt_variant{0};
std::atomic<int> g_abl{0};
std::atomic<int> g_last_gemm{0};
std::atomic<long> g_gemm_count[GEMM_COUNT_SLOTS];

int current_device(int* dev) {
  const hipError_t e = hipGetDevice(dev);
  if (e != hipSuccess) { clipa_set_error("hipGetDevice: %s", hipGetErrorString(e)); return CLIPA_ERR_LAUNCH; }
  if (*dev < 0 || *dev >= MAX_DEVICES) { clipa_set_error("device ordinal %d out of range", *dev); return CLIPA_ERR_ARG; }
  return 0;
}

int LdsOptIn::ensure(int dev, std::initializer_list<const void*> kernels, int bytes, const char* what) {
  std::call_once(once[dev], [&]() {
    rc[dev] = 0;
    for (const void* k : kernels) {
      const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
      if (e != hipSuccess) { clipa_set_error("hipFuncSetAttribute(%s): %s", what, hipGetErrorString(e)); rc[dev] = CLIPA_ERR_LAUNCH; }
    }
  });
  return rc[dev];
}

int gemm_num_cu(int dev) {
  static std::once_flag once[MAX_DEVICES];
  static int ncu[MAX_DEVICES];
  std::call_once(once[dev], [dev]() {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    ncu[dev] = n;
  });
  return ncu[dev];
}

}  // namespace clipa_gemm

using namespace clipa_gemm;

extern "C" int clipa_internal_debug_set(int gemm_nt_variant, int ablation_flags) {
  if (gemm_nt_variant != 0 || ablation_flags != 0) {      // a reset is always allowed; anything else only in a harness process
    const char* on = getenv("CLIPA_DEBUG_HOOKS");
    if (!on || on[0] != '1') {
      clipa_set_error("clipa_internal_debug_set: kernel-experiment hooks are disabled (set CLIPA_DEBUG_HOOKS=1 in a test / A-B harness process)");
      return CLIPA_ERR_ARG;
    }
  }
  g_nt_variant.store(gemm_nt_variant, std::memory_order_relaxed);
  g_abl.store(ablation_flags, std::memory_order_relaxed);
  return CLIPA_OK;
}

extern "C" int clipa_internal_last_gemm(void) { return g_last_gemm.load(std::memory_order_relaxed); }
extern "C" int clipa_internal_debug_flags(void) { return g_abl.load(std::memory_order_relaxed); }
extern "C" int clipa_internal_gemm_counts(long* out, int n, int reset) {
  for (int i = 0; i < n && i < GEMM_COUNT_SLOTS; ++i) {
    if (out) out[i] = g_gemm_count[i].load(std::memory_order_relaxed);
    if (reset) g_gemm_count[i].store(0, std::memory_order_relaxed);
  }
  return GEMM_COUNT_SLOTS;
}

extern "C" int clipa_gemm_nt(const void* A, const void* B, void* C, void* C2, const float* bias,
                             const void* aux, int64_t M, int64_t N, int64_t K, int64_t lda,
                             int64_t ldb, int64_t ldc, int64_t ldaux, float alpha, int epi, int act,
                             int out_f32, void* stream) {
  if (M <= 0 || N <= 0) return CLIPA_OK;
  if (K <= 0 || K % 8 != 0) { clipa_set_error("gemm_nt: K=%ld must be a positive multiple of 8", (long)K); return CLIPA_ERR_ARG; }
  if (N % 8 != 0 || ldc % 8 != 0 || lda % 8 != 0 || ldb % 8 != 0) { clipa_set_error("gemm_nt: N, lda, ldb, ldc must be multiples of 8"); return CLIPA_ERR_ARG; }
  if (epi < CLIPA_EPI_NONE || epi > CLIPA_EPI_DACT8) { clipa_set_error("gemm_nt: unknown epilogue %d", epi); return CLIPA_ERR_ARG; }
  // e4m3 pre-activation flavours: the same epilogues with a 1-byte second output / operand, four-wave kernel only
  const int pre8 = epi == CLIPA_EPI_ACT_PRE8, aux8 = epi == CLIPA_EPI_DACT8;
  if (pre8 && !C2) { clipa_set_error("gemm_nt: CLIPA_EPI_ACT_PRE8 needs C2"); return CLIPA_ERR_ARG; }
  if (pre8) epi = CLIPA_EPI_ACT;
  if (aux8) epi = CLIPA_EPI_DACT;
  if ((epi == CLIPA_EPI_ADD || epi == CLIPA_EPI_DACT) && (!aux || ldaux % 8 != 0)) { clipa_set_error("gemm_nt: epilogue %d needs aux with ldaux%%8==0", epi); return CLIPA_ERR_ARG; }
  if (C2 && epi != CLIPA_EPI_ACT && !aux8) { clipa_set_error("gemm_nt: C2 goes with CLIPA_EPI_ACT (pre-activation copy) or CLIPA_EPI_DACT8 (activation output) only"); return CLIPA_ERR_ARG; }
  if (out_f32 && epi != CLIPA_EPI_NONE) { clipa_set_error("gemm_nt: f32 output supports epilogue NONE only"); return CLIPA_ERR_ARG; }
  if (256 * lda * 2 >= (1L << 30) || 256 * ldb * 2 >= (1L << 30) || 256 * ldc * 2 >= (1L << 30) || 256 * ldaux * 2 >= (1L << 30)) { clipa_set_error("gemm_nt: leading dimension too large"); return CLIPA_ERR_ARG; }
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (int rc = ensure_nt_attrs(dev)) return rc;
  const int num_cu = gemm_num_cu(dev);
  NTArgs a;
  a.A = (const char*)A; a.B = (const char*)B; a.C = (char*)C; a.C2 = (char*)C2; a.bias = bias; a.aux = (const char*)aux;
  a.M = (int)M; a.N = (int)N; a.K = (int)K; a.lda = lda; a.ldb = ldb; a.ldc = ldc; a.ldaux = ldaux;
  a.alpha = alpha; a.epi = epi; a.act = act; a.abl = g_abl.load(std::memory_order_relaxed);
  a.pre8 = pre8; a.aux8 = aux8;
  a.gm = nt_group_size((N + BN - 1) / BN, 256L * K * 2);
  if ((a.abl >> 20) & 63) a.gm = (a.abl >> 20) & 63;       // experiment: tile-group size override (clipa_internal_debug_set flags bits 20..25)
  hipStream_t st = (hipStream_t)stream;
  // whole-tile bf16 shapes (every block GEMM of the BASELINE configurations at batch multiples of 256) run on the four-wave
  // kernel with the hand-scheduled main loop (gemm_nta.hip); bit-identical outputs.  clipa_internal_debug_set(1, .) keeps them on
  // gemm_nt2, clipa_internal_debug_set(2 + s, .) selects generated schedule s (A/B harnesses)
  const int variant = g_nt_variant.load(std::memory_order_relaxed);
  note_gemm(1);
  if (variant != 1 && !(a.abl & 13 & 0xfffff) && nta_eligible(a, out_f32))
    return nta_launch(a, dev, num_cu, variant >= 2 ? variant - 2 : NTA_DEFAULT_SCHEDULE, st);
  if (pre8 || aux8) { clipa_set_error("gemm_nt: e4m3 pre-activation epilogues need whole 256 x 256 x 128 tiles (M=%ld N=%ld K=%ld)", (long)M, (long)N, (long)K); return CLIPA_ERR_ARG; }
  const long tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  if (out_f32) {
    const unsigned grid = (unsigned)(tiles < num_cu ? tiles : num_cu);
    hipLaunchKernelGGL((gemm_nt2_kernel<true, false>), dim3(grid), dim3(NTHREADS), LDS2_BYTES, st, a);
    return clipa_check_launch("gemm_nt2<f32>");
  }
  // bf16 output: the 16x16x32 main loop with the LDS-window epilogue for every shape; one instantiation per epilogue.
  // A block's backward-time recompute must reproduce its forward bit for bit: the one-output and the two-output
  // (pre-activation copy) form of the activation epilogue run the same arithmetic (epi_chunk), PRE only adds a store
  // (tests/test_kernels_gpu.py::test_recompute_equals_stored_activations).
  const unsigned grid = (unsigned)(tiles < num_cu ? tiles : num_cu);
#define LAUNCH_NT(E, P2) hipLaunchKernelGGL((gemm_nt2_kernel<false, true, true, E, P2>), dim3(grid), dim3(NTHREADS), LDS2_BYTES, st, a)
  if (epi == CLIPA_EPI_NONE) LAUNCH_NT(CLIPA_EPI_NONE, false);
  else if (epi == CLIPA_EPI_ACT && C2) LAUNCH_NT(CLIPA_EPI_ACT, true);
  else if (epi == CLIPA_EPI_ACT) LAUNCH_NT(CLIPA_EPI_ACT, false);
  else if (epi == CLIPA_EPI_ADD) LAUNCH_NT(CLIPA_EPI_ADD, false);
  else LAUNCH_NT(CLIPA_EPI_DACT, false);
#undef LAUNCH_NT
  return clipa_check_launch("gemm_nt2<bf16>");
}
