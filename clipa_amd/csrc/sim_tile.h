// Main loop of the fused similarity losses (simce.hip: MI = 4, a 256 x 256 tile; simce_distill.hip: MI = 2, 128 x 256):
// 8 waves, a two-stage LDS ring at BK = 64 filled by 16-byte LDS-DMA with XOR-swizzled chunks, v_mfma_f32_32x32x16_bf16 -
// the structure of gemm_nt2<f32> with one output tile per workgroup.
#pragma once
#include "gemm_common.h"

namespace clipa_gemm {

template <int MI>
constexpr int sim_stage_bytes() { return MI * 64 * BK * 2 + IMG_BYTES; }   // A image of MI * 64 rows + B image of 256

// acc[ni][mi] = tile of A[0 : MI * 64] . B[0 : 256]^T over K (bf16, rows past rowsA / rowsB and k >= K read 0) through the
// first 2 * sim_stage_bytes<MI>() bytes of smem.  D[n][m] fragment: lane holds row m = wm*MI*32 + mi*32 + l31 and columns
// n = wn*64 + ni*32 + 8*(r>>2) + 4*hi + (r&3).  No barrier before the first stage nor after the last step: a caller that
// reuses the ring synchronises first.
template <int MI>
__device__ __forceinline__ void sim_tile(char* smem, const char* A, const char* B, long lda, long ldb, int K, int rowsA,
                                         int rowsB, f32x16 (&acc)[2][MI]) {
  constexpr int IMG_A = MI * 64 * BK * 2, STAGE = sim_stage_bytes<MI>();
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const int wm = wave >> 2, wn = wave & 3;   // wave tile: MI * 32 (m) x 64 (n)
  const __amdgpu_buffer_rsrc_t rsA = make_rsrc(A, (unsigned)(rowsA * lda * 2));
  const __amdgpu_buffer_rsrc_t rsB = make_rsrc(B, (unsigned)(rowsB * ldb * 2));

  // DMA piece pc = j * 8 + wave (1 KiB = 8 rows of an image); the A image takes the first MI of the 4 j-steps
  unsigned voffA[MI], voffB[4];
  int kel[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = (j * 8 + wave) * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ ((row >> 1) & 7);
    if (j < MI) voffA[j] = (unsigned)(row * lda * 2 + chunk * 16);
    voffB[j] = (unsigned)(row * ldb * 2 + chunk * 16);
    kel[j] = chunk * 8;
  }
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ni][mi][r] = 0.f;
  auto stage = [&](int buf, int k0) {
    char* sA = smem + buf * STAGE;
    char* sB = sA + IMG_A;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int pc = j * 8 + wave;
      const unsigned oob = (k0 + kel[j] >= K) ? 0x80000000u : 0u;
      if (j < MI) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, LDS_PTR(sA + pc * 1024), 16, voffA[j] | oob, k0 * 2, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, LDS_PTR(sB + pc * 1024), 16, voffB[j] | oob, k0 * 2, 0, 0);
    }
  };
  const int sw = (l31 >> 1) & 7;
  const int rowoffA = (wm * MI * 32 + l31) * 128;
  const int rowoffB = (wn * 64 + l31) * 128;
  const int nkt = (K + BK - 1) / BK;
  stage(0, 0);
  for (int kt = 0; kt < nkt; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nkt) stage((kt + 1) & 1, (kt + 1) * BK);
    const char* sA = smem + (kt & 1) * STAGE;
    const char* sB = sA + IMG_A;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int coff = ((2 * ks + hi) ^ sw) << 4;
      bf16x8 fa[MI], fb[2];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) fa[mi] = *(const bf16x8*)(sA + rowoffA + mi * 4096 + coff);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) fb[ni] = *(const bf16x8*)(sB + rowoffB + ni * 4096 + coff);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
          acc[ni][mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[ni], fa[mi], acc[ni][mi], 0, 0, 0);
    }
  }
}

}  // namespace clipa_gemm
