// Retrieval ranks of the validation metrics (get_clip_metrics, clipa_torch/training/train.py:432-449) without the
// [N, N] logit matrix: v_ij = fl(s * x_ij), x_ij = A_i . B_j in fp32, and per image row i / text column j the number of
// OTHER entries of that row / column that beat (gt) or tie (eq) the positive v_ii / v_jj.  The reference's 0-based rank
// of the positive from an unstable descending argsort lies in [gt, gt + eq]; the engine reports gt (ties resolved in the
// positive's favour, deterministically).
//
// Arithmetic: v_mfma_f32_32x32x2_f32, one accumulator chain per output in ascending k (bit for bit a chain of fp32 fmaf),
// no split-K.  Every x_ij - the diagonal included - comes out of the same code, so v_ii compares with itself exactly:
//   launch 1 (DIAG): the diagonal tiles only; writes v_ii to the workspace and zeroes the four count arrays of its rows;
//   launch 2: every tile; the epilogue counts v_ij > / == v_ii (row i) and v_jj (column j), i != j excluded, reduces
//             within the wave and across waves in LDS and adds one int per row and per column of the tile atomically.
// Memory: O(N) (the workspace is N floats).
//
// Tile 128 x 128, 4 waves as 2 x 2, each wave 2 x 2 accumulators of 32 x 32; k-chunks of 32 fp32 staged by 4-byte LDS-DMA
// into a double-buffered ring (2 x 32 KiB: two workgroups per CU).  The per-dword DMA lets the LDS image put, for each row,
// the pair {k = 4q + h, 4q + 2 + h} of lane half h in one 8-byte slot: one ds_read_b64 feeds two consecutive MFMA k-steps,
// and the slot index is XOR-swizzled with the row (swz below) so 16 consecutive rows hit 16 distinct slots and the 32 rows of a
// lane half 32 distinct bank pairs: conflict-free as ds_read_b64 and as the ds_read2st64_b64 hipcc pairs them into.
#include "gemm_common.h"

namespace clipa_gemm {
namespace {

constexpr int RT = 128;                       // output tile (rows of A and of B)
constexpr int RK = 32;                        // k per stage
constexpr int RTHREADS = 256;
constexpr int R_IMG = RT * RK * 4;            // one operand image: 16 KiB
constexpr int R_STAGE = 2 * R_IMG;

struct RankArgs {
  const char* A; const char* B;
  int N, E;
  long lda, ldb;                              // elements
  const float* scale;
  float* diag;                                // [N] v_ii
  int* i2t_gt; int* i2t_eq; int* t2i_gt; int* t2i_eq;
};

// 8-byte slot swizzle of image row r: a bijection of 0..15 over any 16 consecutive rows that also differs between r and r + 16
__device__ __forceinline__ int swz(int r) { return (r & 15) ^ ((r >> 4) & 1); }

template <bool DIAG>
__global__ __launch_bounds__(RTHREADS, 2) void retrieval_kernel(RankArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = lane & 31, hi = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;   // wave tile: 64 (i) x 64 (j)
  const int T = (p.N + RT - 1) / RT;
  int tm, tn;
  if (DIAG) {
    tm = tn = blockIdx.x;
  } else {
    tm = blockIdx.x / T;
    tn = blockIdx.x - tm * T;
  }
  const int m0 = tm * RT, n0 = tn * RT;
  const int rowsA = min(RT, p.N - m0), rowsB = min(RT, p.N - n0);
  const __amdgpu_buffer_rsrc_t rsA = make_rsrc(p.A + (size_t)m0 * p.lda * 4, (unsigned)(rowsA * p.lda * 4));
  const __amdgpu_buffer_rsrc_t rsB = make_rsrc(p.B + (size_t)n0 * p.ldb * 4, (unsigned)(rowsB * p.ldb * 4));

  // the positives of this tile's rows (tid < 128) and columns: loaded now, used in the epilogue
  float dpos = 0.f;
  if (!DIAG) {
    const int g = tid < RT ? m0 + tid : n0 + tid - RT;
    if (g < p.N) dpos = p.diag[g];
  }

  // DMA piece pc (256 B = two rows of the image) = 16 j-steps x 4 waves; lane -> row 2 pc + hi, dword L of the row:
  // 8-byte slot L / 2 holds pair (slot ^ swz(row)) = (q, h), element L & 1 is k = 4q + h + 2 (L & 1).
  int kel[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int pr = (L >> 1) ^ swz(8 * j + 2 * wave + hi);
    kel[j] = 4 * (pr >> 1) + (pr & 1) + 2 * (L & 1);
  }
  const unsigned rowA0 = (unsigned)((2 * wave + hi) * p.lda * 4), rowB0 = (unsigned)((2 * wave + hi) * p.ldb * 4);
  const unsigned stepA = (unsigned)(8 * p.lda * 4), stepB = (unsigned)(8 * p.ldb * 4);

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  auto stage = [&](int buf, int k0) {
    char* sA = smem + buf * R_STAGE;
    char* sB = sA + R_IMG;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int pc = 4 * j + wave;
      const int k = k0 + kel[j & 3];
      const unsigned oob = k >= p.E ? 0x80000000u : 0u;   // ragged E: the buffer range check returns 0
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, LDS_PTR(sA + pc * 256), 4, (rowA0 + j * stepA + k * 4) | oob, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, LDS_PTR(sB + pc * 256), 4, (rowB0 + j * stepB + k * 4) | oob, 0, 0, 0);
    }
  };

  const int sw = swz(L);                      // fragment rows start at multiples of 32
  const int rowoffA = (wm * 64 + L) * 128;
  const int rowoffB = (wn * 64 + L) * 128;
  const int nkt = (p.E + RK - 1) / RK;
  stage(0, 0);
  for (int kt = 0; kt < nkt; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nkt) stage((kt + 1) & 1, (kt + 1) * RK);
    const char* sA = smem + (kt & 1) * R_STAGE;
    const char* sB = sA + R_IMG;
#pragma unroll
    for (int q = 0; q < RK / 4; ++q) {
      const int off = ((2 * q + hi) ^ sw) * 8;
      f32x2 fa[2], fb[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) fa[mi] = *(const f32x2*)(sA + rowoffA + mi * 32 * 128 + off);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) fb[ni] = *(const f32x2*)(sB + rowoffB + ni * 32 * 128 + off);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[mi].x, fb[ni].x, acc[mi][ni], 0, 0, 0);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[mi].y, fb[ni].y, acc[mi][ni], 0, 0, 0);
    }
  }

  // D fragment: lane holds column j = n0 + wn*64 + ni*32 + L and rows i = m0 + wm*64 + mi*32 + (r&3) + 8*(r>>2) + 4*hi
  const float s = p.scale ? p.scale[0] : 1.0f;
  if (DIAG) {
    // zero the counts of this tile's rows, write v_ii
    if (tid < RT && m0 + tid < p.N) {
      p.i2t_gt[m0 + tid] = 0; p.i2t_eq[m0 + tid] = 0; p.t2i_gt[m0 + tid] = 0; p.t2i_eq[m0 + tid] = 0;
    }
    if (wm == wn) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int il = mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
          const int i = m0 + wm * 64 + il;
          if (il == mi * 32 + L && i < p.N) p.diag[i] = s * acc[mi][mi][r];
        }
    }
    return;
  }

  __syncthreads();                            // the ring is dead: reuse its first bytes
  float* dpl = (float*)smem;                  // [256]: positives of the tile's rows, then of its columns
  int* rowp = (int*)(smem + 1024);            // [2 wn][128]  packed gt | eq << 16 per row
  int* colp = rowp + 2 * RT;                  // [2 wm][128]  per column
  dpl[tid] = dpos;
  __syncthreads();

  const bool dtile = tm == tn;
  float dcol[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) dcol[ni] = dpl[RT + wn * 64 + ni * 32 + L];
  int rc[32];                                 // per (mi, r): this lane's packed row counts over its two columns
  int cc[2] = {0, 0};                         // per ni: packed column counts over this lane's 32 rows
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int il = wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      const float drow = dpl[il];
      int c = 0;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int jl = wn * 64 + ni * 32 + L;
        const float v = s * acc[mi][ni][r];
        const bool keep = !dtile || il != jl;
        const bool ok = keep && n0 + jl < p.N && m0 + il < p.N;
        c += ok ? (int)(v > drow) + ((int)(v == drow) << 16) : 0;
        cc[ni] += ok ? (int)(v > dcol[ni]) + ((int)(v == dcol[ni]) << 16) : 0;
      }
      rc[mi * 16 + r] = c;
    }
  // rows: sum over the 32 lanes of each half; recursive halving leaves lane L with the total of value index L
#pragma unroll
  for (int b = 16; b >= 1; b >>= 1) {
    const bool up = (L & b) != 0;
#pragma unroll
    for (int c = 0; c < b; ++c) {
      const int send = up ? rc[c] : rc[c + b];
      const int keep = up ? rc[c + b] : rc[c];
      rc[c] = keep + __shfl_xor(send, b, 64);
    }
  }
  {
    const int r = L & 15;
    rowp[wn * RT + wm * 64 + (L >> 4) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi] = rc[0];
  }
  // columns: add the other lane half
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) cc[ni] += __shfl_xor(cc[ni], 32, 64);
  colp[wm * RT + wn * 64 + hi * 32 + L] = hi ? cc[1] : cc[0];
  __syncthreads();
  if (tid < RT) {
    const int v = rowp[tid] + rowp[RT + tid];
    const int i = m0 + tid;
    if (i < p.N) {
      if (v & 0xffff) atomicAdd(p.i2t_gt + i, v & 0xffff);
      if (v >> 16) atomicAdd(p.i2t_eq + i, v >> 16);
    }
  } else {
    const int t = tid - RT;
    const int v = colp[t] + colp[RT + t];
    const int j = n0 + t;
    if (j < p.N) {
      if (v & 0xffff) atomicAdd(p.t2i_gt + j, v & 0xffff);
      if (v >> 16) atomicAdd(p.t2i_eq + j, v >> 16);
    }
  }
}

std::once_flag g_rk_once[MAX_DEVICES];
int g_rk_rc[MAX_DEVICES];
int ensure_rk_attrs(int dev) {
  std::call_once(g_rk_once[dev], [dev]() {
    g_rk_rc[dev] = 0;
    const void* ks[2] = {(const void*)retrieval_kernel<true>, (const void*)retrieval_kernel<false>};
    for (int i = 0; i < 2; ++i) {
      const hipError_t e = hipFuncSetAttribute(ks[i], hipFuncAttributeMaxDynamicSharedMemorySize, 2 * R_STAGE);
      if (e != hipSuccess) { clipa_set_error("hipFuncSetAttribute(retrieval): %s", hipGetErrorString(e)); g_rk_rc[dev] = CLIPA_ERR_LAUNCH; }
    }
  });
  return g_rk_rc[dev];
}

}  // namespace
}  // namespace clipa_gemm

using namespace clipa_gemm;

extern "C" int64_t clipa_retrieval_ranks_workspace(int64_t N) {
  return (N > 0 ? N : 1) * (int64_t)sizeof(float);          // v_ii
}

extern "C" int clipa_retrieval_ranks(const float* A, const float* B, int64_t N, int64_t E, int64_t lda, int64_t ldb,
                                     const float* scale, int32_t* i2t_gt, int32_t* i2t_eq, int32_t* t2i_gt,
                                     int32_t* t2i_eq, void* workspace, int64_t workspace_bytes, void* stream) {
  if (N < 1 || E < 1) { clipa_set_error("retrieval_ranks: N = %ld and E = %ld must be >= 1", (long)N, (long)E); return CLIPA_ERR_ARG; }
  if (lda < E || ldb < E || lda % 4 != 0 || ldb % 4 != 0) {
    clipa_set_error("retrieval_ranks: lda = %ld and ldb = %ld must be >= E = %ld and multiples of 4", (long)lda, (long)ldb, (long)E);
    return CLIPA_ERR_ARG;
  }
  if ((int64_t)RT * lda * 4 >= (1L << 30) || (int64_t)RT * ldb * 4 >= (1L << 30) || N >= (1L << 30)) {
    clipa_set_error("retrieval_ranks: N or leading dimension too large");
    return CLIPA_ERR_ARG;
  }
  const void* ptrs[7] = {A, B, i2t_gt, i2t_eq, t2i_gt, t2i_eq, workspace};
  for (int i = 0; i < 7; ++i)
    if (!ptrs[i] || ((uintptr_t)ptrs[i] & 15)) { clipa_set_error("retrieval_ranks: pointer argument %d is null or not 16-byte aligned", i); return CLIPA_ERR_ARG; }
  if (((uintptr_t)scale & 3)) { clipa_set_error("retrieval_ranks: scale is not 4-byte aligned"); return CLIPA_ERR_ARG; }
  if (workspace_bytes < clipa_retrieval_ranks_workspace(N)) { clipa_set_error("retrieval_ranks: workspace too small"); return CLIPA_ERR_ARG; }
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (int rc = ensure_rk_attrs(dev)) return rc;
  const int64_t T = (N + RT - 1) / RT;
  RankArgs a = {};
  a.A = (const char*)A; a.B = (const char*)B; a.N = (int)N; a.E = (int)E; a.lda = lda; a.ldb = ldb; a.scale = scale;
  a.diag = (float*)workspace; a.i2t_gt = i2t_gt; a.i2t_eq = i2t_eq; a.t2i_gt = t2i_gt; a.t2i_eq = t2i_eq;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(retrieval_kernel<true>, dim3((unsigned)T), dim3(RTHREADS), 2 * R_STAGE, st, a);
  if (int rc = clipa_check_launch("retrieval_diag")) return rc;
  hipLaunchKernelGGL(retrieval_kernel<false>, dim3((unsigned)(T * T)), dim3(RTHREADS), 2 * R_STAGE, st, a);
  return clipa_check_launch("retrieval_ranks");
}
