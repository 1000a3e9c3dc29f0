// Multi-caption image-text retrieval ranks (clipa_jax/evaluators/proj/image_text/image_text_retrieval.py,
// image_to_text_retrieval_eval / text_to_image_retrieval_eval) without the [Ni, Nt] similarity matrix.  Image features
// A [Ni, E], text features B [Nt, E], text t describes image c(t); v_it = fl(s * x_it), x_it = A_i . B_t in fp32:
//   p_t = v_{c(t), t}   m_i = max over {t : c(t) = i} of p_t (-inf: image i has no caption)
//   t2i_gt[t] = #{i : v_it > p_t}   t2i_eq[t] = #{i != c(t) : v_it == p_t}          (column t, text -> image)
//   i2t_gt[i] = #{t : v_it > m_i}   i2t_eq[i] = #{t : c(t) != i, v_it == m_i}       (row i, image -> text)
// i2t_gt is the 0-based position of image i's best caption (its other captions cannot beat m_i), t2i_gt that of text
// t's image; ties resolve in the positive's favour, as in retrieval.hip.
//
// Arithmetic: rank_tile below, the main loop of retrieval.hip's kernel kept instruction for instruction in the same k order
// (one ascending-k fp32 MFMA chain per output, no split-K; tests/test_retrieval_multi_gpu.py checks the two agree bit for
// bit), so every x_it - the positives included - comes out of the same code whichever launch or tile computes it.  Three launches:
//   init: counts = 0, p_t = NaN, m_i = key(-inf);
//   POS:  one workgroup per 128-text tile, over the image tiles [min c, max c] of its texts (tiles that hold none of their
//         images skipped): writes p_t and takes m_i by an integer atomicMax on an order-preserving key of the float.
//         Sorted c (the captions of an image adjacent) makes this about Ti + Tt tiles;
//   count: every Ti x Tt tile; the epilogue counts against m_i (rows) and p_t (columns), c of the tile's columns gives the
//         eq exclusions, reduces as retrieval.hip does and adds one int per row and per column of the tile atomically.
// Memory: O(Ni + Nt) (the workspace is p_t and the keys of m_i).
#include "gemm_common.h"

namespace clipa_gemm {
namespace {

constexpr int RT = 128;                       // output tile (rows of A and of B)
constexpr int RK = 32;                        // k per stage
constexpr int RTHREADS = 256;
constexpr int R_IMG = RT * RK * 4;            // one operand image: 16 KiB
constexpr int R_STAGE = 2 * R_IMG;

// 8-byte slot swizzle of image row r: a bijection of 0..15 over any 16 consecutive rows that also differs between r and r + 16
__device__ __forceinline__ int swz(int r) { return (r & 15) ^ ((r >> 4) & 1); }

// acc[mi][ni] = the 32 x 32 block (mi, ni) of this wave's 64 x 64 quarter of the 128 x 128 tile of A rows (rsA) times B
// rows (rsB), rows past a resource's range and k >= E reading 0.  Uses the first 2 * R_STAGE bytes of smem; the caller
// synchronises before reusing them.
// D fragment: lane holds column j = wn*64 + ni*32 + L and rows i = wm*64 + mi*32 + (r&3) + 8*(r>>2) + 4*hi of the tile.
__device__ __forceinline__ void rank_tile(char* smem, __amdgpu_buffer_rsrc_t rsA, __amdgpu_buffer_rsrc_t rsB, long lda,
                                          long ldb, int E, f32x16 (&acc)[2][2]) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = lane & 31, hi = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;   // wave tile: 64 (i) x 64 (j)

  // DMA piece pc (256 B = two rows of the image) = 16 j-steps x 4 waves; lane -> row 2 pc + hi, dword L of the row:
  // 8-byte slot L / 2 holds pair (slot ^ swz(row)) = (q, h), element L & 1 is k = 4q + h + 2 (L & 1).
  int kel[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int pr = (L >> 1) ^ swz(8 * j + 2 * wave + hi);
    kel[j] = 4 * (pr >> 1) + (pr & 1) + 2 * (L & 1);
  }
  const unsigned rowA0 = (unsigned)((2 * wave + hi) * lda * 4), rowB0 = (unsigned)((2 * wave + hi) * ldb * 4);
  const unsigned stepA = (unsigned)(8 * lda * 4), stepB = (unsigned)(8 * ldb * 4);

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
      const unsigned oob = k >= E ? 0x80000000u : 0u;   // ragged E: the buffer range check returns 0
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, LDS_PTR(sA + pc * 256), 4, (rowA0 + j * stepA + k * 4) | oob, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, LDS_PTR(sB + pc * 256), 4, (rowB0 + j * stepB + k * 4) | oob, 0, 0, 0);
    }
  };

  const int sw = swz(L);                      // fragment rows start at multiples of 32
  const int rowoffA = (wm * 64 + L) * 128;
  const int rowoffB = (wn * 64 + L) * 128;
  const int nkt = (E + RK - 1) / RK;
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
}

struct MultiArgs {
  const char* A; const char* B; const int* c;
  int Ni, Nt, E;
  long lda, ldb;                              // elements
  const float* scale;
  float* pos;                                 // [Nt] p_t
  unsigned* mkey;                             // [Ni] key(m_i)
  int* i2t_gt; int* i2t_eq; int* t2i_gt; int* t2i_eq;
};

// order-preserving map float -> unsigned (a < b  <=>  key(a) < key(b) for non-NaN a, b; -0 < +0) and its inverse
__device__ __forceinline__ unsigned fkey(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float fdekey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? k & 0x7fffffffu : ~k); }

__global__ __launch_bounds__(RTHREADS) void multi_init_kernel(MultiArgs p) {
  const int g = blockIdx.x * RTHREADS + threadIdx.x;
  if (g < p.Ni) { p.mkey[g] = fkey(-__builtin_huge_valf()); p.i2t_gt[g] = 0; p.i2t_eq[g] = 0; }
  if (g < p.Nt) { p.pos[g] = __builtin_nanf(""); p.t2i_gt[g] = 0; p.t2i_eq[g] = 0; }
}

template <bool POS>
__global__ __launch_bounds__(RTHREADS, 2) void retrieval_multi_kernel(MultiArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = lane & 31, hi = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const int Tt = (p.Nt + RT - 1) / RT;
  const int tm0 = POS ? 0 : blockIdx.x / Tt;
  const int tn = POS ? blockIdx.x : blockIdx.x - tm0 * Tt;
  const int n0 = tn * RT;
  const int rowsB = min(RT, p.Nt - n0);
  const __amdgpu_buffer_rsrc_t rsB = make_rsrc(p.B + (size_t)n0 * p.ldb * 4, (unsigned)(rowsB * p.ldb * 4));
  const float s = p.scale ? p.scale[0] : 1.0f;
  // c of this lane's two accumulator columns (-1 past Nt); only ever compared, never used as an index
  int cj[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int jl = wn * 64 + ni * 32 + L;
    cj[ni] = jl < rowsB ? p.c[n0 + jl] : -1;
  }
  f32x16 acc[2][2];

  if (POS) {
    // image-tile range of this tile's texts; values outside [0, Ni) are ignored (their p_t stays NaN)
    __shared__ int srange[2];
    const int ct = tid < rowsB ? p.c[n0 + tid] : -1;
    const bool valid = ct >= 0 && ct < p.Ni;
    if (tid == 0) { srange[0] = 0x7fffffff; srange[1] = -1; }
    __syncthreads();
    if (valid) { atomicMin(&srange[0], ct / RT); atomicMax(&srange[1], ct / RT); }
    __syncthreads();
    const int lo = srange[0], hi_t = srange[1];
    for (int tm = lo; tm <= hi_t; ++tm) {
      // doubles as the barrier before the ring is staged again
      if (!__syncthreads_or(valid && ct / RT == tm)) continue;
      const int m0 = tm * RT;
      const int rowsA = min(RT, p.Ni - m0);
      const __amdgpu_buffer_rsrc_t rsA = make_rsrc(p.A + (size_t)m0 * p.lda * 4, (unsigned)(rowsA * p.lda * 4));
      rank_tile(smem, rsA, rsB, p.lda, p.ldb, p.E, acc);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = m0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
            if (cj[ni] == i && i < p.Ni) {      // rows past Ni: a bad c must not reach them
              const float v = s * acc[mi][ni][r];
              p.pos[n0 + wn * 64 + ni * 32 + L] = v;
              atomicMax(p.mkey + i, fkey(v));
            }
        }
    }
    return;
  }

  const int m0 = tm0 * RT;
  const int rowsA = min(RT, p.Ni - m0);
  const __amdgpu_buffer_rsrc_t rsA = make_rsrc(p.A + (size_t)m0 * p.lda * 4, (unsigned)(rowsA * p.lda * 4));
  // the positives of this tile's rows (tid < 128: m_i) and columns (p_t): loaded now, used in the epilogue
  float dpos = 0.f;
  if (tid < RT) {
    if (tid < rowsA) dpos = fdekey(p.mkey[m0 + tid]);
  } else if (tid - RT < rowsB) {
    dpos = p.pos[n0 + tid - RT];
  }
  rank_tile(smem, rsA, rsB, p.lda, p.ldb, p.E, acc);

  __syncthreads();                            // the ring is dead: reuse its first bytes
  float* dpl = (float*)smem;                  // [256]: positives of the tile's rows, then of its columns
  int* rowp = (int*)(smem + 1024);            // [2 wn][128]  packed gt | eq << 16 per row
  int* colp = rowp + 2 * RT;                  // [2 wm][128]  per column
  dpl[tid] = dpos;
  __syncthreads();

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
        const bool ok = jl < rowsB && il < rowsA;
        const bool other = cj[ni] != m0 + il;  // eq counts entries that are not the text's own image
        c += ok ? (int)(v > drow) + ((int)(other && v == drow) << 16) : 0;
        cc[ni] += ok ? (int)(v > dcol[ni]) + ((int)(other && v == dcol[ni]) << 16) : 0;
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
    if (tid < rowsA) {
      if (v & 0xffff) atomicAdd(p.i2t_gt + m0 + tid, v & 0xffff);
      if (v >> 16) atomicAdd(p.i2t_eq + m0 + tid, v >> 16);
    }
  } else {
    const int t = tid - RT;
    const int v = colp[t] + colp[RT + t];
    if (t < rowsB) {
      if (v & 0xffff) atomicAdd(p.t2i_gt + n0 + t, v & 0xffff);
      if (v >> 16) atomicAdd(p.t2i_eq + n0 + t, v >> 16);
    }
  }
}

std::once_flag g_rkm_once[MAX_DEVICES];
int g_rkm_rc[MAX_DEVICES];
int ensure_rkm_attrs(int dev) {
  std::call_once(g_rkm_once[dev], [dev]() {
    g_rkm_rc[dev] = 0;
    const void* ks[2] = {(const void*)retrieval_multi_kernel<true>, (const void*)retrieval_multi_kernel<false>};
    for (int i = 0; i < 2; ++i) {
      const hipError_t e = hipFuncSetAttribute(ks[i], hipFuncAttributeMaxDynamicSharedMemorySize, 2 * R_STAGE);
      if (e != hipSuccess) { clipa_set_error("hipFuncSetAttribute(retrieval_multi): %s", hipGetErrorString(e)); g_rkm_rc[dev] = CLIPA_ERR_LAUNCH; }
    }
  });
  return g_rkm_rc[dev];
}

}  // namespace
}  // namespace clipa_gemm

using namespace clipa_gemm;

static int64_t round4(int64_t n) { return ((n > 0 ? n : 1) + 3) / 4 * 4; }

extern "C" int64_t clipa_retrieval_ranks_multi_workspace(int64_t Ni, int64_t Nt) {
  return (round4(Nt) + round4(Ni)) * (int64_t)sizeof(float);          // p_t, key(m_i)
}

extern "C" int clipa_retrieval_ranks_multi(const float* A, const float* B, const int32_t* txt2img, int64_t Ni, int64_t Nt,
                                           int64_t E, int64_t lda, int64_t ldb, const float* scale, int32_t* i2t_gt,
                                           int32_t* i2t_eq, int32_t* t2i_gt, int32_t* t2i_eq, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
  if (Ni < 1 || Nt < 1 || E < 1) {
    clipa_set_error("retrieval_ranks_multi: Ni = %ld, Nt = %ld and E = %ld must be >= 1", (long)Ni, (long)Nt, (long)E);
    return CLIPA_ERR_ARG;
  }
  if (lda < E || ldb < E || lda % 4 != 0 || ldb % 4 != 0) {
    clipa_set_error("retrieval_ranks_multi: lda = %ld and ldb = %ld must be >= E = %ld and multiples of 4", (long)lda, (long)ldb, (long)E);
    return CLIPA_ERR_ARG;
  }
  const int64_t Ti = (Ni + RT - 1) / RT, Tt = (Nt + RT - 1) / RT;
  if ((int64_t)RT * lda * 4 >= (1L << 30) || (int64_t)RT * ldb * 4 >= (1L << 30) || Ni >= (1L << 30) || Nt >= (1L << 30) ||
      Ti * Tt >= (1L << 31)) {
    clipa_set_error("retrieval_ranks_multi: Ni, Nt or leading dimension too large");
    return CLIPA_ERR_ARG;
  }
  const void* ptrs[8] = {A, B, txt2img, i2t_gt, i2t_eq, t2i_gt, t2i_eq, workspace};
  for (int i = 0; i < 8; ++i)
    if (!ptrs[i] || ((uintptr_t)ptrs[i] & 15)) { clipa_set_error("retrieval_ranks_multi: pointer argument %d is null or not 16-byte aligned", i); return CLIPA_ERR_ARG; }
  if (((uintptr_t)scale & 3)) { clipa_set_error("retrieval_ranks_multi: scale is not 4-byte aligned"); return CLIPA_ERR_ARG; }
  if (workspace_bytes < clipa_retrieval_ranks_multi_workspace(Ni, Nt)) { clipa_set_error("retrieval_ranks_multi: workspace too small"); return CLIPA_ERR_ARG; }
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (int rc = ensure_rkm_attrs(dev)) return rc;
  MultiArgs a = {};
  a.A = (const char*)A; a.B = (const char*)B; a.c = txt2img; a.Ni = (int)Ni; a.Nt = (int)Nt; a.E = (int)E;
  a.lda = lda; a.ldb = ldb; a.scale = scale;
  a.pos = (float*)workspace; a.mkey = (unsigned*)((char*)workspace + round4(Nt) * sizeof(float));
  a.i2t_gt = i2t_gt; a.i2t_eq = i2t_eq; a.t2i_gt = t2i_gt; a.t2i_eq = t2i_eq;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nmax = Ni > Nt ? Ni : Nt;
  hipLaunchKernelGGL(multi_init_kernel, dim3((unsigned)((nmax + RTHREADS - 1) / RTHREADS)), dim3(RTHREADS), 0, st, a);
  if (int rc = clipa_check_launch("retrieval_multi_init")) return rc;
  hipLaunchKernelGGL(retrieval_multi_kernel<true>, dim3((unsigned)Tt), dim3(RTHREADS), 2 * R_STAGE, st, a);
  if (int rc = clipa_check_launch("retrieval_multi_positives")) return rc;
  hipLaunchKernelGGL(retrieval_multi_kernel<false>, dim3((unsigned)(Ti * Tt)), dim3(RTHREADS), 2 * R_STAGE, st, a);
  return clipa_check_launch("retrieval_ranks_multi");
}
