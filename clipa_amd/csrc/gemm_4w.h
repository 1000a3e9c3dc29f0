// Scaffolding shared by the four-wave, hand-scheduled GEMM kernels: gemm_nta.hip / gemm_f8a.hip (the NT pair: forward and
// input gradient, bf16 and fp8) and gemm_tna.hip / gemm_tn8.hip (the TN pair: weight gradient, bf16 and fp8).  One wave per
// SIMD, a 128 x 128 wave tile in a[0:255], the K loop of a tile ONE generated inline-asm statement (tools/gen_gemm_*.py ->
// gemm_*_asm.inc).  Here: the accumulator read, the NT pair's output descriptor, store guard, operand ring, marker-bracketed
// epilogue with its per-activation dispatch, "no epilogue" ablation and persistent grid, and the TN pair's fp32 tile store.
// In the four sources: the statement's operand list, the per-chunk epilogue arithmetic (nta_chunk / f8a_chunk: worth reading
// side by side), each kernel's extras - and the tile walk, lane_consts, the per-tile fill of the descriptor, the e4m3 table
// builder and the TN tile / slice selection, which are still per-file copies: moved here, each of them made hipcc order or
// allocate some instantiation differently, and in these kernels identical device code is worth more than the lines
// (profiles/four_wave_shared_isa.md).  Everything here is __forceinline__ and leaves the device code as it was.
#pragma once
#include "gemm_common.h"
#include <type_traits>
#include <utility>

namespace clipa_gemm {
namespace {      // internal linkage, as the copies in the four sources had: every function here is inlined into its kernels

// The accumulators live in a[0:255] between the tile statement and these reads, which hipcc does not know: the build audits the
// ISA for scratch and for compiler-generated v_accvgpr_* (clipa_amd/isa_audit.py).
template <int IDX>
__device__ __forceinline__ float acc_rd() {
  float x;
  asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(x) : "n"(IDX));
  return x;
}

// ===================================================================================================================
// The NT pair
// ===================================================================================================================

// The weight-row permutation.  The LDS-DMA of the weight operand permutes the rows inside each 32-row group - LDS row R holds
// weight row 8 ((R & 15) >> 2) + 4 ((R >> 4) & 1) + (R & 3) (browB in the kernels' lane_consts) - so that a lane's accumulators
// of two neighbouring 16 x 16 blocks are 8 consecutive output features: one 16-byte store straight from the registers, no LDS
// epilogue window and no epilogue barriers.  That is what makes a "chunk" below.

// Where a lane's 32 chunks of the tile go and where its second operand comes from.  Chunk I = 4 ai + p: rows 16 ai + (lane & 15)
// of the wave's 128, output features 32 p + 8 (lane >> 4) .. +7.  The kernels derive their descriptor from it, add their extras and fill it per tile.
struct Out4w {
  __amdgpu_buffer_rsrc_t rsC, rsC2, rsAux;
  unsigned lane_c, lane_aux;     // byte offset of this lane's chunk (ai = 0, p = 0) inside the tile
  unsigned row16_c, row16_aux;   // bytes per 16 rows
  unsigned lane_c2, row16_c2;    // the same at 1 byte per element (e4m3 outputs)
  int act;
};

// gfx950: a 16-byte store reads its data registers over several cycles after it issues; a VALU instruction that overwrites the
// third or fourth of them in the very next slot wins the race (profiles/NOTEBOOK.md 7c; observed in gemm_f8a: lanes 12-15 of
// every 16 stored the NEXT chunk's scale product; hipcc does not model the hazard when the store has an SGPR offset, and the
// accumulator reads are inline asm it cannot see into).  The guard reads the four registers after the store, so the next writer
// is at least one instruction away; clipa_amd/isa_audit.py rejects the pattern in the ISA of the audited kernels.  ON = false:
// instantiations that never produce the pattern (the audit checks every one) keep their instruction streams.
template <bool ON>
__device__ __forceinline__ void store_guard(const u32x4& v) {
  if constexpr (ON) asm volatile("s_nop 0" : : "v"(v) : "memory");
}

// Residual / pre-activation operand of the epilogue: the lane's 32 chunks, 16 bytes each as bf16, 8 as e4m3 (AUX8), loaded
// straight into registers (the 128 fragment registers are idle in the epilogue).
// The ring rule: RING chunks are requested before the first one is consumed; chunk I + RING is requested as soon as chunk I has
// been consumed.  A load requested behind a store waits for that store's acknowledgement (vmcnt counts in order), so where the
// registers are there the ring holds all 32 (the kernels' *_ring() give the depth per instantiation and say what was measured).
template <bool AUX8>
using Aux4w = std::conditional_t<AUX8, u32x2, u32x4>;

template <bool AUX8, int I>
__device__ __forceinline__ Aux4w<AUX8> aux_load(const Out4w& o) {
  constexpr int AI = I >> 2, P = I & 3;
  if constexpr (AUX8) return __builtin_amdgcn_raw_buffer_load_b64(o.rsAux, (int)(o.lane_aux + P * 32), (int)(AI * o.row16_aux), 0);
  else return __builtin_amdgcn_raw_buffer_load_b128(o.rsAux, (int)(o.lane_aux + P * 64), (int)(AI * o.row16_aux), 0);
}

template <bool AUX8, int RING, int... Js>
__device__ __forceinline__ void aux_first(const Out4w& o, Aux4w<AUX8> (&av)[RING], std::integer_sequence<int, Js...>) {
  ((av[Js] = aux_load<AUX8, Js>(o)), ...);
}

// The tile epilogue, generic over the per-chunk routine.  CHUNK names the kernel's routine and what the plumbing has to know:
//   static constexpr int EPI, RING; static constexpr bool AUX8;
//   template <int ACT, int I> static void run(const Out& o, X&... x, const Aux4w<AUX8>& aux);
// x... are the kernel's per-tile operands (gemm_nta: bias; gemm_f8a: sam, sb, bias, som, cs), passed through by reference.
template <typename CHUNK, int ACT, int I, typename Out, typename... X>
__device__ __forceinline__ void chunk_roll(const Out& o, Aux4w<CHUNK::AUX8> (&av)[CHUNK::RING], X&... x) {
  constexpr int RING = CHUNK::RING;
  CHUNK::template run<ACT, I>(o, x..., av[I % RING]);
  if constexpr (I + RING < 32) av[I % RING] = aux_load<CHUNK::AUX8, I + RING>(o);
}

// One straight-line copy of the 32 chunks.  The marker rule: the copy sits between two comments in the ISA, unique per copy so
// that hipcc cannot tail-merge a store across them; clipa_amd/isa_audit.py counts the 16-byte stores between them against what
// the tile statement's vmcnt assumes.
template <typename CHUNK, int ACT, int... Is, typename Out, typename... X>
__device__ __forceinline__ void epilogue_act(std::integer_sequence<int, Is...>, const Out& o, X&... x) {
  constexpr bool HAS_AUX = CHUNK::EPI == CLIPA_EPI_ADD || CHUNK::EPI == CLIPA_EPI_DACT;
  asm volatile("; CLIPA_EPI_BEGIN %0" ::"n"(ACT));
  if constexpr (HAS_AUX) {
    Aux4w<CHUNK::AUX8> av[CHUNK::RING];
    aux_first<CHUNK::AUX8>(o, av, std::make_integer_sequence<int, CHUNK::RING>{});
    (chunk_roll<CHUNK, ACT, Is>(o, av, x...), ...);
  } else {
    const Aux4w<CHUNK::AUX8> none = {};
    (CHUNK::template run<ACT, Is>(o, x..., none), ...);
  }
  asm volatile("; CLIPA_EPI_END %0" ::"n"(ACT));
}

// the activation is a run-time argument of the C ABI: one straight-line copy of the tile epilogue per activation
template <typename CHUNK, typename Out, typename... X>
__device__ __forceinline__ void epilogue_4w(const Out& o, X&... x) {
  constexpr auto seq = std::make_integer_sequence<int, 32>{};
  if constexpr (CHUNK::EPI == CLIPA_EPI_ACT || CHUNK::EPI == CLIPA_EPI_DACT) {
    if (o.act == ACT_GELU_ERF) epilogue_act<CHUNK, ACT_GELU_ERF>(seq, o, x...);
    else if (o.act == ACT_GELU_TANH) epilogue_act<CHUNK, ACT_GELU_TANH>(seq, o, x...);
    else epilogue_act<CHUNK, ACT_QUICK_GELU>(seq, o, x...);
  } else {
    epilogue_act<CHUNK, ACT_GELU_ERF>(seq, o, x...);
  }
}

// Ablation "no epilogue" (clipa_internal_debug_set flag 2): main loop only; keeps the accumulators observable.  (The address is
// built here, from an opaque copy of the thread id, not hoisted into a register that lives across the loop.)
__device__ __forceinline__ void acc_keep_observable(char* C, int tid, float v) {
  int t3 = tid;
  asm volatile("" : "+v"(t3));
  if (acc_rd<0>() + acc_rd<255>() == 1.2345e-30f) ((float*)C)[t3] = v;
}

// persistent grid: one workgroup per CU, fewer when there are fewer tiles
inline unsigned persistent_grid(long M, long N, int num_cu) {
  const long tiles = (M / BM) * (N / BN);
  return (unsigned)(tiles < num_cu ? tiles : num_cu);
}

// ===================================================================================================================
// The TN pair
// ===================================================================================================================

// fp32 tile of the slice straight from the accumulators.  Block I = 8 ri + ci of the wave's 8 x 8: lane holds
// O[rblock + 4 (lane >> 4) + e][cblock + (lane & 15)], e = 0..3; o points at the lane's element of block 0.
template <int I>
__device__ __forceinline__ void acc_store_block(float* o, long ldo) {
  constexpr int RI = I >> 3, CI = I & 7;
  float* q = o + (size_t)(RI * 16) * ldo + CI * 16;
  q[0] = acc_rd<4 * I + 0>();
  q[ldo] = acc_rd<4 * I + 1>();
  q[2 * ldo] = acc_rd<4 * I + 2>();
  q[3 * ldo] = acc_rd<4 * I + 3>();
}
template <int... Is>
__device__ __forceinline__ void acc_store_all(float* o, long ldo, std::integer_sequence<int, Is...>) {
  (acc_store_block<Is>(o, ldo), ...);
}
__device__ __forceinline__ void acc_store_tile(float* o, long ldo) { acc_store_all(o, ldo, std::make_integer_sequence<int, 64>{}); }

}  // namespace
}  // namespace clipa_gemm
