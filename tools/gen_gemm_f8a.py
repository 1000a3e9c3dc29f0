#!/usr/bin/env python
"""Generator of clipa_amd/csrc/gemm_f8a_asm.inc: the hand-scheduled main loop of gemm_f8a_kernel (gemm_f8a.hip), the fp8
NT GEMM on four waves of 512 registers.

    python tools/gen_gemm_f8a.py            # rewrites the .inc (tests/test_gemm_nta_gen_cpu.py checks it is up to date)

Same LDS images, swizzle, ring, LDS-DMA and tile-edge handling as gen_gemm_nta.py (an operand image is 256 rows x 128
BYTES = 128 fp8 k-values), but one `v_mfma_f32_16x16x128_f8f6f4` consumes a whole image row of a block: a lane's operand
is chunks g and 4 + g of its row = the bf16 kernel's two k-halves side by side in 8 registers, so a K step is 64 MFMAs and
there is no "other k-half" to read under the first half of them.  The read-ahead follows the registers instead:

  registers  a[0:255]     accumulators, block (bj, ai) at a[4 (8 bj + ai) : +3]
             v[128:191]   A block ai (token rows) at v[128 + 8 ai : +7]  (registers 0-3 = chunk g, 4-7 = chunk 4 + g)
             v[192:255]   B block bj (weight rows) at v[192 + 8 bj : +7]
             v[96:119]    LDS-DMA offsets and fragment-read addresses as in gen_gemm_nta.py
  MFMA order bj-major (m = 8 bj + ai): weight block bj is dead after MFMA 8 bj + 7, token block ai after MFMA 56 + ai, and
             the next step needs them in the same order (B0 + A0 at its MFMA 0, A1 at 1, ... B1 at 8, ...).  So a step
               - reads ITS OWN last weight block B7 at the top (needed at MFMA 56), waits for token block ai of the read-ahead
                 in front of MFMA ai (counted lgkmcnt: LDS returns in order),
               - after MFMA 8: every fragment of this step is in registers -> barrier 1 frees the slot, the 16 LDS-DMA of
                 step + 2 go out one per two MFMAs (MFMAs 9..40),
               - after MFMA 42: `s_waitcnt vmcnt(16)` + barrier 2 publish step + 1 (issued a step ago), whose weight blocks
                 0..4 are read at once, 5 and 6 as they die (MFMAs 48, 56), token block ai right behind MFMA 56 + ai - eight
                 MFMAs (256 clocks) ahead of its first use.
  tile edge  as in gen_gemm_nta.py; the tile's vectors (row scales | bias | column scales, 1 KiB each) ride the last step as one
             LDS-DMA per wave 0..2 into a 3 KiB window behind the ring, older than the step's 16 pieces.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_gen import (BLOCK, NT_DMA, VADDR_A, VADDR_B, VOFF_A, acc, blk, c_string, clobbers, define, header, main,  # noqa: E402
                      nt_prologue_text, nt_setup_text, out_path, tile_scaffold)

OUT = out_path("f8a")
FA, FB = 128, 192
BAR1, DMA0, PUBLISH = 8, 9, 42


def reads(kind, b, slot):
    """Both 16-byte reads of block b (chunk g into registers 0-3, chunk 4 + g into 4-7) from ring slot `slot`."""
    base, addr = (FB, VADDR_B) if kind == "B" else (FA, VADDR_A)
    r = base + 8 * b
    return [f"ds_read_b128 v[{r}:{r + 3}], v{addr + 2 * slot} offset:{b * BLOCK}",
            f"ds_read_b128 v[{r + 4}:{r + 7}], v{addr + 2 * slot + 1} offset:{b * BLOCK}"]


def step_text(slot, srd, first, last, vmcnt):
    """One K step computing from registers; slot = ring slot of its data (re-filled for step + 2); see the module docstring."""
    pre = {m: [] for m in range(64)}        # in front of MFMA m
    fill = {m: [] for m in range(64)}       # behind MFMA m
    pre[0] += reads("B", 7, slot)
    for m in range(8):
        pre[m].append(f"s_waitcnt lgkmcnt({min(15, 16 - 2 * m)})")
    fill[BAR1] += ["s_waitcnt lgkmcnt(0)", "s_barrier"]
    if last:
        # the tile's vectors: one 1 KiB LDS-DMA per wave (a 0-byte descriptor for wave 3), OLDER than the step's 16 pieces
        fill[BAR1 - 2].append("s_mov_b32 m0, %[ldsv]")
        fill[BAR1 - 1].append("buffer_load_dwordx4 %[vvec], %[srdVec], 0 offen lds")
    NT_DMA.place(fill, DMA0, 2, slot, srd, advance_at=PUBLISH - 1)
    if not last:
        fill[PUBLISH] += [f"s_waitcnt vmcnt({vmcnt})", "s_barrier"]
        for bj in range(5):
            fill[PUBLISH + 1 + bj] += reads("B", bj, slot ^ 1)
        fill[48] += reads("B", 5, slot ^ 1)
        fill[56] += reads("B", 6, slot ^ 1)
        for ai in range(8):
            fill[56 + ai] += reads("A", ai, slot ^ 1)
    lines = []
    for m in range(64):
        bj, ai = m // 8, m % 8
        lines += pre[m]
        c = "0" if first else acc(bj, ai)
        lines.append(f"v_mfma_f32_16x16x128_f8f6f4 {acc(bj, ai)}, {blk(FB, bj)}, {blk(FA, ai)}, {c}@FMT@")
        lines += fill[m]
    return lines


def tile_text():
    t = nt_setup_text()
    t.append("s_mov_b32 %[sk], 256")
    t += ["s_waitcnt vmcnt(@#VMS@)", "s_barrier"]
    for bj in range(7):
        t += reads("B", bj, 0)
    for ai in range(8):
        t += reads("A", ai, 0)
    t.append("s_waitcnt lgkmcnt(0)")
    steady = [step_text(slot, "cur", False, False, "16") for slot in (0, 1)]
    steps = [step_text(0, "cur", True, False, "@#VM0@"), steady[1]] + steady
    steps += [step_text(0, "nxt", False, False, "16"), step_text(1, "nxt", False, True, None)]
    # the vectors are older than the 16 LDS-DMA of the last step; the barrier makes every wave's vector visible to the epilogue
    return t + tile_scaffold("F8A", steps, ["s_mov_b32 %[sk], 0"], ["s_waitcnt vmcnt(16)", "s_barrier"])


def render():
    p = header("f8a") + define("F8A_PROLOGUE_ASM", c_string(nt_prologue_text()))
    p.append("// VMS: wait in front of the tile's first fragment reads (16 + stores the epilogue before it may leave in flight);")
    p.append("// VM0: publish wait of the tile's first step (likewise).  FMT: a string, the format suffix of the MFMAs (\" cbsz:1\" ...).")
    p.append("#define F8A_TILE_ASM(S, FMT) F8A_TILE_ASM_I(F8A_VM_##S, F8A_VM_##S, FMT)")
    p.append("#define F8A_TILE_ASM_I(VMS, VM0, FMT) F8A_TILE_ASM_II(VMS, VM0, FMT)")
    p += define("F8A_TILE_ASM_II(VMS, VM0, FMT)", c_string(tile_text()))
    for st in (0, 32, 64):
        p.append(f"#define F8A_VM_{st} {min(63, 16 + st)}")
    p.append("")
    p += define("F8A_CLOBBERS", clobbers(VOFF_A))
    return "\n".join(p)


if __name__ == "__main__":
    main(OUT, render)
