#!/usr/bin/env python
"""Generator of clipa_amd/csrc/gemm_nta_asm.inc: the hand-scheduled main loop of gemm_nta_kernel (gemm_nta.hip).

    python tools/gen_gemm_nta.py            # rewrites the .inc (tests/test_gemm_nta_gen_cpu.py checks it is up to date)

Why a generator: the K loop of the 4-wave / 512-register bf16 GEMM is ONE inline-asm statement per output tile (every
issue slot placed by hand: 128 MFMAs, 32 fragment reads, 16 LDS-DMA, 2 barriers and 3 waits per K step); writing ~1500
lines of it by hand is how schedules rot.  The schedule is data (`SCHEDULES`), the text is derived; what the text has in
common with the three sibling kernels' (LDS-DMA issue, tile scaffold, rendering as a macro) is derived in tools/gemm_gen.py.

Structure of one tile (256 x 256 outputs, K = 64 * nkt, nkt even >= 4; wave (wm, wn) owns 128 x 128 = 8 x 8 blocks of 16 x 16):

  registers  a[0:255]     accumulators, block (bj, ai) at a[4 (8 bj + ai) : +3]   (bj: weight-row block, ai: token-row block)
             v[128:159]   A0 = token-row fragments of k-half 0 (8 x 4 registers)   v[160:191]  A1 (k-half 1)
             v[192:223]   B0 = weight-row fragments of k-half 0                    v[224:255]  B1
             v[96:103] / v[104:111]   per-lane byte offsets of the 8 A / 8 B LDS-DMA pieces of a K step
             v[112:115] / v[116:119]  fragment-read addresses: A (slot 0 k0, slot 0 k1, slot 1 k0, slot 1 k1) / B likewise
  LDS        two ring slots of 64 KiB (A image 256 rows x 128 B at +0, B image at +32 KiB), the production image and swizzle
  pipeline   K step i computes from registers: its k-half-0 fragments were read at the end of step i-1, its k-half-1
             fragments are read under the first MFMAs; barrier 1 (every wave is done reading slot i&1) frees the slot for
             the LDS-DMA of step i+2 (two steps ahead: ~1.5 K steps to land instead of < 1 in gemm_nt2); `s_waitcnt vmcnt`
             + barrier 2 publish step i+1's operands, whose k-half-0 fragments are read under the last MFMAs.
  tile edge  the last two steps fetch the NEXT tile's first two K steps (other descriptors, k offset 0), so the ring
             never drains; the tile's bias vector is fetched to registers under the last step.
  (tried)    keeping 12 of a lane's 32 packed output chunks in registers and storing them from inside the next tile's first
             two K steps, one store per 20 MFMAs, with exact in-order vmcnt accounting (commit 'gemm_nta: 12 of a lane's 32
             output chunks ...'): bit-identical and 3..5 % SLOWER on every shape - a store issued inside the K loop stalls
             the matrix pipe as long as one issued after it (profiles/r03_gemm_nta_deferred_stores_ab.jsonl).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_gen import (BLOCK, NT_DMA, VADDR_A, VADDR_B, VOFF_A, acc, c_string, clobbers, define, header, main, nt_prologue_text,  # noqa: E402
                      nt_setup_text, out_path, tile_scaffold, vr, younger)

OUT = out_path("nta")
A0, A1, B0, B1 = 128, 160, 192, 224          # fragment register bases

# schedule = issue slots (index of the MFMA after which the instruction is placed; 0..127) of everything that is not an MFMA
SCHEDULES_ALL = {
    # two barriers per step; fragment reads and LDS-DMA one per two MFMAs (the pacing of the vendor's assembly kernel)
    0: dict(rd1_start=0, rd1_stride=2, bar1=34, dma_start=36, dma_stride=2, vmwait=74, rd0_start=76, rd0_stride=2, lgk_end=126),
    # denser front: reads one per MFMA, slot freed at MFMA 20, DMA issued by MFMA 54, operands published later
    1: dict(rd1_start=0, rd1_stride=1, bar1=20, dma_start=22, dma_stride=2, vmwait=88, rd0_start=90, rd0_stride=2, lgk_end=126),
    # DMA spread one per three MFMAs, publish as late as the fragment reads allow
    2: dict(rd1_start=0, rd1_stride=2, bar1=34, dma_start=36, dma_stride=3, vmwait=92, rd0_start=94, rd0_stride=2, lgk_end=126),
    # DMA one per four MFMAs (the issue spans half a K step), read-ahead packed into the last 24 MFMAs
    3: dict(rd1_start=0, rd1_stride=2, bar1=34, dma_start=36, dma_stride=4, vmwait=100, rd0_start=102, rd0_stride=1, lgk_end=126),
    # early slot release (reads one per MFMA) + DMA one per four MFMAs
    4: dict(rd1_start=0, rd1_stride=1, bar1=20, dma_start=22, dma_stride=4, vmwait=96, rd0_start=98, rd0_stride=1, lgk_end=126),
    # schedule 2 with the publish point pushed to MFMA 104
    5: dict(rd1_start=0, rd1_stride=2, bar1=34, dma_start=36, dma_stride=3, vmwait=104, rd0_start=106, rd0_stride=1, lgk_end=126),
    # early release, DMA one per six MFMAs: the issue spans the step, the publish wait leaves the DMA issued before it in flight
    6: dict(rd1_start=0, rd1_stride=1, bar1=20, dma_start=22, dma_stride=6, vmwait=96, rd0_start=98, rd0_stride=1, lgk_end=126),
    # early release, DMA one per five MFMAs, publish after the last one
    7: dict(rd1_start=0, rd1_stride=1, bar1=20, dma_start=22, dma_stride=5, vmwait=100, rd0_start=102, rd0_stride=1, lgk_end=126),
}


# the schedules compiled into the library (the rest were A/B'd on hardware: profiles/r03_gemm_nta_schedules_*.jsonl)
SCHEDULES = {k: SCHEDULES_ALL[k] for k in (0, 3, 4)}


def step_text(S, slot, srd, first, last, vmcnt, bias):
    """One K step.  slot: ring slot it computes from (and re-fills for step + 2).  srd: 'cur' | 'nxt' descriptors of the
    LDS-DMA it issues.  first: accumulators start from 0.  last: last step of the tile (no publish / read-ahead; the
    bias fetch rides here).  vmcnt: text of the immediate of the publish wait."""
    fill = {m: [] for m in range(128)}
    # k-half-1 fragments of THIS step (weights first: their registers were last used earliest in the previous step)
    order = [("B", b) for b in range(8)] + [("A", a) for a in range(8)]
    m = S["rd1_start"]
    for kind, b in order:
        base, addr = (B1, VADDR_B) if kind == "B" else (A1, VADDR_A)
        fill[m].append(f"ds_read_b128 {vr(base, b)}, v{addr + 2 * slot + 1} offset:{b * BLOCK}")
        m += S["rd1_stride"]
    assert m - S["rd1_stride"] < S["bar1"]
    fill[S["bar1"]] += ["s_waitcnt lgkmcnt(0)", "s_barrier"]
    # LDS-DMA of step + 2 into the slot just freed
    m = S["dma_start"]
    assert m > S["bar1"]
    if bias:
        # last step of the tile: the bias vector is fetched to registers here, OLDER than the step's 16 LDS-DMA, so that the
        # statement's final vmcnt(16) covers it.  (Fetching the first residual / pre-activation chunks of the epilogue here as
        # well was measured and changed nothing - profiles/r03_gemm_nta_aux_prefetch_ab.jsonl: those epilogues are bound by
        # the store path, not by the operand latency.)
        for p in range(4):
            for h in range(2):
                fill[m - 1 - (p * 2 + h)].append(f"buffer_load_dwordx4 %[bias{p * 2 + h}], %[vbias], %[srdBias], 0 offen offset:{p * 128 + h * 16}")
    NT_DMA.place(fill, m, S["dma_stride"], slot, srd)
    if not last:
        # step + 1's operands are older than everything this step has issued so far: `younger(S)` LDS-DMA may stay in flight
        assert vmcnt in ("@#VM0@", str(younger(S)))
        fill[S["vmwait"]] += [f"s_waitcnt vmcnt({vmcnt})", "s_barrier"]
        m = S["rd0_start"]
        for kind, b in order:
            base, addr = (B0, VADDR_B) if kind == "B" else (A0, VADDR_A)
            fill[m].append(f"ds_read_b128 {vr(base, b)}, v{addr + 2 * (slot ^ 1)} offset:{b * BLOCK}")
            m += S["rd0_stride"]
        assert m - S["rd0_stride"] < S["lgk_end"]
        fill[S["lgk_end"]].append("s_waitcnt lgkmcnt(0)")
    lines = []
    for m in range(128):
        kk, r = m // 64, m % 64
        bj, ai = r // 8, r % 8
        fb, fa = (B0, A0) if kk == 0 else (B1, A1)
        c = "0" if (first and kk == 0) else acc(bj, ai)
        lines.append(f"v_mfma_f32_16x16x32_bf16 {acc(bj, ai)}, {vr(fb, bj)}, {vr(fa, ai)}, {c}")
        lines += fill[m]
    return lines


def tile_text(S):
    order = [("B", b) for b in range(8)] + [("A", a) for a in range(8)]
    t = nt_setup_text()
    t.append("s_mov_b32 %[sk], 256")
    # this tile's step 0 has landed (younger: step 1's 16 LDS-DMA + whatever the epilogue before us left in flight)
    t += ["s_waitcnt vmcnt(@#VMS@)", "s_barrier"]
    for kind, b in order:
        base, addr = (B0, VADDR_B) if kind == "B" else (A0, VADDR_A)
        t.append(f"ds_read_b128 {vr(base, b)}, v{addr} offset:{b * BLOCK}")
    t.append("s_waitcnt lgkmcnt(0)")
    k = str(younger(S))
    steady = [step_text(S, slot, "cur", False, False, k, False) for slot in (0, 1)]
    steps = [step_text(S, 0, "cur", True, False, "@#VM0@", False), steady[1]] + steady
    steps += [step_text(S, 0, "nxt", False, False, k, False), step_text(S, 1, "nxt", False, True, None, True)]
    # the bias is older than the 16 LDS-DMA of the last step
    return t + tile_scaffold("NTA", steps, ["s_mov_b32 %[sk], 0"], ["s_waitcnt vmcnt(16)"])


def render():
    p = header("nta") + define("NTA_PROLOGUE_ASM", c_string(nt_prologue_text()))
    for v, S in SCHEDULES.items():
        k = younger(S)
        p.append(f"// schedule {v}: {S}")
        p.append(f"// VMS: wait in front of the tile's first fragment reads (16 + stores the epilogue before it may leave in flight);")
        p.append(f"// VM0: publish wait of the tile's first step ({k} + those stores).  Both capped at the counter's 63.")
        p.append(f"#define NTA_TILE_ASM_{v}(S) NTA_TILE_ASM_{v}_I(NTA_VMS_##S, NTA_VM0_{v}_##S)")
        for st in (0, 32, 64):
            p.append(f"#define NTA_VM0_{v}_{st} {min(63, k + st)}")
        p.append(f"#define NTA_TILE_ASM_{v}_I(VMS, VM0) NTA_TILE_ASM_{v}_II(VMS, VM0)")
        p += define(f"NTA_TILE_ASM_{v}_II(VMS, VM0)", c_string(tile_text(S)))
    for st in (0, 32, 64):
        p.append(f"#define NTA_VMS_{st} {min(63, 16 + st)}")
    p.append("")
    p += define("NTA_CLOBBERS", clobbers(VOFF_A))
    return "\n".join(p)


if __name__ == "__main__":
    main(OUT, render)
