"""What the generators of the four-wave GEMM main loops (tools/gen_gemm_{nta,f8a,tna,tn8}.py -> clipa_amd/csrc/gemm_*_asm.inc)
share: the LDS ring, the register names, the 16 operand LDS-DMA of a K step, the slot flip, the tile scaffold and the rendering
of lines as a C macro of inline-asm text.  A library, not a script; what a kernel schedules differently (fragment reads, MFMA
order, waits) is in its own generator, next to its register map.
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# bytes: a ring slot (two operand images), an operand image, the part of an image one LDS-DMA of a wave fills, a 16-row block
SLOT, IMG, PIECE, BLOCK = 65536, 32768, 4096, 2048


def out_path(kernel):
    return os.path.join(ROOT, "clipa_amd", "csrc", f"gemm_{kernel}_asm.inc")


def acc(i, j):
    """Accumulators of the 16 x 16 output block (i, j) of a wave's 8 x 8."""
    b = 4 * (8 * i + j)
    return f"a[{b}:{b + 3}]"


def vr(base, i):
    return f"v[{base + 4 * i}:{base + 4 * i + 3}]"


def blk(base, i):
    return f"v[{base + 8 * i}:{base + 8 * i + 7}]"


def younger(S, key="vmwait"):
    """LDS-DMA of a step issued before its publish wait (the wait sits after MFMA S[key], DMA q after MFMA dma_start + 1 + q stride)."""
    return sum(1 for q in range(16) if S["dma_start"] + 1 + q * S["dma_stride"] <= S[key])


class Dma:
    """The 16 operand LDS-DMA of a K step: 8 pieces per operand image.  names: the operands' letters ("AB" | "PQ"), voff: first
    of the 8 registers of per-lane byte offsets of each, sk: the scalar-offset operand of each, advance: the instruction(s)
    that move the scalar offset(s) to the next K step."""

    def __init__(self, names, voff, sk, advance):
        self.names, self.voff, self.sk, self.advance = names, voff, sk, advance

    def piece(self, q, slot, srd):
        """(M0 write, load) of piece q into ring slot `slot` through the descriptors `srd` ('cur' | 'nxt' | 'nul')."""
        img, j = q // 8, q % 8
        return (f"s_add_u32 m0, %[ldsw], {slot * SLOT + img * IMG + j * PIECE}",
                f"buffer_load_dwordx4 v{self.voff[img] + j}, %[{srd}{self.names[img]}], %[{self.sk[img]}] offen lds")

    def place(self, fill, start, stride, slot, srd, advance_at=None, wrap=str):
        """Into fill (issue slot -> items behind that MFMA): piece q's M0 write at start + q stride, its load one MFMA later (the
        wait state M0 needs), the advance from `advance_at` (default: right behind the last load), one instruction per slot."""
        for q in range(16):
            m0, load = self.piece(q, slot, srd)
            fill[start + q * stride].append(wrap(m0))
            fill[start + q * stride + 1].append(wrap(load))
        last_dma = start + 15 * stride + 1
        at = last_dma + 1 if advance_at is None else advance_at
        assert last_dma < at and at + len(self.advance) - 1 < len(fill) - 1
        for i, a in enumerate(self.advance):
            fill[at + i].append(wrap(a))

    def prologue(self, step):
        """Straight-line form for K steps 0 and 1 of a workgroup: `s_nop 0` is the wait state of M0."""
        t = []
        for q in range(16):
            m0, load = self.piece(q, step, "cur")
            t += [m0, "s_nop 0", load]
        return t


def place_flip(fill, start, stride, vaddr, wrap=str):
    """Flip the 2 x 8 fragment-read address registers (vaddr: first register of each operand) to the other ring slot, one per
    `stride` issue slots from `start`.  Returns the last slot used."""
    for i in range(16):
        reg = vaddr[i // 8] + i % 8
        fill[start + i * stride].append(wrap(f"v_xor_b32 v{reg}, 0x10000, v{reg}"))
    return start + 15 * stride


def tile_scaffold(prefix, steps, before_tail, final_wait):
    """A tile from six step texts: the first two, the two of the loop (run %[nloop] times), the last two.  before_tail: lines
    in front of the last two steps; final_wait: the wait(s) behind them (MFMA results must be readable by v_accvgpr_read
    afterwards: two `s_nop 7`)."""
    s0, s1, l0, l1, t0, t1 = steps
    return (s0 + s1
            + ["s_cmp_eq_u32 %[nloop], 0", f"s_cbranch_scc1 {prefix}_TAIL_%=", "s_mov_b32 %[cnt], %[nloop]", f"{prefix}_LOOP_%=:"]
            + l0 + l1
            + ["s_sub_u32 %[cnt], %[cnt], 1", "s_cmp_lg_u32 %[cnt], 0", f"s_cbranch_scc1 {prefix}_LOOP_%=", f"{prefix}_TAIL_%=:"]
            + before_tail + t0 + t1 + final_wait + ["s_nop 7", "s_nop 7"])


def c_string(lines):
    """Lines as C string literals.  `@NAME@` becomes the macro argument NAME (itself a string: FMT), `@#NAME@` the stringified
    one (an immediate that differs per instantiation: VM0, VMS)."""
    return ['  "' + re.sub(r"@(#?\w+)@", r'" \1 "', l) + '\\n\\t"' for l in lines]


def clobbers(first_vgpr):
    regs = [f"v{i}" for i in range(first_vgpr, 256)] + [f"a{i}" for i in range(256)]
    out, line = [], "  "
    for r in regs:
        tok = f'"{r}", '
        if len(line) + len(tok) > 124:
            out.append(line.rstrip())
            line = "  "
        line += tok
    out.append(line.rstrip().rstrip(","))
    return out


def define(name, body):
    """A multi-line macro from body lines (c_string() or clobbers()), and the empty line behind it."""
    return [f"#define {name} \\", " \\\n".join(body), ""]


def header(kernel):
    return [f"// GENERATED by tools/gen_gemm_{kernel}.py - do not edit (tests/test_gemm_nta_gen_cpu.py compares it with the generator).",
            f"// Main loop of gemm_{kernel}_kernel as inline-asm text; register map, pipeline and schedule: see the generator's docstring.",
            "#pragma once", ""]


def main(out, render):
    """`python tools/gen_gemm_<k>.py` rewrites the .inc, `--check` exits 0 if it is up to date and 1 if not."""
    text = render()
    if "--check" in sys.argv:
        sys.exit(0 if open(out).read() == text else 1)
    open(out, "w").write(text)
    print("wrote", out, len(text.splitlines()), "lines")


# --- the NT pair (nta: bf16, f8a: fp8): same LDS images, so the same LDS-DMA, read addresses, statement setup and prologue ---
VOFF_A, VOFF_B = 96, 104                     # LDS-DMA per-lane offsets
VADDR_A, VADDR_B = 112, 116                  # + 2 * slot + khalf
NT_DMA = Dma("AB", (VOFF_A, VOFF_B), ("sk", "sk"), ["s_add_u32 %[sk], %[sk], 128"])


def nt_setup_text():
    """Per-lane addresses from the four "v" inputs (recomputed per statement: nothing of ours lives in registers the
    compiler may touch between statements except the accumulators)."""
    t = ["s_nop 4",
         f"v_mov_b32 v{VADDR_A}, %[va]", f"v_xor_b32 v{VADDR_A + 1}, 64, v{VADDR_A}",
         f"v_add_u32 v{VADDR_A + 2}, 0x10000, v{VADDR_A}", f"v_add_u32 v{VADDR_A + 3}, 0x10000, v{VADDR_A + 1}",
         f"v_mov_b32 v{VADDR_B}, %[vb]", f"v_xor_b32 v{VADDR_B + 1}, 64, v{VADDR_B}",
         f"v_add_u32 v{VADDR_B + 2}, 0x10000, v{VADDR_B}", f"v_add_u32 v{VADDR_B + 3}, 0x10000, v{VADDR_B + 1}",
         f"v_mov_b32 v{VOFF_A}, %[voffA]", f"v_mov_b32 v{VOFF_B}, %[voffB]"]
    for j in range(1, 8):
        t.append(f"v_add_u32 v{VOFF_A + j}, %[sA32], v{VOFF_A + j - 1}")
        t.append(f"v_add_u32 v{VOFF_B + j}, %[sB32], v{VOFF_B + j - 1}")
    return t


def nt_prologue_text():
    """Very first tile of a workgroup: fetch its K steps 0 and 1 (32 LDS-DMA per wave)."""
    t = nt_setup_text()
    for step in range(2):
        t += [f"s_mov_b32 %[sk], {step * 128}"] + NT_DMA.prologue(step)
    return t
