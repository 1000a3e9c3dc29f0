"""A/B of the HBM-streaming kernels (LayerNorm forward / backward in all its forms, MLP re-materialisation from bf16 and from
e4m3, row quantisation with and without column sums, LayerNorm + quantise) between builds of the library, in ONE process on
torch-allocated buffers.

Timing (default): the bench's sizes, interleaved rounds, median.  Two settings per kernel: "hot" = the same launch back to back;
"after_writer" = each launch preceded by a torch kernel that rewrites the input (what a training step looks like: the input was
just produced, its tail is dirty in L2 / MALL) - there the time is writer + kernel for both libraries, so only the DIFFERENCE is
meaningful.
    python tools/stream_lib_ab.py old.so new.so [rows=806912] [D=1024] [--rounds=7] [--only=ln_bwd_f32,ln_fwd]
(--rounds: interleaved rounds per kernel and setting, the first is a warm-up; --only: these kernels of the list)
Bits: every LayerNorm / row-quantise entry point of both libraries on the same seeded inputs at small shapes that reach every
kernel instantiation, every ragged last chunk and every multi-pass loop; outputs and workspaces are poisoned before each call,
every output tensor is compared byte for byte.  Prints the number of tensors compared and the number that differ, exits 1 if
any differ.
    python tools/stream_lib_ab.py --bits old.so new.so
The two libraries hold only the streaming kernels (seconds to build):
    git archive <old-commit> clipa_amd/csrc include | tar -x -C /tmp/old
    (cd /tmp/old && hipcc -O3 --offload-arch=gfx950 -shared -fPIC -I clipa_amd/csrc -I include clipa_amd/csrc/{layernorm,misc,quant,runtime}.hip \\
         -o $REPO/tools/probes/lnvar/libstream_old.so)
    hipcc ... (same, from the working tree) -o tools/probes/lnvar/libstream_new.so"""
import ctypes
import json
import os
import statistics
import sys

import torch

paths = [p for p in sys.argv[1:] if p.endswith(".so")]
nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
BITS = "--bits" in sys.argv[1:]
OPTS = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
ROUNDS = int(OPTS.get("rounds", 7))
ONLY = OPTS["only"].split(",") if "only" in OPTS else None
libs = [ctypes.CDLL(os.path.abspath(p)) for p in paths]
P, I64, F, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_int
for L in libs:
    L.clipa_layernorm_fwd.argtypes = [P, P, P, P, I64, I64, F, I, I, P]
    for ws in ("clipa_layernorm_bwd_workspace", "clipa_layernorm_bwd_q8_workspace", "clipa_quantize_rows_colsum_workspace"):
        getattr(L, ws).argtypes = [I64, I64]
        getattr(L, ws).restype = I64
    L.clipa_layernorm_bwd.argtypes = [P, P, P, P, P, P, P, I64, I64, F, I, I, P, I64, P]
    L.clipa_layernorm_bwd_y.argtypes = [P, P, P, P, P, P, P, P, P, I64, I64, F, I, I, P, I64, P]
    L.clipa_layernorm_bwd_q8.argtypes = [P, P, P, P, P, P, P, P, P, P, P, P, P, I64, I64, F, I, P, I64, P]
    L.clipa_activation_fwd.argtypes = [P, P, I64, I, P]
    L.clipa_activation_fwd_e4m3.argtypes = [P, P, I64, I, P]
    L.clipa_quantize_rows.argtypes = [P, P, P, I64, I64, I64, I64, I, P]
    L.clipa_quantize_rows_colsum.argtypes = [P, P, P, P, P, I64, I64, I64, I64, I, P, I64, P]
    L.clipa_layernorm_fwd_q8.argtypes = [P, P, P, P, P, P, I64, I64, F, P]
    L.clipa_layernorm_fwd_q8n.argtypes = [P, P, P, P, P, P, P, I64, I64, F, P]
    L.clipa_layernorm_fwd_q8s.argtypes = [P, P, P, P, P, P, I64, I64, F, P]
dev = "cuda"
bf16, f32, u8 = torch.bfloat16, torch.float32, torch.uint8
st = torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


# ---- bits ------------------------------------------------------------------------------------------------------------------
def poisoned(shape, dtype):
    """An output or workspace nobody has written: every byte 0xFF (a NaN in bf16 / f32)."""
    n = 1
    for s in shape:
        n *= s
    return torch.full((n * torch.empty((), dtype=dtype).element_size(),), 0xFF, dtype=u8, device=dev).view(dtype).view(*shape)


def ln_calls(L, rows, D, gen):
    """name -> dict of output tensors, for every LayerNorm entry point at one shape."""
    def rnd(*shape, scale=1.0):
        return torch.randn(*shape, generator=gen) * scale
    x32 = (rnd(rows, D, scale=2.0) + 0.3).to(dev)
    dy32 = (rnd(rows, D, scale=1e-2) * torch.exp(rnd(rows, 1))).to(dev)
    dres32 = rnd(rows, D, scale=1e-2).to(dev)
    if rows > 5:
        x32[5], dy32[5], dres32[5] = 0.0, 0.0, 0.0
    gam, bet = (1 + 0.1 * rnd(D)).to(dev), (0.1 * rnd(D)).to(dev)
    rowscale, t = (rnd(rows).abs() + 0.1).to(dev), torch.full((1,), 0.37, device=dev)
    xs, dys, drs = {0: x32.to(bf16), 1: x32}, {0: dy32.to(bf16), 1: dy32}, {0: dres32.to(bf16), 1: dres32}
    dt = {0: bf16, 1: f32}
    out = {}

    def run(name, fn, **tensors):
        rc = fn()
        assert rc == 0, (name, rc)
        torch.cuda.synchronize()
        out[name] = tensors

    for xf in (0, 1):
        for yf in (0, 1):
            y = poisoned((rows, D), dt[yf])
            run(f"fwd x{xf} y{yf}", lambda: L.clipa_layernorm_fwd(ptr(xs[xf]), ptr(gam), ptr(bet), ptr(y), rows, D, 1e-5, xf, yf, st), y=y)
            for res in (True, False):
                for emit in (False, True):
                    wsb = int(L.clipa_layernorm_bwd_workspace(rows, D))
                    ws, dx, dg, db = poisoned((wsb,), u8), poisoned((rows, D), dt[xf]), poisoned((D,), f32), poisoned((D,), f32)
                    dr = drs[xf] if res else None
                    if emit:
                        y = poisoned((rows, D), dt[yf])
                        run(f"bwd_y x{xf} y{yf} res{res:d}", lambda: L.clipa_layernorm_bwd_y(
                            ptr(xs[xf]), ptr(gam), ptr(bet), ptr(dys[yf]), ptr(dr), ptr(dx), ptr(y), ptr(dg), ptr(db), rows, D, 1e-5, xf, yf,
                            ptr(ws), wsb, st), dx=dx, y=y, dgamma=dg, dbeta=db)
                    else:
                        run(f"bwd x{xf} y{yf} res{res:d}", lambda: L.clipa_layernorm_bwd(
                            ptr(xs[xf]), ptr(gam), ptr(dys[yf]), ptr(dr), ptr(dx), ptr(dg), ptr(db), rows, D, 1e-5, xf, yf, ptr(ws), wsb, st),
                            dx=dx, dgamma=dg, dbeta=db)
    for fmt in (0, 1):
        for res in (True, False):
            for emit in (False, True):
                wsb = int(L.clipa_layernorm_bwd_q8_workspace(rows, D))
                ws, dx, dg, db = poisoned((wsb,), u8), poisoned((rows, D), bf16), poisoned((D,), f32), poisoned((D,), f32)
                q, dq, cs, rn = poisoned((rows, D), u8), poisoned((rows,), f32), poisoned((D,), f32), poisoned((rows,), f32)
                y = poisoned((rows, D), bf16) if emit else None
                run(f"bwd_q8 fmt{fmt} res{res:d} y{emit:d}", lambda: L.clipa_layernorm_bwd_q8(
                    ptr(xs[0]), ptr(gam), ptr(bet) if emit else None, ptr(dys[0]), ptr(drs[0]) if res else None, ptr(dx), ptr(y), ptr(q), ptr(dq),
                    ptr(cs), ptr(rn), ptr(dg), ptr(db), rows, D, 1e-5, fmt, ptr(ws), wsb, st),
                    dx=dx, q=q, dq=dq, colsum=cs, rownorm=rn, dgamma=dg, dbeta=db, **({"y": y} if emit else {}))
    y, q, dq, rn = poisoned((rows, D), bf16), poisoned((rows, D), u8), poisoned((rows,), f32), poisoned((rows,), f32)
    run("fwd_q8n", lambda: L.clipa_layernorm_fwd_q8n(ptr(xs[0]), ptr(gam), ptr(bet), ptr(y), ptr(q), ptr(dq), ptr(rn), rows, D, 1e-5, st),
        y=y, q=q, dq=dq, rownorm=rn)
    q, dq = poisoned((rows, D), u8), poisoned((rows,), f32)
    run("fwd_q8", lambda: L.clipa_layernorm_fwd_q8(ptr(xs[0]), ptr(gam), ptr(bet), None, ptr(q), ptr(dq), rows, D, 1e-5, st), q=q, dq=dq)
    q = poisoned((rows, D), u8)
    run("fwd_q8s", lambda: L.clipa_layernorm_fwd_q8s(ptr(xs[0]), ptr(gam), ptr(bet), ptr(rowscale), ptr(t), ptr(q), rows, D, 1e-5, st), q=q)
    return out


def quant_calls(L, rows, K, ldx, gen):
    x = torch.randn(rows, ldx, generator=gen) * torch.exp(torch.randn(rows, 1, generator=gen) * 3.0)   # row magnitudes over ~5 decades
    x[rows // 2] = 0.0                                                                                    # an all-zero row
    x = x.to(bf16).to(dev)
    out = {}
    for fmt in (0, 1):
        q, dq = poisoned((rows, K), u8), poisoned((rows,), f32)
        rc = L.clipa_quantize_rows(ptr(x), ptr(q), ptr(dq), rows, K, ldx, K, fmt, st)
        assert rc == 0, rc
        out[f"quantize_rows fmt{fmt}"] = dict(q=q, dq=dq)
        wsb = int(L.clipa_quantize_rows_colsum_workspace(rows, K))
        ws, q, dq, cs, rn = poisoned((wsb,), u8), poisoned((rows, K), u8), poisoned((rows,), f32), poisoned((K,), f32), poisoned((rows,), f32)
        rc = L.clipa_quantize_rows_colsum(ptr(x), ptr(q), ptr(dq), ptr(cs), ptr(rn), rows, K, ldx, K, fmt, ptr(ws), wsb, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        out[f"quantize_rows_colsum fmt{fmt}"] = dict(q=q, dq=dq, colsum=cs, rownorm=rn)
    return out


def bits():
    ln_shapes = [(1031, D) for D in (264, 520, 1032, 1544, 2048)] + [(40003, 256), (9001, 1280), (1, 2048)]
    q_shapes = [(37, K, K) for K in (8, 520, 1032, 1544, 2568, 3592, 4616, 7688, 8192)] + [(8200, 520, 520), (37, 1032, 1032 + 64)]
    compared, differ = 0, []
    for kind, shapes in (("ln", ln_shapes), ("quant", q_shapes)):
        for shape in shapes:
            res = []
            for L in libs:
                gen = torch.Generator().manual_seed(1000 * shape[0] + shape[1])
                res.append({k: {n: t.cpu().view(-1).view(u8) for n, t in v.items()}
                            for k, v in (ln_calls(L, *shape, gen) if kind == "ln" else quant_calls(L, *shape, gen)).items()})
            for call, tensors in res[0].items():
                for name, ref in tensors.items():
                    for other in res[1:]:
                        compared += 1
                        if not torch.equal(ref, other[call][name]):
                            differ.append(f"{kind} {shape} {call}: {name}")
    for d in differ:
        print("DIFFERS", d)
    print(json.dumps({"mode": "bits", "libs": [os.path.basename(p) for p in paths], "tensors_compared": compared, "tensors_differ": len(differ)}), flush=True)
    return 1 if differ else 0


if BITS:
    sys.exit(bits())

# ---- timing ----------------------------------------------------------------------------------------------------------------
rows = nums[0] if nums else 806912
D = nums[1] if len(nums) > 1 else 1024
x = torch.randn(rows, D, device=dev).to(bf16)
src = torch.randn(rows, D, device=dev).to(bf16)
dy = torch.randn(rows, D, device=dev).to(bf16)
dres = torch.randn(rows, D, device=dev).to(bf16)
y = torch.empty_like(x)
y2 = torch.empty_like(x)
x32, src32, dy32, dres32 = (torch.randn(rows, D, device=dev) for _ in range(4))
y32 = torch.empty_like(x32)
g = torch.ones(D, device=dev)
b = torch.zeros(D, device=dev)
dg, db = torch.empty(D, device=dev), torch.empty(D, device=dev)
H = 4 * D
wsb = max(max(int(L.clipa_layernorm_bwd_q8_workspace(rows, D)), int(L.clipa_quantize_rows_colsum_workspace(rows, H))) for L in libs)
ws = torch.empty(wsb, device=dev, dtype=u8)
h = torch.randn(rows, H, device=dev).to(bf16)
hsrc = torch.randn(rows, H, device=dev).to(bf16)
hout = torch.empty_like(h)
h8 = torch.randint(0, 120, (rows, H), device=dev, dtype=u8)
h8src = h8.clone()
q = torch.empty(rows, H, device=dev, dtype=u8)
dq = torch.empty(rows, device=dev)
rn = torch.empty(rows, device=dev)
cs = torch.empty(H, device=dev)
rowscale = torch.rand(rows, device=dev) + 0.1
tdev = torch.full((1,), 0.37, device=dev)
GB = 1e-9


def cases(L):
    a = dict(x=ptr(x), g=ptr(g), b=ptr(b), y=ptr(y), y2=ptr(y2), dy=ptr(dy), dres=ptr(dres), dg=ptr(dg), db=ptr(db), ws=ptr(ws), q=ptr(q), dq=ptr(dq),
             rn=ptr(rn), cs=ptr(cs), h=ptr(h))
    return {
        "ln_fwd": (lambda: L.clipa_layernorm_fwd(a["x"], a["g"], a["b"], a["y"], rows, D, 1e-5, 0, 0, st), lambda: x.copy_(src), 4 * rows * D),
        "ln_fwd_f32": (lambda: L.clipa_layernorm_fwd(ptr(x32), a["g"], a["b"], ptr(y32), rows, D, 1e-5, 1, 1, st), lambda: x32.copy_(src32), 8 * rows * D),
        "ln_bwd": (lambda: L.clipa_layernorm_bwd(a["x"], a["g"], a["dy"], a["dres"], a["y"], a["dg"], a["db"], rows, D, 1e-5, 0, 0, a["ws"], wsb, st),
                   lambda: dy.copy_(src), 8 * rows * D),
        "ln_bwd_f32": (lambda: L.clipa_layernorm_bwd(ptr(x32), a["g"], ptr(dy32), ptr(dres32), ptr(y32), a["dg"], a["db"], rows, D, 1e-5, 1, 1, a["ws"], wsb, st),
                       lambda: dy32.copy_(src32), 16 * rows * D),
        "ln_bwd_y": (lambda: L.clipa_layernorm_bwd_y(a["x"], a["g"], a["b"], a["dy"], a["dres"], a["y"], a["y2"], a["dg"], a["db"], rows, D, 1e-5, 0, 0,
                                                     a["ws"], wsb, st), lambda: dy.copy_(src), 10 * rows * D),
        "ln_bwd_q8": (lambda: L.clipa_layernorm_bwd_q8(a["x"], a["g"], None, a["dy"], a["dres"], a["y"], None, a["q"], a["dq"], a["cs"], a["rn"], a["dg"],
                                                       a["db"], rows, D, 1e-5, 0, a["ws"], wsb, st), lambda: dy.copy_(src), 9 * rows * D),
        "activation_fwd": (lambda: L.clipa_activation_fwd(a["h"], ptr(hout), rows * H, 0, st), lambda: h.copy_(hsrc), 4 * rows * H),
        "activation_fwd_e4m3": (lambda: L.clipa_activation_fwd_e4m3(ptr(h8), ptr(hout), rows * H, 0, st), lambda: h8.copy_(h8src), 3 * rows * H),
        "quantize_rows": (lambda: L.clipa_quantize_rows(a["h"], a["q"], a["dq"], rows, H, H, H, 0, st), lambda: h.copy_(hsrc), 3 * rows * H),
        "quantize_rows_colsum": (lambda: L.clipa_quantize_rows_colsum(a["h"], a["q"], a["dq"], a["cs"], a["rn"], rows, H, H, H, 0, a["ws"], wsb, st),
                                 lambda: h.copy_(hsrc), 3 * rows * H),
        "ln_fwd_q8": (lambda: L.clipa_layernorm_fwd_q8(a["x"], a["g"], a["b"], a["y"], a["q"], a["dq"], rows, D, 1e-5, st), lambda: x.copy_(src), 5 * rows * D),
        "ln_fwd_q8n": (lambda: L.clipa_layernorm_fwd_q8n(a["x"], a["g"], a["b"], a["y"], a["q"], a["dq"], a["rn"], rows, D, 1e-5, st),
                       lambda: x.copy_(src), 5 * rows * D),
        "ln_fwd_q8s": (lambda: L.clipa_layernorm_fwd_q8s(a["x"], a["g"], a["b"], ptr(rowscale), ptr(tdev), a["q"], rows, D, 1e-5, st),
                       lambda: x.copy_(src), 3 * rows * D),
    }


def timed(fn, pre, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        if pre is not None:
            pre()
        rc = fn()
        assert rc == 0, rc
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


table = [cases(L) for L in libs]
for name in table[0]:
    if ONLY is not None and name not in ONLY:
        continue
    for setting in ("hot", "after_writer"):
        ts = [[] for _ in libs]
        for rnd in range(ROUNDS):
            for i in range(len(libs)):
                fn, pre, nbytes = table[i][name]
                t = timed(fn, pre if setting == "after_writer" else None, 4)
                if rnd:
                    ts[i].append(t)
        med = [statistics.median(t) for t in ts]
        rec = {"kernel": name, "rows": rows, "D": D, "setting": setting, "rounds": ROUNDS, "ms": [round(m, 4) for m in med], "libs": [os.path.basename(p) for p in paths]}
        if setting == "hot":
            rec["gbps"] = [round(table[0][name][2] / m * 1e-6) for m in med]
        else:
            rec["new_minus_old_ms"] = round(med[-1] - med[0], 4)
        print(json.dumps(rec), flush=True)
