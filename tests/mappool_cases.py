"""TEST INFRASTRUCTURE: the case table, fp64 references and bounds of the attention-pooling kernels (csrc/mappool.hip), shared by
tests/test_mappool_cpu.py (torch stand-ins, tests/mappool_cpu_ops.py) and tests/test_mappool_gpu.py (the kernels).

Shapes: the smallest at which the kernel can go wrong.  The kernel walks a sample in chunks of CHUNK = 32 rows (MP_CH), so
L in {1, 2, 31, 32, 33, 50, 197, 257, 577} puts the last row on the first / last row of a chunk and one past it; (D, H) covers
one to sixteen heads, every accumulator-count instantiation of the kernel (D / 64 <= 4, 12, 16, 22, 32) and widths that are
no multiple of 128; B in {1, 3, 5}; `wg` < B limits the launch to that many workgroups, so a workgroup takes a second (and
third) sample and the dU partial reduction sums more than one term.

Reference: the unfused definition in fp64 on the SAME bf16-rounded x and, at kernel level, the same bf16 U.
Bounds (with p64, dp64, delta64 ... the fp64 quantities):
  z     |z - z64| <= 2^-8 sum_l p64[l,h] |x[l,d]| + 2^-20 max|x|       twice the bf16 half-ulp of p; fp32 accumulation is
                                                                      negligible beside it
  dx    |dx - dx64| <= 2^-7 |dx64| + KAPPA_DX mag_dx                   (2^-7 |ref| covers the bf16 rounding of the stored dx twice over)
  dU    |dU - dU64| <= 2^-7 |dU64| + KAPPA_DU mag_dU
with the magnitudes the sums of absolute values of the terms each output is made of (A = the magnitude of dS):
  A[b,l,h]    = p64[b,l,h] (sum_d |x[b,l,d]| |dz[b,h,d]| + sum_d |z64[b,h,d]| |dz[b,h,d]|)
  mag_dx[b,l,d] = sum_h p64[b,l,h] |dz[b,h,d]| + sum_h A[b,l,h] |U[h,d]|
  mag_dU[h,d]   = sum_{b,l} A[b,l,h] |x[b,l,d]|
KAPPA_* come from the CPU stand-in, never from the kernel: 4 x the stand-in's worst normalised error
max((|err| - 2^-7 |ref|) / mag) over the whole table (the factor covers another summation order on the device).  Measured by

    python -m tests.mappool_cases

which prints the worst normalised errors; the constants below are 4 x those figures, rounded up to two digits.  Moving a
rounding point of the kernel means re-deriving them the same way.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import clip_oracle as O

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
CHUNK = 32

# 4 x (worst normalised error of tests/mappool_cpu_ops over TABLE): `python -m tests.mappool_cases` printed
# "worst: z error / bound 0.786   dx 2.647e-03   dU 3.415e-04" (dx: the bf16 half-ulp 2^-9 = 1.95e-03 of P, dS and dz, two of
# which meet in a term; dU sums the roundings of hundreds of rows, which average out)
KAPPA_DX = 1.1e-2
KAPPA_DU = 1.4e-3


def _case(name, B, L, D, H, kind="gauss", wg=0):
    return {"name": name, "B": B, "L": L, "D": D, "H": H, "kind": kind, "wg": wg}


_DH = [(64, 1), (128, 2), (384, 6), (768, 12), (1280, 16), (1408, 16)]
TABLE = (
    [_case(f"L{L}_D128_H2_B3", 3, L, 128, 2) for L in (1, 2, 31, 32, 33, 50, 197, 257, 577)]
    + [_case(f"L50_D{D}_H{H}_B{B}", B, 50, D, H) for (D, H), B in zip(_DH, (1, 3, 5, 1, 3, 1))]
    + [_case(f"L257_D{D}_H{H}_B{B}", B, 257, D, H) for (D, H), B in zip(_DH, (5, 1, 3, 1, 1, 1))]
    + [_case("second_sample_L33_D128_H2_B5_wg2", 5, 33, 128, 2, wg=2),
       _case("second_sample_L50_D384_H6_B5_wg2", 5, 50, 384, 6, wg=2),
       _case("spread_L197_D128_H2_B3", 3, 197, 128, 2, kind="spread"),
       _case("equal_L65_D128_H2_B3", 3, 65, 128, 2, kind="equal"),
       _case("strided_L50_D128_H2_B3", 3, 50, 128, 2, kind="strided"),
       _case("misaligned_L50_D128_H2_B3", 3, 50, 128, 2, kind="misaligned")]
)


def names(cases):
    return [c["name"] for c in cases]


_CACHE = {}


def inputs(case):
    """-> dict(x bf16 [B*L, D] (possibly a strided view), u bf16 [H, D], dz f32 [B, H, D]) on the CPU, deterministic; computed once."""
    key = case["name"]
    if key in _CACHE:
        return _CACHE[key]
    B, L, D, H, kind = case["B"], case["L"], case["D"], case["H"], case["kind"]
    rng = np.random.RandomState(B * 1000003 + L * 1009 + D * 17 + H)
    x = rng.standard_normal((B, L, D)).astype(np.float32)
    x[..., 3] *= 24.0                                        # a planted large-magnitude channel
    u = (rng.standard_normal((H, D)) * (1.5 / math.sqrt(D))).astype(np.float32)
    u[:, 3] *= 0.25
    if kind == "spread":       # scores that climb by > 60 along the sample, so the running maximum moves in every chunk - and by < 80,
        # so that no probability leaves fp32's normal range (exp(-87) is the smallest): the bounds are relative to p
        x[..., 5] = np.linspace(-3.0, 3.0, L, dtype=np.float32)[None, :] * (1.0 + 0.03 * np.arange(B, dtype=np.float32)[:, None])
        u[:, 5] = 10.0 + 0.5 * np.arange(H, dtype=np.float32)
    if kind == "equal":
        u[:] = 0.0                                           # all scores equal
    dz = rng.standard_normal((B, H, D)).astype(np.float32)
    xt = torch.from_numpy(x).reshape(B * L, D).to(bf16)
    if kind in ("strided", "misaligned"):                    # a column window of a wider buffer: 16-byte aligned rows / rows at 8 bytes
        off = 8 if kind == "strided" else 4
        buf = torch.zeros(B * L, D + 16, dtype=bf16)
        buf[:, off:off + D] = xt
        xt = buf[:, off:off + D]
    r = {"x": xt, "u": torch.from_numpy(u).to(bf16), "dz": torch.from_numpy(dz)}
    _CACHE[key] = r
    return r


_REF = {}


def reference(case, inp=None):
    """The fp64 unfused definition at kernel level and the magnitudes of the bounds; computed once per case."""
    key = case["name"]
    if key in _REF and inp is None:
        return _REF[key]
    inp = inp or inputs(case)
    B, L, D, H = case["B"], case["L"], case["D"], case["H"]
    x = inp["x"].double().reshape(B, L, D).detach().requires_grad_(True)
    u = inp["u"].double().detach().requires_grad_(True)
    dz = inp["dz"].double()
    s = torch.einsum("bld,hd->blh", x, u)
    p = torch.softmax(s, dim=1)
    z = torch.einsum("blh,bld->bhd", p, x)
    z.backward(dz)
    with torch.no_grad():
        xa, ua, dza = x.abs(), u.abs(), dz.abs()
        A = p * (torch.einsum("bld,bhd->blh", xa, dza) + (z.abs() * dza).sum(-1)[:, None])
        r = {"z": z.detach(), "p": p.detach(), "dx": x.grad, "du": u.grad,
             "mag_z": torch.einsum("blh,bld->bhd", p, xa), "xmax": float(xa.max()),
             "mag_dx": torch.einsum("blh,bhd->bld", p, dza) + torch.einsum("blh,hd->bld", A, ua),
             "mag_du": torch.einsum("blh,bld->hd", A, xa), "spread": float((s.amax(1) - s.amin(1)).max())}
    if key not in _REF:
        _REF[key] = r
    return r


def run(ops, dev, case, inp=None, **kw):
    """Forward and backward of `ops` on the case -> (z, stats, dx, du) as CPU tensors."""
    inp = inp or inputs(case)
    B, L, H = case["B"], case["L"], case["H"]
    x = inp["x"].to(dev) if dev != "cpu" else inp["x"]
    if dev != "cpu" and case["kind"] in ("strided", "misaligned"):      # rebuild the view on the device (.to() would densify it)
        off = 8 if case["kind"] == "strided" else 4
        buf = torch.zeros(x.shape[0], x.shape[1] + 16, dtype=bf16, device=dev)
        buf[:, off:off + x.shape[1]] = x
        x = buf[:, off:off + x.shape[1]]
    u, dz = inp["u"].to(dev), inp["dz"].to(dev)
    z, stats = ops.mappool_fwd(x, u, B, L, H, _max_workgroups=case["wg"], **kw.get("fwd", {}))
    dx, du = ops.mappool_bwd(x, u, z, stats, dz, B, L, H, _max_workgroups=case["wg"], **kw.get("bwd", {}))
    return z.cpu(), stats.cpu(), dx.cpu(), du.cpu()


def errors(case, got, inp=None):
    """-> (worst z error / its bound, normalised dx error, normalised dU error); a figure <= 1 / KAPPA_DX / KAPPA_DU passes."""
    ref = reference(case, inp)
    z, stats, dx, du = got
    B, L, D = case["B"], case["L"], case["D"]
    assert torch.isfinite(z).all() and torch.isfinite(dx.float()).all() and torch.isfinite(du).all() and torch.isfinite(stats).all()
    zb = 2.0 ** -8 * ref["mag_z"] + 2.0 ** -20 * ref["xmax"]
    ez = float(((z.double() - ref["z"]).abs() / zb).max())
    edx = (dx.double().reshape(B, L, D) - ref["dx"]).abs() - 2.0 ** -7 * ref["dx"].abs()
    edu = (du.double() - ref["du"]).abs() - 2.0 ** -7 * ref["du"].abs()
    tiny = 1e-300
    return ez, float((edx / (ref["mag_dx"] + tiny)).max().clamp_min(0)), float((edu / (ref["mag_du"] + tiny)).max().clamp_min(0))


def check(ops, dev, case, kdx=KAPPA_DX, kdu=KAPPA_DU, **kw):
    got = run(ops, dev, case, **kw)
    ez, edx, edu = errors(case, got)
    print(f"[{case['name']}] z error / bound {ez:.3f}   dx normalised {edx:.3e} (kappa {kdx:.1e})   dU normalised {edu:.3e} (kappa {kdu:.1e})")
    ref = reference(case)
    m64 = torch.einsum("bld,hd->blh", inputs(case)["x"].double().reshape(case["B"], case["L"], case["D"]), inputs(case)["u"].double()).amax(1)
    assert (got[1][..., 0].double() - m64).abs().max() <= 1e-5 * (1.0 + m64.abs().max()), "softmax statistics: row maximum"
    assert ez <= 1.0, f"z outside its bound by {ez:.3f}x"
    assert edx <= kdx, f"dx normalised error {edx:.3e} > {kdx:.1e}"
    assert edu <= kdu, f"dU normalised error {edu:.3e} > {kdu:.1e}"
    if case["kind"] == "spread":
        assert 60.0 < ref["spread"] < 80.0
    return got


# ---- exact "routed" cases -----------------------------------------------------------------------------------------------------
# Small-integer x; head h looks at channel h alone (U[h, h] = 128), and x[b, l, h] = 1 at the one row l*(b, h), <= 0 elsewhere:
# the winner's score exceeds every other by >= 128 > 104, every other exp() is exactly 0 in fp32, so z[b,h,:] = x[b, l*, :] bit
# for bit; dS = p (dp - delta) is exactly zero (delta = dp at the winner, p = 0 elsewhere), so dx[b, l, :] = the sum of dz[b,h,:]
# over the heads routed to l (small integers: exact in bf16), zero elsewhere, and dU = 0.  The winners differ per head and, over
# the cases, walk over every row position of a chunk.
ROUTED = [
    {"name": "routed_rows0-31_L50_D128_H16_B2", "B": 2, "L": 50, "D": 128, "H": 16, "first": 0, "wg": 0},
    {"name": "routed_rows18-49_L50_D128_H16_B2", "B": 2, "L": 50, "D": 128, "H": 16, "first": 18, "wg": 0},
    {"name": "routed_rows31-32_L33_D64_H2_B1", "B": 1, "L": 33, "D": 64, "H": 2, "first": 31, "wg": 0},
    {"name": "routed_shared_row_L40_D1280_H16_B3_wg2", "B": 3, "L": 40, "D": 1280, "H": 16, "first": 5, "wg": 2, "pair": True},
]


def routed(case):
    """-> (inputs dict, winners int64 [B, H], expected z f32, expected dx bf16 [B*L, D])."""
    B, L, D, H = case["B"], case["L"], case["D"], case["H"]
    rng = np.random.RandomState(L * 131 + D)
    x = rng.randint(-4, 5, size=(B, L, D)).astype(np.float32)
    x[:, :, :H] = rng.randint(-2, 1, size=(B, L, H))
    win = np.zeros((B, H), dtype=np.int64)
    for b in range(B):
        for h in range(H):
            k = b * H + h
            win[b, h] = case["first"] + ((k // 2) if case.get("pair") else k) % (L - case["first"])     # pair: two heads share a row
            x[b, win[b, h], h] = 1.0
    u = np.zeros((H, D), dtype=np.float32)
    u[np.arange(H), np.arange(H)] = 128.0
    dz = rng.randint(-3, 4, size=(B, H, D)).astype(np.float32)
    z = np.stack([x[b, win[b]] for b in range(B)])                       # [B, H, D]
    dx = np.zeros((B, L, D), dtype=np.float32)
    for b in range(B):
        for h in range(H):
            dx[b, win[b, h]] += dz[b, h]
    inp = {"x": torch.from_numpy(x).reshape(B * L, D).to(bf16), "u": torch.from_numpy(u).to(bf16), "dz": torch.from_numpy(dz)}
    assert torch.equal(inp["x"].float().reshape(B, L, D), torch.from_numpy(x))
    return inp, torch.from_numpy(win), torch.from_numpy(z), torch.from_numpy(dx).reshape(B * L, D).to(bf16)


def check_routed(ops, dev, case):
    inp, win, z_want, dx_want = routed(case)
    case = dict(case, kind="routed")
    z, stats, dx, du = run(ops, dev, case, inp)
    assert torch.equal(z, z_want), "z is not the routed row bit for bit"
    assert torch.equal(stats[..., 0], torch.full_like(stats[..., 0], 128.0)) and torch.equal(stats[..., 1], torch.ones_like(stats[..., 1]))
    assert torch.equal(dx, dx_want), "dx is not the routed dz bit for bit"
    assert torch.equal(du, torch.zeros_like(du))


# ---- the head and the model, unfused, in fp64 -----------------------------------------------------------------------------------
def head_unfused(x, sd, pre, H, act, proj, eps=1e-5):
    """The MAP head as clipa_jax/models/vit.py:187-207 states it - K and V projections of every token, one-query multihead
    attention through torch's own multi_head_attention_forward with separate q / k / v weights, LayerNorm, MLP with residual,
    proj - in the dtype of its inputs.  x [B, L, D]; sd: state dict; pre: e.g. "visual.map_head."."""
    B, L, D = x.shape
    w, b = sd[pre + "attn.in_proj_weight"], sd[pre + "attn.in_proj_bias"]
    q = sd[pre + "probe"].expand(1, B, D)
    kv = x.transpose(0, 1)                                               # [L, B, D]
    a, _ = F.multi_head_attention_forward(
        q, kv, kv, D, H, None, b, None, None, False, 0.0, sd[pre + "attn.out_proj.weight"], sd[pre + "attn.out_proj.bias"],
        training=False, need_weights=False, use_separate_proj_weight=True, q_proj_weight=w[:D], k_proj_weight=w[D:2 * D],
        v_proj_weight=w[2 * D:])
    a = a[0]                                                             # [B, D]
    y = O.layer_norm(a, sd[pre + "ln.weight"], sd[pre + "ln.bias"], eps)
    hid = O.activation(y @ sd[pre + "mlp.c_fc.weight"].T + sd[pre + "mlp.c_fc.bias"], act)
    out = a + hid @ sd[pre + "mlp.c_proj.weight"].T + sd[pre + "mlp.c_proj.bias"]
    return out @ proj


def head_folded(x, sd, pre, H, act, proj, eps=1e-5):
    """The same head through the fold the engine uses (engine._map_fold, MapHeadFn), in the dtype of its inputs: U from the probe,
    softmax over x U^T, z = P^T x, the V projection per head on B rows.  bk never enters."""
    B, L, D = x.shape
    dh = D // H
    w, b = sd[pre + "attn.in_proj_weight"], sd[pre + "attn.in_proj_bias"]
    q = sd[pre + "probe"].reshape(1, D) @ w[:D].T + b[:D]
    u = torch.stack([dh ** -0.5 * q[0, h * dh:(h + 1) * dh] @ w[D + h * dh:D + (h + 1) * dh] for h in range(H)])     # [H, D]
    p = torch.softmax(torch.einsum("bld,hd->blh", x, u), dim=1)
    z = torch.einsum("blh,bld->bhd", p, x)
    heads = torch.cat([z[:, h] @ w[2 * D + h * dh:2 * D + (h + 1) * dh].T + b[2 * D + h * dh:2 * D + (h + 1) * dh] for h in range(H)], 1)
    a = heads @ sd[pre + "attn.out_proj.weight"].T + sd[pre + "attn.out_proj.bias"]
    y = O.layer_norm(a, sd[pre + "ln.weight"], sd[pre + "ln.bias"], eps)
    hid = O.activation(y @ sd[pre + "mlp.c_fc.weight"].T + sd[pre + "mlp.c_fc.bias"], act)
    out = a + hid @ sd[pre + "mlp.c_proj.weight"].T + sd[pre + "mlp.c_proj.bias"]
    return out @ proj


TOY = {"embed_dim": 64,
       "vision_cfg": {"image_size": 112, "layers": 2, "width": 128, "patch_size": 16, "pool_style": "big_vision_map",
                      "gelu_approximate": "tanh"},
       "text_cfg": {"context_length": 8, "vocab_size": 64, "width": 64, "heads": 1, "layers": 2}}
TOY_BATCH = 4


def toy_model(patch_dropout=0.0, seed=0, **kw):
    """The toy MAP model (width 128, 2 heads, 2 layers, 112 / 16 = 50 tokens, text width 64) with every parameter moved off its
    initial value (biases and LayerNorm affines are zeros / ones at init), and its batch.  logit_scale starts at log 10, where
    SigLIP - the family this head belongs to - starts its temperature.  That also matters for ONE number of the comparison:
    d loss / d logit_scale is a sum of cancelling terms whose bf16 noise does not shrink with its size and grows with the scale;
    at open_clip's 1 / 0.07 and this batch of 4 its absolute error on the device was measured at 2.5e-4 .. 8.0e-3 over five seeds for
    the MAP head AND for the existing CLS head on the same toy towers (7.9e-3 at seed 0 with MAP, 8.0e-3 at seed 4 with CLS) -
    around the 6e-3 floor tests/test_model_gpu.py::_compare_gradients states for that scalar, so the outcome was a matter of the
    seed, not of the head."""
    import clipa_amd
    torch.manual_seed(seed)
    cfg = {**TOY, "vision_cfg": dict(TOY["vision_cfg"], patch_dropout=patch_dropout)}
    kw.setdefault("init_logit_scale", math.log(10.0))
    m = clipa_amd.CLIP(**cfg, output_dict=True, **kw)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n not in ("logit_scale", "logit_bias"):
                p.add_(torch.randn(p.shape, generator=g) * (0.1 if p.ndim < 2 else 0.02))
    images, texts = O.synthetic_batch(TOY_BATCH, 112, 8, 64, seed + 2)
    return m, images, texts


def toy_reference(m, images, texts, patch_keep=None, loss="clip"):
    """Features, loss and every parameter gradient of the toy model from the unfused definition in fp64 (the towers through
    oracle.clip_oracle's blocks, the head through head_unfused) -> (image features, text features, loss, {name: grad})."""
    sd = {k: v.detach().double().cpu().clone().requires_grad_(v.dtype.is_floating_point) for k, v in m.state_dict().items()}
    ocfg = O.oracle_cfg({k: v for k, v in TOY.items()})
    v = ocfg["vision"]
    P, D, H = v["patch_size"], v["width"], v["heads"]
    image = O.normalize_images(images.cpu(), dtype=f64)
    B, _, S, _ = image.shape
    g = S // P
    x = image.reshape(B, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, 3 * P * P) @ sd["visual.conv1.weight"].reshape(D, -1).T
    x = torch.cat([sd["visual.class_embedding"].expand(B, 1, D), x], dim=1) + sd["visual.positional_embedding"]
    if patch_keep is not None:
        x = torch.cat((x[:, :1], x[:, 1:][torch.arange(B)[..., None], patch_keep]), dim=1)
    x = O.layer_norm(x, sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"])
    for i in range(O._n_layers(sd, "visual.transformer.")):
        x = O.resblock(x, sd, f"visual.transformer.resblocks.{i}.", H, False, v["act"])
    fi = O.l2_normalize(head_unfused(x, sd, "visual.map_head.", H, v["act"], sd["visual.proj"]))
    ft = O.l2_normalize(O.encode_text(sd, ocfg, texts.cpu()))
    scale = sd["logit_scale"].exp()
    if loss == "clip":
        val, _ = O.clip_loss(fi, ft, scale)
    else:      # the pairwise sigmoid loss, clipa_jax/losses/common.py:25-32 (mean over the batch of the row sums)
        logits = scale * fi @ ft.T + sd["logit_bias"]
        y = 2.0 * torch.eye(B, dtype=f64) - 1.0
        val = F.softplus(-y * logits).sum() / B
    val.backward()
    return fi.detach(), ft.detach(), float(val.detach()), {k: t.grad for k, t in sd.items() if t.requires_grad and t.grad is not None}


if __name__ == "__main__":      # the command that measures KAPPA_DX / KAPPA_DU (see the module docstring)
    from . import mappool_cpu_ops as cpu_ops
    worst = [0.0, 0.0, 0.0]
    for c in TABLE:
        e = errors(c, run(cpu_ops, "cpu", c))
        worst = [max(a, b) for a, b in zip(worst, e)]
        print(f"{c['name']:40s} z error / bound {e[0]:.3f}   dx {e[1]:.3e}   dU {e[2]:.3e}")
    print(f"worst: z error / bound {worst[0]:.3f}   dx {worst[1]:.3e}   dU {worst[2]:.3e}   -> KAPPA_DX = {4 * worst[1]:.2e}, KAPPA_DU = {4 * worst[2]:.2e}")
