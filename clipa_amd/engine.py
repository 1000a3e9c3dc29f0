"""Autograd glue of the MI355X engine: coarse-grained torch.autograd.Functions whose forward and
backward are sequences of HIP launches (clipa_amd.ops).  Mirrors, per function, the reference module
it stands in for (paths relative to /root/reference/clipa_torch):

  ResBlockFn     ResidualAttentionBlock.forward            open_clip/transformer.py:238-250
                 (LayerScale, transformer.py:43-50, folded into out_proj / c_proj: _fold_layerscale)
  LastBlockFn    the same for a tower's last block when the head reads one row per sample (returns those rows only)
  VisionStemFn   conv1 + cls/pos + ln_pre                  open_clip/transformer.py:480-503
                 (dual PatchNorm, transformer.py:362-371,483-489, folded into the stem GEMM's operands: _fold_patchnorm)
  TokenDropFn    PatchDropout (row selection)              open_clip/transformer.py:53-83,501-502
  TextStemFn     token_embedding + positional_embedding    open_clip/model.py:245-247
  HeadFn         pool + ln_post/ln_final + projection      transformer.py:509-529, model.py:251-260
  MapHeadFn      multihead attention pooling + projection  clipa_jax/models/vit.py:187-207,282-284 (JAX tree)
  L2NormFn       F.normalize(dim=-1)                       open_clip/model.py:240,263

Activation policy: a block keeps only its bf16 input and recomputes the rest in backward (what the
reference does with --grad-checkpointing, transformer.py:320-325), so ViT-L/16 at local batch 4096
(806 912 tokens) fits in HBM with whole-batch GEMMs (M = 806 912) instead of micro-batches.
"""
import collections
import dataclasses
import weakref

import torch

from . import ops

bf16, f32 = torch.bfloat16, torch.float32


class WeightCache:
    """bf16 operand copies of the parameters ([N,K] forward form and [K,N] transposed form for the
    input-gradient GEMMs), refreshed when the parameter's version counter changes (i.e. once per
    optimizer step).  An entry is valid for (this parameter object, its version counter, its storage address): writes
    that go through `p.data` (EMA, manual weight surgery) bump no counter - call `clear()` (CLIP.invalidate_weight_cache)
    after such writes; `load_state_dict` does it by itself."""

    def __init__(self):
        self._c = {}

    def _get(self, p, kind, make):
        key = (id(p), kind)
        ver = p._version
        ent = self._c.get(key)
        if ent is None or ent[0] != ver or ent[1] != p.data_ptr() or ent[3]() is not p:   # id() may be recycled: weakref check
            with torch.no_grad():
                ent = (ver, p.data_ptr(), make(p.detach()), weakref.ref(p))
            self._c[key] = ent
        return ent[2]

    def w(self, p):   # [N,K] bf16
        return self._get(p, "w", lambda t: t if t.dtype == bf16 else ops.to_bf16(t))

    def wt(self, p):  # [K,N] bf16
        return self._get(p, "wt", ops.transpose_bf16)

    def f32(self, p):  # biases / LN affine as f32 vectors
        return self._get(p, "f32", lambda t: t if t.dtype == f32 else ops.to_f32(t))

    def custom(self, p, kind, make):
        return self._get(p, kind, make)

    def multi(self, ps, kind, make):
        """An operand built from SEVERAL parameters (a LayerScale fold: weight, bias and gamma): valid while every one of them
        is the same object with the same version counter and storage address.  make(*detached tensors)."""
        key = (tuple(id(p) for p in ps), kind)
        state = tuple((p._version, p.data_ptr()) for p in ps)
        ent = self._c.get(key)
        if ent is None or ent[0] != state or any(r() is not p for r, p in zip(ent[2], ps)):
            with torch.no_grad():
                ent = (state, make(*[p.detach() for p in ps]), tuple(weakref.ref(p) for p in ps))
            self._c[key] = ent
        return ent[1]

    def clear(self):
        self._c.clear()


def _like_param(g, p):
    return g if g.dtype == p.dtype else g.to(p.dtype)


def _finish_grads(grads, params, P=None):
    """The gradient tuple an autograd.Function returns for `params`: the LayerScale unfold of a block (P: its operands), each
    gradient in its parameter's dtype, None for a frozen or absent parameter and where nothing was computed."""
    if P is not None:
        grads = _unfold_layerscale(P, grads)
    return tuple(_like_param(g, p) if g is not None and p is not None and p.requires_grad else None for g, p in zip(grads, params))


# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class BlockCfg:
    """A residual block's settings, built by model.Transformer.run.  keep: what the block stores for its backward besides its
    input - "qkv", "a" (attention output + softmax statistics), "x1", "h" (bf16 MLP pre-activation) or "h8" (the same as saturating
    e4m3 bytes written by the c_fc epilogue); the bf16 backward-time recompute adds the LayerNorm outputs and the activation
    that its launches leave behind (Inter, _fill).  fp8 blocks: grad_fmt = ops.FMT_* of the gradient operands, predict = the fp8_predicted_scales knob,
    handoff = the tower's GradHandoff; offer: the LayerNorm-1 backward hands dx to the block in front (not a tower's first)."""
    B: int
    L: int
    H: int
    causal: bool
    act: int
    eps: float
    varlen: object
    fp8: bool
    grad_fmt: int
    predict: bool
    keep: frozenset
    handoff: object
    offer: bool


@dataclasses.dataclass
class Inter:
    """A block's intermediates, named as in BlockCfg.keep: LayerNorm-1 output, qkv, attention output and softmax statistics, x1 =
    x + out_proj(a), LayerNorm-2 output, MLP pre-activation (bf16, or e4m3 bytes: "h8") and activation.  None: not there - not
    kept, not made yet, or already handed on.  The fp8 engine has qkv, a, stats, x1 and hpre only."""
    h1: object = None
    qkv: object = None
    a: object = None
    stats: object = None
    x1: object = None
    h2: object = None
    hpre: object = None
    g: object = None

    def kept(self, keep):
        """What a block stores of these for its backward: the tensors `keep` names; the statistics and the pre-activation are
        there only where "a" / "h" / "h8" made the forward ask for them."""
        return Inter(stats=self.stats, hpre=self.hpre,
                     **{k: getattr(self, k) for k in ("h1", "qkv", "a", "x1", "h2", "g") if k in keep})

    def take(self, *names):
        """-> the named tensors, which leave the container: the taker's locals are then their only owners, and its `del` frees
        them where it stands."""
        vals = [getattr(self, n) for n in names]
        for n in names:
            setattr(self, n, None)
        return vals


def _attn_fwd(qkv, cfg, want_stats):
    """-> (attention output, softmax statistics | None); fixed-length batches or packed variable-length sequences."""
    if cfg.varlen is not None:
        r = ops.attention_fwd_varlen(qkv, cfg.varlen, cfg.H, cfg.causal, want_stats=want_stats)
    else:
        r = ops.attention_fwd(qkv, cfg.B, cfg.L, cfg.H, cfg.causal, want_stats=want_stats)
    return r if want_stats else (r, None)


def _attn_bwd(qkv, a, da, stats, cfg):
    if cfg.varlen is not None:
        return ops.attention_bwd_varlen(qkv, a, da, stats, cfg.varlen, cfg.H, cfg.causal)
    return ops.attention_bwd(qkv, a, da, stats, cfg.B, cfg.L, cfg.H, cfg.causal)


# ---- the half-block stages, bf16.  A stage sees operands (P), a few settings and rows: all tokens of a tower or B gathered rows
def _in_proj(x, P, eps):
    """LayerNorm-1 + in-projection -> (h1, qkv)."""
    h1 = ops.layernorm_fwd(x, P["ln1_w"], P["ln1_b"], eps)
    return h1, ops.gemm_nt(h1, P["w_in"], P["b_in"])


def _out_proj(a, x, P):
    """x1 = x + out_proj(a)."""
    return ops.gemm_nt(a, P["w_out"], P["b_out"], epi=ops.EPI_ADD, aux=x)


def _fc(x1, P, act, eps, want_pre):
    """LayerNorm-2 + c_fc + activation -> (h2, g, hpre); want_pre: False (hpre = None), True (the bf16 pre-activation) or "e4m3"
    (the same as saturating e4m3 bytes written by the epilogue)."""
    h2 = ops.layernorm_fwd(x1, P["ln2_w"], P["ln2_b"], eps)
    if want_pre:
        g, hpre = ops.gemm_nt(h2, P["w_fc"], P["b_fc"], epi=ops.EPI_ACT, act=act, want_pre=want_pre)
    else:
        g, hpre = ops.gemm_nt(h2, P["w_fc"], P["b_fc"], epi=ops.EPI_ACT, act=act), None
    return h2, g, hpre


def _proj(g, x1, P):
    """y = x1 + c_proj(g)."""
    return ops.gemm_nt(g, P["w_proj"], P["b_proj"], epi=ops.EPI_ADD, aux=x1)


def _fill(x, it, P, cfg, want_stats=True, want_pre=True):
    """Whatever `it` lacks of qkv, attention output + statistics, x1 and the MLP pre-activation (with the LayerNorm outputs and
    the activation their launches leave behind), made bit for bit as the forward makes it.  The defaults are the backward's: a
    "medium" block re-runs LN2 + c_fc (one GEMM instead of four + attention), a block that kept nothing re-runs everything but
    c_proj - its output is the next block's input, which that block kept.  The forward fills from nothing and asks only for
    what it keeps (want_stats, want_pre)."""
    if it.qkv is None:
        it.h1, it.qkv = _in_proj(x, P, cfg.eps)
    if it.a is None:
        it.a, it.stats = _attn_fwd(it.qkv, cfg, want_stats)
    if it.x1 is None:
        it.x1 = _out_proj(it.a, x, P)
    if it.hpre is None:
        it.h2, it.g, it.hpre = _fc(it.x1, P, cfg.act, cfg.eps, want_pre)


def _block_forward(x, P, cfg, keep):
    """x [M,D] bf16. P: dict of operand tensors. keep: BlockCfg.keep.  -> (y, the intermediates the block keeps, None: no scales)."""
    it = Inter()
    _fill(x, it, P, cfg, want_stats="a" in keep, want_pre="e4m3" if "h8" in keep else "h" in keep)
    return _proj(it.g, it.x1, P), it.kept(keep), None


# ---- the fp8 engine ----------------------------------------------------------------------------------------------------------
def _lin8(xq, xs, P, name, **kw):
    """fp8 linear: row-quantised activation (xq, xs) against the cached row-quantised weight."""
    wq, ws = P["w8_" + name]
    return ops.gemm_nt_f8(xq, xs, wq, ws, P["b_" + name], **kw)


def _gradq8(dy, cfg):
    """The incoming gradient of a linear layer as fp8 operand, quantised ONCE per token for both of its products (input gradient
    and weight gradient), and its column sums = the layer's bias gradient from the same pass: -> (dq, ds, colsum)."""
    return ops.quantize_rows(dy, cfg.grad_fmt, want_colsum=True)


def _dlin8(dq, ds, P, name, cfg, **kw):
    """fp8 input gradient: the per-token quantised gradient against the cached quantised W^T."""
    wq, ws = P["wt8_" + name]
    return ops.gemm_nt_f8(dq, ds, wq, ws, None, fmt_a=cfg.grad_fmt, **kw)


def _wgrad8(dq, ds, sx, emit, out_dtype, cfg):
    """fp8 weight gradient dW = dY^T X (round 6).  The reduction runs over tokens, so the per-token scale ds of the quantised
    gradient cannot leave the product: the activation operand absorbs it before it is quantised, X8[m,:] = e4m3(ds[m] X[m,:] / t),
    with one device scalar t = max_m ds[m] sx[m] (sx = the activation's own row scale of the forward pass: nothing saturates, no
    amax history, recompute reproduces the bytes) and dW = t * dq^T X8.  emit(ds, t) -> X8 (the kernel that has X at hand)."""
    t = ops.rowscale_max(ds, sx)
    return ops.gemm_tn_f8(dq, emit(ds, t), t=t, fmt_p=cfg.grad_fmt, out_dtype=out_dtype)


def _in_proj_fp8(x, P, eps):
    """LayerNorm-1 (emitting the e4m3 operand) + in-projection -> (qkv, s1: the LayerNorm output's per-token scale)."""
    _, q1, s1 = ops.layernorm_fwd_q8(x, P["ln1_w"], P["ln1_b"], eps)
    return _lin8(q1, s1, P, "in"), s1


def _out_proj_fp8(a, x, P):
    """x1 = x + out_proj(a) -> (x1, sa: the attention output's per-token scale)."""
    qa, sa = ops.quantize_rows(a)
    return _lin8(qa, sa, P, "out", epi=ops.EPI_ADD, aux=x), sa


def _fc_fp8(x1, P, cfg, want_pre):
    """LayerNorm-2 + c_fc + activation -> (qg, sg: the activation as e4m3 operand of c_proj; s2: the LayerNorm output's per-token
    scale; hpre).  want_pre: False / True / "e4m3" as in _fc, or "only" - the backward's rebuild, which wants the bf16
    pre-activation and nothing else (the weight gradient of c_proj re-materialises the activation as an fp8 operand from it,
    _block_backward_fp8): LN2 + the c_fc GEMM with a plain epilogue -> (None, None, s2, hpre)."""
    # Engine knob `fp8_predicted_scales` (round 6, off by default): the activation leaves the c_fc GEMM as the e4m3 operand of
    # c_proj (no bf16 copy, no row quantiser pass).  A tile of the GEMM cannot know its row's maximum, so the row scale is PREDICTED: |h[m,c]| <= ||LN2(x1)[m,:]|| * max_c ||W_fc[c,:]|| +
    # max |b_fc| (Cauchy-Schwarz; 1.13 covers the e4m3 rounding of both operands) and |gelu(h)| <= |h| - a rigorous bound, a few
    # binades above the row's true maximum, well inside e4m3's range.  Every tier uses the same scales (bit-identical forwards);
    # ragged shapes run GEMM + scaled quantiser with the same arithmetic.  Price (tests/test_fp8_gpu.py,
    # DESIGN 4): per-tensor gradient cosines against the fp32 reference 0.001-0.009 lower than with the rows' true maxima.
    if cfg.predict and want_pre != "only":
        _, q2, s2, rn2 = ops.layernorm_fwd_q8(x1, P["ln2_w"], P["ln2_b"], cfg.eps, want_rownorm=True)    # (4 bytes per row)
        sg, so = ops.row_bound(rn2, P["wn_fc"], P["bmax_fc"], 1.13)
        r = _lin8(q2, s2, P, "fc", epi=ops.EPI_ACT, act=cfg.act, want_pre=want_pre, out_scale=so)
        qg, hpre = r if want_pre else (r, None)
        return qg, sg, s2, hpre
    _, q2, s2 = ops.layernorm_fwd_q8(x1, P["ln2_w"], P["ln2_b"], cfg.eps)
    if want_pre == "only":
        return None, None, s2, _lin8(q2, s2, P, "fc")     # bf16(LN2(x1) W^T + b): what the activation epilogue's second output holds
    # the default: bf16 activation + a row quantiser with the row's TRUE maximum
    r = _lin8(q2, s2, P, "fc", epi=ops.EPI_ACT, act=cfg.act, want_pre=want_pre)
    g, hpre = r if want_pre else (r, None)
    del r
    qg, sg = ops.quantize_rows(g)
    return qg, sg, s2, hpre


def _fill_fp8(x, it, P, cfg, want_stats=True, want_pre="only"):
    """_fill for an fp8 block: whatever `it` lacks of (qkv, attention output + statistics, x1, pre-activation), made bit for bit
    as the forward makes it.  -> (qg, (s1, sa, s2, sg)): the e4m3 activation and the per-token scales of the four GEMM inputs
    (LN1 output, attention output, LN2 output, activation), as far as this call made them - the forward, which fills from
    nothing, gets all of them; the backward has the forward's and drops these."""
    s1 = sa = s2 = sg = qg = None
    if it.qkv is None:
        it.qkv, s1 = _in_proj_fp8(x, P, cfg.eps)
    if it.a is None:
        it.a, it.stats = _attn_fwd(it.qkv, cfg, want_stats)
    if it.x1 is None:
        it.x1, sa = _out_proj_fp8(it.a, x, P)
    if it.hpre is None:
        qg, sg, s2, it.hpre = _fc_fp8(it.x1, P, cfg, want_pre)
    return qg, (s1, sa, s2, sg)


def _block_forward_fp8(x, P, cfg, keep):
    """_block_forward with the four linear layers on the fp8 MFMA path (BASELINE.json configs[3]): the LayerNorms emit the
    e4m3 operand of the GEMM that follows them, the attention output and the MLP activation are quantised per token by
    clipa_quantize_rows; everything between the GEMMs (residual stream, attention, softmax statistics, kept tensors) is
    bf16 exactly as in the bf16 engine.  keep: the names of BlockCfg.keep; the LayerNorm outputs and the activation are never
    kept (the fp8 backward re-materialises them as e4m3 operands).  -> (y, the kept intermediates, scales): scales = the
    per-token scales (s1, sa, s2, sg) of the four GEMM inputs, a few MB that every block keeps - the fp8 weight gradients of
    the backward derive their tensor scale from them (_wgrad8)."""
    it = Inter()
    qg, scales = _fill_fp8(x, it, P, cfg, want_stats="a" in keep, want_pre="e4m3" if "h8" in keep else "h" in keep)
    return _lin8(qg, scales[3], P, "proj", epi=ops.EPI_ADD, aux=it.x1), it.kept(keep), scales


class GradHandoff:
    """The LayerNorm-1 backward of block i writes dx = the gradient block i-1 receives - and, in fp8 mode, that gradient's
    row-quantised form with its column sums (ops.layernorm_bwd(q8_fmt=...)): block i-1's backward starts from exactly that (its
    c_proj products and bias gradient).  The autograd edge between two ResBlockFn nodes carries one tensor, so the operand
    travels beside it: one slot per tower, taken (and cleared) by the next fp8 block backward of that tower.  The slot holds dx
    itself, so its memory cannot be recycled while the offer stands: a gradient that arrives with dx's address, shape and version
    IS dx (a summed or copied gradient is another allocation and is quantised the ordinary way)."""

    def __init__(self):
        self._slot = None

    def offer(self, dx, q8, fmt):
        self._slot = (dx, dx._version, fmt, q8)

    def take(self, dy, fmt):
        slot, self._slot = self._slot, None
        if slot is not None:
            dx, version, f, q8 = slot
            if f == fmt and dy.data_ptr() == dx.data_ptr() and dy.shape == dx.shape and dy.stride() == dx.stride() \
                    and dy.dtype == dx.dtype and dy._version == version:      # (the version at the offer: an in-place hook would move it)
                return q8
        return None

    def clear(self):
        self._slot = None


def _in_proj_backward_fp8(x, grad, s1, P, cfg):
    """Input and weight gradient of the in-projection on the fp8 path -> (dh1, d_w_in, d_b_in); the LayerNorm-1 backward that
    takes dh1 is the caller's.  grad: one-element list holding dqkv, popped: this frame is its only owner and frees it early."""
    dq, ds, d_b_in = _gradq8(grad.pop(), cfg)
    d_w_in = _wgrad8(dq, ds, s1, lambda r, t: ops.layernorm_fwd_q8s(x, P["ln1_w"], P["ln1_b"], r, t, cfg.eps), P["dt_w_in"], cfg)
    return _dlin8(dq, ds, P, "in", cfg), d_w_in, d_b_in


def _block_backward_fp8(x, dy, it, P, cfg, scales, offer):
    """Backward of a block in fp8 mode: every matrix product - input gradients AND (round 6) weight gradients - on
    v_mfma_f32_16x16x128_f8f6f4.  Each incoming gradient is quantised once per token (its column sums = the bias gradient ride
    the same pass) and feeds both products of its layer; the activation operand of a weight gradient is emitted as e4m3 by the
    kernel that re-materialises it anyway (LayerNorm, GELU) with the gradient's token scale folded in (_wgrad8).  it: the block's
    intermediates, filled (_fill_fp8) and taken out of it here; offer: hand dx and its fp8 form to the block in front of this
    one (cfg.handoff).  -> (dx, the twelve gradients in param_tuple() order)."""
    act, eps, fmt = cfg.act, cfg.eps, cfg.grad_fmt
    qkv, a, stats, x1, hpre = it.take("qkv", "a", "stats", "x1", "hpre")
    s1, sa, s2, sg = scales
    dy = dy.contiguous()
    # y = x1 + c_proj(gelu(hpre)); (dq, ds, colsum[, rownorm: the predicted scales only])
    q8 = cfg.handoff.take(dy, fmt) or ops.quantize_rows(dy, fmt, want_colsum=True, want_rownorm=cfg.predict)
    dq, ds, d_b_proj = q8[:3]
    predict_dh = cfg.predict and fmt == ops.FMT_E4M3
    if hpre.dtype == torch.uint8 and not predict_dh:
        # (round 6) the GELU-backward epilogue of the input-gradient GEMM reads the kept e4m3 pre-activation anyway: it also emits the
        # activation operand of this layer's weight gradient (ops.gemm_nt_f8_emit) - the weight gradient then follows the input gradient
        t = ops.rowscale_max(ds, sg)
        wq, ws = P["wt8_proj"]
        dh, x8 = ops.gemm_nt_f8_emit(dq, ds, wq, ws, hpre, t, act=act, fmt_a=fmt)
        d_w_proj = ops.gemm_tn_f8(dq, x8, t=t, fmt_p=fmt, out_dtype=P["dt_w_proj"])
        del x8
        dq, ds, d_b_fc = _gradq8(dh, cfg)
        del dh
    else:
        d_w_proj = _wgrad8(dq, ds, sg, lambda r, t: ops.scale_quantize_rows(hpre, r, t, act=act), P["dt_w_proj"], cfg)
        if predict_dh:
            # the gradient of the pre-activation leaves the GEMM as the e4m3 operand of the next two products, with its column
            # sums (the bias gradient of c_fc) from the same epilogue; row scale predicted as in the forward: |dh[m,c]| <=
            # ||dy[m,:]|| * max_c ||W_proj[:,c]|| * max gelu' (1.13), times 1.13 for the operands' rounding
            sdh, sodh = ops.row_bound(q8[3], P["wn_projT"], None, 1.13 * 1.13)
            dq, d_b_fc = _dlin8(dq, ds, P, "proj", cfg, epi=ops.EPI_DACT, act=act, aux=hpre, out_scale=sodh, want_colsum=True)
            ds = sdh
        else:   # bf16 gradient + the row quantiser
            dh = _dlin8(dq, ds, P, "proj", cfg, epi=ops.EPI_DACT, act=act, aux=hpre)     # [M,4D]
            dq, ds, d_b_fc = _gradq8(dh, cfg)
            del dh
    del hpre, q8
    d_w_fc = _wgrad8(dq, ds, s2, lambda r, t: ops.layernorm_fwd_q8s(x1, P["ln2_w"], P["ln2_b"], r, t, eps), P["dt_w_fc"], cfg)
    dh2 = _dlin8(dq, ds, P, "fc", cfg)                                            # [M,D]
    del dq, ds
    # (round 6) the two LayerNorm backwards hand the next product its fp8 operand themselves: the rows are in registers
    dx1, d_ln2_w, d_ln2_b, (dq, ds, d_b_out) = ops.layernorm_bwd(x1, P["ln2_w"], dh2, dres=dy, eps=eps, q8_fmt=fmt)
    del dh2, x1
    # x1 = x + out_proj(a)
    d_w_out = _wgrad8(dq, ds, sa, lambda r, t: ops.scale_quantize_rows(a, r, t), P["dt_w_out"], cfg)
    da = _dlin8(dq, ds, P, "out", cfg)
    del dq, ds
    grad = [_attn_bwd(qkv, a, da, stats, cfg)]
    del da, a, qkv, stats
    dh1, d_w_in, d_b_in = _in_proj_backward_fp8(x, grad, s1, P, cfg)
    if offer:      # the block in front of this one runs the same engine: its backward starts from (q, dq, colsum[, rownorm])
        dx, d_ln1_w, d_ln1_b, q8 = ops.layernorm_bwd(x, P["ln1_w"], dh1, dres=dx1, eps=eps, q8_fmt=fmt, want_rownorm=cfg.predict)
        cfg.handoff.offer(dx, q8, fmt)
    else:
        dx, d_ln1_w, d_ln1_b = ops.layernorm_bwd(x, P["ln1_w"], dh1, dres=dx1, eps=eps)
    return dx, (d_ln1_w, d_ln1_b, d_w_in, d_b_in, d_w_out, d_b_out, d_ln2_w, d_ln2_b, d_w_fc, d_b_fc, d_w_proj, d_b_proj)


def _mlp_backward(dy, it, P, act, eps):
    """Backward of y = x1 + c_proj(act(c_fc(LN2(x1)))) on the rows of dy -> (dx1, (d_ln2_w, d_ln2_b, d_w_fc, d_b_fc, d_w_proj,
    d_b_proj)).  Takes x1, h2, hpre and g out of `it` and frees each after its last use.  hpre is there; g and h2 may be missing:"""
    x1, h2, hpre, g = it.take("x1", "h2", "hpre", "g")
    # "light8" block: the GELU-backward epilogue below reads the e4m3 bytes anyway and writes act(hpre) beside its own output
    # (round 6: one more store per chunk instead of an HBM-bound pass over the same bytes; bit for bit what activation_fwd writes)
    fuse_act = g is None and hpre.dtype == torch.uint8
    if g is None and not fuse_act:      # "light" block: cheap HBM-bound re-materialisation instead of 4 GEMMs + attention
        g = ops.activation_fwd(hpre, act)
    # A LayerNorm output that only the weight gradient still needs (h2 of a block that kept its MLP pre-activation; likewise h1
    # of a block that kept qkv, _block_backward) is written by the LayerNorm BACKWARD pass, which has every row and its
    # statistics in registers anyway (ops.layernorm_bwd(beta=...): bit for bit ln_fwd's output) - one more store per row instead of
    # a second ln_fwd launch over the same rows; the weight gradient of c_fc / the in-projection then follows its LayerNorm
    # backward instead of preceding it.
    emit2 = h2 is None
    # y = x1 + c_proj(g).  The weight gradient goes first: g ([M, 4D], the largest transient of the block) is released before
    # the GELU-backward GEMM allocates its output of the same size
    if fuse_act:         # (here g and dh coexist: dy + g + dh = 1.65 GB more than the block's later peak dh + dh2 + dx1 + h2 + dy)
        dh, g = ops.gemm_nt(dy, P["wt_proj"], epi=ops.EPI_DACT, act=act, aux=hpre, want_act=True)
        del hpre
        d_w_proj, d_b_proj = ops.gemm_tn(dy, g, P["dt_w_proj"], want_colsum=True)
        del g
    else:
        d_w_proj, d_b_proj = ops.gemm_tn(dy, g, P["dt_w_proj"], want_colsum=True)
        del g
        dh = ops.gemm_nt(dy, P["wt_proj"], epi=ops.EPI_DACT, act=act, aux=hpre)     # [M,4D]
        del hpre
    dh2 = ops.gemm_nt(dh, P["wt_fc"])       # [M,D]
    if emit2:
        dx1, d_ln2_w, d_ln2_b, h2 = ops.layernorm_bwd(x1, P["ln2_w"], dh2, dres=dy, eps=eps, beta=P["ln2_b"])
        del dh2, x1
        d_w_fc, d_b_fc = ops.gemm_tn(dh, h2, P["dt_w_fc"], want_colsum=True)
        del dh, h2
    else:
        d_w_fc, d_b_fc = ops.gemm_tn(dh, h2, P["dt_w_fc"], want_colsum=True)
        del dh, h2
        dx1, d_ln2_w, d_ln2_b = ops.layernorm_bwd(x1, P["ln2_w"], dh2, dres=dy, eps=eps)
        del dh2, x1
    return dx1, (d_ln2_w, d_ln2_b, d_w_fc, d_b_fc, d_w_proj, d_b_proj)


def _out_proj_backward(dx1, a, P):
    """Backward of x1 = x + out_proj(a) -> (da, d_w_out, d_b_out)."""
    da = ops.gemm_nt(dx1, P["wt_out"])
    d_w_out, d_b_out = ops.gemm_tn(dx1, a, P["dt_w_out"], want_colsum=True)
    return da, d_w_out, d_b_out


def _block_backward(x, dy, it, P, cfg):
    """it: the block's intermediates, filled (_fill); they are taken out of it so that they can be freed early.  bf16 engines
    (the fp8 engine: _block_backward_fp8).  -> (dx, the twelve gradients in param_tuple() order)."""
    dy = dy.contiguous()
    dx1, d_mlp = _mlp_backward(dy, it, P, cfg.act, cfg.eps)
    qkv, a, stats, h1 = it.take("qkv", "a", "stats", "h1")
    da, d_w_out, d_b_out = _out_proj_backward(dx1, a, P)
    dqkv = _attn_bwd(qkv, a, da, stats, cfg)
    del da, a, qkv, stats
    dh1 = ops.gemm_nt(dqkv, P["wt_in"])
    if h1 is None:      # a block that kept qkv: the LayerNorm backward emits h1 (see _mlp_backward)
        dx, d_ln1_w, d_ln1_b, h1 = ops.layernorm_bwd(x, P["ln1_w"], dh1, dres=dx1, eps=cfg.eps, beta=P["ln1_b"])
        d_w_in, d_b_in = ops.gemm_tn(dqkv, h1, P["dt_w_in"], want_colsum=True)
        del dqkv, h1
    else:
        d_w_in, d_b_in = ops.gemm_tn(dqkv, h1, P["dt_w_in"], want_colsum=True)
        del dqkv, h1
        dx, d_ln1_w, d_ln1_b = ops.layernorm_bwd(x, P["ln1_w"], dh1, dres=dx1, eps=cfg.eps)
    return dx, (d_ln1_w, d_ln1_b, d_w_in, d_b_in, d_w_out, d_b_out) + d_mlp


def _fold_layerscale(P, cache, cfg, fp8_names, name, w, b, gamma):
    """LayerScale (transformer.py:43-50: x + gamma * (a W^T + b), :248-249) of the layer `name` ("out" / "proj"), folded into its
    operands: W' = diag(gamma) W and b' = gamma * b replace W and b in every operand form the block's launches read (forward,
    transposed, fp8, the predicted scales' row norm), so no launch changes.  The folded copies live in the weight cache under
    (W, b, gamma) together: a step of any of the three rebuilds them.  The layer's weight-gradient product is requested in f32:
    it is dW' = dY^T X, from which _unfold_layerscale takes the parameters' gradients."""
    ps = (w, b, gamma)
    fold = lambda: cache.multi(ps, "ls", lambda wt, bt, gt: ops.layerscale_fold(wt, cache.f32(gamma), cache.f32(b)))
    wT = lambda: cache.multi(ps, "ls_wt", lambda *t: ops.transpose_bf16(fold()[0]))
    P["w_" + name], P["b_" + name] = fold()
    P["wt_" + name] = wT()
    P["dt_w_" + name] = f32
    if cfg.fp8 and name in fp8_names:
        P["w8_" + name] = cache.multi(ps, "ls_w8", lambda *t: ops.quantize_rows(fold()[0]))
        P["wt8_" + name] = cache.multi(ps, "ls_wt8", lambda *t: ops.quantize_rows(wT()))
        if cfg.predict and name == "proj" and "fc" in fp8_names:
            P["wn_projT"] = cache.multi(ps, "ls_wnT", lambda *t: ops.rownorm_max(wT()))
    return (name, w, b, gamma, cache.f32(gamma), cache.f32(b))


def _unfold_layerscale(P, grads):
    """Blocks with LayerScale: the gradients of the two folded layers (dW' in f32, db') become those of the parameters, dW =
    diag(gamma) dW', db = gamma * db', plus dgamma = rowsum(dW' * W) + db' * b (ops.layerscale_unfold); -> the block's gradient
    tuple with d(ls_1.gamma), d(ls_2.gamma) appended.  A frozen parameter's gradient is not computed."""
    if "ls" not in P:
        return grads
    grads = list(grads)
    slot = {"out": (4, 5), "proj": (10, 11)}      # (weight, bias) of the layer in the gradient tuple
    for name, w, b, gamma, gamma32, b32 in P["ls"]:
        iw, ib = slot[name]
        grads[iw], grads[ib], dg = ops.layerscale_unfold(grads[iw], w.detach(), gamma32, grads[ib], b32, out_dtype=w.dtype,
                                                         want=(w.requires_grad, b.requires_grad, gamma.requires_grad))
        grads.append(dg)
    return tuple(grads)


def _mlp_operands(cache, ln_w, ln_b, layers, backward=True):
    """Operands of a LayerNorm + linear layers: the LayerNorm's affine as f32 ("ln2_w", "ln2_b": the one in front of an MLP) and
    per (name, weight, bias) layer "w_" ([N,K] bf16), "b_" (f32) and - backward - "wt_" (the transposed [K,N] copy of the input
    gradient) and "dt_w_" (the dtype its weight gradient is asked for)."""
    P = {"ln2_w": cache.f32(ln_w), "ln2_b": cache.f32(ln_b)}
    for name, w, b in layers:
        P["w_" + name], P["b_" + name] = cache.w(w), cache.f32(b)
        if backward:
            P["wt_" + name], P["dt_w_" + name] = cache.wt(w), w.dtype
    return P


def _block_operands(params, cache, cfg, fp8_names=("in", "out", "fc", "proj")):
    """params: _ResBlockParams.param_tuple() - twelve tensors, and the two LayerScale gammas behind them when the block has any."""
    ln1_w, ln1_b, w_in, b_in, w_out, b_out, ln2_w, ln2_b, w_fc, b_fc, w_proj, b_proj = params[:12]
    layers = (("in", w_in, b_in), ("out", w_out, b_out), ("fc", w_fc, b_fc), ("proj", w_proj, b_proj))
    # layers whose operands are the LayerScale-folded ones (_fold_layerscale) instead of the parameter's own copies
    folded = {"out": params[12], "proj": params[13]} if len(params) > 12 else {}
    P = _mlp_operands(cache, ln2_w, ln2_b, [layer for layer in layers if layer[0] not in folded])
    P["ln1_w"], P["ln1_b"] = cache.f32(ln1_w), cache.f32(ln1_b)
    if cfg.fp8:   # e4m3 copies, one scale per output channel of the GEMM they feed (rows of W forward, rows of W^T backward); only
        # of the layers that run on the fp8 path (LastBlockFn: the in-projection alone - its B pooled rows take the bf16 GEMMs)
        for name, w, _ in layers:
            if name not in fp8_names or name in folded:
                continue
            P["w8_" + name] = cache.custom(w, "w8", lambda t, w=w: ops.quantize_rows(cache.w(w)))
            P["wt8_" + name] = cache.custom(w, "wt8", lambda t, w=w: ops.quantize_rows(cache.wt(w)))
        if cfg.predict and "fc" in fp8_names:
            # the two scalars per layer behind the PREDICTED row scales of the MLP's 4 D-wide products (ops.row_bound): the largest
            # row norm of c_fc.weight and |c_fc.bias| bound the pre-activation, the largest row norm of c_proj.weight^T the
            # gradient that comes back through c_proj; device scalars, refreshed with the operand copies once per optimizer step
            P["wn_fc"] = cache.custom(w_fc, "wn", lambda t: ops.rownorm_max(cache.w(w_fc)))
            P["bmax_fc"] = cache.custom(b_fc, "bmax", lambda t: ops.absmax(cache.f32(b_fc)))
            if "proj" not in folded:
                P["wn_projT"] = cache.custom(w_proj, "wnT", lambda t: ops.rownorm_max(cache.wt(w_proj)))
    if folded:
        P["ls"] = tuple(_fold_layerscale(P, cache, cfg, fp8_names, name, w, b, folded[name]) for name, w, b in layers
                        if name in folded)
    return P


class ResBlockFn(torch.autograd.Function):
    """x + MHA(LN1(x)); then + MLP(LN2(.)) on a [M, D] bf16 token matrix (transformer.py:238-250)."""

    @staticmethod
    def forward(ctx, x, cfg, cache, *params):
        P = _block_operands(params, cache, cfg)
        needs_grad = any(ctx.needs_input_grad)
        y, kept, scales = (_block_forward_fp8 if cfg.fp8 else _block_forward)(x, P, cfg, cfg.keep if needs_grad else frozenset())
        ctx.cfg, ctx.cache, ctx.params = cfg, cache, params
        if needs_grad:
            ctx.save_for_backward(x)
            ctx.inter, ctx.scales = kept, scales
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        cfg, params = ctx.cfg, ctx.params
        P = _block_operands(params, ctx.cache, cfg)
        it, ctx.inter = ctx.inter, None
        if cfg.fp8:
            scales, ctx.scales = ctx.scales, None
            _fill_fp8(x, it, P, cfg)
            dx, grads = _block_backward_fp8(x, dy, it, P, cfg, scales, offer=cfg.offer and ctx.needs_input_grad[0])
        else:
            _fill(x, it, P, cfg)
            dx, grads = _block_backward(x, dy, it, P, cfg)
        return (dx, None, None) + _finish_grads(grads, params, P)


# ---------------------------------------------------------------------------------------------
class LastBlockFn(torch.autograd.Function):
    """The LAST residual block of a tower whose head reads ONE row per sample (the class token of a CLS-pooled image tower,
    transformer.py:509-529; the EOT token of the text tower, model.py:251-254): returns that row only, [B, D].

    Every other row of the last block's output is dead - nothing reads it, its gradient is exactly zero - so only the keys and
    values need all tokens: LN1, the in-projection and attention run on every row, the out-projection, LN2 and the MLP on the B
    pooled rows (the reference computes all B * L of them and the pooling discards them; same kind of identity as taking the
    pooled row before ln_post, SURVEY 8a identity 8).  fp8 engines (round 5): the token-level part - LN1, in-projection and its
    input gradient - runs on the fp8 path like every other block; the B pooled rows (0.5 % of a block's rows) run the bf16 GEMMs.  Forward values of the pooled rows and all gradients are those of the full
    block (zero rows add nothing to a weight gradient).  `rows`: int64 device tensor [B], row index of the pooled token of each
    sample in x.  The token-level part (qkv, attention output, softmax statistics) is kept or recomputed like any other block's;
    the B-row part is always kept (a few MB).  Both parts are the block's own stages, on M rows and on B rows."""

    @staticmethod
    def forward(ctx, x, rows, cfg, cache, *params):
        P = _block_operands(params, cache, cfg, fp8_names=("in",))
        needs_grad = any(ctx.needs_input_grad)
        # token-level tensors this block keeps: the block's keep set like any other block's ("qkv", "a" = attention output +
        # softmax statistics); x1 / the pre-activation exist for the B pooled rows only
        keep = cfg.keep if needs_grad else frozenset()
        tokens = Inter()
        s1 = LastBlockFn._fill_tokens(x, tokens, P, cfg, "a" in keep)
        a_c, x_c = ops.gather_rows(tokens.a, rows), ops.gather_rows(x, rows)
        small = Inter(a=a_c, x1=_out_proj(a_c, x_c, P))
        small.h2, small.g, small.hpre = _fc(small.x1, P, cfg.act, cfg.eps, True)
        y = _proj(small.g, small.x1, P)
        ctx.cfg, ctx.cache, ctx.params = cfg, cache, params
        if needs_grad:
            ctx.save_for_backward(x, rows)
            ctx.tokens, ctx.small, ctx.s1 = tokens.kept(keep), small, s1
        return y

    @staticmethod
    def _fill_tokens(x, it, P, cfg, want_stats):
        """The token-level part of _fill / _fill_fp8: qkv and the attention output where `it` lacks them.  -> fp8 engines, when
        qkv was made: the LayerNorm output's per-token scale (the weight gradient's tensor scale, _wgrad8)."""
        s1 = None
        if it.qkv is None:
            if cfg.fp8:
                it.qkv, s1 = _in_proj_fp8(x, P, cfg.eps)
            else:
                it.qkv = _in_proj(x, P, cfg.eps)[1]
        if it.a is None:
            it.a, it.stats = _attn_fwd(it.qkv, cfg, want_stats)
        return s1

    @staticmethod
    def backward(ctx, dy):
        x, rows = ctx.saved_tensors
        cfg, params = ctx.cfg, ctx.params
        P = _block_operands(params, ctx.cache, cfg, fp8_names=("in",))
        small, ctx.small = ctx.small, None
        a_c, M = small.a, x.shape[0]
        dy = dy.contiguous()
        dx1, d_mlp = _mlp_backward(dy, small, P, cfg.act, cfg.eps)
        da_c, d_w_out, d_b_out = _out_proj_backward(dx1, a_c, P)
        tokens, ctx.tokens = ctx.tokens, None
        refilled = tokens.qkv is None or tokens.a is None
        LastBlockFn._fill_tokens(x, tokens, P, cfg, True)      # whatever the block did not keep is recomputed bit for bit
        qkv, a, stats = tokens.take("qkv", "a", "stats")
        # A block that recomputed any of them has always held the attention output and the statistics to the end of its backward
        # (a second pair of names kept them from the `del` below).  The keep planner's budget is measured against that peak, so
        # this stays as it is here; letting them go with qkv is one line, and a change of the step's memory profile of its own.
        held = (a, stats) if refilled else None  # noqa: F841
        grad = [_attn_bwd(qkv, a, ops.scatter_rows(da_c, rows, M), stats, cfg)]
        del qkv, a, stats
        if cfg.fp8:      # token-level products of the block on the fp8 path: input and weight gradient of the in-projection
            s1, ctx.s1 = ctx.s1, None
            dh1, d_w_in, d_b_in = _in_proj_backward_fp8(x, grad, s1, P, cfg)
        else:      # (not _block_backward's: h1 comes from a second ln_fwd between the two products, not from the LayerNorm backward)
            dqkv = grad.pop()
            dh1 = ops.gemm_nt(dqkv, P["wt_in"])
            h1 = ops.layernorm_fwd(x, P["ln1_w"], P["ln1_b"], cfg.eps)
            d_w_in, d_b_in = ops.gemm_tn(dqkv, h1, P["dt_w_in"], want_colsum=True)
            del dqkv, h1
        # x1 = x[rows] + out_proj(a[rows]): the residual gradient reaches x at the pooled rows only
        dx, d_ln1_w, d_ln1_b = ops.layernorm_bwd(x, P["ln1_w"], dh1, dres=ops.scatter_rows(dx1, rows, M), eps=cfg.eps)
        grads = (d_ln1_w, d_ln1_b, d_w_in, d_b_in, d_w_out, d_b_out) + d_mlp
        return (dx, None, None, None) + _finish_grads(grads, params, P)


# ---------------------------------------------------------------------------------------------
def _conv_weight_operand(w, Kp):
    """conv1.weight [D,3,P,P] -> bf16 [D,Kp] in (ph,pw,c) element order, zero padded to Kp."""
    D = w.shape[0]
    k = w.shape[1] * w.shape[2] * w.shape[3]
    m = w.permute(0, 2, 3, 1).reshape(D, k)
    if Kp != k:
        m = torch.nn.functional.pad(m, (0, Kp - k))
    return ops.to_bf16(m.contiguous())


# VisionStemFn: B images of L tokens, P x P patches (K = 3 P P zero-padded to Kp), mean / std of uint8 images (None: float
# input), whether ln_pre exists, patchnorm: dual PatchNorm (input_patchnorm) - a LayerNorm over each patch in front of a Linear
StemCfg = collections.namedtuple("StemCfg", "B L P Kp eps ln_pre mean std patchnorm", defaults=(False,))


def _vision_stem_forward(image, P, cfg):
    if cfg.patchnorm:      # xhat W'^T + b' == LayerNorm_K(patches) W^T + b (_fold_patchnorm)
        patches = ops.patchify_ln(image, cfg.P, cfg.Kp, cfg.mean, cfg.std, cfg.eps)
        pe = ops.gemm_nt(patches, P["w_conv"], P["b_conv"])
    else:
        patches = ops.patchify(image, cfg.P, cfg.Kp, cfg.mean, cfg.std)
        pe = ops.gemm_nt(patches, P["w_conv"])
    tok = ops.assemble_tokens(pe, P["cls"], P["pos"], cfg.B, cfg.L)
    x0 = ops.layernorm_fwd(tok, P["ln_w"], P["ln_b"], cfg.eps) if cfg.ln_pre else tok
    return patches, tok, x0


def _fold_patchnorm(cache, cfg, conv_w, conv_b, pn_w, pn_b):
    """Dual PatchNorm (transformer.py:362-371,483-489: patchnorm_pre_ln = LayerNorm(K), conv1 = nn.Linear(K, width)) folded into
    the stem GEMM's operands: LayerNorm_K(x) W^T + b == xhat (W diag(gamma))^T + (b + W beta), xhat = (x - mean) * rstd from
    ops.patchify_ln.  -> (W' bf16 [D,Kp] in the engine's (ph,pw,c) column order, b' f32 [D]); cached under the four parameters
    together: a step of any of them rebuilds the pair."""
    return cache.multi((conv_w, conv_b, pn_w, pn_b), "pn%d" % cfg.Kp,
                       lambda w, b, g, bt: ops.patchnorm_fold(w, cache.f32(conv_b), cache.f32(pn_w), cache.f32(pn_b), cfg.P, cfg.Kp))


class VisionStemFn(torch.autograd.Function):
    """uint8/float image -> normalise -> patch GEMM -> [cls; patches] + pos -> ln_pre
    (train.py:191-197 + transformer.py:480-503).  cfg.patchnorm: `pn` = (conv1.bias, patchnorm_pre_ln.weight,
    patchnorm_pre_ln.bias) and conv_w is the Linear's [D, K] matrix; else `pn` is empty and conv_w the convolution's [D,3,P,P]."""

    @staticmethod
    def forward(ctx, image, cfg, cache, conv_w, cls, pos, ln_w, ln_b, *pn):
        if len(pn) != (3 if cfg.patchnorm else 0):
            raise RuntimeError("VisionStemFn: patchnorm takes conv1.bias, patchnorm_pre_ln.weight and patchnorm_pre_ln.bias")
        P = VisionStemFn._operands(cfg, cache, conv_w, cls, pos, ln_w, ln_b, *pn)
        _, _, x0 = _vision_stem_forward(image, P, cfg)
        ctx.cfg, ctx.cache = cfg, cache
        ctx.params = (conv_w, cls, pos, ln_w, ln_b) + pn
        ctx.save_for_backward(image)
        return x0

    @staticmethod
    def _operands(cfg, cache, conv_w, cls, pos, ln_w, ln_b, *pn):
        Kp = cfg.Kp
        if cfg.patchnorm:
            P = dict(zip(("w_conv", "b_conv"), _fold_patchnorm(cache, cfg, conv_w, *pn)))
        else:
            P = {"w_conv": cache.custom(conv_w, "conv%d" % Kp, lambda t: _conv_weight_operand(t, Kp))}
        P["cls"], P["pos"] = cache.f32(cls), cache.f32(pos)
        if cfg.ln_pre:
            P["ln_w"], P["ln_b"] = cache.f32(ln_w), cache.f32(ln_b)
        return P

    @staticmethod
    def backward(ctx, dx0):
        (image,) = ctx.saved_tensors
        cfg = ctx.cfg
        conv_w, cls, pos, ln_w, ln_b = ctx.params[:5]
        P = VisionStemFn._operands(cfg, ctx.cache, *ctx.params)
        patches, tok, _ = _vision_stem_forward(image, P, cfg)
        dx0 = dx0.contiguous()
        d_ln_w = d_ln_b = None
        if cfg.ln_pre:
            dtok, d_ln_w, d_ln_b = ops.layernorm_bwd(tok, P["ln_w"], dx0, eps=cfg.eps)
        else:
            dtok = dx0
        dpatch, dcls, dpos = ops.assemble_tokens_bwd(dtok, cfg.B, cfg.L, need_pos=pos.requires_grad)
        d_conv, d_pn = None, ()
        if cfg.patchnorm:
            # G = dPE^T xhat (f32, as the LayerScale layers ask for theirs) and s = colsum(dPE) = d conv1.bias: one reduction
            # kernel turns them into dW = gamma G + beta s, dgamma = sum_n W G, dbeta = sum_n W s.  No input-gradient GEMM:
            # the image gets no gradient
            conv_b, pn_w, pn_b = ctx.params[5:]
            d_pn = (None, None, None)
            if any(p.requires_grad for p in (conv_w, conv_b, pn_w, pn_b)):
                G, s = ops.gemm_tn(dpatch, patches, f32, want_colsum=True)      # [D, Kp (ph,pw,c)], [D]
                want = (conv_w.requires_grad, pn_w.requires_grad, pn_b.requires_grad)
                if any(want):
                    d_conv, d_g, d_b = ops.patchnorm_unfold(G, s, conv_w.detach(), ctx.cache.f32(pn_w), ctx.cache.f32(pn_b), cfg.P,
                                                            out_dtype=conv_w.dtype, want=want)
                    d_pn = (s, d_g, d_b)
                else:
                    d_pn = (s, None, None)
        elif conv_w.requires_grad:
            D, C, Pp, _ = conv_w.shape
            k = C * Pp * Pp
            dw = ops.gemm_tn(dpatch, patches, f32)[:, :k]                     # [D, (ph,pw,c)]
            d_conv = dw.reshape(D, Pp, Pp, C).permute(0, 3, 1, 2).contiguous()
        return (None, None, None) + _finish_grads((d_conv, dcls, dpos, d_ln_w, d_ln_b) + d_pn, ctx.params)


class TokenDropFn(torch.autograd.Function):
    """PatchDropout (transformer.py:53-83, applied at :501-502): keep the rows `rows` (int64, device) of the [B*L, D] token
    matrix - the class token of every sample and its randomly kept patches.  Forward = row gather, backward = row scatter
    into zeros.  (The reference drops BEFORE ln_pre; LayerNorm is per token, so dropping after it selects the same values.)"""

    @staticmethod
    def forward(ctx, x, rows):
        ctx.save_for_backward(rows)
        ctx.n_src = x.shape[0]
        return ops.gather_rows(x, rows)

    @staticmethod
    def backward(ctx, dy):
        (rows,) = ctx.saved_tensors
        return ops.scatter_rows(dy.contiguous(), rows, ctx.n_src), None


class TextStemFn(torch.autograd.Function):
    """token_embedding(text).to(bf16) + positional_embedding.to(bf16) (model.py:245-247)."""

    @staticmethod
    def forward(ctx, ids, cache, table, pos):
        x0 = ops.embed_tokens(ids, table.detach(), cache.f32(pos))
        ctx.save_for_backward(ids)
        ctx.params = (table, pos)
        return x0

    @staticmethod
    def backward(ctx, dx0):
        (ids,) = ctx.saved_tensors
        table, pos = ctx.params
        dtable, dpos = ops.embed_tokens_bwd(ids, dx0.contiguous(), table.shape[0], need_table=table.requires_grad,
                                            need_pos=pos.requires_grad)
        return (None, None) + _finish_grads((dtable, dpos), ctx.params)


HeadCfg = collections.namedtuple("HeadCfg", "B L mode eps")      # HeadFn: B samples of L rows, pooled by ops.POOL_* `mode`


class HeadFn(torch.autograd.Function):
    """pool -> LayerNorm -> @ proj, returning f32 features [B,E].  Pooling commutes with the per-token
    LayerNorm, so LN runs on B rows instead of B*L (SURVEY 8a identity 8)."""

    @staticmethod
    def forward(ctx, x, idx, cfg, cache, ln_w, ln_b, proj):
        B, L, mode = cfg.B, cfg.L, cfg.mode
        pooled = ops.pool_fwd(x, B, L, mode, idx)                            # f32 [B,D]
        y = ops.layernorm_fwd(pooled, cache.f32(ln_w), cache.f32(ln_b), cfg.eps, out_dtype=bf16)
        feat = ops.gemm_nt(y, cache.wt(proj), out_f32=True) if proj is not None else ops.to_f32(y)
        ctx.cfg, ctx.cache, ctx.params = cfg, cache, (ln_w, ln_b, proj)
        ctx.save_for_backward(pooled, y, idx if idx is not None else torch.empty(0, device=x.device))
        ctx.has_idx = idx is not None
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        pooled, y, idx = ctx.saved_tensors
        idx = idx if ctx.has_idx else None
        cfg, cache = ctx.cfg, ctx.cache
        ln_w, ln_b, proj = ctx.params
        dfb = ops.to_bf16(dfeat.contiguous())
        d_proj = None
        if proj is not None:
            dy = ops.gemm_nt(dfb, cache.w(proj))                              # [B,E] @ proj[D,E]^T -> [B,D]
            if proj.requires_grad:
                d_proj = _like_param(ops.gemm_tn(y, dfb, f32), proj)          # [D,E] (cast here: the f32 product is gone before dx)
        else:
            dy = dfb
        dpooled, d_ln_w, d_ln_b = ops.layernorm_bwd(pooled, cache.f32(ln_w), dy, eps=cfg.eps)
        dx = ops.pool_bwd(dpooled, cfg.B, cfg.L, cfg.mode, idx)
        return (dx, None, None, None) + _finish_grads((d_ln_w, d_ln_b, d_proj), ctx.params)


@dataclasses.dataclass(frozen=True)
class MapHeadCfg:
    """MapHeadFn: B samples of L tokens, H heads, the MLP's activation (ops.ACT_*), the LayerNorm's eps."""
    B: int
    L: int
    H: int
    act: int
    eps: float


def _map_fold(cache, probe, w_in, b_in, H):
    """The folded query of the MAP head, rebuilt when probe / in_proj_weight / in_proj_bias change: q = probe Wq^T + bq (one
    query for every sample), Qs[h, j] = dh^-0.5 q[j] for the channels j of head h (zero elsewhere, bf16) and
    U = Qs Wk ([H, D] bf16): s[b,l,h] = x[b,l,:] . U[h,:].  The bk_h . q_h term of the scores is constant over l and cancels in
    the softmax: it is never computed.  -> (U, Qs, head mask [H, D] f32)."""
    def make(pr, w, b):
        D = w.shape[1]
        dh = D // H
        wq, bq = cache.w(w_in)[:D], cache.f32(b_in)[:D]
        q = ops.gemm_nt(ops.to_bf16(pr.reshape(1, D)), wq, bq, out_f32=True)                     # [1, D] f32
        mask = (torch.arange(D, device=w.device) // dh == torch.arange(H, device=w.device)[:, None]).to(f32)
        qs = ops.to_bf16((q * float(dh) ** -0.5).expand(H, D) * mask)
        u = ops.gemm_nt(qs, cache.wt(w_in)[:, D:2 * D])                                           # [H, D(j)] x [D(d), D(j)]^T
        return u, qs, mask
    return cache.multi((probe, w_in, b_in), "map_fold%d" % H, make)


class MapHeadFn(torch.autograd.Function):
    """Multihead attention pooling + projection (clipa_jax/models/vit.py:187-207,282-284; no encoder_norm in front, no ln_post):
        a = MHA_H(probe Wq^T + bq, x Wk^T + bk, x Wv^T + bv) Wo^T + bo;  out = a + c_proj(act(c_fc(LayerNorm(a))));  feat = out @ proj
    on the [B*L, D] bf16 output of the tower -> f32 [B, E] like HeadFn.  LayerNorm eps is the engine's 1e-5 (flax's default is
    1e-6).  The one query is the same for every sample, so the K and V projections fold out of the token-level work (_map_fold;
    csrc/mappool.hip): z[b,h,:] = sum_l softmax_l(x U_h^T) x[b,l,:] in one read of x, then head_h = Wv_h z[b,h,:] + bv_h (sum_l p
    = 1) and everything after it on B rows with the engine's GEMM / LayerNorm launches.  Saved for backward: z, the softmax
    statistics and B-row tensors; the only [B*L]-row tensor the head allocates is dx.  Rounding points beside the kernel's own
    (P, dS, dz as bf16 MFMA operands): q, U, z and dU are rounded to bf16 where a bf16 GEMM takes them.  d bk = 0 exactly."""

    @staticmethod
    def forward(ctx, x, cfg, cache, probe, w_in, b_in, w_out, b_out, ln_w, ln_b, w_fc, b_fc, w_proj, b_proj, proj):
        B, L, H = cfg.B, cfg.L, cfg.H
        D = x.shape[1]
        dh = D // H
        u, _, _ = _map_fold(cache, probe, w_in, b_in, H)
        z, stats = ops.mappool_fwd(x, u, B, L, H)
        zb = ops.to_bf16(z)                                                  # [B, H, D]
        wv, bv = cache.w(w_in)[2 * D:], cache.f32(b_in)[2 * D:]
        heads = torch.empty((B, D), device=x.device, dtype=bf16)
        for h in range(H):
            hs = slice(h * dh, (h + 1) * dh)
            ops.gemm_nt(zb[:, h], wv[hs], bv[hs], out=heads[:, hs])
        ctx.params = (probe, w_in, b_in, w_out, b_out, ln_w, ln_b, w_fc, b_fc, w_proj, b_proj, proj)
        P = MapHeadFn._operands(cache, ctx.params, backward=False)      # (a frozen head never builds the transposed copies)
        mlp = Inter(x1=ops.gemm_nt(heads, P["w_out"], P["b_out"]))            # the out-projection, without a residual
        mlp.h2, mlp.g, mlp.hpre = _fc(mlp.x1, P, cfg.act, cfg.eps, True)
        out = _proj(mlp.g, mlp.x1, P)
        feat = ops.gemm_nt(out, cache.wt(proj), out_f32=True)
        ctx.cfg, ctx.cache = cfg, cache
        ctx.save_for_backward(x, z, stats)
        ctx.rows = (zb, heads, mlp, out)      # the B-row tensors: released in backward before dx is allocated
        return feat

    @staticmethod
    def _operands(cache, params, backward=True):
        """The operands of the head's B-row layers under the names the block's stages read (_mlp_operands)."""
        _, _, _, w_out, b_out, ln_w, ln_b, w_fc, b_fc, w_proj, b_proj, _ = params
        return _mlp_operands(cache, ln_w, ln_b, (("out", w_out, b_out), ("fc", w_fc, b_fc), ("proj", w_proj, b_proj)), backward)

    @staticmethod
    def backward(ctx, dfeat):
        x, z, stats = ctx.saved_tensors
        (zb, heads, mlp, out), ctx.rows = ctx.rows, None
        cfg, cache = ctx.cfg, ctx.cache
        probe, w_in, b_in, *_, proj = ctx.params
        P = MapHeadFn._operands(cache, ctx.params)
        B, L, H = cfg.B, cfg.L, cfg.H
        D = x.shape[1]
        dh = D // H
        u, qs, mask = _map_fold(cache, probe, w_in, b_in, H)
        # the input-gradient chain on B rows down to dz, with the weight gradients of the MLP and the out-projection on its way
        dfb = ops.to_bf16(dfeat.contiguous())
        dout = ops.gemm_nt(dfb, cache.w(proj))                               # [B,E] @ proj[D,E]^T -> [B,D]
        da, d_mlp = _mlp_backward(dout, mlp, P, cfg.act, cfg.eps)
        dheads, d_w_out, d_b_out = _out_proj_backward(da, heads, P)          # [B, D]
        wt_in = cache.wt(w_in)                                               # [D, 3D]
        dz = torch.empty((B, H, D), device=x.device, dtype=f32)
        for h in range(H):                                                   # head_h = Wv_h z[b,h,:] + bv_h
            ops.gemm_nt(dheads[:, h * dh:(h + 1) * dh], wt_in[:, 2 * D + h * dh:2 * D + (h + 1) * dh], out_f32=True, out=dz[:, h])
        # every weight gradient that does not wait for dU - BEFORE the token-level launch: their split-M workspaces and the B-row
        # tensors are gone by the time dx, the head's one [B*L]-row tensor, is allocated
        d_proj = ops.gemm_tn(out, dfb, f32)
        # dWv_h = dheads[:, head h]^T z[:, h, :] per head, on DENSE copies of the two B-row operands: ops.gemm_tn reads whole
        # 256-column images of its operands, so it is not handed column windows of a wider matrix
        wv_parts = [ops.gemm_tn(dheads[:, h * dh:(h + 1) * dh].contiguous(), zb[:, h].contiguous(), f32, want_colsum=True)
                    for h in range(H)]
        d_wv, d_bv = torch.cat([w for w, _ in wv_parts]), torch.cat([b for _, b in wv_parts])
        del wv_parts
        del zb, heads, out, dfb, dout, da, dheads
        dx, du = ops.mappool_bwd(x, u, z, stats, dz, B, L, H)
        del dz
        # U = Qs Wk, Qs[h, j] = dh^-0.5 q[j] on head h's channels, q = probe Wq^T + bq
        dub = ops.to_bf16(du)
        d_wk = ops.gemm_tn(qs, dub, f32)                                     # dWk[j, d] = Qs[h(j), j] dU[h(j), d]
        dqs = ops.gemm_nt(dub, cache.w(w_in)[D:2 * D], out_f32=True)         # [H, D(j)] = sum_d dU[h, d] Wk[j, d]
        dq = (dqs * mask).sum(0, keepdim=True) * float(dh) ** -0.5           # [1, D]: the head's own row of each channel
        dqb = ops.to_bf16(dq)
        d_wq = ops.gemm_tn(dqb, ops.to_bf16(probe.detach().reshape(1, D)), f32)
        d_probe = ops.gemm_nt(dqb, wt_in[:, :D], out_f32=True).reshape(probe.shape)
        d_w_in = torch.cat([d_wq, d_wk, d_wv])
        d_b_in = torch.cat([dq[0], torch.zeros_like(dq[0]), d_bv])           # d bk = 0: bk cancels in the softmax
        grads = (d_probe, d_w_in, d_b_in, d_w_out, d_b_out) + d_mlp + (d_proj,)
        return (dx, None, None) + _finish_grads(grads, ctx.params)


class L2NormFn(torch.autograd.Function):
    """F.normalize(x, dim=-1), eps 1e-12 (model.py:240,263)."""

    @staticmethod
    def forward(ctx, x):
        y, _, inv = ops.l2norm_fwd(x.contiguous())
        ctx.save_for_backward(y, inv)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, inv = ctx.saved_tensors
        return ops.l2norm_bwd(y, inv, dy.contiguous())
