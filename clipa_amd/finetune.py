"""Supervised fine-tuning of the image tower on a labelled set (e.g. ImageNet fine-tuning after CLIPA pre-training) through the
MI355X engine.  Mirrors, from the reference's JAX tree (paths relative to clipa_jax):

  ImageClassifier            the bias-free `num_classes` head of the ViT            models/vit.py:298-306 (head_zeroinit)
  SoftTargetCrossEntropy     softmax_xent on mixed, smoothed labels                 losses/common.py:104-109, transforms/mixup.py:203-211
  sample_mixcut              the random draws of MixupAndCutmix                     transforms/mixup.py:110-115,136-173
  DeviceMixCut               its image half, on the uint8 device batch              transforms/mixup.py:141-201 (csrc/mixcut.hip)
  evaluate_classification    the classification evaluator (prec@1, loss)            evaluators/classification.py:88-89

The tower is the engine's VisionTransformer as it stands (`clip.visual`); the head is one autograd Function on the existing GEMM
wrappers, the loss one fused kernel (csrc/softce.hip) whose single pass gives loss and logit gradient, the image mixing one
in-place kernel after DeviceAugment.  Targets stay compact - (ya, yb, lam) and a scalar smoothing: no [B, C] matrix exists.
Not covered: stochastic depth, layer-wise lr decay, random erasing, sigmoid_xent.
"""
import torch
from torch import nn

from . import engine, ops
from ._eval_common import _inference
from .engine import _like_param

bf16, f32 = torch.bfloat16, torch.float32


# ---- the classifier head ---------------------------------------------------------------------------------------------------
def _pad8(n):
    return (n + 7) // 8 * 8


def _head_operand(w):
    """head.weight [C, E] -> bf16 [C rounded up to 8, E], the extra class rows zero (the GEMMs take multiples of 8)."""
    wb = w if w.dtype == bf16 else ops.to_bf16(w)
    C, E = w.shape
    if C % 8 == 0:
        return wb
    out = torch.zeros((_pad8(C), E), device=w.device, dtype=bf16)
    out[:C] = wb
    return out


def _head_operand_t(w):
    """head.weight [C, E] -> bf16 [E, C rounded up to 8], the extra class columns zero."""
    wt = ops.transpose_bf16(w)
    C, E = w.shape
    if C % 8 == 0:
        return wt
    out = torch.zeros((E, _pad8(C)), device=w.device, dtype=bf16)
    out[:, :C] = wt
    return out


class HeadLinearFn(torch.autograd.Function):
    """logits = feat @ weight^T (vit.py:304-306: a Dense without bias), fp32 [B, C] from bf16 operands - the way engine.HeadFn
    applies `proj`.  The class dimension is padded to a multiple of 8 with zero rows in the cached operand only: the returned
    logits are the [B, C] view of the [B, C8] product, whose other columns a loss must not read (ops.soft_target_ce does not)."""

    @staticmethod
    def forward(ctx, feat, weight, cache):
        C, E = weight.shape
        fb = ops.to_bf16(feat)
        logits = ops.gemm_nt(fb, cache.custom(weight, "head_w8", _head_operand), out_f32=True)        # [B, C8]
        ctx.cache, ctx.weight, ctx.feat_dtype = cache, weight, feat.dtype
        ctx.save_for_backward(fb)
        return logits[:, :C]

    @staticmethod
    def backward(ctx, dlogits):
        fb, = ctx.saved_tensors
        weight, cache = ctx.weight, ctx.cache
        C, C8 = weight.shape[0], _pad8(weight.shape[0])
        if C8 == C:
            dp = ops.to_bf16(dlogits.contiguous())
        else:                                           # the pad columns of the operand are zero
            dp = torch.zeros((dlogits.shape[0], C8), device=dlogits.device, dtype=bf16)
            dp[:, :C].copy_(dlogits)
        dfeat = dw = None
        if ctx.needs_input_grad[0]:
            dfeat = ops.gemm_nt(dp, cache.custom(weight, "head_wt8", _head_operand_t), out_f32=True)  # [B, C8] @ [E, C8]^T
            dfeat = dfeat if dfeat.dtype == ctx.feat_dtype else dfeat.to(ctx.feat_dtype)
        if weight.requires_grad:
            dw = _like_param(ops.gemm_tn(dp, fb, f32)[:C], weight)                                    # [C8, E] -> [C, E]
        return dfeat, dw, None


class _Head(nn.Module):
    """Parameter container: `head.weight` [C, E]; the arithmetic is HeadLinearFn."""

    def __init__(self, num_classes, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(num_classes, dim))

    def forward(self, *a, **k):
        raise RuntimeError("clipa_amd: the classifier head is applied by ImageClassifier.forward")


class ImageClassifier(nn.Module):
    """A VisionTransformer (typically `clip.visual`, whose parameters and WeightCache are shared, not copied) with a bias-free
    `num_classes` head on its output features (vit.py:298-306).  init: "normal" - std E^-0.5 (vit.py:302-303), "zeros" -
    head_zeroinit, or a [C, E] tensor - the WiSE-FT start, e.g. zero_shot.build_classifier(...) times the logit scale together
    with normalize=True, which puts the L2 normalisation of encode_image in front of the head.  forward(images) -> fp32 logits
    [B, C].  state_dict: the tower's keys under `visual.` plus `head.weight`."""

    def __init__(self, visual, num_classes, normalize=False, init="normal"):
        super().__init__()
        C, E = int(num_classes), int(visual.output_dim)
        if not 2 <= C <= ops.SOFTCE_MAX_CLASSES:
            raise ValueError(f"ImageClassifier: num_classes = {num_classes}; the loss kernel takes 2 to {ops.SOFTCE_MAX_CLASSES}")
        if E % 8:
            raise ValueError(f"ImageClassifier: the tower's output_dim = {E} must be a multiple of 8 (the head runs on the GEMM kernels)")
        self.visual = visual
        self.num_classes, self.normalize = C, bool(normalize)
        self.head = _Head(C, E)
        if torch.is_tensor(init):
            if tuple(init.shape) != (C, E):
                raise ValueError(f"ImageClassifier: init tensor must be [{C}, {E}], got {tuple(init.shape)}")
            with torch.no_grad():
                self.head.weight.copy_(init.detach().to(f32))
        elif init == "normal":
            nn.init.normal_(self.head.weight, std=E ** -0.5)
        elif init != "zeros":
            raise ValueError(f"ImageClassifier: init must be 'normal', 'zeros' or a [C, E] tensor, got {init!r}")
        self.head.to(next(visual.parameters()).device)
        self._cache = visual._cache
        self.register_load_state_dict_post_hook(lambda module, incompatible_keys: module._cache.clear())

    def invalidate_weight_cache(self):
        """Call after writing weights through `p.data`: such writes bump no version counter."""
        self._cache.clear()

    def lock(self, unlocked_groups=0, freeze_bn_stats=False):
        """Freeze the tower as VisionTransformer.lock does (LiT-style groups); the head stays trainable."""
        self.visual.lock(unlocked_groups=unlocked_groups, freeze_bn_stats=freeze_bn_stats)

    @torch.jit.ignore
    def set_grad_checkpointing(self, enable=True):
        self.visual.set_grad_checkpointing(enable)

    def features(self, images):
        """The head's input: the tower's fp32 features [B, E], L2-normalised with normalize=True."""
        f = self.visual(images)
        return engine.L2NormFn.apply(f) if self.normalize else f

    def head_logits(self, features):
        return HeadLinearFn.apply(features, self.head.weight, self._cache)

    def forward(self, images):
        return self.head_logits(self.features(images))


# ---- the loss --------------------------------------------------------------------------------------------------------------
def _labels32(t, name):
    if not torch.is_tensor(t) or t.dtype.is_floating_point or t.dtype == torch.bool or t.dim() != 1:
        raise RuntimeError(f"clipa_amd.soft_target_cross_entropy: {name} must be a 1-D integer tensor of class indices")
    return t if t.dtype == torch.int32 else t.to(torch.int32)


class SoftTargetCEFn(torch.autograd.Function):
    """mean_i (lse_i - sum_c t_ic z_ic): loss and dlogits from the one pass of ops.soft_target_ce, as ClipLossFn does it."""

    @staticmethod
    def forward(ctx, logits, ya, yb, lam, smoothing):
        B, C = logits.shape
        need = ctx.needs_input_grad[0]
        rows, _, dl = ops.soft_target_ce(logits, ya, yb, lam, smoothing, gscale=1.0 / B if need else None)
        loss = ops.sum_scale(rows, 1.0 / B)             # one block, fixed order
        if need:
            ctx.save_for_backward(dl)
            ctx.meta = (C, logits.dtype)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        dl, = ctx.saved_tensors
        C, dt = ctx.meta
        full = dl.as_strided((dl.shape[0], dl.stride(0)), (dl.stride(0), 1))      # the whole [B, C8] buffer: one flat cast
        d = ops.to_f32(full)[:, :C] * dloss.to(f32)
        return d if d.dtype == dt else d.to(dt), None, None, None, None


def soft_target_cross_entropy(logits, ya, yb=None, lam=None, smoothing=0.0):
    """The scalar mean of the soft-target cross-entropy rows (losses/common.py:104-109 with reduction) for the targets
    t_c = (1 - smoothing) (lam [c = ya] + (1 - lam) [c = yb]) + smoothing / C (mixup.py:203-211; no yb: hard labels).
    logits fp32 [B, C] on the GPU; ya, yb integer [B]; lam f32 [B]."""
    if (yb is None) != (lam is None):
        raise RuntimeError("clipa_amd.soft_target_cross_entropy: yb and lam come together")
    if logits.dim() != 2 or logits.shape[0] < 1:
        raise RuntimeError(f"clipa_amd.soft_target_cross_entropy: logits must be [B >= 1, C], got {tuple(logits.shape)}")
    ya = _labels32(ya, "ya")
    if yb is not None:
        yb, lam = _labels32(yb, "yb"), lam.to(f32)
    return SoftTargetCEFn.apply(logits.float(), ya, yb, lam, float(smoothing))


class SoftTargetCrossEntropy(nn.Module):
    """loss(logits, target): target a label vector [B] or the triple (ya, yb, lam) that DeviceMixCut returns."""

    def __init__(self, smoothing=0.0):
        super().__init__()
        if not 0.0 <= float(smoothing) <= 1.0:
            raise ValueError(f"SoftTargetCrossEntropy: smoothing = {smoothing} outside [0, 1]")
        self.smoothing = float(smoothing)

    def forward(self, logits, target):
        ya, yb, lam = target if isinstance(target, (tuple, list)) else (target, None, None)
        return soft_target_cross_entropy(logits, ya, yb, lam, self.smoothing)


# ---- Mixup / CutMix --------------------------------------------------------------------------------------------------------
def sample_mixcut(batch, image_size, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, correct_lam=True,
                  generator=None):
    """One batch's random draws of MixupAndCutmix on the host -> (mode, lam f32 [B], box int32 [B,4] = (y0, y1, x0, x1)).
    mode "mixup" | "cutmix" | "none", chosen once per batch (mixup.py:110-115; an alpha of 0 disables that arm, :70-73; with
    probability 1 - prob the batch is left alone: lam = 1, empty boxes).  lam ~ Beta(alpha, alpha) per image as a ratio of two
    gammas (:136-139).  mixup: lam is the pixel and the label weight.  cutmix (:147-173, random_erasing.py:35-38): cut =
    int(sqrt(1 - lam) S), an integer centre uniform in [0, S), half size cut // 2, rows [max(0, cy - h), min(S, cy + h)) and
    columns likewise; the returned lam is the label weight: 1 - pasted pixels / S^2 of the clipped box (correct_lam=True, so the
    label matches the pixels) or the reference's 1 - cut^2 / S^2 of the unclipped size (correct_lam=False, :172-173)."""
    B, S = int(batch), int(image_size)
    lam = torch.ones(B, dtype=f32)
    box = torch.zeros((B, 4), dtype=torch.int32)
    u = torch.rand(2, generator=generator)
    if not (mixup_alpha or cutmix_alpha) or not float(u[0]) < prob:
        return "none", lam, box
    cut = bool(cutmix_alpha) and (not mixup_alpha or float(u[1]) < switch_prob)
    alpha = torch.full((B,), float(cutmix_alpha if cut else mixup_alpha), dtype=f32)
    ga, gb = torch._standard_gamma(alpha, generator=generator), torch._standard_gamma(alpha, generator=generator)
    lam = (ga / (ga + gb)).to(f32)
    lam = torch.where(torch.isfinite(lam), lam, torch.ones_like(lam))        # both gammas underflowed (tiny alpha)
    if not cut:
        return "mixup", lam.contiguous(), box
    size = (torch.sqrt(1 - lam) * float(S)).to(torch.int32)
    cy = torch.randint(0, S, (B,), generator=generator, dtype=torch.int32)
    cx = torch.randint(0, S, (B,), generator=generator, dtype=torch.int32)
    h = size // 2
    box = torch.stack([(cy - h).clamp(min=0), (cy + h).clamp(max=S), (cx - h).clamp(min=0), (cx + h).clamp(max=S)], 1)
    if correct_lam:
        area = (box[:, 1] - box[:, 0]).double() * (box[:, 3] - box[:, 2]).double()
    else:
        area = size.double() * size.double()
    lam = (1.0 - area / float(S * S)).to(f32)
    return "cutmix", lam.contiguous(), box.to(torch.int32).contiguous()


class DeviceMixCut:
    """MixupAndCutmix (transforms/mixup.py:30-211) on a uint8 [B,3,S,S] device batch, in place - a DeviceAugment output as it
    stands - on the current stream.  __call__(images_u8, labels) -> (images_u8, (ya, yb, lam)): ya = labels, yb = labels.flip(0),
    lam f32 [B] on the device - the triple SoftTargetCrossEntropy takes (the smoothing is the loss's)."""

    def __init__(self, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, correct_lam=True, seed=0):
        self.cfg = dict(mixup_alpha=float(mixup_alpha), cutmix_alpha=float(cutmix_alpha), prob=float(prob),
                        switch_prob=float(switch_prob), correct_lam=bool(correct_lam))
        self.gen = torch.Generator(device="cpu").manual_seed(int(seed))

    def __call__(self, images_u8, labels):
        B, S = images_u8.shape[0], images_u8.shape[-1]
        mode, lam, box = sample_mixcut(B, S, generator=self.gen, **self.cfg)
        put = lambda t: t.pin_memory().to(images_u8.device, non_blocking=True)
        lam = put(lam)
        if mode == "mixup":
            ops.mixcut_u8(images_u8, lam=lam)
        elif mode == "cutmix":
            ops.mixcut_u8(images_u8, box=put(box))
        ya = _labels32(labels.to(images_u8.device), "labels")
        return images_u8, (ya, ya.flip(0), lam)


# ---- evaluation ------------------------------------------------------------------------------------------------------------
def evaluate_classification(classifier, batches, topk=(1, 5)):
    """The classification evaluator (evaluators/classification.py): batches yields (images, labels [b]) on the device.  Per
    batch: the tower's features, the fp32 rank kernel on features and head.weight (zero_shot._ranks_and_stats: a hit at k means
    fewer than k classes beat the label), the loss kernel with hard labels on the head's logits; counts and the loss sum are
    added on the device, one host sync per dataset.  no_grad and eval mode, the model's previous mode put back.
    -> {"prec@1", f"top{k}" for the other k, "loss", "count"} (:88-89)."""
    from . import zero_shot
    ks = zero_shot._topk(topk, "evaluate_classification")
    with _inference(classifier) as m:
        w = m.head.weight.detach().float()
        total = loss_sum = None
        for images, labels in batches:
            f = m.features(images)
            lab = zero_shot._labels2d(labels, f.shape[0], f.device, "evaluate_classification")
            if lab.shape[1] != 1:
                raise RuntimeError("clipa_amd.evaluate_classification: one label per image")
            stats = zero_shot._ranks_and_stats(f, w, lab, ks)[3]
            # every image has a label here: -1 ("no label" to the rank kernel) is as wrong as any other value outside [0, C).
            # Such a batch raises below; the loss kernel sees the labels clamped, so that the one error is reported once.
            stats = torch.cat([stats, ((lab < 0) | (lab >= m.num_classes)).sum().reshape(1)])
            rows, _, _ = ops.soft_target_ce(m.head_logits(f), lab[:, 0].to(torch.int32).clamp(0, m.num_classes - 1))
            total = stats if total is None else total + stats
            loss_sum = ops.sum_scale(rows, 1.0, out=loss_sum, accumulate=loss_sum is not None)
        if total is None:
            raise RuntimeError("clipa_amd.evaluate_classification: no batches")
        total = torch.cat([total.double(), loss_sum.double().reshape(1)]).tolist()          # the one host sync
    stats, loss = [int(v) for v in total[:-1]], total[-1]
    if stats[-1]:
        raise RuntimeError(f"clipa_amd.evaluate_classification: {stats[-1]} labels outside [0, C)")
    if stats[-2]:
        raise RuntimeError(f"clipa_amd.evaluate_classification: non-finite values in {stats[-2]} image feature rows")
    n = stats[len(ks) + 1]
    out = {("prec@1" if k == 1 else f"top{k}"): stats[i] / n for i, k in enumerate(ks)}
    out.update(loss=loss / n, count=n)
    return out
