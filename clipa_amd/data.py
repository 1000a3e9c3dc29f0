"""Synthetic LAION-shaped batches for benchmarks and smoke runs (the reference's own SyntheticDataset,
clipa_torch/training/data.py:469-486, yields an all-black image - useless for numerics and power).

images: uint8 [B, 3, S, S] uniform 0..255 - the `--to-float-on-device` wire format (open_clip/transform.py:171-174,
training/train.py:191-197) - returned in channels_last memory (physical NHWC: what a decoder produces and what the
patch gather reads in contiguous 3*P-byte runs).  texts: int64 [B, ctx] rows [SOT, k random ids, EOT, 0 ...] with
caption length k+2 ~ clip(N(20, 8), 3, ctx); EOT is the row maximum because pooling is text.argmax(-1) (model.py:254)."""
import torch


def synthetic_batch(batch, image_size, ctx, vocab, seed, device="cpu", channels_last=True):
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    base = min(batch, 256)                                     # host-side generation stays small; tiled on the device
    img = torch.randint(0, 256, (base, 3, image_size, image_size), generator=g, dtype=torch.uint8)
    sot, eot = vocab - 2, vocab - 1
    n = torch.clamp(torch.round(torch.randn(base, generator=g) * 8 + min(20.0, ctx * 0.6)), 3, ctx).long()
    txt = torch.randint(1, vocab - 2, (base, ctx), generator=g, dtype=torch.int64)
    pos = torch.arange(ctx).unsqueeze(0)
    txt = torch.where(pos < (n - 1).unsqueeze(1), txt, torch.zeros_like(txt))
    txt[:, 0] = sot
    txt[torch.arange(base), n - 1] = eot
    img, txt = img.to(device), txt.to(device)
    reps = (batch + base - 1) // base
    img = img.repeat(reps, 1, 1, 1)[:batch]
    txt = txt.repeat(reps, 1)[:batch].contiguous()
    # de-duplicate the tiled rows so no two pairs of the batch are identical
    img = img + (torch.arange(batch, device=img.device) % 251).to(torch.uint8).view(batch, 1, 1, 1)
    txt[:, 1] = 1 + (torch.arange(batch, device=txt.device) % (vocab - 3))
    img = img.contiguous(memory_format=torch.channels_last) if channels_last else img.contiguous()
    return img, txt


# ---------------------------------------------------------------------------------------------------------------------
# Device-side input pipeline.  The reference decodes, crops, resizes and colour-converts every image
# on host CPU workers (open_clip/transform.py:152-168 inside the loaders of training/data.py:332-436 /
# reader_tfds.py:322-350) and ships the finished uint8 tensor (`images.to(device, non_blocking=True)`,
# training/train.py:187-189); it already moved the float conversion to the device because the hosts could not keep up at
# ~9 k pairs/s.  Here the loader only has to deliver decoded uint8 NHWC images at a fixed staging resolution; the copy is
# double-buffered through pinned memory on its own HIP stream and RandomResizedCrop / Grayscale run as HIP kernels
# (clipa_amd/csrc/augment.hip, bit-exact with the Pillow code torchvision calls) while the previous step computes.
import collections
import math


def random_resized_crop_params(height, width, scale=(0.9, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), generator=None):
    """torchvision.transforms.RandomResizedCrop.get_params (the box sampler behind open_clip/transform.py:153-157),
    restated with an explicit torch.Generator: up to 10 attempts at (area fraction ~ U(scale), aspect ~ log-U(ratio)) that
    fit the image, else the largest central crop inside the ratio bounds.  -> (top, left, h, w)."""
    area = height * width
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=generator).item()
        aspect = math.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=generator).item())
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if 0 < w <= width and 0 < h <= height:
            i = int(torch.randint(0, height - h + 1, (1,), generator=generator).item())
            j = int(torch.randint(0, width - w + 1, (1,), generator=generator).item())
            return i, j, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def sample_crop_boxes(batch, height, width, scale=(0.9, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), generator=None):
    """The same distribution for a whole batch in a handful of tensor ops (a Python loop over 4096 samples would cost more
    host time than the step it feeds): int32 [batch, 4] = (top, left, h, w) on the CPU."""
    area = float(height * width)
    u = torch.rand(batch, 10, generator=generator, dtype=torch.float64)
    v = torch.rand(batch, 10, generator=generator, dtype=torch.float64)
    target = area * (scale[0] + (scale[1] - scale[0]) * u)
    aspect = torch.exp(math.log(ratio[0]) + (math.log(ratio[1]) - math.log(ratio[0])) * v)
    w = torch.round(torch.sqrt(target * aspect)).long()
    h = torch.round(torch.sqrt(target / aspect)).long()
    ok = (w > 0) & (w <= width) & (h > 0) & (h <= height)
    first = torch.where(ok.any(1), ok.float().argmax(1), torch.zeros(batch, dtype=torch.long))
    idx = torch.arange(batch)
    w, h = w[idx, first], h[idx, first]
    fi, fj, fh, fw = random_resized_crop_params(height, width, (2.0, 2.0), ratio)     # scale 2 never fits: the fallback box
    none = ~ok.any(1)
    w = torch.where(none, torch.full_like(w, fw), w)
    h = torch.where(none, torch.full_like(h, fh), h)
    ri = torch.rand(batch, generator=generator, dtype=torch.float64)
    rj = torch.rand(batch, generator=generator, dtype=torch.float64)
    top = torch.minimum((ri * (height - h + 1).double()).long(), height - h)
    left = torch.minimum((rj * (width - w + 1).double()).long(), width - w)
    top = torch.where(none, torch.full_like(top, fi), top)
    left = torch.where(none, torch.full_like(left, fj), left)
    return torch.stack([top, left, h, w], 1).to(torch.int32).contiguous()


def sample_crop_boxes_ragged(heights, widths, scale=(0.9, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), generator=None):
    """sample_crop_boxes for images of different sizes: heights, widths [B] -> int32 [B, 4] = (top, left, h, w), each box inside
    its own image.  The generator is consumed in the same order, so for equal sizes the boxes are those of sample_crop_boxes
    from the same generator state; the fallback of a sample none of whose ten attempts fits is its own largest central crop
    inside the ratio bounds (random_resized_crop_params past its loop, computed here without drawing anything)."""
    height = torch.as_tensor(heights).cpu().long().reshape(-1)
    width = torch.as_tensor(widths).cpu().long().reshape(-1)
    batch = height.numel()
    area = (height * width).double().unsqueeze(1)
    u = torch.rand(batch, 10, generator=generator, dtype=torch.float64)
    v = torch.rand(batch, 10, generator=generator, dtype=torch.float64)
    target = area * (scale[0] + (scale[1] - scale[0]) * u)
    aspect = torch.exp(math.log(ratio[0]) + (math.log(ratio[1]) - math.log(ratio[0])) * v)
    w = torch.round(torch.sqrt(target * aspect)).long()
    h = torch.round(torch.sqrt(target / aspect)).long()
    ok = (w > 0) & (w <= width.unsqueeze(1)) & (h > 0) & (h <= height.unsqueeze(1))
    first = torch.where(ok.any(1), ok.float().argmax(1), torch.zeros(batch, dtype=torch.long))
    idx = torch.arange(batch)
    w, h = w[idx, first], h[idx, first]
    in_ratio = width.double() / height.double()
    narrow, wide = in_ratio < min(ratio), in_ratio > max(ratio)
    fh = torch.where(narrow, torch.round(width.double() / min(ratio)).long(), height)
    fw = torch.where(wide & ~narrow, torch.round(height.double() * max(ratio)).long(), width)
    fi = torch.div(height - fh, 2, rounding_mode="floor")
    fj = torch.div(width - fw, 2, rounding_mode="floor")
    none = ~ok.any(1)
    w, h = torch.where(none, fw, w), torch.where(none, fh, h)
    ri = torch.rand(batch, generator=generator, dtype=torch.float64)
    rj = torch.rand(batch, generator=generator, dtype=torch.float64)
    top = torch.minimum((ri * (height - h + 1).double()).long(), height - h)
    left = torch.minimum((rj * (width - w + 1).double()).long(), width - w)
    top, left = torch.where(none, fi, top), torch.where(none, fj, left)
    return torch.stack([top, left, h, w], 1).to(torch.int32).contiguous()


# ---- batches of images of different sizes ---------------------------------------------------------------------------------
# Decoded dataset images differ in size from sample to sample; resizing them to a common staging size on the host would be the
# per-sample CPU work this pipeline removes (and a second resample of the pixels).  A batch travels as ONE packed byte buffer
# plus a size table, and clipa_amd/csrc/resample_ragged.hip resamples every image from its own geometry.
class RaggedImages:
    """A batch of H_b x W_b x 3 uint8 images in one buffer: data uint8 [bytes], offsets int64 [B] (byte offset of image b),
    sizes int32 [B, 2] = (H_b, W_b).  The two tables also stay on the host (host_tables), where the launch geometry is derived."""

    def __init__(self, data, offsets, sizes, host=None):
        self.data, self.offsets, self.sizes = data, offsets, sizes
        if data.dim() != 1 or data.dtype != torch.uint8 or offsets.dtype != torch.int64 or sizes.dtype != torch.int32:
            raise ValueError("RaggedImages: data uint8 [bytes], offsets int64 [B], sizes int32 [B,2]")
        if sizes.dim() != 2 or sizes.shape[1] != 2 or offsets.shape != sizes.shape[:1]:
            raise ValueError(f"RaggedImages: offsets [B] and sizes [B,2], got {tuple(offsets.shape)} and {tuple(sizes.shape)}")
        self._host = host

    def __len__(self):
        return self.offsets.numel()

    @property
    def device(self):
        return self.data.device

    def host_tables(self):
        """-> (offsets, sizes) on the CPU (copied back once if this batch was built from device tensors)."""
        if self._host is None:
            self._host = (self.offsets.cpu(), self.sizes.cpu())
        return self._host

    def to(self, device, non_blocking=False):
        host = self.host_tables()
        put = lambda t: t.to(device, non_blocking=non_blocking)
        return RaggedImages(put(self.data), put(self.offsets), put(self.sizes), host)

    def pin_memory(self):
        return RaggedImages(self.data.pin_memory(), self.offsets.pin_memory(), self.sizes.pin_memory(), self._host)

    def is_pinned(self):
        return self.data.is_pinned() and self.offsets.is_pinned() and self.sizes.is_pinned()

    def record_stream(self, stream):
        for t in (self.data, self.offsets, self.sizes):
            t.record_stream(stream)

    def image(self, i):
        """Image i as an [H, W, 3] view of the buffer."""
        offsets, sizes = self.host_tables()
        o, h, w = int(offsets[i]), int(sizes[i, 0]), int(sizes[i, 1])
        return self.data[o:o + h * w * 3].view(h, w, 3)

    @staticmethod
    def from_uniform(batch):
        """A contiguous uint8 [B, H, W, 3] tensor as a ragged batch of equal sizes (a view: no pixel is copied)."""
        if batch.dim() != 4 or batch.shape[3] != 3 or batch.dtype != torch.uint8:
            raise ValueError(f"RaggedImages.from_uniform: uint8 [B,H,W,3], got {batch.dtype} {tuple(batch.shape)}")
        B, H, W, _ = batch.shape
        offsets = torch.arange(B, dtype=torch.int64) * (H * W * 3)
        sizes = torch.tensor([[H, W]], dtype=torch.int32).repeat(B, 1)
        put = (lambda t: t.pin_memory().to(batch.device, non_blocking=True)) if batch.is_cuda else (lambda t: t)
        return RaggedImages(batch.contiguous().view(-1), put(offsets), put(sizes), (offsets, sizes))


RAGGED_ALIGN = 16      # every image of a packed batch starts at a multiple of this many bytes


def _image_tables(images):
    """Sizes and aligned offsets of a list of uint8 [H, W, 3] arrays / tensors -> (tensors, offsets, sizes, total bytes)."""
    tensors = []
    for i, im in enumerate(images):
        t = torch.as_tensor(im)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"pack_images: image {i} must be a uint8 [H, W, 3] array, got {t.dtype} {tuple(t.shape)}")
        tensors.append(t)
    sizes = torch.tensor([[t.shape[0], t.shape[1]] for t in tensors], dtype=torch.int32).reshape(-1, 2)
    nbytes = (sizes[:, 0].long() * sizes[:, 1].long() * 3 + RAGGED_ALIGN - 1) // RAGGED_ALIGN * RAGGED_ALIGN
    offsets = torch.cumsum(nbytes, 0) - nbytes
    return tensors, offsets, sizes, int(nbytes.sum())


def _fill_packed(data, tensors, offsets):
    for t, o in zip(tensors, offsets.tolist()):
        data[o:o + t.numel()].view(t.shape).copy_(t)
    return data


def pack_images(images, pinned=False):
    """A list of uint8 [H, W, 3] arrays or tensors (decoded images, any sizes) -> RaggedImages on the CPU (in pinned memory if
    asked); each image starts at a 16-byte aligned offset."""
    tensors, offsets, sizes, total = _image_tables(images)
    data = _fill_packed(torch.zeros(total, dtype=torch.uint8, pin_memory=bool(pinned)), tensors, offsets)
    return RaggedImages(data, offsets, sizes, (offsets, sizes))


def ragged_collate(samples):
    """collate_fn for datasets whose samples are (uint8 [H, W, 3] image, rest...): -> (RaggedImages, default_collate(rest))."""
    from torch.utils.data import default_collate
    rest = [s[1] if len(s) == 2 else tuple(s[1:]) for s in samples]
    return pack_images([s[0] for s in samples]), default_collate(rest)


def eval_geometry(sizes, image_size, square_resize_only=False):
    """The geometry of the inference transform (open_clip/transform.py:186-213) for images of sizes int [B, 2] = (H, W): int32
    [B, 8] = (box top, left, height, width, out_h, out_w, oy, ox) as ops.resample_ragged_u8 takes it.  The box is the whole image.
    Resize(S) + CenterCrop(S): the short side becomes S and the long side int(S * long / short) (the image is left as it is when
    its short side already is S), the window starts at int(round((out - S) / 2.)) - Python's round, half to even.  The long
    side is >= S after Resize(S), so CenterCrop's padding branch never occurs.  square_resize_only: Resize((S, S)), window (0, 0)."""
    S = int(image_size)
    hw = torch.as_tensor(sizes).cpu().long().reshape(-1, 2)
    H, W = hw[:, 0], hw[:, 1]
    zero = torch.zeros_like(H)
    if square_resize_only:
        oh = ow = torch.full_like(H, S)
        oy = ox = zero
    else:
        short, long = torch.minimum(H, W), torch.maximum(H, W)
        new_long = torch.where(short == S, long, ((S * long).double() / short.double()).long())
        oh = torch.where(W <= H, new_long, torch.full_like(H, S))
        ow = torch.where(W <= H, torch.full_like(H, S), new_long)
        oy = torch.round((oh - S).double() / 2.0).long()
        ox = torch.round((ow - S).double() / 2.0).long()
    return torch.stack([zero, zero, H, W, oh, ow, oy, ox], 1).to(torch.int32).contiguous()


class DeviceEvalTransform:
    """The reference's inference transform up to PILToTensor (image_transform(is_train=False), open_clip/transform.py:186-213:
    Resize(S, interpolation) + CenterCrop(S), or Resize((S, S)) with square_resize_only) on a device batch: a RaggedImages, or a
    uniform uint8 [B, H, W, 3] tensor (taken as a ragged batch of equal sizes).  Returns uint8 [B, 3, S, S] in channels_last
    memory - the model's input format; mean / std are applied by the patch gather."""

    def __init__(self, image_size, interpolation="bicubic", square_resize_only=False):
        if interpolation not in ("bicubic", "bilinear"):
            raise ValueError(f"DeviceEvalTransform: interpolation must be 'bicubic' or 'bilinear', got {interpolation!r}")
        self.size, self.interpolation, self.square = int(image_size), interpolation, bool(square_resize_only)

    def __call__(self, images):
        from . import ops
        if not isinstance(images, RaggedImages):
            images = RaggedImages.from_uniform(images)
        geometry = eval_geometry(images.host_tables()[1], self.size, self.square)
        return ops.resample_ragged_u8(images, geometry, self.size, self.interpolation).permute(0, 3, 1, 2)


def sample_color_jitter(batch, brightness, contrast, saturation, hue, prob, generator=None):
    """Per-sample parameters of `color_jitter(brightness, contrast, saturation, hue, p)` (open_clip/transform.py:61-72 around
    torchvision ColorJitter.get_params): apply ~ Bernoulli(prob) uint8 [B], a random permutation of the four operations
    int32 [B,4] (0 brightness, 1 contrast, 2 saturation, 3 hue) and factors f32 [B,4] indexed by operation: U(max(0, 1 - x), 1 + x)
    for the first three, U(-hue, hue) for the hue shift."""
    apply = (torch.rand(batch, generator=generator) < prob).to(torch.uint8)
    order = torch.argsort(torch.rand(batch, 4, generator=generator), dim=1).to(torch.int32).contiguous()
    lo = torch.tensor([max(0.0, 1 - brightness), max(0.0, 1 - contrast), max(0.0, 1 - saturation), -hue])
    hi = torch.tensor([1 + brightness, 1 + contrast, 1 + saturation, hue])
    factors = (lo + (hi - lo) * torch.rand(batch, 4, generator=generator)).to(torch.float32).contiguous()
    return apply, order, factors


class DeviceAugment:
    """The reference's train transform (open_clip/transform.py:152-168) on a staged uint8 NHWC device batch:
    RandomResizedCrop(image_size, scale, ratio, BICUBIC) -> [color_jitter(b, c, s, h) with probability color_jitter_prob] ->
    [gray_scale with probability gray_scale_prob].  Returns uint8 [B, 3, S, S] in channels_last memory - the model's input
    format.  Random parameters are sampled on the host (a few bytes per sample); the pixels never leave the device.
    A RaggedImages batch (images of different sizes) is taken as well: every crop box is sampled inside its own image."""

    def __init__(self, image_size, scale=(0.9, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), color_jitter=None, color_jitter_prob=0.0,
                 gray_scale_prob=0.0, seed=0):
        self.size, self.scale, self.ratio = int(image_size), tuple(scale), tuple(ratio)
        self.jitter = tuple(float(v) for v in color_jitter) if color_jitter else None
        if self.jitter is not None and len(self.jitter) != 4:
            raise ValueError("color_jitter = (brightness, contrast, saturation, hue)")
        self.jitter_p = float(color_jitter_prob or 0.0) if self.jitter else 0.0
        self.gray_p = float(gray_scale_prob or 0.0)
        self.gen = torch.Generator(device="cpu").manual_seed(int(seed))

    def sample(self, B, Hs, Ws):
        """-> boxes int32 [B,4], (apply, order, factors) | None, gray uint8 [B] | None: one batch's random parameters (CPU).
        Hs, Ws: the staged size, or per-sample heights and widths [B] of a ragged batch (the same random stream)."""
        if torch.is_tensor(Hs) or isinstance(Hs, (list, tuple)):
            boxes = sample_crop_boxes_ragged(Hs, Ws, self.scale, self.ratio, self.gen)
        else:
            boxes = sample_crop_boxes(B, Hs, Ws, self.scale, self.ratio, self.gen)
        jit = sample_color_jitter(B, *self.jitter, self.jitter_p, self.gen) if self.jitter_p > 0 else None
        gray = (torch.rand(B, generator=self.gen) < self.gray_p).to(torch.uint8) if self.gray_p > 0 else None
        return boxes, jit, gray

    def __call__(self, staged):
        from . import ops
        ragged = isinstance(staged, RaggedImages)
        on_gpu = (staged.data if ragged else staged).is_cuda
        put = (lambda t: t.pin_memory().to(staged.device, non_blocking=True)) if on_gpu else (lambda t: t)
        if ragged:                            # images of different sizes: every box is sampled inside its own image
            B, sizes = len(staged), staged.host_tables()[1]
            boxes, jit, gray = self.sample(B, sizes[:, 0], sizes[:, 1])
            geometry = torch.cat([boxes, torch.tensor([[self.size, self.size, 0, 0]], dtype=torch.int32).repeat(B, 1)], 1)
            resize = lambda flags: ops.resample_ragged_u8(staged, geometry, self.size, "bicubic", flags)
        else:
            B, Hs, Ws, _ = staged.shape
            boxes, jit, gray = self.sample(B, Hs, Ws)
            boxes = put(boxes)
            resize = lambda flags: ops.resized_crop_u8(staged, boxes, self.size, flags)
        gray = put(gray) if gray is not None else None
        if jit is None:                       # grayscale rides in the resize kernel's store
            return resize(gray).permute(0, 3, 1, 2)
        out = resize(None)
        apply, order, factors = (put(t) for t in jit)
        ops.color_jitter_u8_(out, apply, order, factors, gray)
        return out.permute(0, 3, 1, 2)


class DevicePrefetcher:
    """Iterate a host loader of (images uint8 [B,H,W,3] or [B,3,H,W], texts int64 [B,ctx]) batches `depth` batches ahead:
    each batch is staged in a pinned buffer, copied on a dedicated HIP stream and (optionally) augmented there, so the H2D
    copy of training/train.py:187-189 and the transform overlap the previous step instead of preceding this one.
    The first element may also be a batch of images of different sizes - a RaggedImages (ragged_collate) or a list of uint8
    [H, W, 3] arrays - for a transform that takes one (DeviceEvalTransform, DeviceAugment); the second may be any tensor
    (labels, ids), so the output feeds the evaluators as a loader of (images, ...) batches."""

    def __init__(self, loader, device, transform=None, depth=2):
        self.loader, self.device, self.transform, self.depth = loader, torch.device(device), transform, max(1, int(depth))
        self.cuda = self.device.type == "cuda"
        self.stream = torch.cuda.Stream(self.device) if self.cuda else None
        self._pins = [dict() for _ in range(self.depth)]      # slot -> {name: pinned tensor}
        self._free = [None] * self.depth                       # slot -> event after which the pinned buffers may be rewritten

    def _stage(self, slot, name, t):
        t = torch.as_tensor(t)
        if not self.cuda or t.is_pinned():
            return t
        buf = self._pins[slot].get(name)
        if buf is None or buf.shape != t.shape or buf.dtype != t.dtype:
            buf = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            self._pins[slot][name] = buf
        buf.copy_(t)
        return buf

    def _grown(self, slot, name, numel, dtype):
        """A pinned 1-D buffer of this slot with room for numel elements: kept, and replaced only by a larger one."""
        buf = self._pins[slot].get(name)
        if buf is None or buf.numel() < numel or buf.dtype != dtype:
            buf = torch.empty(max(int(numel), 1), dtype=dtype, pin_memory=True)
            self._pins[slot][name] = buf
        return buf

    def _stage_ragged(self, slot, images):
        """Images of different sizes - a RaggedImages or a list of uint8 [H, W, 3] arrays - in this slot's pinned buffers, which
        grow to the largest batch seen."""
        if not self.cuda:
            return images if isinstance(images, RaggedImages) else pack_images(images)
        if isinstance(images, RaggedImages):
            if images.is_pinned():
                return images
            data = self._grown(slot, "ragged", images.data.numel(), torch.uint8)[:images.data.numel()]
            data.copy_(images.data)
            offsets, sizes = images.host_tables()
        else:
            tensors, offsets, sizes, total = _image_tables(images)
            data = _fill_packed(self._grown(slot, "ragged", total, torch.uint8)[:total], tensors, offsets)
        B = offsets.numel()
        p_off = self._grown(slot, "ragged_offsets", B, torch.int64)[:B]
        p_size = self._grown(slot, "ragged_sizes", 2 * B, torch.int32)[:2 * B].view(B, 2)
        p_off.copy_(offsets)
        p_size.copy_(sizes)
        return RaggedImages(data, p_off, p_size, (offsets, sizes))

    def _submit(self, slot, batch):
        images, texts = batch
        if self._free[slot] is not None:
            self._free[slot].synchronize()                     # the copy that last read this slot's pinned buffers is done
        if isinstance(images, (RaggedImages, list, tuple)):
            images = self._stage_ragged(slot, images)
        else:
            images = self._stage(slot, "images", images)
        texts = self._stage(slot, "texts", texts)
        if not self.cuda:
            return (self.transform(images) if self.transform else images), texts, None
        with torch.cuda.stream(self.stream):
            d_img = images.to(self.device, non_blocking=True)
            d_txt = texts.to(self.device, non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(self.stream)
            self._free[slot] = copied
            if self.transform is not None:
                d_img = self.transform(d_img)
            ready = torch.cuda.Event()
            ready.record(self.stream)
        return d_img, d_txt, ready

    def __iter__(self):
        queue = collections.deque()
        slot = 0
        for batch in self.loader:
            queue.append(self._submit(slot, batch))
            slot = (slot + 1) % self.depth
            if len(queue) >= self.depth:
                yield self._hand_over(queue.popleft())
        while queue:
            yield self._hand_over(queue.popleft())

    def _hand_over(self, item):
        d_img, d_txt, ready = item
        if ready is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ready)
            d_img.record_stream(cur)
            d_txt.record_stream(cur)
        return d_img, d_txt
