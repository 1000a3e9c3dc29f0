"""GPU parity of the ragged device input pipeline (clipa_resample_ragged_u8 through ops.resample_ragged_u8, DeviceEvalTransform,
DeviceAugment and DevicePrefetcher on RaggedImages) - byte work, so the bar is BIT-EXACT against the numpy reference of
tests/ragged_cases.py (which tests/test_ragged_input_cpu.py pins to live Pillow) and, where Pillow imports, against Pillow."""
import numpy as np
import pytest
import torch

from clipa_amd import data as D
from oracle import color_oracle as C
from oracle import resize_oracle as R

from . import ragged_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ops():
    from clipa_amd import ops as _ops
    return _ops


def _same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape and np.array_equal(got, want), (what, float((got != want).mean()))


@pytest.mark.parametrize("interpolation", RC.INTERPOLATIONS)
@pytest.mark.parametrize("mode", RC.MODES)
@pytest.mark.parametrize("S", RC.SIZES)
def test_case_table_one_launch(S, mode, interpolation):
    packed = D.pack_images([np.array(im) for im in RC.images(S)]).to(DEV)
    out = ops().resample_ragged_u8(packed, torch.from_numpy(RC.geometry(S, mode)), S, interpolation).cpu().numpy()
    want = RC.expected(S, mode, interpolation)
    assert out.shape == want.shape and out.dtype == np.uint8
    for i in range(len(want)):
        _same(out[i], want[i], (S, mode, interpolation, RC.CASES[S][i]))
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        flt = Image.BICUBIC if interpolation == "bicubic" else Image.BILINEAR
        for i, (img, g) in enumerate(zip(RC.images(S), RC.geometry(S, mode))):
            oh, ow, oy, ox = (int(v) for v in g[4:])
            pil = np.asarray(Image.fromarray(img).resize((ow, oh), flt).crop((ox, oy, ox + S, oy + S)))
            _same(out[i], pil, ("pillow", S, mode, interpolation, RC.CASES[S][i]))
    ops().check_token_ids(wait=True)


def test_uniform_batch_equals_resized_crop():
    B, Hs, Ws, S = 12, 72, 90, 48
    g = torch.Generator().manual_seed(21)
    src = torch.randint(0, 256, (B, Hs, Ws, 3), generator=g, dtype=torch.uint8).to(DEV)
    boxes = D.sample_crop_boxes(B, Hs, Ws, (0.08, 1.0), (3 / 4, 4 / 3), g)
    boxes[0] = torch.tensor([0, 0, Hs, Ws], dtype=torch.int32)
    boxes[1] = torch.tensor([Hs - 9, Ws - 11, 9, 11], dtype=torch.int32)
    gray = (torch.rand(B, generator=g) < 0.5).to(torch.uint8).to(DEV)
    geometry = torch.cat([boxes, torch.tensor([[S, S, 0, 0]], dtype=torch.int32).repeat(B, 1)], 1)
    for flags in (None, gray):
        want = ops().resized_crop_u8(src, boxes.to(DEV), S, flags)
        got = ops().resample_ragged_u8(D.RaggedImages.from_uniform(src), geometry, S, "bicubic", flags)
        assert torch.equal(got, want)
    ops().check_token_ids(wait=True)


def test_hand_built_table():
    """Shuffled order, gaps, two samples on one image, unaligned offsets, the last image ending exactly at packed_bytes with
    other bytes behind it in the allocation."""
    S = 16
    imgs = RC.images(S)
    order = [4, 0, 2, 0, 9, 1]                                   # image 0 twice; image 1 (23 x 40 x 3 = 2760 bytes) last
    place = {4: 7, 0: 2101, 2: 15003, 9: 20001, 1: None}
    end = 20001 + imgs[9].size + 37
    place[1] = end
    packed_bytes = end + imgs[1].size
    alloc = torch.full((packed_bytes + 4096,), 255, dtype=torch.uint8)
    alloc[:packed_bytes] = torch.randint(0, 256, (packed_bytes,), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    for k, o in place.items():
        alloc[o:o + imgs[k].size] = torch.from_numpy(np.array(imgs[k])).reshape(-1)
    dev = alloc.to(DEV)
    offsets = torch.tensor([place[k] for k in order], dtype=torch.int64)
    sizes = torch.tensor([RC.CASES[S][k] for k in order], dtype=torch.int32)
    ragged = D.RaggedImages(dev[:packed_bytes], offsets.to(DEV), sizes.to(DEV), (offsets, sizes))
    for mode in RC.MODES:
        geometry = torch.from_numpy(RC.geometry(S, mode)[order])
        out = ops().resample_ragged_u8(ragged, geometry, S).cpu().numpy()
        _same(out, RC.expected(S, mode, "bicubic")[order], mode)
    ops().check_token_ids(wait=True)


def test_offsets_past_two_gib():
    """4096 decoded photographs exceed 2 GiB: an image behind byte 2^31 of the packed buffer (device memory only, never filled)."""
    S = 16
    imgs = RC.images(S)
    dev = torch.empty(2 ** 31 + 65536, dtype=torch.uint8, device=DEV)
    offsets = torch.tensor([3, 2 ** 31 + 5, 2 ** 31 + 65536 - imgs[2].size], dtype=torch.int64)
    sizes = torch.tensor(RC.CASES[S][:3], dtype=torch.int32)
    for o, im in zip(offsets.tolist(), imgs):
        dev[o:o + im.size] = torch.from_numpy(np.array(im)).reshape(-1).to(DEV)
    ragged = D.RaggedImages(dev, offsets.to(DEV), sizes.to(DEV), (offsets, sizes))
    out = ops().resample_ragged_u8(ragged, torch.from_numpy(RC.geometry(S, "eval")[:3].copy()), S)
    _same(out, RC.expected(S, "eval", "bicubic")[:3], "past 2 GiB")
    ops().check_token_ids(wait=True)


def test_rejected_descriptors_are_zeros():
    """Descriptors that leave their bounds, given to the device unchecked: the data tensor is a narrow view of a larger
    allocation and the bad image descriptor stays inside that allocation, so a missing check can only fail this test."""
    S = 16
    imgs = RC.images(S)
    good = D.pack_images([np.array(im) for im in imgs[:5]])
    n = good.data.numel()
    alloc = torch.zeros(n + 65536, dtype=torch.uint8)
    alloc[:n] = good.data
    alloc[n:] = 200
    dev = alloc.to(DEV)
    offsets, sizes = (t.clone() for t in good.host_tables())
    geometry = torch.from_numpy(RC.geometry(S, "eval")[:5].copy())
    offsets[1] = n - 100                                         # 40 x 23 x 3 bytes from here: past the view, inside the allocation
    sizes[1] = torch.tensor([40, 23], dtype=torch.int32)
    geometry[1] = torch.tensor(RC.eval_row(40, 23, S), dtype=torch.int32)
    geometry[2, 0:4] = torch.tensor([30, 0, 20, 37], dtype=torch.int32)      # box rows 30 .. 50 of a 37-row image
    geometry[3, 6] = 1                                           # window row 1 + 16 > out_h = 16
    ragged = D.RaggedImages(dev[:n], offsets.to(DEV), sizes.to(DEV), (offsets, sizes))
    with pytest.raises(ValueError, match="sample 1"):
        ops().resample_ragged_u8(ragged, geometry, S)            # the host check names the first of them
    ops().check_token_ids(wait=True)
    out = ops().resample_ragged_u8(ragged, geometry, S, validate=False).cpu().numpy()
    want = RC.expected(S, "eval", "bicubic")
    for i in (1, 2, 3):
        assert int(out[i].max()) == 0, i
    for i in (0, 4):
        _same(out[i], want[i], i)
    with pytest.raises(RuntimeError, match="3 samples rejected"):
        ops().check_token_ids(wait=True)


def test_eval_transform_under_prefetcher():
    S = 16
    imgs = [np.array(im) for im in RC.images(S)]
    picks = [[0, 1, 2], [3, 4, 5, 6, 7, 8, 9], [1, 9, 4, 5], [6, 7]]           # the pinned buffers grow, then serve smaller batches
    batches = [([imgs[k] for k in p], torch.tensor(p, dtype=torch.int64)) for p in picks]
    want = RC.expected(S, "eval", "bilinear")
    got = list(D.DevicePrefetcher(iter(batches), DEV, transform=D.DeviceEvalTransform(S, "bilinear"), depth=2))
    assert len(got) == 4
    for p, (img, labels) in zip(picks, got):
        assert img.shape == (len(p), 3, S, S) and img.dtype == torch.uint8 and img.is_cuda
        assert img.is_contiguous(memory_format=torch.channels_last)
        assert labels.is_cuda and labels.dtype == torch.int64 and labels.tolist() == p
        _same(img.permute(0, 2, 3, 1), want[p], p)
    uniform = torch.from_numpy(np.stack([imgs[0]] * 3)).to(DEV)                  # a uniform [B, H, W, 3] tensor is accepted too
    out = D.DeviceEvalTransform(S, square_resize_only=True)(uniform)
    _same(out[2].permute(1, 2, 0), RC.expected(S, "square", "bicubic")[0], "uniform")
    ops().check_token_ids(wait=True)


def test_device_augment_ragged_full_recipe():
    """The reference GPU recipe (scale (0.4, 1), color_jitter (0.32, 0.32, 0.32, 0.08) p = 0.8, gray_scale p = 0.2) on batches
    of mixed sizes equals the oracle's composition driven by the augmenter's own random stream."""
    S = 33
    kw = dict(scale=(0.4, 1.0), color_jitter=(0.32, 0.32, 0.32, 0.08), color_jitter_prob=0.8, gray_scale_prob=0.2)
    aug, twin = D.DeviceAugment(S, seed=9, **kw), D.DeviceAugment(S, seed=9, **kw)
    for src in (48, 16):
        imgs = [np.array(im) for im in RC.images(src) if min(im.shape[:2]) >= 9]
        packed = D.pack_images(imgs)
        out = aug(packed.to(DEV))
        assert out.shape == (len(imgs), 3, S, S) and out.is_contiguous(memory_format=torch.channels_last)
        boxes, (apply, order, factors), gray = twin.sample(len(imgs), packed.sizes[:, 0], packed.sizes[:, 1])
        for i, im in enumerate(imgs):
            ref = RC.reference(im, tuple(boxes[i].tolist()) + (S, S, 0, 0), S)
            if int(apply[i]):
                ref = C.color_jitter(ref, order[i].numpy(), factors[i].numpy())
            if int(gray[i]):
                ref = R.grayscale3(ref)
            _same(out[i].permute(1, 2, 0), ref, (src, i, boxes[i].tolist()))
    gray_only = D.DeviceAugment(S, scale=(0.4, 1.0), gray_scale_prob=0.5, seed=2)         # grayscale in the resize kernel's store
    imgs = [np.array(im) for im in RC.images(48)]
    out = gray_only(D.pack_images(imgs).to(DEV))
    sizes = torch.tensor([im.shape[:2] for im in imgs])
    boxes, _, gray = D.DeviceAugment(S, scale=(0.4, 1.0), gray_scale_prob=0.5, seed=2).sample(len(imgs), sizes[:, 0], sizes[:, 1])
    assert 0 < int(gray.sum()) < len(imgs)
    for i, im in enumerate(imgs):
        ref = RC.reference(im, tuple(boxes[i].tolist()) + (S, S, 0, 0), S)
        _same(out[i].permute(1, 2, 0), R.grayscale3(ref) if int(gray[i]) else ref, ("gray", i))
    ops().check_token_ids(wait=True)


def test_model_end_to_end():
    """encode_image and zero_shot.run over device-transformed ragged batches equal the same images preprocessed on the host by
    clipa_amd.transform (Pillow)."""
    Image = pytest.importorskip("PIL.Image")
    import clipa_amd
    from clipa_amd import zero_shot
    from .conftest import load_golden
    gd = load_golden("cls_erf")
    m = clipa_amd.CLIP(**gd.cfg, output_dict=True)
    m.load_state_dict(gd.sd)
    m.to(DEV).eval()
    S = gd.cfg["vision_cfg"]["image_size"]
    imgs = [np.array(im) for src in (48, 33, 32) for im in RC.images(src)]
    host_tf = clipa_amd.image_transform(S, is_train=False, to_float_on_device=True)
    host = torch.stack([host_tf(Image.fromarray(im)) for im in imgs])
    dev_tf = D.DeviceEvalTransform(S)
    x = dev_tf(D.pack_images(imgs).to(DEV))
    assert torch.equal(x.cpu(), host)
    with torch.no_grad():
        a = m.encode_image(x, normalize=True)
        b = m.encode_image(host.to(DEV), normalize=True)
    assert torch.equal(a, b)
    ctx = gd.texts.shape[1]
    classes = min(4, gd.texts.shape[0] // 2)
    classifier, C_ = zero_shot.zero_shot_classifier(m, gd.texts[:2 * classes].view(classes, 2, ctx).to(DEV))
    labels = torch.arange(len(imgs), dtype=torch.int64) % classes
    cuts = [(0, 5), (5, 9), (9, len(imgs))]
    ragged = D.DevicePrefetcher(((D.pack_images(imgs[s:e]), labels[s:e]) for s, e in cuts), DEV, transform=dev_tf)
    hosted = ((host[s:e].to(DEV), labels[s:e].to(DEV)) for s, e in cuts)
    assert zero_shot.run(m, classifier, C_, ragged, topk=(1, 2)) == zero_shot.run(m, classifier, C_, hosted, topk=(1, 2))
    ops().check_token_ids(wait=True)
