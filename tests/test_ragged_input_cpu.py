"""Host side of the ragged device input pipeline, without a GPU: the numpy reference of tests/ragged_cases.py is bit-equal to
live Pillow on every case of the table (so the GPU tests that are held to it are held to Pillow), eval_geometry is the
Resize / CenterCrop arithmetic, the ragged box sampler is sample_crop_boxes sample by sample, packing round-trips, and what the
C entry refuses is refused on the host with the sample's index."""
import numpy as np
import pytest
import torch

from clipa_amd import data as D
from clipa_amd import ops, transform as T

from . import ragged_cases as RC


@pytest.mark.parametrize("interpolation", RC.INTERPOLATIONS)
@pytest.mark.parametrize("S", RC.SIZES)
def test_reference_equals_pillow(S, interpolation):
    Image = pytest.importorskip("PIL.Image")
    mode = Image.BICUBIC if interpolation == "bicubic" else Image.BILINEAR
    for square in (False, True):
        want = RC.expected(S, "square" if square else "eval", interpolation)
        pipeline = T.Compose([T.Resize((S, S), interpolation)] if square else [T.Resize(S, interpolation), T.CenterCrop(S)])
        for i, (img, g) in enumerate(zip(RC.images(S), RC.geometry(S, "square" if square else "eval"))):
            _, _, _, _, oh, ow, oy, ox = (int(v) for v in g)
            pil = Image.fromarray(img)
            direct = pil.resize((ow, oh), mode).crop((ox, oy, ox + S, oy + S))
            assert np.array_equal(np.asarray(direct), want[i]), ("resize + crop", S, RC.CASES[S][i], square)
            assert np.array_equal(np.asarray(pipeline(pil)), want[i]), ("transform", S, RC.CASES[S][i], square)


@pytest.mark.parametrize("interpolation", RC.INTERPOLATIONS)
def test_reference_equals_pillow_on_crop_boxes(interpolation):
    """The train geometry: crop(box) then resize to S x S, also past the 11.5x of the uniform kernel."""
    Image = pytest.importorskip("PIL.Image")
    mode = Image.BICUBIC if interpolation == "bicubic" else Image.BILINEAR
    img = RC.images(32)[0]                                    # 400 x 420
    for box in ((0, 0, 400, 420), (17, 3, 380, 391), (100, 200, 9, 11), (5, 7, 33, 300)):
        t, l, h, w = box
        want = np.asarray(Image.fromarray(img).crop((l, t, l + w, t + h)).resize((32, 32), mode))
        assert np.array_equal(RC.reference(img, box + (32, 32, 0, 0), 32, interpolation), want), box


@pytest.mark.parametrize("S", [16, 33])
def test_eval_geometry_is_resize_center_crop(S):
    sizes = torch.cartesian_prod(torch.arange(1, 97), torch.arange(1, 97)).to(torch.int32)
    for square in (False, True):
        got = D.eval_geometry(sizes, S, square)
        assert got.dtype == torch.int32 and tuple(got.shape) == (96 * 96, 8)
        want = torch.tensor([RC.eval_row(int(h), int(w), S, square) for h, w in sizes.tolist()], dtype=torch.int32)
        assert torch.equal(got, want)
        oh, ow, oy, ox = (got[:, k].long() for k in (4, 5, 6, 7))      # CenterCrop never pads: the window is inside
        assert bool(((oy >= 0) & (ox >= 0) & (oy + S <= oh) & (ox + S <= ow)).all())


def test_case_table_hits_the_rounding_edges():
    assert RC.eval_row(75, 131, 48)[4:] == (48, 83, 0, 18)      # 83.84 -> 83, 17.5 -> 18
    assert RC.eval_row(75, 133, 48)[4:] == (48, 85, 0, 18)      # 85.12 -> 85, 18.5 -> 18
    assert RC.eval_row(16, 50, 16)[4:] == (16, 50, 0, 17)
    assert any(h * w * 3 % 2 for S in RC.SIZES for h, w in RC.CASES[S])


def test_ragged_boxes_equal_uniform_sampler():
    for H, W, scale in ((256, 256, (0.08, 1.0)), (72, 200, (0.4, 1.0)), (3, 200, (0.9, 1.0))):
        a = D.sample_crop_boxes(64, H, W, scale, (3 / 4, 4 / 3), torch.Generator().manual_seed(5))
        g = torch.Generator().manual_seed(5)
        b = D.sample_crop_boxes_ragged(torch.full((64,), H), torch.full((64,), W), scale, (3 / 4, 4 / 3), g)
        assert b.dtype == torch.int32 and torch.equal(a, b), (H, W)
        g2 = torch.Generator().manual_seed(5)                      # the generator is left in the same state
        D.sample_crop_boxes(64, H, W, scale, (3 / 4, 4 / 3), g2)
        assert torch.equal(g.get_state(), g2.get_state())


def test_ragged_boxes_stay_inside_mixed_sizes():
    g = torch.Generator().manual_seed(9)
    hs = torch.randint(1, 3000, (512,), generator=g)
    ws = torch.randint(1, 3000, (512,), generator=g)
    hs[:4], ws[:4] = torch.tensor([3, 200, 1, 4000]), torch.tensor([200, 3, 1, 7])
    boxes = D.sample_crop_boxes_ragged(hs, ws, (0.08, 1.0), (3 / 4, 4 / 3), g).long()
    top, left, h, w = boxes.unbind(1)
    assert bool(((top >= 0) & (left >= 0) & (h > 0) & (w > 0) & (top + h <= hs) & (left + w <= ws)).all())


def test_ragged_boxes_fall_back_per_sample():
    ratio = (3 / 4, 4 / 3)
    sizes = [(3, 200), (200, 3), (2, 900), (1000, 7)]              # no attempt at scale (0.9, 1) fits these aspect ratios
    boxes = D.sample_crop_boxes_ragged([h for h, _ in sizes], [w for _, w in sizes], (0.9, 1.0), ratio,
                                       torch.Generator().manual_seed(1))
    for (h, w), box in zip(sizes, boxes.tolist()):
        assert tuple(box) == D.random_resized_crop_params(h, w, (2.0, 2.0), ratio), (h, w)


def test_device_augment_sample_ragged_stream():
    kw = dict(scale=(0.4, 1.0), color_jitter=(0.32, 0.32, 0.32, 0.08), color_jitter_prob=0.8, gray_scale_prob=0.2, seed=4)
    a = D.DeviceAugment(32, **kw).sample(8, 60, 90)
    b = D.DeviceAugment(32, **kw).sample(8, torch.full((8,), 60), torch.full((8,), 90))
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and torch.equal(a[2], b[2])


def test_pack_images_round_trip():
    imgs = [np.array(im) for im in RC.images(16)] + [torch.from_numpy(np.array(RC.images(33)[0]))]
    packed = D.pack_images(imgs)
    assert len(packed) == len(imgs) and packed.data.dtype == torch.uint8 and packed.data.dim() == 1
    assert packed.offsets.dtype == torch.int64 and packed.sizes.dtype == torch.int32 and tuple(packed.sizes.shape) == (len(imgs), 2)
    assert bool((packed.offsets % 16 == 0).all())
    ends = packed.offsets + packed.sizes[:, 0].long() * packed.sizes[:, 1].long() * 3
    assert bool((ends[:-1] <= packed.offsets[1:]).all()) and int(ends[-1]) <= packed.data.numel()
    for i, im in enumerate(imgs):
        assert np.array_equal(packed.image(i).numpy(), np.asarray(im)), i
    same = packed.to("cpu")
    assert torch.equal(same.data, packed.data) and torch.equal(same.sizes, packed.sizes)


@pytest.mark.parametrize("bad", [np.zeros((4, 4, 3), np.float32), np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8),
                                 np.zeros((0, 4, 3), np.uint8), torch.zeros(2, 4, 4, 3, dtype=torch.uint8)])
def test_pack_images_rejects(bad):
    with pytest.raises(ValueError, match="image 1"):
        D.pack_images([np.zeros((2, 2, 3), np.uint8), bad])


def test_ragged_collate():
    samples = [(np.array(im), i) for i, im in enumerate(RC.images(33))]
    images, labels = D.ragged_collate(samples)
    assert isinstance(images, D.RaggedImages) and len(images) == len(samples)
    assert labels.dtype == torch.int64 and labels.tolist() == list(range(len(samples)))
    assert np.array_equal(images.image(2).numpy(), RC.images(33)[2])


def test_prefetcher_passes_ragged_batches_on_the_host():
    imgs = [np.array(im) for im in RC.images(33)]
    batches = [(imgs[:2], torch.tensor([4, 5])), (D.pack_images(imgs[2:]), torch.tensor([6, 7]))]
    got = list(D.DevicePrefetcher(iter(batches), "cpu"))
    assert [len(g[0]) for g in got] == [2, 2] and all(isinstance(g[0], D.RaggedImages) for g in got)
    assert np.array_equal(got[0][0].image(1).numpy(), imgs[1]) and np.array_equal(got[1][0].image(0).numpy(), imgs[2])
    assert got[1][1].tolist() == [6, 7]


def test_from_uniform_is_a_view():
    t = torch.arange(2 * 3 * 5 * 3, dtype=torch.uint8).view(2, 3, 5, 3)
    r = D.RaggedImages.from_uniform(t)
    assert r.data.data_ptr() == t.data_ptr() and r.offsets.tolist() == [0, 45] and r.sizes.tolist() == [[3, 5], [3, 5]]
    assert torch.equal(r.image(1), t[1])


def _layout(sizes, geometry, S, packed_bytes=None, **kw):
    sizes = torch.tensor(sizes, dtype=torch.int32)
    nbytes = (sizes[:, 0].long() * sizes[:, 1].long() * 3 + 15) // 16 * 16
    return ops.ragged_layout(torch.cumsum(nbytes, 0) - nbytes, sizes, torch.tensor(geometry, dtype=torch.int32), S,
                             packed_bytes=int(nbytes.sum()) if packed_bytes is None else packed_bytes, **kw)


def test_host_refuses_what_the_entry_refuses():
    ok = RC.eval_row(40, 23, 16)
    with pytest.raises(ValueError, match=r"sample 1: down-scale above 64x"):
        _layout([(40, 23), (2100, 40)], [ok, (0, 0, 2100, 40, 32, 32, 0, 0)], 16)
    _layout([(40, 23), (2048, 40)], [ok, (0, 0, 2048, 40, 32, 32, 0, 0)], 16)                 # exactly 64x is served
    with pytest.raises(ValueError, match=r"sample 1: .*1\.\.16384"):
        _layout([(40, 23), (16385, 4)], [ok, RC.eval_row(16385, 4, 16, True)], 16)
    with pytest.raises(ValueError, match=r"sample 2: .*window lies outside"):
        _layout([(40, 23)] * 3, [ok, ok, (0, 0, 40, 23, 27, 16, 12, 0)], 16)
    with pytest.raises(ValueError, match=r"sample 0: crop box outside"):
        _layout([(40, 23)], [(30, 0, 11, 23, 16, 16, 0, 0)], 16)
    with pytest.raises(ValueError, match=r"sample 1: image outside the packed buffer"):
        _layout([(40, 23), (40, 23)], [ok, ok], 16, packed_bytes=2 * 2768 - 16)
    with pytest.raises(ValueError, match="size must be in"):
        _layout([(40, 23)], [ok], 4097)
    with pytest.raises(ValueError, match="interpolation"):
        _layout([(40, 23)], [ok], 16, interpolation="nearest")


def test_layout_is_ragged():
    """Every sample owns exactly the storage its own geometry needs: a large photograph does not multiply the others'."""
    sizes = [(40, 23), (4000, 6000), (23, 40)]
    geo = [RC.eval_row(h, w, 224) for h, w in sizes]
    geo[0], geo[2] = RC.eval_row(40, 23, 16, True), RC.eval_row(23, 40, 16, True)
    S = 16
    geo[1] = (0, 0, 4000, 6000, 224, 336, 104, 160)               # a 16 x 16 window out of the middle of the photograph
    desc, max_rows, tmp_bytes, coef_ints, _ = _layout(sizes, geo, S)
    kh, kv, rows = desc[:, 13].tolist(), desc[:, 14].tolist(), desc[:, 15].tolist()
    assert kh == [7, 2 * 36 + 1, 11] and kv == [11, 2 * 36 + 1, 7]         # 2 * ceil(2 * max(1, in / out)) + 1
    assert rows[0] == 40 and rows[2] == 23 and rows[1] < 16 * 18 + 80 and max_rows == rows[1]
    assert tmp_bytes == sum((r * S * 3 + 15) // 16 * 16 for r in rows) and coef_ints == sum(S * (a + b) for a, b in zip(kh, kv))
    assert desc[:, 11].tolist() == [0, 1920, 1920 + (rows[1] * 48 + 15) // 16 * 16]
    assert desc[:, 12].tolist() == [0, S * 18, S * 18 + S * 146]
