"""The case table and the numpy reference of the ragged device input pipeline (clipa_amd/csrc/resample_ragged.hip), shared by
tests/test_ragged_input_cpu.py (which pins the reference to live Pillow) and tests/test_ragged_input_gpu.py (which holds the
kernels to it, byte for byte).

    reference(img, geometry, S, interpolation) = resize(crop(img, box), (out_h, out_w), filter)[oy : oy + S, ox : ox + S]

with geometry = (box top, left, height, width, out_h, out_w, oy, ox).  Bicubic is oracle.resize_oracle (precompute_coeffs /
resize_u8); the triangle filter of Pillow's BILINEAR (Resample.c bilinear_filter, support 1) is restated here on the same
integer passes.  Every image is uniform noise - the hardest input for a bit-exactness check - from a seed of its own."""
import functools
import math

import numpy as np

from oracle import resize_oracle as R

# (H, W) per output size S: the smallest shapes at which the geometry or the kernels can go wrong
CASES = {
    16: [(40, 23),        # portrait
         (23, 40),        # landscape
         (37, 37),        # square, odd byte size
         (16, 50),        # short side == S: the vertical axis is untouched
         (41, 16),        # short side == S: the horizontal axis is untouched
         (16, 16),        # both sides == S: identity
         (9, 13),         # short side < S: up-scaling
         (3, 50),         # three rows
         (50, 1),         # one column
         (97, 160),       # more than one block of intermediate rows
         (1024, 20)],     # square: exactly 64x, the 257 bicubic taps the entry serves at most
    32: [(400, 420),      # 12.5x / 13.1x: beyond the 11.5x of clipa_resized_crop_u8
         (32, 1300),      # short side == S and a 40.6x square resize
         (45, 61)],
    33: [(50, 70),        # odd S
         (35, 34),
         (33, 33),
         (71, 33)],
    48: [(75, 131),       # long side 83.84 -> 83, crop remainder 17.5 -> 18 (half to even)
         (75, 133),       # long side 85.12 -> 85, crop remainder 18.5 -> 18
         (131, 75),
         (20, 31),        # up-scaling to 48 x 74
         (48, 48)],
}
SIZES = sorted(CASES)
INTERPOLATIONS = ("bicubic", "bilinear")
MODES = ("eval", "square")


@functools.lru_cache(maxsize=None)
def images(S):
    """The images of CASES[S], uint8 [H, W, 3] noise (read-only: shared between tests)."""
    out = []
    for i, (h, w) in enumerate(CASES[S]):
        a = np.random.default_rng(1000 * S + i).integers(0, 256, (h, w, 3), dtype=np.uint8)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def eval_row(h, w, S, square=False):
    """Geometry of the inference transform in plain Python, the arithmetic of torchvision's Resize / CenterCrop as
    clipa_amd/transform.py states it: the checker of clipa_amd.data.eval_geometry."""
    if square:
        return (0, 0, h, w, S, S, 0, 0)
    short, long = (w, h) if w <= h else (h, w)
    new_long = long if short == S else int(S * long / short)
    oh, ow = (new_long, S) if w <= h else (S, new_long)
    return (0, 0, h, w, oh, ow, int(round((oh - S) / 2.0)), int(round((ow - S) / 2.0)))


def geometry(S, mode):
    """int32 [len(CASES[S]), 8] for mode 'eval' or 'square'."""
    return np.array([eval_row(h, w, S, mode == "square") for h, w in CASES[S]], np.int32)


def triangle_coeffs(in_size, out_size):
    """Resample.c precompute_coeffs + normalize_coeffs_8bpc with bilinear_filter (support 1) over the whole axis."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = []
        for x in range(xmax):
            v = abs((x + xmin - center + 0.5) * ss)
            k.append(1.0 - v if v < 1.0 else 0.0)
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        for x, w in enumerate(k):
            v = w * (1 << R.PRECISION_BITS)
            kk[xx, x] = int(-0.5 + v) if w < 0 else int(0.5 + v)
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def resize_bilinear_u8(img, out_h, out_w):
    """Pillow Image.resize((out_w, out_h), BILINEAR) of a uint8 [h, w, c] image: the passes of oracle.resize_oracle.resize_u8."""
    h, w = img.shape[:2]
    if out_w != w:
        bx, kx = triangle_coeffs(w, out_w)
        img = np.ascontiguousarray(np.swapaxes(R._resample_axis0(np.ascontiguousarray(np.swapaxes(img, 0, 1)), bx, kx), 0, 1))
    if out_h != h:
        by, ky = triangle_coeffs(h, out_h)
        img = R._resample_axis0(img, by, ky)
    return img


def reference(img, geometry, S, interpolation="bicubic"):
    top, left, bh, bw, oh, ow, oy, ox = (int(v) for v in geometry)
    crop = np.ascontiguousarray(img[top:top + bh, left:left + bw])
    full = R.resize_u8(crop, oh, ow) if interpolation == "bicubic" else resize_bilinear_u8(crop, oh, ow)
    assert 0 <= oy and oy + S <= oh and 0 <= ox and ox + S <= ow, "the window leaves the resized image"
    return np.ascontiguousarray(full[oy:oy + S, ox:ox + S])


@functools.lru_cache(maxsize=None)
def expected(S, mode, interpolation):
    """uint8 [len(CASES[S]), S, S, 3]: the reference of every case (computed once, read-only)."""
    out = np.stack([reference(im, g, S, interpolation) for im, g in zip(images(S), geometry(S, mode))])
    out.setflags(write=False)
    return out
