"""dgan.filters.dejpeg_ref, the definition of the shift-averaged JPEG re-application: the literal
64-fold loop over `jpeg_ref`, its integer types, its tables, its arguments, and the condition that
it improves a JPEG-coded image-like frame."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_jpeg import image


def photo():
    """uint8 [128,128,3]: correlated channels, a stripe pattern and a coloured disk."""
    from dataloader import synthetic_pair
    _, y = synthetic_pair(1, 128, seed=3)
    g = y[0].mean(-1, keepdims=True)
    yy, xx = np.mgrid[0:128, 0:128]
    base = (g * 0.4 + 0.5) * 255 + 0.15 * 255 * y[0] * 0.3
    base = base + (((xx * 0.7 + yy * 0.4) % 37 < 18) * 50 - 25)[..., None]
    base = base + (((xx - 64) ** 2 + (yy - 60) ** 2 < 900)[..., None] * np.array([40, -10, -30]))
    return np.clip(base, 0, 255).astype(np.uint8)


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize("h,w", [(13, 21), (1, 1)])
def test_the_reference_is_the_loop_over_jpeg_ref_in_both_types_and_with_tables(h, w):
    from dgan.filters import dejpeg_ref
    from dgan.jpeg import jpeg_ref, quant_tables
    a = image("random", h, w)
    acc = np.zeros(a.shape, np.int64)
    for dy in range(8):
        for dx in range(8):
            acc += jpeg_ref(np.pad(a, ((dy, 0), (dx, 0), (0, 0)), mode="edge"), 50)[dy:, dx:]
    want = ((acc + 32) >> 6).astype(np.uint8)
    got = dejpeg_ref(a, 50)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(dejpeg_ref(a, 50, dtype=np.int32), want)
    assert np.array_equal(dejpeg_ref(a, tables=quant_tables(50)), want)
    assert np.array_equal(dejpeg_ref(a, 7, tables=quant_tables(50)), want)
    assert np.array_equal(dejpeg_ref(a[None], 50), want[None])
    assert not np.array_equal(dejpeg_ref(a, 20), want) or (h, w) == (1, 1)


@pytest.mark.parametrize("quality", [10, 50, 100])
def test_a_flat_frame_comes_back_unchanged(quality):
    """Every shift of a flat frame is flat, so the 64 round trips agree: the frame comes back as the
    round trip itself returns it (the quantised DC moves a flat colour; mid-grey is exact at any
    quality and comes back unchanged)."""
    from dgan.filters import dejpeg_ref
    from dgan.jpeg import jpeg_ref
    grey = np.full((9, 20, 3), 128, np.uint8)
    assert np.array_equal(dejpeg_ref(grey, quality), grey)
    a = np.full((9, 20, 3), (200, 30, 77), np.uint8)
    assert np.array_equal(dejpeg_ref(a, quality), jpeg_ref(a, quality))


@pytest.mark.parametrize("kw,match", [
    (dict(quality=0), "quality"), (dict(quality=101), "quality"), (dict(quality=50.0), "quality"),
    (dict(quality=True), "quality"), (dict(tables=np.ones((2, 63), np.uint8)), "tables"),
    (dict(tables=np.ones((2, 64), np.int64)), "tables"), (dict(tables=np.zeros((2, 64), np.uint8)), "tables"),
    (dict(dtype=np.int16), "dtype"), (dict(a=np.zeros((8, 8, 3), np.float32)), "uint8"),
    (dict(a=np.zeros((0, 8, 3), np.uint8)), "empty")])
def test_bad_arguments_raise_naming_the_argument(kw, match):
    from dgan.filters import dejpeg_ref
    with pytest.raises(ValueError, match=match):
        dejpeg_ref(kw.pop("a", np.zeros((8, 8, 3), np.uint8)), **kw)


@pytest.mark.parametrize("quality", [10, 50])
def test_re_application_improves_a_jpeg_coded_image_like_frame(quality):
    from dgan.filters import dejpeg_ref
    from dgan.jpeg import jpeg_ref
    img = photo()
    coded = jpeg_ref(img, quality)
    before, after = psnr(coded, img), psnr(dejpeg_ref(coded, quality), img)
    print(f"quality {quality}: {before:.2f} dB -> {after:.2f} dB")
    assert after > before


def test_the_definition_needs_neither_torch_nor_the_library():
    import dgan
    code = ("import sys; import dgan.filters as F; import numpy as np; F.dejpeg_ref(np.zeros((3, 3, 3), np.uint8)); "
            "assert 'torch' not in sys.modules and 'dgan._lib' not in sys.modules")
    root = os.path.dirname(os.path.dirname(os.path.abspath(dgan.__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root)
    assert r.returncode == 0, r.stderr
