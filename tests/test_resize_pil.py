"""Pillow's resize restated (dgan/resize.py pil_coeffs, resize_pil_ref; no GPU) against
`Image.resize` itself, bit for bit; int32 against int64; the argument errors."""
import numpy as np
import pytest

# (hi, wi, h, w): identity, single-axis, x4 up, ragged down, a factor of 100, 1x1 at both ends
SHAPES = [(1, 1, 1, 1), (1, 1, 3, 5), (5, 7, 1, 1), (16, 16, 4, 4), (17, 33, 5, 9), (33, 17, 132, 68),
          (67, 130, 16, 33), (64, 48, 64, 12), (64, 48, 16, 48), (40, 56, 160, 224), (97, 136, 24, 34),
          (200, 31, 7, 31), (300, 9, 3, 2)]
# for the kernel: tiles (16 x 64 at most) crossed raggedly on both axes; a vertical factor of 30 at
# more than 64 columns, where the tile's rows shrink from 16 (11 outputs) to 4
RAGGED, STEEP = (131, 259, 37, 71), (330, 70, 11, 65)
FILTERS = ("box", "bilinear", "hamming", "bicubic", "lanczos")


def image(kind, shape, seed):
    """A random image, or one of 0 / 255 only: bicubic and lanczos overshoot it into the clip."""
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == "random":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return (rng.integers(0, 2, shape, dtype=np.uint8) * 255).astype(np.uint8)


@pytest.mark.parametrize("kind", ["random", "extremes"])
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
@pytest.mark.parametrize("filter", FILTERS)
def test_reference_equals_pillow_bit_for_bit(filter, shape, C, kind):
    from PIL import Image
    from dgan.resize import resize_pil_ref
    hi, wi, h, w = shape
    a = image(kind, (hi, wi, C), hi * 1000 + wi + C)
    pil = Image.fromarray(a if C == 3 else a[..., 0], "RGB" if C == 3 else "L")
    want = np.asarray(pil.resize((w, h), getattr(Image.Resampling, filter.upper()))).reshape(h, w, C)
    got = resize_pil_ref(a, h, w, filter)
    assert got.dtype == np.uint8 and np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("filter", FILTERS)
def test_int32_equals_int64_and_the_coefficients_keep_their_bounds(filter):
    from dgan.resize import pil_coeffs, resize_pil_ref
    a = image("extremes", (2, 67, 130, 3), 5)
    assert np.array_equal(resize_pil_ref(a, 16, 33, filter, dtype=np.int32), resize_pil_ref(a, 16, 33, filter))
    for n_in, n_out in [(67, 16), (130, 33), (33, 132), (300, 3), (1, 5), (7, 1)]:
        first, count, k = pil_coeffs(n_in, n_out, filter)
        assert first.min() >= 0 and count.min() >= 1 and (first + count).max() <= n_in and count.max() <= k.shape[1]
        assert 255 * int(np.abs(k.astype(np.int64)).sum(1).max()) + (1 << 21) < 2 ** 31   # int32 holds a pass
        assert int(np.abs(k).max()) < 2 ** 23                                             # a 24-bit multiply holds k
        assert np.abs(k.sum(1) - (1 << 22)).max() <= k.shape[1]                           # rounding only


def test_the_tile_shrinks_with_the_factor_and_a_factor_beyond_the_lds_is_refused():
    from dgan import ops, resize as R
    assert R.pil_tile(*STEEP)[:2] == (4, 64) and R.pil_tile(*RAGGED)[:2] == (16, 64)
    assert R.pil_tile(1080, 1920, 270, 480, "lanczos")[:2] == (16, 64) and R.pil_tile(300, 9, 3, 2, C=1)[:2] == (4, 2)
    with pytest.raises(ops.DGError, match="65536 bytes of LDS"):
        ops.resize_pil_tile(100000, 64, 3, 10, 64, 1, 40001)


def test_argument_errors():
    from dgan.resize import pil_coeffs, resize_pil_ref
    a = np.zeros((4, 4, 3), np.uint8)
    assert np.array_equal(resize_pil_ref(a[None], 4, 4), a[None]) and resize_pil_ref(a, 2, 3).shape == (2, 3, 3)
    with pytest.raises(ValueError, match="uint8"):
        resize_pil_ref(a.astype(np.float32), 2, 2)
    with pytest.raises(ValueError, match="uint8"):
        resize_pil_ref(a[0], 2, 2)
    with pytest.raises(ValueError, match="empty"):
        resize_pil_ref(a, 0, 2)
    with pytest.raises(ValueError, match="empty"):
        resize_pil_ref(a[:, :0], 2, 2)
    with pytest.raises(ValueError, match="filter"):
        resize_pil_ref(a, 2, 2, "nearest")
    with pytest.raises(ValueError, match="dtype"):
        resize_pil_ref(a, 2, 2, dtype=np.int16)
    with pytest.raises(ValueError, match="filter"):
        pil_coeffs(4, 2, "cubic")
    with pytest.raises(ValueError, match="at least 1"):
        pil_coeffs(4, 0)
