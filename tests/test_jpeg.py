"""The JPEG round trip's definition (dgan/jpeg.py jpeg_ref, quant_tables) against Pillow's codec,
bit for bit, and the 32-bit working type against the 64-bit one.  No GPU."""
import io
import sys

import numpy as np
import pytest

SIZES = [(8, 8), (16, 16), (17, 23), (5, 7), (64, 64), (33, 48), (1, 9), (9, 1), (3, 4), (67, 130), (256, 256)]
QUALITIES = [1, 10, 50, 75, 95, 100]
KINDS = ["random", "gradient", "binary"]
# the zigzag scan: ZIGZAG[k] = the row-major index of the k-th coefficient written to a file
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
          21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
          60, 61, 54, 47, 55, 62, 63]


def image(kind, h, w, seed=0):
    """uint8 [h,w,3]: uniform random, a colour gradient, or 0 / 255 only."""
    rng = np.random.Generator(np.random.PCG64(1000 * h + w + seed))
    if kind == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    g = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(h + w - 2, 1)], axis=-1)
    return g.astype(np.uint8)


def pillow_roundtrip(a, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a, "RGB").save(buf, format="JPEG", quality=quality, subsampling=2)
    buf.seek(0)
    return np.asarray(Image.open(buf).convert("RGB"), np.uint8)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_jpeg_ref_equals_pillow_bit_for_bit(size):
    pytest.importorskip("PIL")
    from dgan.jpeg import jpeg_ref
    for kind in KINDS:
        a = image(kind, *size)
        for q in QUALITIES:
            got, want = jpeg_ref(a, q), pillow_roundtrip(a, q)
            assert got.dtype == np.uint8 and got.shape == want.shape
            assert np.array_equal(got, want), (size, kind, q, int((got != want).sum()))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_32_bit_working_type_equals_the_64_bit_one(size):
    from dgan.jpeg import jpeg_ref
    for kind in KINDS:
        a = image(kind, *size)
        for q in QUALITIES:
            assert np.array_equal(jpeg_ref(a, q, dtype=np.int32), jpeg_ref(a, q, dtype=np.int64)), (size, kind, q)


@pytest.mark.parametrize("quality", [1, 25, 50, 75, 100])
def test_quant_tables_equal_the_tables_pillow_writes(quality):
    pytest.importorskip("PIL")
    from PIL import Image
    from dgan.jpeg import quant_tables
    buf = io.BytesIO()
    Image.fromarray(image("random", 16, 16), "RGB").save(buf, format="JPEG", quality=quality, subsampling=2)
    buf.seek(0)
    written = Image.open(buf).quantization
    # a file holds its tables in zigzag order; Pillow hands them out as stored before 8.3 and
    # row-major from 8.3 on
    import PIL
    stored = tuple(int(v) for v in PIL.__version__.split(".")[:2]) < (8, 3)
    got = quant_tables(quality)
    assert got.dtype == np.uint8 and got.shape == (2, 64)
    for k in (0, 1):
        natural = np.asarray(written[k], np.int64)
        if stored:
            natural = np.zeros(64, np.int64)
            natural[ZIGZAG] = np.asarray(written[k])
        assert np.array_equal(got[k], natural), (quality, k)


def test_a_single_image_equals_the_batch_of_one_and_batches_are_independent():
    from dgan.jpeg import jpeg_ref
    a, b = image("random", 17, 23), image("gradient", 17, 23)
    one = jpeg_ref(a, 50)
    assert one.shape == a.shape and np.array_equal(one, jpeg_ref(a[None], 50)[0])
    both = jpeg_ref(np.stack([a, b]), 50)
    assert np.array_equal(both[0], one) and np.array_equal(both[1], jpeg_ref(b, 50))


def test_bad_arguments_raise():
    from dgan.jpeg import jpeg_ref, quant_tables
    a = image("random", 8, 8)
    for q in (0, 101, -1, 50.0, None, True):
        with pytest.raises(ValueError, match="quality"):
            jpeg_ref(a, q)
        with pytest.raises(ValueError, match="quality"):
            quant_tables(q)
    with pytest.raises(ValueError, match="uint8"):
        jpeg_ref(a.astype(np.float32), 50)
    with pytest.raises(ValueError, match="uint8"):
        jpeg_ref(a[..., :1], 50)
    with pytest.raises(ValueError, match="uint8"):
        jpeg_ref(a[0], 50)
    with pytest.raises(ValueError, match="empty"):
        jpeg_ref(np.zeros((0, 8, 3), np.uint8), 50)
    with pytest.raises(ValueError, match="dtype"):
        jpeg_ref(a, 50, dtype=np.int16)


def test_the_definition_needs_neither_torch_nor_the_library():
    import subprocess
    code = ("import sys; import dgan.jpeg as J; import numpy as np; J.jpeg_ref(np.zeros((8, 8, 3), np.uint8), 50); "
            "assert 'torch' not in sys.modules and 'dgan._lib' not in sys.modules")
    import dgan
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(dgan.__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root)
    assert r.returncode == 0, r.stderr
