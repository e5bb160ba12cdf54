"""The JPEG encoder's definition (dgan/jpeg.py jpeg_encode_ref) against the files Pillow writes,
byte for byte, and the corners of the entropy coder its inputs reach.  No GPU."""
import io

import numpy as np
import pytest

from test_jpeg import KINDS, image

QUALITIES = [1, 10, 50, 90, 100]
# 17x33 / 33x17: padded to 8 but not to 16 to the right / below, so dummy luma blocks
SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (33, 17), (9, 40), (40, 9), (48, 64)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_reference_equals_pillows_file_byte_for_byte(size):
    pytest.importorskip("PIL")
    from PIL import Image
    from dgan.jpeg import jpeg_encode_ref
    for kind in KINDS:
        a = image(kind, *size)
        for q in QUALITIES:
            buf = io.BytesIO()
            Image.fromarray(a, "RGB").save(buf, format="JPEG", quality=q, subsampling=2)
            got = jpeg_encode_ref(a, q)
            assert isinstance(got, bytes) and got == buf.getvalue(), (size, kind, q, len(got), len(buf.getvalue()))


def test_the_inputs_reach_the_corners_of_the_coder():
    """Over the sizes, qualities and kinds above (what the GPU test encodes too): a ZRL code, an
    EOB, a block that ends on coefficient 63 and has none, a stuffed 0xFF, scans that end on a
    partial and on a full byte, DC differences of category >= 8 of both signs, dummy blocks."""
    from dgan.jpeg import jpeg_encode_ref, jpeg_header, scan_coefficients, scan_entries
    hit = dict.fromkeys(["zrl", "eob", "no_eob", "stuffed", "partial", "full", "dc_up", "dc_down", "dummy"], 0)
    for size in SIZES:
        for kind in KINDS:
            a = image(kind, *size)
            for q in QUALITIES:
                coef = scan_coefficients(a, q)
                e = scan_entries(coef)
                scan = jpeg_encode_ref(a, q)[len(jpeg_header(*size, q)):-2]
                dc, cat = e["coef"][..., 0], e["symbol"][..., 0]
                hit["zrl"] += bool((e["zrl"] > 0).any())
                hit["eob"] += bool((e["symbol"][..., 64] == 0).any())
                hit["no_eob"] += bool((e["symbol"][..., 64] < 0).any())
                hit["stuffed"] += b"\xff\x00" in scan
                hit["partial"] += int(e["length"].sum()) % 8 != 0
                hit["full"] += int(e["length"].sum()) % 8 == 0
                hit["dc_up"] += bool(((cat >= 8) & (dc > 0)).any())
                hit["dc_down"] += bool(((cat >= 8) & (dc < 0)).any())
                if size in ((17, 33), (33, 17)):   # the last MCU column / row: block 1 / 2 repeats the DC before it
                    last = coef.reshape(-(-size[0] // 16), -(-size[1] // 16), 6, 64)
                    d = last[:, -1, 1] if size == (17, 33) else last[-1, :, 2]
                    before = last[:, -1, 0] if size == (17, 33) else last[-1, :, 1]
                    hit["dummy"] += bool(not d[..., 1:].any() and np.array_equal(d[..., 0], before[..., 0]))
    assert all(hit.values()), hit
    assert hit["dummy"] == 2 * len(KINDS) * len(QUALITIES), hit


def test_bad_arguments_raise():
    from dgan.jpeg import jpeg_encode_ref, jpeg_header
    a = image("random", 8, 8)
    for q in (0, 101, -1, 50.0, None, True):
        with pytest.raises(ValueError, match="quality"):
            jpeg_encode_ref(a, q)
    for bad in (a.astype(np.float32), a[..., :1], a[None], a[0]):
        with pytest.raises(ValueError, match="uint8"):
            jpeg_encode_ref(bad, 50)
    with pytest.raises(ValueError, match="empty"):
        jpeg_encode_ref(np.zeros((0, 8, 3), np.uint8), 50)
    with pytest.raises(ValueError, match="65535"):
        jpeg_header(8, 65536, 50)
