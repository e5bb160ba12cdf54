"""The JPEG decoder's definition (dgan/jpeg.py jpeg_parse, jpeg_decode_ref) against Pillow's decoder
on the files Pillow writes, bit for bit.  No GPU."""
import io

import numpy as np
import pytest

from test_jpeg import KINDS, image

# (3,4): cw <= 2, replicated chroma; (17,33) / (33,17): dummy luma blocks; (67,130): 45 MCUs
SIZES = [(1, 1), (8, 8), (3, 4), (17, 33), (33, 17), (67, 130)]


def pillow_file(a, mode="RGB", **options):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a, mode).save(buf, format="JPEG", **dict({"subsampling": 2}, **options))
    return buf.getvalue()


def pillow_pixels(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), np.uint8)


def flat_file(quality=50):
    return pillow_file(np.full((128, 256, 3), 77, np.uint8), quality=quality)


def cut_file(data):
    """`data` with the second half of its scan cut off."""
    from dgan.jpeg import jpeg_parse
    first, end = jpeg_parse(data).scan
    return data[:first + (end - first) // 2] + b"\xff\xd9"


def cases(sizes):
    """(id, file) of every kind x quality x optimize at every size, and the flat image."""
    for size in sizes:
        for kind in KINDS:
            for q in (1, 50, 100):
                for opt in (False, True):   # optimised tables reach 14-bit codes
                    yield f"{size[0]}x{size[1]}-{kind}-q{q}-opt{int(opt)}", pillow_file(image(kind, *size), quality=q, optimize=opt)
    yield "flat", flat_file()


@pytest.mark.parametrize("size", SIZES + ["flat"], ids=str)
def test_the_definition_equals_pillow_bit_for_bit(size):
    pytest.importorskip("PIL")
    from dgan.jpeg import jpeg_decode_ref
    for name, data in ([("flat", flat_file())] if size == "flat" else cases([size])):
        if name == "flat" and size != "flat":
            continue
        got, want = jpeg_decode_ref(data), pillow_pixels(data)
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), (name, int((got != want).sum()))


@pytest.mark.parametrize("what, options", [("progressive", {"progressive": True}), ("sampling factors", {"subsampling": 0}),
                                           ("restart", {"restart_marker_blocks": 1}), ("components", {"mode": "L"})])
def test_parse_refuses_what_is_out_of_scope_and_names_it(what, options):
    pytest.importorskip("PIL")
    from dgan.jpeg import JpegUnsupported, jpeg_parse
    a = image("random", 40, 56)
    data = pillow_file(a[..., 0], **options) if options.get("mode") == "L" else pillow_file(a, **options)
    with pytest.raises(JpegUnsupported, match=what):
        jpeg_parse(data)
    assert issubclass(JpegUnsupported, ValueError)


def test_parse_reads_the_encoders_files():
    from dgan.jpeg import HUFFMAN, ZIGZAG, jpeg_decode_ref, jpeg_encode_ref, jpeg_header, jpeg_parse, jpeg_ref, quant_tables
    a = image("random", 33, 17)
    data = jpeg_encode_ref(a, 75)
    info = jpeg_parse(b"\xff\xd8" + b"\xff\xfe\x00\x05abc" + data[2:])   # a COM segment in front
    assert (info.h, info.w, info.components) == (33, 17, ((0, 0, 0), (1, 1, 1), (1, 1, 1)))
    assert all(np.array_equal(info.quant[k], quant_tables(75)[k]) for k in (0, 1))
    assert [info.huffman[k] for k in ((0, 0), (1, 0), (0, 1), (1, 1))] == list(HUFFMAN)
    assert info.scan == (len(jpeg_header(33, 17, 75)) + 7, len(data) + 7 - 2) and len(ZIGZAG) == 64
    assert np.array_equal(jpeg_decode_ref(data), jpeg_ref(a, 75))
    with pytest.raises(TypeError, match="bytes"):
        jpeg_parse(bytearray(data))


def test_a_scan_cut_in_half_raises():
    from dgan.jpeg import jpeg_decode_ref
    with pytest.raises(ValueError, match="scan ends"):
        jpeg_decode_ref(cut_file(pillow_file(image("random", 67, 130), quality=90)))


def test_a_batch_with_more_table_sets_than_the_cache_keeps_points_every_file_at_its_own():
    """70 files with optimised, distinct Huffman tables in one blob: the table cache (64 sets) is
    emptied on the way, and every descriptor must still name the set built from its own file."""
    from dgan import jpeg as J
    files = [pillow_file(image("random", 16, 16, seed=s), quality=30 + s, optimize=True) for s in range(70)]
    infos = [J.jpeg_parse(f) for f in files]
    assert len({J._device_tables(i)[0] for i in infos}) > 64
    J._table_cache.clear()
    blob, _ = J._decode_blob(infos, files)
    words = blob[:70 * J._DESC_WORDS * 4].view(np.uint32).reshape(70, J._DESC_WORDS)
    for i, info in enumerate(infos):
        at = int(words[i, 2])
        want = np.concatenate([J._device_table(info.huffman.get(k)) for k in ((0, 0), (0, 1), (1, 0), (1, 1))])
        assert np.array_equal(blob[at:at + 16 * J._TABLE_WORDS].view(np.uint32), want), i
