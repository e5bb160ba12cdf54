"""The PNG encoder's numpy definition (dgan/png.py): its files decode to the input with Pillow and
zlib, every token and code-length path round-trips, and size caps that a broken coder cannot meet.
No GPU."""
import io
import zlib

import numpy as np
import pytest

from test_jpeg import KINDS, image

SIZES = [(1, 1), (1, 7), (3, 2), (17, 33), (64, 171), (128, 256)]   # 64x171: a span and 128 bytes; 128x256: four
RUNS = [1, 2, 3, 4, 5, 259, 260, 261, 262, 600]


def flat(h, w):
    return np.full((h, w, 3), (200, 17, 90), np.uint8)


def frames(size):
    return [(k, image(k, *size)) for k in KINDS] + [("flat", flat(*size))]


def run_streams():
    """The streams of CPU tests 2 and 3, by name (the device test feeds them to the deflate op)."""
    rng = np.random.Generator(np.random.PCG64(7))
    out = {"runs": b"".join(bytes([65 + k % 2]) * n for k, n in enumerate(RUNS + RUNS[::-1])),
           "crossing": b"ab" * 6384 + b"\0" * 40000 + b"c", "empty": b""}
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    assert fib[-1] == 10946 and sum(fib) == 28656
    d = np.concatenate([np.full(c, 3 * k, np.uint8) for k, c in enumerate(fib + [32768 - 28656])])
    out["fibonacci"] = rng.permutation(d).tobytes()
    return out


def idat(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, kinds, payload = 8, [], b""
    while at < len(data):
        n, kind = int.from_bytes(data[at:at + 4], "big"), data[at + 4:at + 8]
        assert zlib.crc32(data[at + 4:at + 8 + n]) == int.from_bytes(data[at + 8 + n:at + 12 + n], "big")
        kinds.append(kind)
        payload += data[at + 8:at + 8 + n] if kind == b"IDAT" else b""
        at += 12 + n
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and set(kinds[1:-1]) == {b"IDAT"}
    return payload


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_file_decodes_to_the_input(size):
    from PIL import Image
    from dgan.png import png_encode_ref, png_filter_ref
    for kind, a in frames(size):
        data = png_encode_ref(a)
        im = Image.open(io.BytesIO(data))
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), a), (size, kind)
        assert zlib.decompress(idat(data)) == png_filter_ref(a), (size, kind)


@pytest.mark.parametrize("name", ["runs", "crossing", "empty", "fibonacci"])
def test_deflate_round_trips(name):
    """runs: remainders 0 to 3 after the literal and the 258 cap; crossing: a run cut at the span
    boundary; fibonacci: an unlimited Huffman code would be about 20 bits deep."""
    from dgan.png import deflate_ref
    d = run_streams()[name]
    assert zlib.decompress(deflate_ref(d)) == d


def test_size_caps():
    """Conditions that keep a broken coder from hiding behind "it decodes".  The random frame's cap
    counts from the filtered stream, the bytes deflate is given: counted from h w 3 no PNG file meets
    it, as the filter bytes, the container and the stored blocks' headers alone exceed it."""
    from PIL import Image
    from dataloader import synthetic_pair
    from dgan.png import SPAN, png_encode_ref, png_filter_ref
    for a in synthetic_pair(1, 512, seed=3):   # noisy, clean
        a = np.clip(np.floor((a[0] * 0.5 + 0.5) * 255.5), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(a, "RGB").save(buf, format="PNG")
        assert len(png_encode_ref(a)) <= 1.02 * len(buf.getvalue())
    assert len(png_encode_ref(flat(512, 512))) < 0.01 * 512 * 512 * 3
    a = image("random", 128, 256)
    raw = len(png_filter_ref(a))
    assert len(png_encode_ref(a)) <= raw + 64 + 32 * -(-raw // SPAN)
