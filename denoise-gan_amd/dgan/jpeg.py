"""The JPEG round trip of an RGB image, quality Q, 4:2:0 subsampling, without the codec: what
`PIL.Image.save(format="JPEG", quality=Q, subsampling=2)` followed by `Image.open().convert("RGB")`
returns (libjpeg's defaults: the "islow" DCTs, "fancy" chroma upsampling), a host reference and the
device op (csrc/jpeg.hip).

Entropy coding is lossless, so a round trip is what is left without it, and every remaining step is
integer arithmetic that libjpeg defines exactly.  With >> an arithmetic shift, FIX(x) =
int(x * 65536 + 0.5) and DESCALE(x, n) = (x + (1 << (n-1))) >> n:

    tables     Annex K luminance / chrominance, entry = clamp((std * s + 50) // 100, 1, 255) with
               s = 5000 // Q below 50, else 200 - 2 Q
    colour     Y  = ( FIX(.299) R + FIX(.587) G + FIX(.114) B + 32768) >> 16
               Cb = (-FIX(.16874) R - FIX(.33126) G + FIX(.5) B + (128 << 16) + 32767) >> 16
               Cr = ( FIX(.5) R - FIX(.41869) G - FIX(.08131) B + (128 << 16) + 32767) >> 16
    luma       edge-replicated to multiples of 8
    chroma     ch = ceil(h/2), cw = ceil(w/2): the full-resolution plane edge-replicated to 2 ch rows
               and 16 ceil(cw/8) columns, then (a + b + c + d + bias) >> 2 per 2x2 with bias 1 on even
               and 2 on odd output columns, then the downsampled rows replicated to a multiple of 8
    per block  - 128; jfdctint (CONST_BITS 13, PASS1_BITS 2: rows, then columns, output scaled by 8);
               q = sign(c) ((|c| + 4 t) // (8 t)); c' = q t; jidctint (columns descaled by 11, rows
               by 18); the range limit on x & 1023: < 128 -> x + 128, < 512 -> 255, < 896 -> 0,
               else x - 896
    decode     Y cropped to h x w, chroma to ch x cw; cw > 2: the h2v2 triangle filter, vertically
               cs = 3 this + neighbour (the row above for even output rows, below for odd ones,
               clamped), horizontally (3 cs + cs_left + 8) >> 4 on even and (3 cs + cs_right + 7) >> 4
               on odd columns (clamped); cw <= 2: every chroma pixel replicated 2x2
               R = Y + ((FIX(1.402) Cr' + 32768) >> 16), B = Y + ((FIX(1.772) Cb' + 32768) >> 16),
               G = Y + ((-FIX(.34414) Cb' + 32768 - FIX(.71414) Cr') >> 16), C' = C - 128, clamped

Everything fits 32-bit integers at 8-bit samples (the device kernels use them; `jpeg_ref` takes the
working type as an argument and tests/test_jpeg.py holds the two equal), so the device output
equals `jpeg_ref` bit for bit, and `jpeg_ref` equals Pillow.

The encoder finishes the codec: `jpeg_encode_ref` Huffman-codes the same quantised levels into the
baseline file Pillow writes (header, scan order, dummy blocks and coding rules: DESIGN.md section JPEG
encoder), and `jpeg_encode` is the device op (csrc/jpeg_enc.hip), equal to it byte for byte.

The decoder reads such files back: `jpeg_parse` reads a header, `jpeg_decode_ref` is the definition
(a sequential Huffman decode, then the round trip's back half; equal to Pillow's decoder), and
`jpeg_decode` is the device op (csrc/jpeg_dec.hip), equal to it bit for bit (DESIGN.md section JPEG
decoder).

`quant_tables`, `jpeg_ref`, `jpeg_encode_ref`, `jpeg_parse` and `jpeg_decode_ref` are pure numpy and
import neither torch nor the library.
"""
import numpy as np

# Annex K, row-major (natural) order
_STD_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_STD_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


def _check_quality(quality, what):
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise ValueError(f"{what}: quality must be an integer in 1..100, got {quality!r}")
    return int(quality)


def quant_tables(quality):
    """uint8 [2,64]: the luminance and the chrominance table of `quality`, row-major."""
    q = _check_quality(quality, "quant_tables")
    s = 5000 // q if q < 50 else 200 - 2 * q
    std = np.array([_STD_LUMA, _STD_CHROMA], np.int64)
    return np.clip((std * s + 50) // 100, 1, 255).astype(np.uint8)


def _fix(x):
    return int(x * 65536 + 0.5)


# jfdctint / jidctint: FIX(x) at CONST_BITS 13
_C0_298, _C0_390, _C0_541, _C0_765, _C0_899, _C1_175 = 2446, 3196, 4433, 6270, 7373, 9633
_C1_501, _C1_847, _C1_961, _C2_053, _C2_562, _C3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _odd_part(t0, t1, t2, t3):
    """The rotations shared by both DCTs' odd halves: (t0, t1, t2, t3) -> the four sums."""
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * _C1_175
    t0, t1, t2, t3 = t0 * _C0_298, t1 * _C2_053, t2 * _C3_072, t3 * _C1_501
    z1, z2, z3, z4 = z1 * -_C0_899, z2 * -_C2_562, z3 * -_C1_961 + z5, z4 * -_C0_390 + z5
    return t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4


def _fdct_1d(d, first):
    """One jfdctint pass over d[0..7] (arrays): the row pass (first) or the column pass."""
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    z1 = (t12 + t13) * _C0_541
    o0 = (t10 + t11) * 4 if first else _descale(t10 + t11, 2)
    o4 = (t10 - t11) * 4 if first else _descale(t10 - t11, 2)
    o2 = _descale(z1 + t13 * _C0_765, n)
    o6 = _descale(z1 - t12 * _C1_847, n)
    a4, a5, a6, a7 = _odd_part(t4, t5, t6, t7)
    return [o0, _descale(a7, n), o2, _descale(a6, n), o4, _descale(a5, n), o6, _descale(a4, n)]


def _idct_1d(c, first):
    """One jidctint pass over c[0..7]: the column pass (first, descaled by 11) or the row pass (18)."""
    z1 = (c[2] + c[6]) * _C0_541
    t2, t3 = z1 - c[6] * _C1_847, z1 + c[2] * _C0_765
    t0, t1 = (c[0] + c[4]) * 8192, (c[0] - c[4]) * 8192
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = _odd_part(c[7], c[5], c[3], c[1])
    n = 11 if first else 18
    return [_descale(t10 + a3, n), _descale(t11 + a2, n), _descale(t12 + a1, n), _descale(t13 + a0, n),
            _descale(t13 - a0, n), _descale(t12 - a1, n), _descale(t11 - a2, n), _descale(t10 - a3, n)]


def _along(f, x, axis, first):
    return np.stack(f([np.take(x, k, axis=axis) for k in range(8)], first), axis=axis)


def _quantise(plane, table):
    """A plane [n,H,W] (H, W multiples of 8) -> its quantised levels [n,by,bx,row,col]."""
    n, H, W = plane.shape
    b = (plane - 128).reshape(n, H // 8, 8, W // 8, 8).transpose(0, 1, 3, 2, 4)
    c = _along(_fdct_1d, _along(_fdct_1d, b, 4, True), 3, False)
    t = table.astype(plane.dtype).reshape(8, 8)
    return np.sign(c) * ((np.abs(c) + 4 * t) // (8 * t))


def _inverse(c):
    """Dequantised coefficients [n,by,bx,row,col] -> the decoded samples [n,8 by,8 bx]: jidctint and
    the range limit."""
    n, by, bx = c.shape[:3]
    x = _along(_idct_1d, _along(_idct_1d, c, 3, True), 4, False) & 1023
    x = np.where(x < 128, x + 128, np.where(x < 512, 255, np.where(x < 896, 0, x - 896)))
    return x.transpose(0, 1, 3, 2, 4).reshape(n, by * 8, bx * 8)


def _codec(plane, table):
    """A plane [n,H,W] (H, W multiples of 8) through the block pipeline with the table [64]."""
    return _inverse(_quantise(plane, table) * table.astype(plane.dtype).reshape(8, 8))


def _edge(p, H, W):
    return np.pad(p, ((0, 0), (0, H - p.shape[1]), (0, W - p.shape[2])), mode="edge")


def _up8(v):
    return -(-v // 8) * 8


def _upsample(c, fancy):
    """Decoded chroma [n,ch,cw] -> [n,2ch,2cw]."""
    n, ch, cw = c.shape
    if not fancy:
        return np.repeat(np.repeat(c, 2, axis=1), 2, axis=2)
    r = np.arange(2 * ch)
    near = np.clip(r // 2 + np.where(r % 2 == 0, -1, 1), 0, ch - 1)
    cs = 3 * c[:, r // 2] + c[:, near]
    j = np.arange(cw)
    out = np.empty((n, 2 * ch, 2 * cw), c.dtype)
    out[:, :, 0::2] = (3 * cs + cs[:, :, np.maximum(j - 1, 0)] + 8) >> 4
    out[:, :, 1::2] = (3 * cs + cs[:, :, np.minimum(j + 1, cw - 1)] + 7) >> 4
    return out


def _planes(a, dtype):
    """uint8 [n,h,w,3] -> what the block pipeline codes: Y [n,up8(h),up8(w)] and the downsampled
    Cb and Cr [n,up8(ch),up8(cw)], edge-replicated (module docstring: colour, luma, chroma)."""
    n, h, w = a.shape[:3]
    ch, cw = -(-h // 2), -(-w // 2)
    R, G, B = (a[..., k].astype(dtype) for k in range(3))
    Y = (_fix(.299) * R + _fix(.587) * G + _fix(.114) * B + 32768) >> 16
    Cb = (-_fix(.16874) * R - _fix(.33126) * G + _fix(.5) * B + (128 << 16) + 32767) >> 16
    Cr = (_fix(.5) * R - _fix(.41869) * G - _fix(.08131) * B + (128 << 16) + 32767) >> 16
    bias = np.where(np.arange(_up8(cw)) % 2 == 0, 1, 2).astype(dtype)
    chroma = []
    for C in (Cb, Cr):
        C = _edge(C, 2 * ch, 2 * _up8(cw))
        C = (C[:, 0::2, 0::2] + C[:, 0::2, 1::2] + C[:, 1::2, 0::2] + C[:, 1::2, 1::2] + bias) >> 2
        chroma.append(_edge(C, _up8(ch), _up8(cw)))
    return _edge(Y, _up8(h), _up8(w)), chroma[0], chroma[1]


def jpeg_ref(img_u8, quality, dtype=np.int64):
    """The definition on the host: uint8 [n,h,w,3] or [h,w,3] -> the same shape and dtype (module
    docstring).  dtype: the working integer type, np.int64 or np.int32."""
    a = np.asarray(img_u8)
    if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.shape[-1] != 3:
        raise ValueError(f"jpeg_ref: expected uint8 [n,h,w,3] or [h,w,3], got {a.dtype} {a.shape}")
    if min(a.shape[-3:-1]) < 1:
        raise ValueError(f"jpeg_ref: empty image: {a.shape}")
    if np.dtype(dtype) not in (np.dtype(np.int64), np.dtype(np.int32)):
        raise ValueError(f"jpeg_ref: dtype must be np.int64 or np.int32, got {dtype!r}")
    tables = quant_tables(_check_quality(quality, "jpeg_ref"))
    single = a.ndim == 3
    out = _roundtrip(a[None] if single else a, tables, dtype)
    return out[0] if single else out


def _roundtrip(a, tables, dtype):
    """uint8 [n,h,w,3] through the round trip with the uint8 [2,64] tables (luminance, chrominance),
    in the working type `dtype`: `jpeg_ref` with the tables of its quality, and dgan.filters.dejpeg_ref
    with any."""
    h, w = a.shape[1:3]
    Y, Cb, Cr = _planes(a, dtype)
    return _pixels(_codec(Y, tables[0]), _codec(Cb, tables[1]), _codec(Cr, tables[1]), h, w)


def _pixels(Y, Cb, Cr, h, w):
    """The decoded planes [n,H,W] and [n,Hc,Wc] -> uint8 [n,h,w,3] (module docstring: decode)."""
    ch, cw = -(-h // 2), -(-w // 2)
    Y = Y[:, :h, :w]
    Cb, Cr = (_upsample(C[:, :ch, :cw], cw > 2)[:, :h, :w] - 128 for C in (Cb, Cr))
    out = np.stack([Y + ((_fix(1.402) * Cr + 32768) >> 16),
                    Y + ((-_fix(.34414) * Cb + 32768 - _fix(.71414) * Cr) >> 16),
                    Y + ((_fix(1.772) * Cb + 32768) >> 16)], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------
# the baseline encoder: header, scan order, Huffman coding (module docstring of csrc/jpeg_enc.hip)
# ---------------------------------------------------------------------------
# ZIGZAG[k] = the row-major index of the k-th coefficient of a block in a file
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
          21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
          60, 61, 54, 47, 55, 62, 63)
# Annex K.3 - K.6 as (codes per length 1..16, symbols in code order): DC0, AC0, DC1, AC1
_AC_SYMBOLS = (0x00, 0xf0) + tuple(16 * r + s for r in range(16) for s in range(1, 11))   # EOB, ZRL, (run, size)
HUFFMAN = (
    ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d),
     (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
      0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
      0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
      0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
      0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
      0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
      0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
      0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)),
    ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77),
     (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
      0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
      0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
      0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
      0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
      0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
      0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
      0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
      0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)))
assert all(sum(b) == len(v) and sorted(v) == sorted(set(v)) for b, v in HUFFMAN)
assert all(sorted(HUFFMAN[k][1]) == sorted(_AC_SYMBOLS) for k in (1, 3))


def huffman_codes(k):
    """int64 [256]: HUFFMAN[k]'s code of every symbol packed (length << 16) | code, 0 where the
    table has none (Annex C: codes count up within a length, doubled at every longer one)."""
    bits, vals = HUFFMAN[k]
    out, code, i = np.zeros(256, np.int64), 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[i]] = (length << 16) | code
            code, i = code + 1, i + 1
        code <<= 1
    return out


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def jpeg_header(h, w, quality):
    """The bytes of a baseline 4:2:0 file of an h x w image from SOI to the end of SOS, as libjpeg
    writes them by default: JFIF 1.01 without density, two 8-bit DQT, SOF0, four DHT, SOS."""
    if not (1 <= int(h) <= 65535 and 1 <= int(w) <= 65535):
        raise ValueError(f"jpeg_header: a JPEG file holds 1..65535 rows and columns, got {h}x{w}")
    tables = quant_tables(_check_quality(quality, "jpeg_header"))
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    for k in (0, 1):
        out += _segment(0xDB, bytes([k]) + bytes(tables[k][list(ZIGZAG)]))
    out += _segment(0xC0, bytes([8]) + int(h).to_bytes(2, "big") + int(w).to_bytes(2, "big") +
                    bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for k, ident in enumerate((0x00, 0x10, 0x01, 0x11)):
        out += _segment(0xC4, bytes([ident]) + bytes(HUFFMAN[k][0]) + bytes(HUFFMAN[k][1]))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0]))


def scan_coefficients(img_u8, quality):
    """One uint8 [h,w,3] image -> int64 [mcu,6,64]: the quantised coefficients of the scan, MCUs
    row-major over ceil(h/16) x ceil(w/16), blocks Y(0,0) Y(0,1) Y(1,0) Y(1,1) Cb Cr, each in zigzag
    order.  A luma block outside the plane of multiples of 8 is libjpeg's dummy block: no AC, the
    DC of the block before it in its MCU."""
    a = np.asarray(img_u8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[-1] != 3:
        raise ValueError(f"scan_coefficients: expected uint8 [h,w,3], got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f"scan_coefficients: a JPEG file holds 1..65535 rows and columns, got {h}x{w}")
    tables = quant_tables(_check_quality(quality, "scan_coefficients"))
    Y, Cb, Cr = _planes(a[None], np.int64)
    zz = list(ZIGZAG)
    qy = _quantise(Y, tables[0])[0].reshape(Y.shape[1] // 8, Y.shape[2] // 8, 64)[..., zz]
    my, mx = -(-h // 16), -(-w // 16)
    out = np.zeros((my, mx, 6, 64), np.int64)
    for k, C in enumerate((Cb, Cr)):
        out[:, :, 4 + k] = _quantise(C, tables[1])[0].reshape(my, mx, 64)[..., zz]
    for i in range(4):
        sub = qy[i // 2::2, i % 2::2]
        out[:sub.shape[0], :sub.shape[1], i] = sub
        if i:   # the blocks this left empty, below or right of the plane: dummies
            real = np.zeros((my, mx), bool)
            real[:sub.shape[0], :sub.shape[1]] = True
            out[..., i, 0] = np.where(real, out[..., i, 0], out[..., i - 1, 0])
    return out.reshape(my * mx, 6, 64)


def _bit_length(a):
    s = np.zeros(a.shape, np.int64)
    for k in range(16):
        s += (a >> k) > 0
    return s


def scan_entries(coef):
    """scan_coefficients' [mcu,6,64] -> what every coefficient puts into the bit stream, a dict of
    int64 arrays.  "coef" [mcu,6,64]: the coefficients, DC as the difference to the block before of
    its component.  [mcu,6,65] each, entry 64 the block's EOB: "symbol" the (run & 15, size) byte, the
    size category at entry 0, -1 where nothing is coded; "zrl" the ZRL codes in front; "length"
    the bits (0: nothing) and "value" those bits, the first highest: ZRL codes, Huffman code,
    magnitude."""
    v = np.array(coef, np.int64)
    # DC: the difference to the block before of the same component, 0 before the first
    v[:, :4, 0] = np.diff(v[:, :4, 0].reshape(-1), prepend=0).reshape(-1, 4)
    v[:, 4:, 0] = np.diff(v[:, 4:, 0], axis=0, prepend=0)
    size = _bit_length(np.abs(v))
    mag = np.where(v < 0, v + (1 << size) - 1, v)
    k = np.arange(64)
    coded = v != 0
    coded[..., 0] = True
    last = np.maximum.accumulate(np.where(coded, k, 0), axis=-1)
    run = k - 1 - np.concatenate([np.zeros_like(last[..., :1]), last[..., :-1]], axis=-1)
    sym = np.where(coded, ((run & 15) << 4) | size, -1)
    sym[..., 0] = size[..., 0]
    sym = np.concatenate([sym, np.where(v[..., 63:] == 0, 0, -1)], axis=-1)
    val, length, zrls = (np.zeros(sym.shape, np.int64) for _ in range(3))
    for blocks, kdc, kac in ((slice(0, 4), 0, 1), (slice(4, 6), 2, 3)):
        codes = np.stack([huffman_codes(kdc), huffman_codes(kac)])
        which = np.ones(65, np.int64)
        which[0] = 0
        s = sym[:, blocks]
        c = np.where(s >= 0, codes[which, np.maximum(s, 0)], 0)
        assert np.all((c > 0) == (s >= 0)), "a symbol without a code"
        zrl = np.zeros(s.shape, np.int64)
        zrl[..., 1:64] = np.where(coded[:, blocks, 1:], run[:, blocks, 1:] >> 4, 0)
        zc, zl = int(codes[1, 0xF0]) & 0xFFFF, int(codes[1, 0xF0]) >> 16
        head = np.zeros(s.shape, np.int64)
        for r in range(3):
            head = np.where(zrl > r, (head << zl) | zc, head)
        sz = np.concatenate([size[:, blocks], np.zeros_like(size[:, blocks, :1])], axis=-1) * (s >= 0)
        mg = np.concatenate([mag[:, blocks], np.zeros_like(mag[:, blocks, :1])], axis=-1) * (s >= 0)
        val[:, blocks] = (((head << (c >> 16)) | (c & 0xFFFF)) << sz) | mg
        length[:, blocks] = zrl * zl + (c >> 16) + sz
        zrls[:, blocks] = zrl
    return {"coef": v, "symbol": sym, "zrl": zrls, "value": val, "length": length}


def jpeg_encode_ref(img_u8, quality):
    """The encoder's definition on the host: one uint8 [h,w,3] image -> the bytes of the baseline
    JPEG file Pillow writes for `quality=quality, subsampling=2` with its defaults (Annex K Huffman
    tables, no optimisation, no progressive mode, no restart markers)."""
    quality = _check_quality(quality, "jpeg_encode_ref")
    a = np.asarray(img_u8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[-1] != 3:
        raise ValueError(f"jpeg_encode_ref: expected uint8 [h,w,3], got {a.dtype} {a.shape}")
    if min(a.shape[:2]) < 1:
        raise ValueError(f"jpeg_encode_ref: empty image: {a.shape}")
    header = jpeg_header(a.shape[0], a.shape[1], quality)
    e = scan_entries(scan_coefficients(a, quality))
    val, length = e["value"].reshape(-1), e["length"].reshape(-1)
    val, length = val[length > 0], length[length > 0]
    owner = np.repeat(np.arange(length.size), length)
    j = np.arange(owner.size) - np.repeat(np.cumsum(length) - length, length)   # 0: an entry's first bit
    bits = ((val[owner] >> (length[owner] - 1 - j)) & 1).astype(np.uint8)
    bits = np.concatenate([bits, np.ones(-bits.size % 8, np.uint8)])
    return header + np.packbits(bits).tobytes().replace(b"\xff", b"\xff\x00") + b"\xff\xd9"


# ---------------------------------------------------------------------------
# the baseline decoder: header parser, the definition, the device tables (csrc/jpeg_dec.hip)
# ---------------------------------------------------------------------------
class JpegUnsupported(ValueError):
    """A file outside what the decoder reads: baseline, 8 bits, 4:2:0 in one interleaved scan."""


class JpegInfo:
    """What `jpeg_parse` reads from a header.  h, w; quant {id: uint8 [64], natural order};
    components ((quant, dc, ac) table ids of Y, Cb, Cr); huffman {(class, id): (bits[16], values)},
    class 0 DC and 1 AC; scan (first, end) the byte range of the entropy-coded data."""
    __slots__ = ("h", "w", "quant", "components", "huffman", "scan")

    def __init__(self, h, w, quant, components, huffman, scan):
        self.h, self.w, self.quant, self.components, self.huffman, self.scan = h, w, quant, components, huffman, scan


def _huffman_codes_ok(bits):
    code = 0
    for length in range(1, 17):
        code = (code + bits[length - 1]) << 1
        if code > (2 << length):
            return False
    return True


def jpeg_parse(data):
    """The header of a JPEG file (`bytes`) -> JpegInfo.  Reads the marker segments up to SOS and
    finds the scan's end with `bytes.rfind`; APPn and COM segments are skipped.  JpegUnsupported,
    with the reason, for a file that is not SOF0 at 8 bits with three components sampled 2x2, 1x1,
    1x1 in one interleaved scan, Huffman table ids 0 / 1, no restart interval, no Adobe segment and
    component ids other than R, G, B."""
    if not isinstance(data, bytes):
        raise TypeError(f"jpeg_parse: expected bytes, got {type(data).__name__}")
    if data[:2] != b"\xff\xd8":
        raise JpegUnsupported("not a JPEG file (no SOI marker)")
    quant, huffman, frame, at = {}, {}, None, 2
    while True:
        if at + 4 > len(data) or data[at] != 0xFF:
            raise JpegUnsupported(f"no marker at byte {at}")
        marker = data[at + 1]
        if marker == 0xFF:   # a fill byte
            at += 1
            continue
        size = int.from_bytes(data[at + 2:at + 4], "big")
        seg = data[at + 4:at + 2 + size]
        if size < 2 or len(seg) != size - 2:
            raise JpegUnsupported(f"segment {marker:#x} at byte {at} is cut off")
        at += 2 + size
        if marker == 0xDB:
            while seg:
                if seg[0] >> 4 or len(seg) < 65:
                    raise JpegUnsupported("a quantisation table of 16 bits")
                natural = np.zeros(64, np.uint8)
                natural[list(ZIGZAG)] = np.frombuffer(seg[1:65], np.uint8)
                quant[seg[0] & 15] = natural
                seg = seg[65:]
        elif marker == 0xC4:
            while seg:
                cls, ident, bits = seg[0] >> 4, seg[0] & 15, tuple(seg[1:17])
                count = sum(bits)
                if cls > 1 or ident > 1 or len(seg) < 17 + count or count > 256 or not _huffman_codes_ok(bits):
                    raise JpegUnsupported(f"Huffman table class {cls} id {ident}: ids 0 and 1 of well-formed tables only")
                huffman[(cls, ident)] = (bits, tuple(seg[17:17 + count]))
                seg = seg[17 + count:]
        elif marker == 0xC0:
            if len(seg) < 6 or seg[0] != 8:
                raise JpegUnsupported(f"sample precision {seg[0] if seg else None}, not 8 bits")
            h, w, nf = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big"), seg[5]
            comps = [tuple(seg[6 + 3 * k:9 + 3 * k]) for k in range(nf)]
            if nf != 3 or len(seg) < 15:
                raise JpegUnsupported(f"{nf} components, not 3")
            if [c[1] for c in comps] != [0x22, 0x11, 0x11]:
                raise JpegUnsupported("sampling factors " + " ".join(f"{c[1] >> 4}x{c[1] & 15}" for c in comps) +
                                      ", not 2x2 1x1 1x1 (4:2:0)")
            if bytes(c[0] for c in comps) == b"RGB":
                raise JpegUnsupported("component ids R, G, B: an RGB file, not YCbCr")
            if h < 1 or w < 1:
                raise JpegUnsupported(f"image size {h}x{w}")
            frame = (h, w, comps)
        elif 0xC1 <= marker <= 0xCF and marker != 0xC8:
            raise JpegUnsupported(f"frame type SOF{marker - 0xC0}" + (" (progressive)" if marker == 0xC2 else "") +
                                  ", not baseline SOF0")
        elif marker == 0xDD:
            if int.from_bytes(seg[:2], "big"):
                raise JpegUnsupported("restart intervals (DRI)")
        elif marker == 0xEE and seg[:5] == b"Adobe":
            raise JpegUnsupported("an Adobe APP14 segment")
        elif marker == 0xDA:
            break
    if frame is None:
        raise JpegUnsupported("SOS before SOF0")
    h, w, comps = frame
    if len(seg) != 10 or seg[0] != 3 or [seg[1 + 2 * k] for k in range(3)] != [c[0] for c in comps]:
        raise JpegUnsupported("the scan does not interleave the three components")
    if tuple(seg[7:10]) != (0, 63, 0):
        raise JpegUnsupported(f"scan parameters Ss {seg[7]} Se {seg[8]} Ah/Al {seg[9]:#x}, not 0 63 0")
    components = tuple((comps[k][2], seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15) for k in range(3))
    for q, dc, ac in components:
        if q not in quant or (0, dc) not in huffman or (1, ac) not in huffman:
            raise JpegUnsupported(f"a component names a table the file does not define: quant {q}, DC {dc}, AC {ac}")
    end = data.rfind(b"\xff\xd9")
    if end < at:
        raise JpegUnsupported("no EOI marker after the scan")
    return JpegInfo(h, w, quant, components, huffman, (at, end))


def _huffman_lookup(bits, values):
    """A table as (bits[16], values) -> int64 [65536]: (length << 8) | symbol of the code a 16-bit
    window starts with, 0 where it starts with none."""
    lut, code, i = np.zeros(65536, np.int64), 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            lut[code << (16 - length):(code + 1) << (16 - length)] = (length << 8) | values[i]
            code, i = code + 1, i + 1
        code <<= 1
    return lut


def scan_levels(info, data):
    """The entropy-coded scan of `data` (info = jpeg_parse(data)) -> int64 [mcu,6,64]: the
    quantised levels in zigzag order, DC differences summed per component, by a plain sequential
    Huffman decode.  0x00 after 0xFF is stuffing; bits after the last block are ignored.
    ValueError when the bits run out first or start no code."""
    scan = data[info.scan[0]:info.scan[1]].replace(b"\xff\x00", b"\xff")
    total = 8 * len(scan)
    scan += bytes(8)
    luts = {k: _huffman_lookup(*t).tolist() for k, t in info.huffman.items()}
    mcus = -(-info.h // 16) * -(-info.w // 16)
    out = np.zeros((mcus, 6, 64), np.int64)
    p, pred = 0, [0, 0, 0]
    for m in range(mcus):
        for b in range(6):
            comp = max(b - 3, 0)
            dc, ac = luts[(0, info.components[comp][1])], luts[(1, info.components[comp][2])]
            k = 0
            while k < 64:
                window = (int.from_bytes(scan[p >> 3:(p >> 3) + 5], "big") >> (8 - (p & 7))) & 0xFFFFFFFF
                e = (ac if k else dc)[window >> 16]
                length, run, size = e >> 8, (e >> 4) & 15, e & 15
                if not e:
                    raise ValueError(f"jpeg_decode_ref: no Huffman code at bit {p} of the scan (block {6 * m + b})")
                if p + length + size > total:
                    raise ValueError(f"jpeg_decode_ref: the scan ends in block {6 * m + b} of {6 * mcus}")
                v = (window >> (32 - length - size)) & ((1 << size) - 1) if size else 0
                if size and v < (1 << (size - 1)):
                    v -= (1 << size) - 1
                p += length + size
                if k == 0:
                    pred[comp] += v
                    out[m, b, 0] = pred[comp]
                    k = 1
                elif size == 0:
                    k = k + 16 if run == 15 else 64
                else:
                    k += run
                    if k < 64:
                        out[m, b, k] = v
                    k += 1
    return out


def jpeg_decode_ref(data):
    """The decoder's definition on the host: the bytes of a baseline 4:2:0 JPEG file (what
    `jpeg_parse` accepts) -> uint8 [h,w,3], what Pillow's `Image.open().convert("RGB")` returns: the
    sequential Huffman decode of `scan_levels`, then the back half of `jpeg_ref` with every
    component's own quantisation table."""
    info = jpeg_parse(data)
    h, w = info.h, info.w
    my, mx = -(-h // 16), -(-w // 16)
    lv = scan_levels(info, data)
    c = np.zeros_like(lv)
    c[..., list(ZIGZAG)] = lv
    c = c.reshape(my, mx, 6, 8, 8)
    q = [info.quant[info.components[k][0]].astype(np.int64).reshape(8, 8) for k in range(3)]
    luma = c[:, :, :4].reshape(my, mx, 2, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(1, 2 * my, 2 * mx, 8, 8)
    planes = [_inverse(luma * q[0])] + [_inverse(c[None, :, :, 3 + k] * q[k]) for k in (1, 2)]
    return _pixels(planes[0], planes[1], planes[2], h, w)[0]


# the decoder's device tables (csrc/jpeg_dec.hip): sizes in bytes and 32-bit words
DECODE_SUBSEQUENCE = 128   # bytes of the unstuffed scan a lane decodes
DECODE_LANES = 256         # lanes (subsequences) of a workgroup
_LUT_BITS = 9
_TABLE_WORDS = 256 + 18 + 18 + 64
_DESC_WORDS = 4 + 48
_table_cache = {}


def _device_table(table):
    """(bits[16], values) or None -> uint32 [_TABLE_WORDS]: a first-level table of 2^9 uint16
    entries (length << 8) | symbol (0: a longer code), then libjpeg's slow path: maxcode[18] (-1: no
    code of that length), valptr - mincode [18], the 256 symbols."""
    out = np.zeros(_TABLE_WORDS, np.uint32)
    lut, maxcode, valoff, vals = np.zeros(512, np.uint16), np.full(18, -1, np.int32), np.zeros(18, np.int32), \
        np.zeros(256, np.uint8)
    if table is not None:
        bits, values = table
        vals[:len(values)] = values
        code, i = 0, 0
        for length in range(1, 17):
            valoff[length] = i - code
            for _ in range(bits[length - 1]):
                if length <= _LUT_BITS:
                    lut[code << (_LUT_BITS - length):(code + 1) << (_LUT_BITS - length)] = (length << 8) | values[i]
                code, i = code + 1, i + 1
            if bits[length - 1]:
                maxcode[length] = code - 1
            code <<= 1
    out[:256], out[256:274], out[274:292], out[292:] = lut.view(np.uint32), maxcode.view(np.uint32), \
        valoff.view(np.uint32), vals.view(np.uint32)
    return out


def _device_tables(info):
    """-> (key, the four tables DC0, DC1, AC0, AC1 of a file as one uint32 array), cached on their
    contents, the key (nearly every file carries Annex K).  The cache may drop any entry at a later
    call: a caller keeps the array it got."""
    key = tuple(info.huffman.get(k) for k in ((0, 0), (0, 1), (1, 0), (1, 1)))
    if key not in _table_cache:
        if len(_table_cache) >= 64:
            _table_cache.clear()
        _table_cache[key] = np.concatenate([_device_table(t) for t in key])
    return key, _table_cache[key]


def _decode_blob(infos, files):
    """What one upload carries (csrc/jpeg_dec.hip "the blob"): per image a descriptor of
    _DESC_WORDS words (scan offset, scan bytes, offset of its tables, the components' table
    selectors, the three quantisation tables), the distinct table sets, the scans, each at a
    multiple of 16 bytes and followed by at least 16 zero bytes.  -> (uint8 array, longest scan)."""
    n = len(files)
    sets, order, which = {}, [], []   # distinct table sets by content, their arrays, every file's set
    for info in infos:
        key, t = _device_tables(info)
        if key not in sets:
            sets[key] = len(order)
            order.append(t)
        which.append(sets[key])
    at = n * _DESC_WORDS * 4 + len(order) * 4 * _TABLE_WORDS * 4
    starts = []
    for info in infos:
        starts.append(at)
        at += -(-(info.scan[1] - info.scan[0]) // 16) * 16 + 16
    blob = np.zeros(at, np.uint8)
    words = blob[:n * _DESC_WORDS * 4].view(np.uint32).reshape(n, _DESC_WORDS)
    for i, (info, data) in enumerate(zip(infos, files)):
        first, end = info.scan
        sel = sum(((dc & 1) | ((ac & 1) << 1)) << (2 * k) for k, (_, dc, ac) in enumerate(info.components))
        words[i, :4] = starts[i], end - first, (n * _DESC_WORDS + which[i] * 4 * _TABLE_WORDS) * 4, sel
        words[i, 4:] = np.concatenate([info.quant[c[0]] for c in info.components]).view(np.uint32)
        blob[starts[i]:starts[i] + end - first] = np.frombuffer(data, np.uint8, end - first, first)
    tabs = blob[n * _DESC_WORDS * 4:n * _DESC_WORDS * 4 + len(order) * 4 * _TABLE_WORDS * 4].view(np.uint32)
    tabs[:] = np.concatenate(order)
    return blob, max(info.scan[1] - info.scan[0] for info in infos)


# ---------------------------------------------------------------------------
# device code below: torch and the library are imported on use
# ---------------------------------------------------------------------------
class _Plan:
    """The workspace of one (n, h, w, device) and the output buffer of the calls without `out`."""

    def __init__(self, n, h, w, device):
        import torch
        from . import ops
        self.ws = torch.empty(max(ops.jpeg_workspace_bytes(n, h, w), 8), dtype=torch.uint8, device=device)
        self.out = None


MAX_PLANS = 8   # plans kept, least recently used first out (metrics._lru)
_plans = {}


def clear_plans():
    """Drop every kept plan (their device buffers are freed with them)."""
    _plans.clear()


def jpeg_roundtrip(x, quality, out=None):
    """A dense uint8 NHWC device tensor [n,h,w,3] -> its JPEG round trip at `quality`, equal to
    `jpeg_ref` bit for bit.  The result is `out` (which may be x itself) or the plan's own buffer,
    which the next call on the same shape overwrites; a repeated call allocates nothing.  No host
    sync, no table upload: the call can be captured in a graph."""
    import torch
    from . import ops
    from .metrics import _lru
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8:
        raise ValueError(f"jpeg_roundtrip: expected a uint8 tensor, got {getattr(x, 'dtype', type(x))}")
    if x.dim() != 4 or x.shape[3] != 3 or not x.is_contiguous() or not x.is_cuda:
        raise ValueError(f"jpeg_roundtrip: expected a dense [n,h,w,3] device tensor, got shape {tuple(x.shape)} on "
                         f"{x.device}")
    tables = quant_tables(_check_quality(quality, "jpeg_roundtrip"))
    n, h, w, _ = x.shape
    if min(h, w) < 1:
        raise ValueError(f"jpeg_roundtrip: empty image: {tuple(x.shape)}")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.shape != x.shape
                            or not out.is_contiguous() or out.device != x.device):
        raise ValueError(f"jpeg_roundtrip: out must be a dense uint8 {tuple(x.shape)} tensor on {x.device}, got "
                         f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))}")
    if n == 0:
        return torch.empty_like(x) if out is None else out
    p = _lru(_plans, (n, h, w, x.device), lambda: _Plan(n, h, w, x.device), MAX_PLANS)
    if out is None:
        if p.out is None:
            p.out = torch.empty_like(x)
        out = p.out
    return ops.jpeg_roundtrip(x, out, tables, p.ws)


class _EncodePlan:
    """The buffers of jpeg_encode at one (n, h, w, device): the workspace of the first half, and
    the streams and files of the second, which grow to the longest scan seen."""

    def __init__(self, n, h, w, device):
        import torch
        from . import ops
        self.ws = torch.empty(ops.jpeg_encode_workspace_bytes(n, h, w), dtype=torch.uint8, device=device)
        self.bits = torch.empty(n, dtype=torch.int64, device=device)
        self.sizes = torch.empty(n, dtype=torch.int32, device=device)
        self.stream_ws = self.out = None

    def room(self, n, max_bits, header_bytes):
        import torch
        from . import ops
        need, stride = ops.jpeg_encode_out_bytes(n, max_bits, header_bytes)
        if self.out is None or self.stream_ws.numel() < need or self.out.shape[1] < stride:
            self.stream_ws = torch.empty(need, dtype=torch.uint8, device=self.ws.device)
            self.out = torch.empty((n, stride), dtype=torch.uint8, device=self.ws.device)
        return self.stream_ws, self.out


def jpeg_encode(x, quality):
    """A dense uint8 NHWC device tensor [n,h,w,3] -> a list of n `bytes`, every image's baseline JPEG
    file at `quality` and 4:2:0, equal to `jpeg_encode_ref` (and to the file Pillow writes) byte for
    byte; [] for n = 0.  Colour, DCT, quantisation, Huffman coding and byte stuffing run on the
    device (csrc/jpeg_enc.hip); what crosses to the host is n scan lengths, which size the streams,
    n file lengths and the files themselves.  The call waits for those, so it cannot be captured
    in a graph; its buffers are kept per shape in the round trip's plan cache."""
    import torch
    from . import ops
    from .metrics import _lru
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8:
        raise ValueError(f"jpeg_encode: expected a uint8 tensor, got {getattr(x, 'dtype', type(x))}")
    if x.dim() != 4 or x.shape[3] != 3 or not x.is_contiguous() or not x.is_cuda:
        raise ValueError(f"jpeg_encode: expected a dense [n,h,w,3] device tensor, got shape {tuple(x.shape)} on "
                         f"{x.device}")
    quality = _check_quality(quality, "jpeg_encode")
    n, h, w, _ = x.shape
    if min(h, w) < 1:
        raise ValueError(f"jpeg_encode: empty image: {tuple(x.shape)}")
    header = jpeg_header(h, w, quality)
    if n == 0:
        return []
    p = _lru(_plans, ("encode", n, h, w, x.device), lambda: _EncodePlan(n, h, w, x.device), MAX_PLANS)
    ops.jpeg_encode_scan(x, quant_tables(quality), p.ws, p.bits)
    max_bits = int(p.bits.max().item())
    stream_ws, out = p.room(n, max_bits, len(header))
    ops.jpeg_encode_emit(x.shape, p.ws, p.bits, max_bits, header, stream_ws, out, p.sizes)
    sizes = p.sizes.cpu().tolist()
    if min(sizes) < len(header) + 2:
        raise RuntimeError(f"jpeg_encode: the device reports file lengths {sizes}")
    host = torch.empty(sum(sizes), dtype=torch.uint8, pin_memory=True)
    at = 0
    for i, size in enumerate(sizes):
        host[at:at + size].copy_(out[i, :size], non_blocking=True)
        at += size
    torch.cuda.current_stream().synchronize()
    data, files, at = host.numpy().tobytes(), [], 0
    for size in sizes:
        files.append(data[at:at + size])
        at += size
    return files


class _DecodePlan:
    """The buffers of jpeg_decode at one (n, h, w, device): the pinned blob and its device copy
    and the workspace, which grow to the largest blob and the longest scan seen, and the output of
    the calls without `out`."""

    def __init__(self):
        self.host = self.blob = self.ws = self.out = None
        self.max_scan = -1

    def room(self, n, h, w, device, blob_bytes, max_scan):
        import torch
        from . import ops
        if self.host is None or self.host.numel() < blob_bytes:
            self.host = torch.empty(blob_bytes + blob_bytes // 4, dtype=torch.uint8, pin_memory=True)
            self.blob = torch.empty(self.host.numel(), dtype=torch.uint8, device=device)
        if max_scan > self.max_scan:
            self.max_scan = max_scan + max_scan // 4
            self.ws = torch.empty(ops.jpeg_decode_workspace_bytes(n, h, w, self.max_scan), dtype=torch.uint8, device=device)


def jpeg_decode(files, out=None, device=None):
    """A list of n `bytes`, baseline 4:2:0 JPEG files of one size h x w (what `jpeg_parse` accepts;
    their tables may differ) -> a dense uint8 [n,h,w,3] device tensor equal to
    `np.stack([jpeg_decode_ref(f) for f in files])` bit for bit: `out`, or the plan's own buffer,
    which the next call on the same shape overwrites.  [] gives an empty [0,0,0,3] tensor.  The
    host parses the headers, looks up the Huffman tables' device form and uploads one pinned blob;
    it never walks a scan.  Entropy decoding, DC prediction, IDCT, upsampling and colour run on
    the device (csrc/jpeg_dec.hip).  The call reads one word per synchronisation round and the
    status words at the end, so it cannot be captured in a graph.  ValueError, naming the file,
    for a scan that ends early; files of different sizes; anything `jpeg_parse` refuses.  Only a
    short scan is detected: damaged bits that still fill every block decode to unspecified pixels,
    where `jpeg_decode_ref` raises for a window that starts no code."""
    return _decode(files, out, device)[0]


_STATUS = ((1, "the scan ends before the image's last block"), (2, "a symbol reaches past the scan's end"),
           (4, "its descriptor points outside the uploaded blob"))


def _decode(files, out, device):
    """jpeg_decode -> (the tensor, the synchronisation rounds across workgroups the call ran)."""
    import torch
    from . import ops
    from .metrics import _lru
    files = list(files)
    for i, f in enumerate(files):
        if not isinstance(f, bytes):
            raise TypeError(f"jpeg_decode: file {i} is {type(f).__name__}, not bytes")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"jpeg_decode: expected a GPU device (the HIP path has no CPU fallback), got {device}")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    n = len(files)
    if n == 0:
        if out is None:
            return torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=device), 0
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 4 or out.shape[0] != 0
                or out.shape[3] != 3 or out.device != device):
            raise ValueError(f"jpeg_decode: out must be a uint8 [0,h,w,3] tensor on {device}, got "
                             f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))}")
        return out, 0
    infos = [jpeg_parse(f) for f in files]
    h, w = infos[0].h, infos[0].w
    for i, info in enumerate(infos):
        if (info.h, info.w) != (h, w):
            raise ValueError(f"jpeg_decode: file {i} is {info.h}x{info.w}, file 0 is {h}x{w}: one call decodes one size")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, 3)
                            or not out.is_contiguous() or out.device != device):
        raise ValueError(f"jpeg_decode: out must be a dense uint8 {(n, h, w, 3)} tensor on {device}, got "
                         f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))}")
    if (DECODE_SUBSEQUENCE, DECODE_LANES) != ops.jpeg_decode_geometry():
        raise RuntimeError(f"jpeg_decode: the library decodes {ops.jpeg_decode_geometry()}, not "
                           f"{(DECODE_SUBSEQUENCE, DECODE_LANES)} bytes x lanes")
    blob, max_scan = _decode_blob(infos, files)
    p = _lru(_plans, ("decode", n, h, w, device), _DecodePlan, MAX_PLANS)
    with torch.cuda.device(device):
        p.room(n, h, w, device, blob.size, max_scan)
        p.host[:blob.size].numpy()[:] = blob
        p.blob[:blob.size].copy_(p.host[:blob.size], non_blocking=True)
        if out is None:
            if p.out is None:
                p.out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=device)
            out = p.out
        call = ops.JpegDecodeCall(n, h, w, p.blob, blob.size, max_scan, p.ws)
        call.scan()
        groups = -(-max(-(-max_scan // DECODE_SUBSEQUENCE), 1) // DECODE_LANES)
        seen = done = 0
        for r in range(1, groups):   # after round r the workgroups 0..r of every image are final
            call.sync(r)
            done = r
            moved = call.rounds_changed()
            if moved == seen:
                break
            seen = moved
        call.pixels(out)
        status = call.status()
    bad = [i for i, s in enumerate(status) if s]
    if bad:
        why = "; ".join(text for bit, text in _STATUS if status[bad[0]] & bit)
        raise ValueError(f"jpeg_decode: file {bad[0]}: {why} (status {status[bad[0]]}; {len(bad)} of {n} files)")
    return out, done
