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

`quant_tables` / `jpeg_ref` are pure numpy and import neither torch nor the library.
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


def _codec(plane, table):
    """A plane [n,H,W] (H, W multiples of 8) through the block pipeline with the table [64]."""
    n, H, W = plane.shape
    b = (plane - 128).reshape(n, H // 8, 8, W // 8, 8).transpose(0, 1, 3, 2, 4)   # [n,by,bx,row,col]
    c = _along(_fdct_1d, _along(_fdct_1d, b, 4, True), 3, False)
    t = table.astype(plane.dtype).reshape(8, 8)
    c = np.sign(c) * ((np.abs(c) + 4 * t) // (8 * t)) * t
    x = _along(_idct_1d, _along(_idct_1d, c, 3, True), 4, False) & 1023
    x = np.where(x < 128, x + 128, np.where(x < 512, 255, np.where(x < 896, 0, x - 896)))
    return x.transpose(0, 1, 3, 2, 4).reshape(n, H, W)


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
    if single:
        a = a[None]
    n, h, w = a.shape[:3]
    ch, cw = -(-h // 2), -(-w // 2)
    R, G, B = (a[..., k].astype(dtype) for k in range(3))
    Y = (_fix(.299) * R + _fix(.587) * G + _fix(.114) * B + 32768) >> 16
    Cb = (-_fix(.16874) * R - _fix(.33126) * G + _fix(.5) * B + (128 << 16) + 32767) >> 16
    Cr = (_fix(.5) * R - _fix(.41869) * G - _fix(.08131) * B + (128 << 16) + 32767) >> 16
    Y = _codec(_edge(Y, _up8(h), _up8(w)), tables[0])[:, :h, :w]
    bias = np.where(np.arange(_up8(cw)) % 2 == 0, 1, 2).astype(dtype)
    chroma = []
    for C in (Cb, Cr):
        C = _edge(C, 2 * ch, 2 * _up8(cw))
        C = (C[:, 0::2, 0::2] + C[:, 0::2, 1::2] + C[:, 1::2, 0::2] + C[:, 1::2, 1::2] + bias) >> 2
        C = _codec(_edge(C, _up8(ch), _up8(cw)), tables[1])[:, :ch, :cw]
        chroma.append(_upsample(C, cw > 2)[:, :h, :w] - 128)
    Cb, Cr = chroma
    out = np.stack([Y + ((_fix(1.402) * Cr + 32768) >> 16),
                    Y + ((-_fix(.34414) * Cb + 32768 - _fix(.71414) * Cr) >> 16),
                    Y + ((_fix(1.772) * Cb + 32768) >> 16)], axis=-1)
    out = np.clip(out, 0, 255).astype(np.uint8)
    return out[0] if single else out


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
