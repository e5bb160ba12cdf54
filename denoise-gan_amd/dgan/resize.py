"""Image resize with the semantics of `tf.image.resize` (half-pixel centres, no antialiasing),
'bicubic' (ResizeBicubic: Keys cubic a = -0.5 from a 1025-row table, taps outside the image get
weight 0 and the rest are renormalised) and 'bilinear': the 4-tap form of the interpolation
matrices of dataloader.py, a host reference and the device op (csrc/resize.hip).

The evaluation order is part of the definition.  In fp64, every product and every sum rounded on
its own (no FMA), with (iy, wy), (ix, wx) the tap tables of the two axes:

    t = ((wy0 a[iy0] + wy1 a[iy1]) + wy2 a[iy2]) + wy3 a[iy3]      the vertical pass, per input column
    v = ((wx0 t[ix0] + wx1 t[ix1]) + wx2 t[ix2]) + wx3 t[ix3]      the horizontal pass

uint8 images give uint8: floor(clamp(v * mul + bias, 0, 255)); float32 images give float32(v).
The two conversions in use:

    DEGRADE  mul 255.5/255, bias 0   TF's convert_image_dtype float -> uint8, floor(p * 255.5)
                                     saturated, with p = v / 255: what adjust_jpeg_quality sees
    DISPLAY  mul 1, bias 0.5         round to nearest, the rule of dg_u8_unstage

Why a fixed order and not a tolerance: for x2 / x4 upscales the bilinear and the interior bicubic
weights are dyadic, v * mul + bias is then an exact integer on about 5 % of the pixels and comes
within 4e-14 of one beside the renormalised edge taps, so another summation order or a contracted
FMA flips pixels.  With the order fixed the device output equals `resize_ref` bit for bit.

`resize_taps` / `resize_ref` are pure numpy and import neither torch nor the library.
"""
import numpy as np

METHODS = ("bicubic", "bilinear")
DEGRADE = (255.5 / 255.0, 0.0)
DISPLAY = (1.0, 0.5)

_TABLE = 1024


def _keys_table(a=-0.5):
    """TF's bicubic coefficient table: for delta = i / 1024, the weights of the taps at distance
    1 + delta, delta, 1 - delta, 2 - delta (dataloader._keys_table)."""
    def w(t):
        t = np.abs(t)
        return np.where(t <= 1, ((a + 2) * t - (a + 3)) * t * t + 1,
                        np.where(t < 2, ((t - 5) * t + 8) * t * a - 4 * a, 0.0))
    d = np.arange(_TABLE + 1) / _TABLE
    return np.stack([w(1 + d), w(d), w(1 - d), w(2 - d)], axis=1)


_COEFFS = _keys_table()


def resize_taps(n_in, n_out, method="bicubic"):
    """(idx int32 [n_out,4], w float64 [n_out,4]): output o is sum_k w[o,k] * in[idx[o,k]].
    Indices are clamped into [0, n_in-1]; a clamped tap has weight 0."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize_taps: sizes must be at least 1, got {n_in} -> {n_out}")
    if method not in METHODS:
        raise ValueError(f"resize_taps: method must be one of {METHODS}, got {method!r}")
    scale = n_in / n_out
    idx = np.zeros((n_out, 4), np.int32)
    wts = np.zeros((n_out, 4), np.float64)
    for o in range(n_out):
        x = (o + 0.5) * scale - 0.5
        if method == "bicubic":
            i = int(np.floor(x))
            w = _COEFFS[int(np.rint((x - i) * _TABLE))].copy()
            taps = np.array([i - 1, i, i + 1, i + 2])
            w = np.where((taps >= 0) & (taps < n_in), w, 0.0)
            s = w.sum()
            if abs(s) > 0:
                w = w / s
        else:
            x = max(x, 0.0)
            i0 = min(int(np.floor(x)), n_in - 1)
            i1 = min(i0 + 1, n_in - 1)
            f = x - i0
            taps, w = np.array([i0, i1, i1, i1]), np.array([1 - f, f, 0.0, 0.0])
        idx[o] = np.clip(taps, 0, n_in - 1)
        wts[o] = w
    return idx, wts


def _pass(a, axis, idx, w):
    """One 4-tap pass along `axis` of the fp64 array a, in the stated order."""
    shape = [1] * a.ndim
    shape[axis] = -1
    p = [w[:, k].reshape(shape) * np.take(a, idx[:, k], axis=axis) for k in range(4)]
    return ((p[0] + p[1]) + p[2]) + p[3]


def resize_ref(img, h, w, method="bicubic", mul=1.0, bias=0.0):
    """The definition on the host: [n,hi,wi,C] or [hi,wi,C], uint8 or float32 -> the same dtype at
    h x w (module docstring)."""
    a = np.asarray(img)
    if a.dtype not in (np.uint8, np.float32) or a.ndim not in (3, 4):
        raise ValueError(f"resize_ref: expected uint8 or float32 [n,h,w,C] or [h,w,C], got {a.dtype} {a.shape}")
    if a.dtype == np.float32 and (mul != 1.0 or bias != 0.0):
        raise ValueError("resize_ref: mul / bias apply to uint8 images only")
    single = a.ndim == 3
    if single:
        a = a[None]
    iy, wy = resize_taps(a.shape[1], h, method)
    ix, wx = resize_taps(a.shape[2], w, method)
    v = _pass(_pass(a.astype(np.float64), 1, iy, wy), 2, ix, wx)
    if a.dtype == np.uint8:
        out = np.floor(np.clip(v * float(mul) + float(bias), 0.0, 255.0)).astype(np.uint8)
    else:
        out = v.astype(np.float32)
    return out[0] if single else out


# ---------------------------------------------------------------------------
# device code below: torch and the library are imported on use
# ---------------------------------------------------------------------------
class _Plan:
    """The device tap tables of one (hi, wi, h, w, method, device) and the output buffer of the
    last (n, C, dtype) seen on it."""

    def __init__(self, hi, wi, h, w, method, device):
        import torch
        iy, wy = resize_taps(hi, h, method)
        ix, wx = resize_taps(wi, w, method)
        self.iy, self.wy, self.ix, self.wx = (torch.from_numpy(t).to(device) for t in (iy, wy, ix, wx))
        self.out = None


MAX_PLANS = 8   # plans kept, least recently used first out (metrics._lru)
_plans = {}


def clear_plans():
    """Drop every kept plan (their device buffers are freed with them)."""
    _plans.clear()


def resize(x, h, w, method="bicubic", mul=1.0, bias=0.0, out=None):
    """A dense uint8 or fp32 NHWC device tensor [n,hi,wi,C] -> [n,h,w,C] of the same dtype, equal
    to `resize_ref` bit for bit.  The result is `out` or the plan's own buffer, which the next call
    on the same sizes and method overwrites; a repeated call allocates nothing.  No host sync."""
    import torch
    from . import ops
    from .metrics import _lru
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"resize: expected a uint8 or float32 tensor, got {getattr(x, 'dtype', type(x))}")
    if x.dim() != 4 or not x.is_contiguous() or not x.is_cuda:
        raise ValueError(f"resize: expected a dense [n,h,w,C] device tensor, got shape {tuple(x.shape)} on {x.device}")
    if method not in METHODS:
        raise ValueError(f"resize: method must be one of {METHODS}, got {method!r}")
    h, w = int(h), int(w)
    n, hi, wi, C = x.shape
    if min(h, w, hi, wi, C) < 1:
        raise ValueError(f"resize: empty image: {tuple(x.shape)} -> {h}x{w}")
    if x.dtype == torch.float32 and (mul != 1.0 or bias != 0.0):
        raise ValueError("resize: mul / bias apply to uint8 images only")
    p = _lru(_plans, (hi, wi, h, w, method, x.device), lambda: _Plan(hi, wi, h, w, method, x.device), MAX_PLANS)
    shape = (n, h, w, C)
    if out is None:
        if p.out is None or tuple(p.out.shape) != shape or p.out.dtype != x.dtype:
            p.out = torch.empty(shape, dtype=x.dtype, device=x.device)
        out = p.out
    elif (not isinstance(out, torch.Tensor) or out.dtype != x.dtype or tuple(out.shape) != shape
          or not out.is_contiguous() or out.device != x.device):
        raise ValueError(f"resize: out must be a dense {x.dtype} {shape} tensor on {x.device}, got "
                         f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))}")
    if n and out.data_ptr() == x.data_ptr():
        raise ValueError("resize: out must not be the input")
    return ops.resize(x, out, p.iy, p.wy, p.ix, p.wx, mul, bias)
