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

A second convention, Pillow's `Image.resize` (antialiased: the filter's support grows with the
downscale factor; 8-bit fixed point, horizontal pass first, the intermediate rounded to uint8):
`pil_coeffs` / `resize_pil_ref` / `resize_pil` (csrc/resize_pil.hip), integers once the coefficients
exist and equal to Pillow bit for bit.  It shares nothing with the first but the plan cache.

`resize_taps` / `resize_ref` / `pil_coeffs` / `resize_pil_ref` are pure numpy and import neither
torch nor the library.
"""
import math

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
# Pillow's Image.resize: antialiased, 8-bit fixed point.  The filter's support grows with the
# downscale factor; the coefficients are fp64 once, integers from then on (Resample.c).
# ---------------------------------------------------------------------------
PIL_FILTERS = ("box", "bilinear", "hamming", "bicubic", "lanczos")
_PIL_SUPPORT = {"box": 0.5, "bilinear": 1.0, "hamming": 1.0, "bicubic": 2.0, "lanczos": 3.0}
PIL_BITS = 22   # fraction bits of a coefficient (Resample.c PRECISION_BITS = 32 - 8 - 2)


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _pil_filter(name, x):
    """Pillow's filter kernels at the scalar x, in its order of operations."""
    if name == "box":
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if name == "lanczos":
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    x = abs(x)
    if name == "bilinear":
        return 1.0 - x if x < 1.0 else 0.0
    if name == "hamming":
        if x == 0.0:
            return 1.0
        if x >= 1.0:
            return 0.0
        x = x * math.pi
        return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))
    a = -0.5
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pil_coeffs(n_in, n_out, filter="bicubic"):
    """(first int32 [n_out], count int32 [n_out], k int32 [n_out, ksize]) of one axis: output o is
    clip((2^21 + sum_{j < count[o]} k[o,j] * in[first[o] + j]) >> 22, 0, 255).  fp64 in Pillow's
    order (precompute_coeffs, normalize_coeffs_8bpc); entries of k beyond count are 0."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"pil_coeffs: sizes must be at least 1, got {n_in} -> {n_out}")
    if filter not in PIL_FILTERS:
        raise ValueError(f"pil_coeffs: filter must be one of {PIL_FILTERS}, got {filter!r}")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = _PIL_SUPPORT[filter] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    first = np.zeros(n_out, np.int32)
    count = np.zeros(n_out, np.int32)
    k = np.zeros((n_out, ksize), np.int32)
    for o in range(n_out):
        center = (o + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), n_in) - lo
        w = [_pil_filter(filter, (j + lo - center + 0.5) / fs) for j in range(cnt)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        first[o], count[o] = lo, cnt
        k[o, :cnt] = [int(v * (1 << PIL_BITS) - 0.5) if v < 0 else int(v * (1 << PIL_BITS) + 0.5) for v in w]
    return first, count, k


def _pil_pass(a, axis, first, count, k, dtype):
    """One fixed-point pass along `axis` of the uint8 array a -> uint8."""
    a = np.moveaxis(a, axis, -1).astype(dtype)
    out = np.empty(a.shape[:-1] + (len(first),), np.uint8)
    half = dtype(1 << (PIL_BITS - 1))
    for o in range(len(first)):
        s = (a[..., first[o]:first[o] + count[o]] * k[o, :count[o]].astype(dtype)).sum(-1, dtype=dtype) + half
        out[..., o] = np.clip(s >> PIL_BITS, 0, 255)
    return np.moveaxis(out, -1, axis)


def resize_pil_ref(img, h, w, filter="bicubic", dtype=np.int64):
    """Pillow's `Image.resize((w, h), filter)` on the host: uint8 [n,hi,wi,C] or [hi,wi,C] -> uint8
    at h x w.  The horizontal pass runs first (if w != wi), the vertical pass on its uint8 result
    (if h != hi); a same-size call is a copy.  dtype: the working integer type, np.int64 or
    np.int32; they give the same bits, since |2^21 + sum k * in| <= 2^21 + 255 * sum |k| stays
    below 2^31 while sum |k| < 2.006 * 2^22, and a normalised window has sum |k| = (1 + 2 m) * 2^22
    up to rounding with m the weight of its negative lobes: none for box, bilinear and hamming,
    at most 0.14 for bicubic and 0.28 for lanczos, windows cut by the image's edge included
    (sum |k| <= 1.27 and 1.55 times 2^22; tests/test_resize_pil.py asserts the bound itself).

    Equal to Pillow bit for bit wherever it was compared (tests/test_resize_pil.py).  For box,
    bilinear and bicubic the coefficients are fp64 +, *, / only; those of lanczos and hamming go
    through libm's sin / cos on the host, so for these two the equality is an observation on the
    machines it was run on, not a theorem.  The device never evaluates a filter."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (3, 4):
        raise ValueError(f"resize_pil_ref: expected uint8 [n,h,w,C] or [h,w,C], got {a.dtype} {a.shape}")
    if dtype not in (np.int64, np.int32):
        raise ValueError(f"resize_pil_ref: dtype must be np.int64 or np.int32, got {dtype}")
    if filter not in PIL_FILTERS:
        raise ValueError(f"resize_pil_ref: filter must be one of {PIL_FILTERS}, got {filter!r}")
    h, w = int(h), int(w)
    single = a.ndim == 3
    if single:
        a = a[None]
    if min(h, w) < 1 or min(a.shape[1:]) < 1:
        raise ValueError(f"resize_pil_ref: empty image: {a.shape} -> {h}x{w}")
    if w != a.shape[2]:
        a = _pil_pass(a, 2, *pil_coeffs(a.shape[2], w, filter), dtype)
    if h != a.shape[1]:
        a = _pil_pass(a, 1, *pil_coeffs(a.shape[1], h, filter), dtype)
    out = np.array(a, np.uint8)
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


def _pil_identity(n):
    """The tables of an axis that keeps its size: one tap of weight 1, so the pass is a copy."""
    return np.arange(n, dtype=np.int32), np.ones(n, np.int32), np.full((n, 1), 1 << PIL_BITS, np.int32)


def pil_ksize(n_in, n_out, filter):
    """Taps per output of one axis: pil_coeffs' ksize, 1 for an axis that keeps its size."""
    if n_in == n_out:
        return 1
    return int(math.ceil(_PIL_SUPPORT[filter] * max(n_in / n_out, 1.0))) * 2 + 1


def pil_tile(hi, wi, h, w, filter="bicubic", C=3):
    """(th, tw, LDS bytes): the output tile of the kernel for these sizes (host only); ValueError
    when the downscale is steeper than a block's LDS holds."""
    from . import ops
    try:
        return ops.resize_pil_tile(hi, wi, C, h, w, pil_ksize(wi, w, filter), pil_ksize(hi, h, filter))
    except ops.DGError as e:
        raise ValueError(f"resize_pil: {hi}x{wi} -> {h}x{w} is too steep a downscale: {e}") from None


class _PilPlan:
    """The device coefficient tables of one (hi, wi, h, w, filter, device) and the output buffer of
    the last (n, C) seen on it."""

    def __init__(self, hi, wi, h, w, filter, device):
        import torch
        tabs = [pil_coeffs(n_in, n_out, filter) if n_in != n_out else _pil_identity(n_out)
                for n_in, n_out in ((wi, w), (hi, h))]
        self.tx, self.ty = (tuple(torch.from_numpy(t).to(device) for t in tab) for tab in tabs)
        self.out = None


def resize_pil(x, h, w, filter="bicubic", out=None):
    """A dense uint8 NHWC device tensor [n,hi,wi,C], C 1 or 3 -> uint8 [n,h,w,C], equal to
    `resize_pil_ref` (Pillow's `Image.resize((w, h), filter)`) bit for bit.  Four channels are
    refused: Pillow premultiplies RGBA by alpha.  The result is `out` or the plan's own buffer,
    which the next call on the same sizes and filter overwrites; a repeated call allocates nothing.
    One launch, no host sync, no atomics: it can be captured in a graph."""
    import torch
    from . import ops
    from .metrics import _lru
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8:
        raise ValueError(f"resize_pil: expected a uint8 tensor, got {getattr(x, 'dtype', type(x))}")
    if x.dim() != 4 or not x.is_contiguous() or not x.is_cuda:
        raise ValueError(f"resize_pil: expected a dense [n,h,w,C] device tensor, got shape {tuple(x.shape)} on {x.device}")
    if filter not in PIL_FILTERS:
        raise ValueError(f"resize_pil: filter must be one of {PIL_FILTERS}, got {filter!r}")
    h, w = int(h), int(w)
    n, hi, wi, C = x.shape
    if min(h, w, hi, wi) < 1:
        raise ValueError(f"resize_pil: empty image: {tuple(x.shape)} -> {h}x{w}")
    if C not in (1, 3):
        raise ValueError(f"resize_pil: C must be 1 or 3 (Pillow premultiplies a fourth channel), got {C}")
    key = (hi, wi, h, w, "pil:" + filter, x.device)
    pil_tile(hi, wi, h, w, filter, C)   # (a host call: refuses a factor the kernel cannot take, by name)
    p = _lru(_plans, key, lambda: _PilPlan(hi, wi, h, w, filter, x.device), MAX_PLANS)
    shape = (n, h, w, C)
    if out is None:
        if p.out is None or tuple(p.out.shape) != shape:
            p.out = torch.empty(shape, dtype=torch.uint8, device=x.device)
        out = p.out
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape
          or not out.is_contiguous() or out.device != x.device):
        raise ValueError(f"resize_pil: out must be a dense uint8 {shape} tensor on {x.device}, got "
                         f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))}")
    if n and out.data_ptr() == x.data_ptr():
        raise ValueError("resize_pil: out must not be the input")
    if n == 0:
        return out
    return ops.resize_pil(x, out, p.tx, p.ty)
