"""Classical denoisers on uint8 RGB frames: the 3x3 median and joint-RGB non-local means, as exact
integer definitions with a numpy reference each and the device ops (csrc/filters.hip) that equal
the references bit for bit.  They are the baselines a trained denoiser is judged against
(dgan.metrics.Evaluator(baseline=...), evaluate.py --baseline) and the reference's `sr_denoise`
post-filter (infer.py --post median3).

    median3    every channel's median over its 3x3 neighbourhood, the image edge-replicated by one
               pixel: cv2.medianBlur(img, 3), scipy.ndimage.median_filter(img, (3, 3, 1), "nearest")

    nlm        template t in {3, 5, 7}, search window s odd in 3..21, strength h in 1..40;
               rt = t // 2, rs = s // 2.  P: the image padded by rt + rs with np.pad's "reflect"
               (dgan.infer.pad_index, any pad width).  For a pixel p and each of the s*s offsets d
                   D(p,d) = sum over q in the t x t patch and the 3 channels of (P(p+q) - P(p+d+q))^2
                   w(p,d) = W[min(D // (3 t^2), len(W) - 1)]
               with the table W[i] = floor(2^14 exp(-i / h^2) + 0.5) (fp64 on the host), cut after
               its first 0, and
                   out(p,c) = (sum_d w P(p+d,c) + S // 2) // S,   S = sum_d w >= W[0] = 16384.
               D < 2^24, S <= 441 * 2^14 and sum w v < 2^31: everything fits int32 (`nlm_ref` takes
               the working type as an argument; tests/test_filters.py holds int32 equal to int64).

`nlm` is the non-local means of Buades et al. with one weight for the three channels.  It is NOT
claimed equal to cv2.fastNlMeansDenoisingColored, which filters in Lab with separate luminance and
colour strengths and its own fixed-point weights.

`median3_ref` / `nlm_table` / `nlm_ref` are pure numpy and import neither torch nor the library.
"""
import numpy as np

TEMPLATES = (3, 5, 7)
MAX_SEARCH = 21
MAX_H = 40
WEIGHT_ONE = 1 << 14


def _images(a, what, dtype=None):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.shape[-1] != 3:
        raise ValueError(f"{what}: expected uint8 [n,h,w,3] or [h,w,3], got {a.dtype} {a.shape}")
    if min(a.shape[-3:-1]) < 1:
        raise ValueError(f"{what}: empty image: {a.shape}")
    if dtype is not None and np.dtype(dtype) not in (np.dtype(np.int64), np.dtype(np.int32)):
        raise ValueError(f"{what}: dtype must be np.int64 or np.int32, got {dtype!r}")
    return (a[None], True) if a.ndim == 3 else (a, False)


def check_nlm(h, template, search, what="nlm"):
    """(h, template, search) as ints, or ValueError naming the bad one."""
    for name, v in (("h", h), ("template", template), ("search", search)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what}: {name} must be an integer, got {v!r}")
    if not 1 <= h <= MAX_H:
        raise ValueError(f"{what}: h must be in 1..{MAX_H}, got {h}")
    if template not in TEMPLATES:
        raise ValueError(f"{what}: template must be one of {TEMPLATES}, got {template}")
    if not 3 <= search <= MAX_SEARCH or search % 2 == 0:
        raise ValueError(f"{what}: search must be odd in 3..{MAX_SEARCH}, got {search}")
    return int(h), int(template), int(search)


def median3_ref(img_u8):
    """The definition on the host: uint8 [n,h,w,3] or [h,w,3] -> the same shape and dtype."""
    a, single = _images(img_u8, "median3_ref")
    n, h, w = a.shape[:3]
    p = np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
    nine = np.stack([p[:, i:i + h, j:j + w] for i in range(3) for j in range(3)])
    out = np.sort(nine, axis=0)[4]
    return out[0] if single else out


def nlm_table(h):
    """int64 [len]: W[i] = floor(2^14 exp(-i / h^2) + 0.5), cut after its first 0."""
    h = check_nlm(h, TEMPLATES[0], 3, "nlm_table")[0]
    n = int(np.ceil(h * h * np.log(2.0 * WEIGHT_ONE))) + 2   # exp(-i / h^2) < 2^-15 from here on
    w = np.floor(WEIGHT_ONE * np.exp(-np.arange(n, dtype=np.float64) / float(h * h)) + 0.5).astype(np.int64)
    return w[:int(np.argmax(w == 0)) + 1]


def nlm_ref(img_u8, h=10, template=7, search=21, dtype=np.int64):
    """The definition on the host: uint8 [n,h,w,3] or [h,w,3] -> the same shape and dtype (module
    docstring).  dtype: the working integer type, np.int64 or np.int32."""
    from .infer import pad_index
    a, single = _images(img_u8, "nlm_ref", dtype)
    h, t, s = check_nlm(h, template, search, "nlm_ref")
    W = nlm_table(h).astype(dtype)
    n, H, Wd = a.shape[:3]
    rt, rs = t // 2, s // 2
    r = rt + rs
    rows, cols = pad_index(np.arange(-r, H + r), H, "reflect"), pad_index(np.arange(-r, Wd + r), Wd, "reflect")
    P = a[:, rows][:, :, cols].astype(dtype)
    He, We = H + 2 * rt, Wd + 2 * rt            # the positions the patches of the image cover
    base = P[:, rs:rs + He, rs:rs + We]
    S = np.zeros((n, H, Wd), dtype)
    A = np.zeros((n, H, Wd, 3), dtype)
    for dy in range(-rs, rs + 1):
        for dx in range(-rs, rs + 1):
            e = ((base - P[:, rs + dy:rs + dy + He, rs + dx:rs + dx + We]) ** 2).sum(-1, dtype=dtype)
            D = np.zeros((n, H, Wd), dtype)
            for i in range(t):
                for j in range(t):
                    D += e[:, i:i + H, j:j + Wd]
            w = W[np.minimum(D // (3 * t * t), len(W) - 1)]
            S += w
            A += w[..., None] * P[:, r + dy:r + dy + H, r + dx:r + dx + Wd]
    out = ((A + (S // 2)[..., None]) // S[..., None]).astype(np.uint8)
    return out[0] if single else out


# ---------------------------------------------------------------------------
# device code below: torch and the library are imported on use
# ---------------------------------------------------------------------------
MAX_PLANS = 8   # plans kept over both filters, least recently used first out (metrics._lru)
_plans = {}     # (filter, n, h, w, device) -> the output buffers of the calls without `out`: one, and a
                # second from the first call whose input is the first (a filter applied to its own result)
_tables = {}    # (h, device) -> the device int16 weight table, uploaded once (at most MAX_H per device)


def clear_plans():
    """Drop every kept output buffer and weight table."""
    _plans.clear()
    _tables.clear()


def _device_pair(x, out, what):
    import torch
    from .metrics import _lru
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8:
        raise ValueError(f"{what}: expected a uint8 tensor, got {getattr(x, 'dtype', type(x))}")
    if x.dim() != 4 or x.shape[3] != 3 or not x.is_contiguous() or not x.is_cuda:
        raise ValueError(f"{what}: expected a dense [n,h,w,3] device tensor, got shape {tuple(x.shape)} on {x.device}")
    n, h, w, _ = x.shape
    if min(h, w) < 1:
        raise ValueError(f"{what}: empty image: {tuple(x.shape)}")
    if out is x:
        raise ValueError(f"{what}: out must not be the input")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.shape != x.shape
                            or not out.is_contiguous() or out.device != x.device):
        raise ValueError(f"{what}: out must be a dense uint8 {tuple(x.shape)} tensor on {x.device}, got "
                         f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))}")
    if n == 0:
        return torch.empty_like(x) if out is None else out
    if out is None:
        bufs = _lru(_plans, (what, n, h, w, x.device), lambda: [torch.empty_like(x)], MAX_PLANS)
        if bufs[0].data_ptr() == x.data_ptr() and len(bufs) == 1:
            bufs.append(torch.empty_like(x))
        out = bufs[1] if bufs[0].data_ptr() == x.data_ptr() else bufs[0]
    return out


def median3(x, out=None):
    """A dense uint8 NHWC device tensor [n,h,w,3] -> its 3x3 median, equal to `median3_ref` bit for
    bit.  The result is `out` (never x itself) or the plan's own buffer (its second one when x is the
    first: median3(median3(x)) works), which the next call on the
    same shape overwrites; a repeated call allocates nothing and does no host sync."""
    from . import ops
    out = _device_pair(x, out, "median3")
    return ops.median3(x, out) if x.shape[0] else out


def nlm(x, h=10, template=7, search=21, out=None):
    """A dense uint8 NHWC device tensor [n,h,w,3] -> its non-local means, equal to `nlm_ref` bit
    for bit.  `out` as in `median3`.  The weight table of `h` is uploaded on its first use on a
    device; after that a call allocates nothing, does no host sync and can be captured in a graph."""
    import torch
    from . import ops
    h, t, s = check_nlm(h, template, search)
    out = _device_pair(x, out, "nlm")
    if x.shape[0] == 0:
        return out
    key = (h, x.device)
    if key not in _tables:
        _tables[key] = torch.from_numpy(nlm_table(h).astype(np.int16)).to(x.device)
    return ops.nlm(x, out, _tables[key], t, s)
