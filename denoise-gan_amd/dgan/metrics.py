"""Image quality: PSNR and SSIM per image, the `tf.image.psnr` / `tf.image.ssim` defaults stated
in fp64 (the reference has no metrics; BASELINE.json names PSNR as the quality yardstick).

PSNR = 10 log10(max_val^2 / mse), mse the mean of (a - b)^2 over h*w*C; identical images give inf.
SSIM (Wang et al. 2004): 11x11 Gaussian window, sigma 1.5, VALID positions only, c1 = (0.01 max_val)^2,
c2 = (0.03 max_val)^2, the mean of l * cs over the (h-10) x (w-10) map and the channels.

`psnr_ref` / `ssim_ref` are pure numpy (fp64) and import neither torch nor the library: the tests
and the host timings use them.  `psnr` / `ssim` run on the device (csrc/metrics.hip) on dense uint8
or fp32 NHWC tensors and return device fp64 tensors without a host synchronisation; `Evaluator`
scores a `Denoiser`'s input and output frame against a clean frame where they already are, and
`SREvaluator` an `Upscaler`'s output and the bicubic baseline (dgan/resize.py) against the
high-resolution original.  Both can degrade a clean frame themselves with the device JPEG round
trip (dgan/jpeg.py), so a whole evaluation stays on the device.
"""
import numpy as np

SSIM_TAPS = 11
SSIM_SIGMA = 1.5
K1, K2 = 0.01, 0.03


def gaussian_taps():
    """The 1-D window g[i] = exp(-(i-5)^2 / (2 sigma^2)) / sum g, fp64; the 2-D window is its
    outer product."""
    i = np.arange(SSIM_TAPS, dtype=np.float64) - (SSIM_TAPS - 1) / 2
    g = np.exp(-(i * i) / (2.0 * SSIM_SIGMA * SSIM_SIGMA))
    return g / g.sum()


def _ref_pair(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.dtype not in (np.uint8, np.float32, np.float64):
        raise ValueError(f"{what}: expected two uint8, float32 or float64 arrays of one dtype, got {a.dtype} and {b.dtype}")
    if a.shape != b.shape:
        raise ValueError(f"{what}: shapes differ: {a.shape} vs {b.shape}")
    if a.ndim not in (3, 4):
        raise ValueError(f"{what}: expected [n,h,w,C] or [h,w,C], got {a.shape}")
    single = a.ndim == 3
    if single:
        a, b = a[None], b[None]
    return a.astype(np.float64), b.astype(np.float64), single


def _default_max(dtype, max_val, what):
    if max_val is None:
        if np.dtype(dtype) != np.uint8:
            raise ValueError(f"{what}: max_val is required for {np.dtype(dtype)} images")
        return 255.0
    max_val = float(max_val)
    if not max_val > 0.0:
        raise ValueError(f"{what}: max_val must be positive")
    return max_val


def psnr_ref(a, b, max_val=None):
    """fp64 PSNR per image ([n], or a scalar for [h,w,C] inputs)."""
    max_val = _default_max(np.asarray(a).dtype, max_val, "psnr_ref")
    x, y, single = _ref_pair(a, b, "psnr_ref")
    mse = ((x - y) ** 2).reshape(x.shape[0], -1).mean(axis=1)
    with np.errstate(divide="ignore"):
        out = 10.0 * np.log10((max_val * max_val) / mse)
    return out[0] if single else out


def _filter_valid(x, g):
    """Rows then columns of [n,h,w,C] with the taps g, VALID."""
    k = len(g)
    mw, mh = x.shape[2] - k + 1, x.shape[1] - k + 1
    r = np.zeros(x.shape[:2] + (mw, x.shape[3]))
    for t in range(k):
        r += g[t] * x[:, :, t:t + mw, :]
    c = np.zeros((x.shape[0], mh, mw, x.shape[3]))
    for t in range(k):
        c += g[t] * r[:, t:t + mh, :, :]
    return c


def ssim_ref(a, b, max_val=None):
    """fp64 SSIM per image ([n], or a scalar for [h,w,C] inputs)."""
    max_val = _default_max(np.asarray(a).dtype, max_val, "ssim_ref")
    x, y, single = _ref_pair(a, b, "ssim_ref")
    if x.shape[1] < SSIM_TAPS or x.shape[2] < SSIM_TAPS:
        raise ValueError(f"ssim_ref: images of {x.shape[1]}x{x.shape[2]} are smaller than the {SSIM_TAPS}x{SSIM_TAPS} window")
    g = gaussian_taps()
    c1, c2 = (K1 * max_val) ** 2, (K2 * max_val) ** 2
    mua, mub = _filter_valid(x, g), _filter_valid(y, g)
    gaa, gbb, gab = _filter_valid(x * x, g), _filter_valid(y * y, g), _filter_valid(x * y, g)
    ab, aa, bb = mua * mub, mua * mua, mub * mub
    # grouped so that identical images give num == den in both factors: exactly 1.0
    l = (2.0 * ab + c1) / ((aa + bb) + c1)
    cs = (2.0 * (gab - ab) + c2) / (((gaa + gbb) - (aa + bb)) + c2)
    out = (l * cs).reshape(x.shape[0], -1).mean(axis=1)
    return out[0] if single else out


# ---------------------------------------------------------------------------
# device code below: torch and the library are imported on use
# ---------------------------------------------------------------------------
class _Plan:
    """Buffers of one (n, h, w, C, dtype, device): the error sums, the SSIM and error-sum
    workspaces and one output of each metric.  A metric call on a kept plan allocates nothing."""

    def __init__(self, n, h, w, C, dtype, device):
        import torch
        from . import ops
        self.count = h * w * C
        u8 = dtype == torch.uint8
        self.sums = torch.zeros((n, 2), dtype=torch.int64 if u8 else torch.float64, device=device)
        self.err_ws = None if u8 else torch.empty(max(ops.err_sums_workspace_bytes(n, self.count), 8), dtype=torch.uint8,
                                                  device=device)
        self.mse = torch.empty(n, dtype=torch.float64, device=device)
        self.peak = torch.empty(n, dtype=torch.float64, device=device)
        self.psnr = torch.empty(n, dtype=torch.float64, device=device)
        self.ssim = torch.empty(n, dtype=torch.float64, device=device)
        self.ssim_ws = None
        if h >= SSIM_TAPS and w >= SSIM_TAPS:
            self.ssim_ws = torch.empty(max(ops.ssim_workspace_bytes(n, h, w, C), 8), dtype=torch.uint8, device=device)


MAX_PLANS = 8     # plans kept (least recently used first out): a directory of many image sizes
_plans = {}       # stays bounded; a dict keeps insertion order, a hit is moved to the end


def _lru(cache, key, make, limit):
    if key in cache:
        cache[key] = cache.pop(key)
    else:
        while len(cache) >= limit:
            del cache[next(iter(cache))]
        cache[key] = make()
    return cache[key]


def clear_plans():
    """Drop every kept plan (their device buffers are freed with them)."""
    _plans.clear()


def _plan(a, b, what):
    from . import ops
    n, h, w, C = ops._metric_pair(a, b, what)
    key = (n, h, w, C, a.dtype, a.device)
    return _lru(_plans, key, lambda: _Plan(n, h, w, C, a.dtype, a.device), MAX_PLANS)


def _device_max(a, max_val, what):
    import torch
    if max_val is None and isinstance(a, torch.Tensor) and a.dtype != torch.uint8:
        raise ValueError(f"{what}: max_val is required for {a.dtype} images")
    return _default_max(np.uint8, max_val, what)


def err_sums(a, b):
    """Per image {sum (a-b)^2, sum |a-b|} of two dense device tensors [n,h,w,C]: an int64 (uint8
    images, exact) or fp64 (fp32 images) device tensor [n,2], the plan's own (the next call on the
    same shape overwrites it)."""
    from . import ops
    p = _plan(a, b, "err_sums")
    return ops.err_sums(a, b, p.sums, p.err_ws)


def psnr(a, b, max_val=None, out=None):
    """PSNR per image of dense uint8 or fp32 NHWC device tensors: a device fp64 tensor [n] (`out`,
    or the plan's own, which the next call on the same shape overwrites).  No host sync."""
    import torch
    from . import ops
    max_val = _device_max(a, max_val, "psnr")
    p = _plan(a, b, "psnr")
    ops.err_sums(a, b, p.sums, p.err_ws)
    out = p.psnr if out is None else out
    p.mse.copy_(p.sums[:, 0])          # (int64 -> fp64: exact below 2^53)
    p.mse.div_(float(p.count))
    p.peak.fill_(max_val * max_val)
    torch.div(p.peak, p.mse, out=out)  # mse 0 -> inf
    out.log10_().mul_(10.0)
    return out


def ssim(a, b, max_val=None, scale=1.0, shift=0.0, out=None):
    """SSIM per image of dense uint8 or fp32 NHWC device tensors (fp32 values are read as
    v * scale + shift): a device fp64 tensor [n], as `psnr` returns it.  No host sync."""
    from . import ops
    max_val = _device_max(a, max_val, "ssim")
    p = _plan(a, b, "ssim")
    return ops.ssim(a, b, p.ssim if out is None else out, p.ssim_ws, max_val, scale, shift)


SCORES = ("psnr_noisy", "psnr_denoised", "ssim_noisy", "ssim_denoised")


class Evaluator:
    """Scores a `Denoiser`'s frames against clean frames on the device: the noisy input and the
    denoised output stay where `Denoiser` holds them (uint8, dense), the clean frame is uploaded
    beside them, and only the 4 n scalars come back.  With a graph-capturing `Denoiser` the metrics
    run eagerly on the same stream after the replay."""

    MAX_SHAPES = 4   # (clean frame, scores) pairs kept, least recently used first out

    def __init__(self, denoiser):
        self.denoiser = denoiser
        self._bufs = {}

    def buffers(self, shape):
        """(the device uint8 clean frame, the device fp64 scores [4, n] in SCORES order) of one
        image shape (n, h, w, 3): what the last `evaluate` of that shape left."""
        import torch
        dev = self.denoiser.device
        return _lru(self._bufs, tuple(shape),
                    lambda: (torch.empty(shape, dtype=torch.uint8, device=dev),
                             torch.empty((len(SCORES), shape[0]), dtype=torch.float64, device=dev)), self.MAX_SHAPES)

    def evaluate(self, noisy_u8, clean_u8):
        """uint8 [n,h,w,3] (or [h,w,3]) noisy and clean images -> {"psnr_noisy", "psnr_denoised",
        "ssim_noisy", "ssim_denoised"}: fp64 numpy arrays [n] (max_val 255)."""
        import torch
        noisy, clean = np.asarray(noisy_u8), np.asarray(clean_u8)
        if clean.dtype != np.uint8 or clean.shape != noisy.shape:
            raise ValueError(f"evaluate: the clean images ({clean.dtype} {clean.shape}) do not match the noisy ones "
                             f"({noisy.dtype} {noisy.shape})")
        if noisy.ndim == 3:
            noisy, clean = noisy[None], clean[None]
        if noisy.dtype != np.uint8 or noisy.ndim != 4 or noisy.shape[-1] != 3:
            raise ValueError(f"evaluate expects uint8 [n,h,w,3] or [h,w,3], got {noisy.dtype} {noisy.shape}")
        if noisy.shape[0] == 0:
            return {k: np.zeros(0) for k in SCORES}
        f = self.denoiser.run(noisy)
        ref, res = self.buffers(tuple(noisy.shape))
        ref.copy_(torch.from_numpy(np.ascontiguousarray(clean)))
        return self._score(f, ref, res)

    def _score(self, f, ref, res):
        psnr(f.u8_in, ref, out=res[0])
        psnr(f.u8_out, ref, out=res[1])
        ssim(f.u8_in, ref, out=res[2])
        ssim(f.u8_out, ref, out=res[3])
        r = res.cpu().numpy()
        return {k: r[i] for i, k in enumerate(SCORES)}

    def evaluate_degraded(self, clean_u8, jpeg_quality):
        """uint8 [n,h,w,3] (or [h,w,3]) clean images -> the scores of `evaluate` with the noisy
        images made here: the clean frame is uploaded once and its JPEG round trip at
        `jpeg_quality` (dgan.jpeg, the degradation of dataloader.adjust_jpeg_quality) is written
        into the Denoiser frame's `u8_in` on the device."""
        import torch
        from .jpeg import _check_quality, jpeg_roundtrip
        clean = np.asarray(clean_u8)
        if clean.ndim == 3:
            clean = clean[None]
        if clean.dtype != np.uint8 or clean.ndim != 4 or clean.shape[-1] != 3:
            raise ValueError(f"evaluate_degraded expects uint8 [n,h,w,3] or [h,w,3], got {clean.dtype} {clean.shape}")
        quality = _check_quality(jpeg_quality, "evaluate_degraded")
        if clean.shape[0] == 0:
            return {k: np.zeros(0) for k in SCORES}
        f = self.denoiser.frame(*clean.shape[:3])
        ref, res = self.buffers(tuple(clean.shape))
        ref.copy_(torch.from_numpy(np.ascontiguousarray(clean)))
        jpeg_roundtrip(ref, quality, out=f.u8_in)
        self.denoiser.run_frame(f)
        return self._score(f, ref, res)


SR_SCORES = ("psnr_bicubic", "psnr_upscaled", "ssim_bicubic", "ssim_upscaled")


class SREvaluator:
    """Scores an `Upscaler` against high-resolution originals on the device: the original is
    uploaded, degraded by a resize (dgan.resize, the degrade conversion) straight into the
    Upscaler frame's `u8_in`, upscaled into `u8_out`, and the same low-resolution frame resized
    back (the display conversion) is the baseline; both are scored against the original and only
    the 4 n scalars come back.  `method` names the resize of both directions.  With a
    graph-capturing `Upscaler` the resizes and the metrics run eagerly around the replay.
    jpeg_quality Q puts the low-resolution frame through a JPEG round trip at quality Q with 4:2:0
    subsampling (dataloader.jpeg_roundtrip on uint8), in place: codec "device" on the device
    (dgan.jpeg, the same bits), codec "pillow" on the host through Pillow's codec (a read-back, one
    image at a time, and an upload)."""

    MAX_SHAPES = 4   # (original, baseline, scores) triples kept, least recently used first out

    CODECS = ("device", "pillow")

    def __init__(self, upscaler, method="bicubic", jpeg_quality=None, codec="device"):
        from .resize import METHODS
        if method not in METHODS:
            raise ValueError(f"method must be one of {METHODS}, got {method!r}")
        if codec not in self.CODECS:
            raise ValueError(f"codec must be one of {self.CODECS}, got {codec!r}")
        if jpeg_quality is not None and not 1 <= int(jpeg_quality) <= 100:
            raise ValueError(f"jpeg_quality must be in 1..100, got {jpeg_quality}")
        self.upscaler, self.method, self.codec = upscaler, method, codec
        self.jpeg_quality = None if jpeg_quality is None else int(jpeg_quality)
        self._bufs = {}

    def buffers(self, shape):
        """(the device uint8 original, the device uint8 baseline, the device fp64 scores [4, n] in
        SR_SCORES order) of one image shape (n, H, W, 3): what the last `evaluate` of that shape left."""
        import torch
        dev = self.upscaler.device
        return _lru(self._bufs, tuple(shape),
                    lambda: (torch.empty(shape, dtype=torch.uint8, device=dev),
                             torch.empty(shape, dtype=torch.uint8, device=dev),
                             torch.empty((len(SR_SCORES), shape[0]), dtype=torch.float64, device=dev)), self.MAX_SHAPES)

    def _jpeg(self, low):
        """Every image of the device frame `low` through the JPEG round trip, in place."""
        if self.codec == "device":
            from .jpeg import jpeg_roundtrip
            jpeg_roundtrip(low, self.jpeg_quality, out=low)
            return
        import io
        import torch
        from PIL import Image
        host = low.cpu().numpy()
        for i in range(host.shape[0]):
            buf = io.BytesIO()
            Image.fromarray(host[i], "RGB").save(buf, format="JPEG", quality=self.jpeg_quality, subsampling=2)
            buf.seek(0)
            host[i] = np.asarray(Image.open(buf).convert("RGB"), np.uint8)
        low.copy_(torch.from_numpy(host))

    def evaluate(self, hr_u8):
        """uint8 [n,H,W,3] (or [H,W,3]) originals, H and W multiples of the scale and at least 11
        -> {"psnr_bicubic", "psnr_upscaled", "ssim_bicubic", "ssim_upscaled"}: fp64 numpy arrays
        [n] (max_val 255)."""
        import torch
        from .resize import DEGRADE, DISPLAY, resize
        hr = np.asarray(hr_u8)
        if hr.ndim == 3:
            hr = hr[None]
        if hr.dtype != np.uint8 or hr.ndim != 4 or hr.shape[-1] != 3:
            raise ValueError(f"evaluate expects uint8 [n,H,W,3] or [H,W,3], got {hr.dtype} {hr.shape}")
        n, H, W = hr.shape[:3]
        s = self.upscaler.scale
        if H % s or W % s or min(H, W) < SSIM_TAPS:
            raise ValueError(f"evaluate: images of {H}x{W} must be multiples of the scale {s} and at least "
                             f"{SSIM_TAPS}x{SSIM_TAPS}")
        if n == 0:
            return {k: np.zeros(0) for k in SR_SCORES}
        f = self.upscaler.frame(n, H // s, W // s)
        ref, base, res = self.buffers(tuple(hr.shape))
        ref.copy_(torch.from_numpy(np.ascontiguousarray(hr)))
        resize(ref, H // s, W // s, self.method, *DEGRADE, out=f.u8_in)
        if self.jpeg_quality is not None:
            self._jpeg(f.u8_in)
        self.upscaler.run_frame(f)
        resize(f.u8_in, H, W, self.method, *DISPLAY, out=base)
        psnr(base, ref, out=res[0])
        psnr(f.u8_out, ref, out=res[1])
        ssim(base, ref, out=res[2])
        ssim(f.u8_out, ref, out=res[3])
        r = res.cpu().numpy()
        return {k: r[i] for i, k in enumerate(SR_SCORES)}
