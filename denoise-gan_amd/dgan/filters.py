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

    bm3d       stage 1 (hard thresholding) of BM3D with the unnormalised Walsh-Hadamard transform in
               all three dimensions: `bm3d_ref` states it in full.

    bm3d_wiener  stage 2 (the collaborative Wiener filter) on a pilot estimate: `bm3d_wiener_ref`.
    bm3d2      both stages, stage 1's output as the pilot: `bm3d2_ref`.

    dejpeg     JPEG artifact removal by shift-averaged re-application (Nosratinia 2001) with the
               round trip of dgan.jpeg (4:2:0, quality Q in 1..100 or two tables t): for each of the
               64 shifts (dy, dx) in 0..7 x 0..7
                   s = the frame with its first row repeated dy times above and its first column dx
                       times to the left, (h + dy) x (w + dx)
                   r = roundtrip(s)[dy:, dx:], the round trip on the shifted frame's own geometry
                       (its replication to multiples of 8, ch = ceil((h + dy) / 2), cw = ceil((w + dx)
                       / 2), the bias by the shifted column's parity, the upsampler's clamps at
                       ch - 1 / cw - 1, replication when cw <= 2)
               and out = (sum of the 64 r + 32) >> 6.  The sum is at most 64 * 255: int32 holds
               everything (`dejpeg_ref` takes the working type; tests/test_dejpeg.py holds int32 equal
               to int64).

`dejpeg` takes the quality (or the tables) the frame was coded with.  It is NOT a deblocker that
estimates them from the pixels, and it is not claimed equal to any other implementation of
re-application.

`nlm` is the non-local means of Buades et al. with one weight for the three channels.  It is NOT
claimed equal to cv2.fastNlMeansDenoisingColored, which filters in Lab with separate luminance and
colour strengths and its own fixed-point weights.

`bm3d` is BM3D (Dabov et al.) with a Hadamard transform, a known cheap variant.  It is NOT the
Bior / DCT profile of the original paper and is not claimed equal to any other implementation.

`median3_ref` / `nlm_table` / `nlm_ref` / `bm3d_ref` / `bm3d_wiener_ref` / `bm3d2_ref` / `dejpeg_ref` are pure numpy and import neither torch nor the library.
"""
import math

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
# BM3D, stage 1
# ---------------------------------------------------------------------------
PATCH = 8                 # the patch is 8 x 8
STEP = 3                  # reference patches every 3 pixels, from -7
MAX_SIGMA = 40
GROUPS = (2, 4, 8, 16)    # K: the most patches of a group
MATCH_BOUND = 480000      # a candidate matches when D <= 2500 per sample * 192 samples
ESTIMATE_MAX = 1020       # an estimate carries two fraction bits
WEIGHT_SCALE = 1024       # w = max(1, 1024 // N)
_NO_KEY = (1 << 31) - 1   # the sort key of a candidate that does not match


def check_bm3d(sigma, search, group, what="bm3d"):
    """(sigma, search, group) as ints, or ValueError naming the bad one."""
    for name, v in (("sigma", sigma), ("search", search), ("group", group)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what}: {name} must be an integer, got {v!r}")
    if not 1 <= sigma <= MAX_SIGMA:
        raise ValueError(f"{what}: sigma must be in 1..{MAX_SIGMA}, got {sigma}")
    if not 3 <= search <= MAX_SEARCH or search % 2 == 0:
        raise ValueError(f"{what}: search must be odd in 3..{MAX_SEARCH}, got {search}")
    if group not in GROUPS:
        raise ValueError(f"{what}: group must be one of {GROUPS}, got {group}")
    return int(sigma), int(search), int(group)


def hadamard(n):
    """int64 [n,n]: the unnormalised Walsh-Hadamard matrix in Sylvester order, n a power of two."""
    H = np.ones((1, 1), np.int64)
    while len(H) < n:
        H = np.block([[H, H], [H, -H]])
    return H


def bm3d_threshold(sigma, m):
    """T(sigma, m) = isqrt(729 sigma^2 64 m // 100): 2.7 sigma on the scale of the unnormalised
    transform of m x 8 x 8 values, whose coefficients carry a gain of sqrt(64 m)."""
    return math.isqrt(729 * sigma * sigma * PATCH * PATCH * m // 100)


def _wht3(G, Hm, H8):
    """The transform of [g,m,8,8,3] along the group, the rows and the columns."""
    G = np.einsum("ab,gbijc->gaijc", Hm, G)
    G = np.einsum("ab,gkbjc->gkajc", H8, G)
    return np.einsum("ab,gkibc->gkiac", H8, G)


def _bm3d_groups(P, H, W, s, K, bound, wt):
    """The groups of one padded image P [H+2R, W+2R, 3] (R = s // 2 + 7, type wt), matched on P at
    D <= bound: (m, Y, X) per group size m, Y and X [g,m,8,8] the members' pixels in P."""
    rs = s // 2
    R = rs + PATCH - 1
    ri, rj = np.arange(1 - PATCH, H, STEP) + R, np.arange(1 - PATCH, W, STEP) + R   # reference corners in P
    eh, ew = ri[-1] - ri[0] + PATCH, rj[-1] - rj[0] + PATCH                           # what their patches cover
    ar = np.arange(PATCH)
    base = P[rs:rs + eh, rs:rs + ew]
    keys = np.empty((s * s, len(ri), len(rj)), wt)
    for idx in range(s * s):
        dy, dx = idx // s - rs, idx % s - rs
        e = ((base - P[rs + dy:rs + dy + eh, rs + dx:rs + dx + ew]) ** 2).sum(-1, dtype=wt)
        v = sum(e[k:k + eh - PATCH + 1:STEP] for k in range(PATCH))
        D = sum(v[:, k:k + ew - PATCH + 1:STEP] for k in range(PATCH))
        ok = (D <= bound) & bool(dy or dx)
        keys[idx] = np.where(ok, (np.where(ok, D, 0) << 9) | idx, _NO_KEY)   # (D, idx) order in one integer
    keys = np.sort(keys, axis=0)[:K - 1]
    taken = (keys != _NO_KEY).sum(0)
    ms = 1 << np.floor(np.log2(1 + taken)).astype(np.int64)   # (1 + taken <= 16: exact)
    for m in sorted(set(ms.ravel().tolist())):
        ya, xb = np.nonzero(ms == m)
        idx = np.concatenate([np.full((1, len(ya)), (s * s) // 2, wt), keys[:m - 1, ya, xb] & 511]).T   # [g,m]
        Y = (ri[ya][:, None] + idx // s - rs)[:, :, None, None] + ar[:, None]
        X = (rj[xb][:, None] + idx % s - rs)[:, :, None, None] + ar[None, :]
        yield (m,) + tuple(np.broadcast_arrays(Y, X))


def _bm3d_setup(a, sigma, search, group, dtype, what):
    """The checked parameters, the working type, the pad R and the padded rows / columns."""
    from .infer import pad_index
    if np.dtype(dtype) not in (np.dtype(np.int64), np.dtype(np.uint32)):
        raise ValueError(f"{what}: dtype must be np.int64 or np.uint32, got {dtype!r}")
    sigma, s, K = check_bm3d(sigma, search, group, what)
    wt = np.int32 if np.dtype(dtype) == np.dtype(np.uint32) else np.int64   # everything but num / den
    H, W = a.shape[1:3]
    R = s // 2 + PATCH - 1
    rows, cols = pad_index(np.arange(-R, H + R), H, "reflect"), pad_index(np.arange(-R, W + R), W, "reflect")
    return sigma, s, K, wt, R, rows, cols


def bm3d_sums(img_u8, sigma=25, search=21, group=16, dtype=np.int64):
    """(num, den) of `bm3d_ref`, [n,h,w,3] each in the accumulator type: the weighted sum of the
    estimates (two fraction bits) and the sum of the weights.  den >= 1 everywhere."""
    a, _ = _images(img_u8, "bm3d_ref")
    sigma, s, K, wt, R, rows, cols = _bm3d_setup(a, sigma, search, group, dtype, "bm3d_ref")
    n, H, W = a.shape[:3]
    H8 = hadamard(PATCH).astype(wt)
    num, den = np.zeros((n, H, W, 3), dtype), np.zeros((n, H, W, 3), dtype)
    for b in range(n):
        P = a[b][rows][:, cols].astype(wt)
        numP, denP = np.zeros(P.shape, dtype), np.zeros(P.shape, dtype)
        for m, Y, X in _bm3d_groups(P, H, W, s, K, MATCH_BOUND, wt):
            Hm, shift = hadamard(m).astype(wt), 4 + m.bit_length() - 1
            C = _wht3(P[Y, X], Hm, H8)
            assert np.abs(C).max() < 1 << 19
            keep = np.abs(C) > bm3d_threshold(sigma, m)
            keep[:, 0, 0, 0] = True
            wgt = np.maximum(1, WEIGHT_SCALE // keep.sum((1, 2, 3), dtype=wt))[:, None, None, None]   # [g,1,1,1,3]
            E = np.clip((_wht3(np.where(keep, C, 0), Hm, H8) + 8 * m) >> shift, 0, ESTIMATE_MAX)
            np.add.at(numP, (Y, X), (wgt * E).astype(dtype))
            np.add.at(denP, (Y, X), np.broadcast_to(wgt, E.shape).astype(dtype))
        num[b], den[b] = numP[R:R + H, R:R + W], denP[R:R + H, R:R + W]   # members' pixels outside the image drop
    assert den.min() >= 1 and den.max() < 1 << 22 and int(num.max()) < 1 << 32
    return num, den


def bm3d_ref(img_u8, sigma=25, search=21, group=16, dtype=np.int64):
    """Stage 1 of BM3D (block matching, hard thresholding of the group's 3-D transform, aggregation)
    with the unnormalised Walsh-Hadamard transform, Sylvester order, in all three dimensions, as
    exact integers: uint8 [n,h,w,3] or [h,w,3] -> the same shape and dtype.  BM3D with a Hadamard
    transform is a known variant; it is NOT the Bior / DCT profile of Dabov et al.

    sigma 1..40, search s odd in 3..21 (rs = s // 2), group K in {2, 4, 8, 16}; patches 8 x 8.
    P: the image padded by rs + 7 with np.pad's "reflect" (dgan.infer.pad_index, any pad width).
    Reference patches have their corners at (i, j) = (-7 + 3a, -7 + 3b), i <= h-1, j <= w-1, so
    every pixel lies in one.  The candidates of a reference are the s*s patches at (i+dy, j+dx),
    |dy|, |dx| <= rs, idx = (dy+rs) s + dx+rs, D = the sum over the patch and the three channels of
    the squared difference (< 2^24; joint over RGB).  The group is the reference itself followed by
    the first m-1 of the candidates with d != 0 and D <= 480000 in ascending (D, idx), where up to
    K-1 are taken and m is the largest power of two <= 1 + the number taken.  Per channel the
    m x 8 x 8 integers are transformed; a coefficient c stays iff |c| > T = isqrt(729 sigma^2 64 m
    // 100) or it is the DC coefficient, N of them; the same transform again gives v = 64 m times the
    estimate, E = clamp((v + 8m) >> (4 + log2 m), 0, 1020) (a floor shift; two fraction bits).
    Every pixel of every member inside the image adds w E to num and w = max(1, 1024 // N) to den;
    out = (num + 2 den) // (4 den).

    Bounds: a patch position is taken by at most 7^2 = 49 references and a pixel lies in 64
    positions: at most 3136 contributions, num <= 3136 * 1024 * 1020 < 2^32, den < 2^22,
    coefficients < 2^19.  dtype np.uint32 runs num / den in uint32 and everything else in int32
    and equals np.int64 (tests/test_bm3d.py); the bounds are asserted on every call."""
    single = np.asarray(img_u8).ndim == 3
    num, den = bm3d_sums(img_u8, sigma, search, group, dtype)
    out = ((num + 2 * den) // (4 * den)).astype(np.uint8)
    return out[0] if single else out


# ---------------------------------------------------------------------------
# BM3D, stage 2
# ---------------------------------------------------------------------------
MATCH_BOUND2 = 76800      # a candidate matches when the pilot's D <= 400 per sample * 192 samples
ENERGY_MAX = 1 << 23      # the pilot's energy is clamped here: Wq is 256 from here on for sigma <= 40
WIENER_ONE = 256          # the Wiener weight Wq carries eight fraction bits


def bm3d_wiener_sums(noisy_u8, pilot_u8, sigma=25, search=21, group=16, dtype=np.int64):
    """(num, den) of `bm3d_wiener_ref`, as `bm3d_sums` returns them."""
    what = "bm3d_wiener_ref"
    a, _ = _images(noisy_u8, what)
    p, _ = _images(pilot_u8, what)
    if np.shape(noisy_u8) != np.shape(pilot_u8):
        raise ValueError(f"{what}: the pilot {np.shape(pilot_u8)} does not match the noisy images {np.shape(noisy_u8)}")
    sigma, s, K, wt, R, rows, cols = _bm3d_setup(a, sigma, search, group, dtype, what)
    n, H, W = a.shape[:3]
    H8 = hadamard(PATCH).astype(wt)
    num, den = np.zeros((n, H, W, 3), dtype), np.zeros((n, H, W, 3), dtype)
    for b in range(n):
        Pz, Py = a[b][rows][:, cols].astype(wt), p[b][rows][:, cols].astype(wt)
        numP, denP = np.zeros(Pz.shape, dtype), np.zeros(Pz.shape, dtype)
        for m, Y, X in _bm3d_groups(Py, H, W, s, K, MATCH_BOUND2, wt):
            Hm, lg = hadamard(m).astype(wt), m.bit_length() - 1
            Cy, Cz = _wht3(Py[Y, X], Hm, H8), _wht3(Pz[Y, X], Hm, H8)
            assert max(np.abs(Cy).max(), np.abs(Cz).max()) < 1 << 18
            e = Cy.astype(np.int64) ** 2 >> (6 + lg)            # the one 64-bit product: < 2^36, e < 2^26
            assert e.max() < 1 << 26
            e = np.minimum(e, ENERGY_MAX).astype(np.uint32)
            d = e + np.uint32(sigma * sigma)
            Wq = ((WIENER_ONE * e + d // 2) // d).astype(wt)    # 256 e + d // 2 < 2^32
            Wq[:, 0, 0, 0] = WIENER_ONE
            assert Wq.min() >= 0 and Wq.max() <= WIENER_ONE
            F = (Wq * Cz + WIENER_ONE // 2) >> 8
            assert (np.abs(F) <= np.abs(Cz)).all()
            v = _wht3(F, Hm, H8)
            assert np.abs(v).max() <= 1 << 28
            E = np.clip((v + 8 * m) >> (4 + lg), 0, ESTIMATE_MAX)
            N2 = np.maximum(1, ((Wq * Wq).sum((1, 2, 3), dtype=wt) + (1 << 15)) >> 16)
            assert N2.max() <= 1024
            wgt = np.maximum(1, WEIGHT_SCALE // N2)[:, None, None, None]   # [g,1,1,1,3]
            np.add.at(numP, (Y, X), (wgt * E).astype(dtype))
            np.add.at(denP, (Y, X), np.broadcast_to(wgt, E.shape).astype(dtype))
        num[b], den[b] = numP[R:R + H, R:R + W], denP[R:R + H, R:R + W]
    assert den.min() >= 1 and den.max() < 1 << 22 and int(num.max()) < 1 << 32
    return num, den


def bm3d_group_sizes(pilot_u8, search=21, group=16):
    """{m: the number of groups of that size} that stage 2's matching forms on one pilot [h,w,3]."""
    a, single = _images(pilot_u8, "bm3d_group_sizes")
    if not single:
        raise ValueError(f"bm3d_group_sizes: expected one image [h,w,3], got {a.shape}")
    _, s, K, wt, _, rows, cols = _bm3d_setup(a, 1, search, group, np.int64, "bm3d_group_sizes")
    return {m: len(Y) for m, Y, _ in _bm3d_groups(a[0][rows][:, cols].astype(wt), *a.shape[1:3], s, K, MATCH_BOUND2, wt)}


def bm3d_wiener_ref(noisy_u8, pilot_u8, sigma=25, search=21, group=16, dtype=np.int64):
    """Stage 2 of BM3D (block matching on a pilot estimate, a Wiener weight per coefficient of the
    group's 3-D transform, aggregation) as exact integers: uint8 [n,h,w,3] or [h,w,3] twice, of the
    same shape -> that shape and dtype.  Everything not said here is `bm3d_ref`'s.

    D is the squared difference of PILOT patches, and a candidate matches iff D <= 76800; both
    images are padded with the same indices and the group's positions serve both.  Per channel,
    Cy = the transform of the pilot's m x 8 x 8 integers, Cz of the noisy ones (|C| <= 255 * 64 m <
    2^18).  With lg = log2 m: e = min((Cy Cy) >> (6 + lg), 2^23), the pilot's energy on the
    normalised scale (the product < 2^36; e < 2^26 before the clamp); d = e + sigma^2;
    Wq = (256 e + d // 2) // d in 0..256 (256 e + d // 2 < 2^32; every e >= 2^23 gives 256 for
    sigma <= 40, so the clamp loses nothing), and Wq = 256 for the DC coefficient, which returns a
    flat frame unchanged.  F = (Wq Cz + 128) >> 8 (a floor shift, |F| <= |Cz|); v = the transform of
    F (|v| <= 2^28); E = clamp((v + 8m) >> (4 + lg), 0, 1020).  The group's weight per channel:
    N2 = max(1, (sum Wq^2 + 2^15) >> 16) in 1..1024, w = max(1, 1024 // N2).  num, den and the output
    as in `bm3d_ref`, with its bounds.

    dtype np.uint32 runs num / den in uint32, the Cy Cy product in 64 bits, the division in uint32
    and everything else in int32, and equals np.int64 (tests/test_bm3d2.py); the bounds are
    asserted on every call."""
    single = np.asarray(noisy_u8).ndim == 3
    num, den = bm3d_wiener_sums(noisy_u8, pilot_u8, sigma, search, group, dtype)
    out = ((num + 2 * den) // (4 * den)).astype(np.uint8)
    return out[0] if single else out


def bm3d2_ref(img_u8, sigma=25, search=21, group=16, dtype=np.int64):
    """Both stages of BM3D with one set of parameters: `bm3d_wiener_ref` with `bm3d_ref`'s output as
    the pilot."""
    return bm3d_wiener_ref(img_u8, bm3d_ref(img_u8, sigma, search, group, dtype), sigma, search, group, dtype)


# ---------------------------------------------------------------------------
# JPEG artifact removal: shift-averaged re-application
# ---------------------------------------------------------------------------
def check_dejpeg(quality, tables, what="dejpeg"):
    """The uint8 [2,64] tables of a call: `tables` checked, or those of `quality`; ValueError naming
    the bad argument."""
    from .jpeg import _check_quality, quant_tables
    quality = _check_quality(quality, what)
    if tables is None:
        return quant_tables(quality)
    t = np.asarray(tables)
    if t.dtype != np.uint8 or t.shape != (2, 64) or int(t.min()) < 1:
        raise ValueError(f"{what}: tables must be uint8 [2,64] with entries >= 1, got {t.dtype} {t.shape}")
    return np.ascontiguousarray(t)


def dejpeg_ref(img_u8, quality=50, tables=None, dtype=np.int64):
    """The definition on the host: uint8 [n,h,w,3] or [h,w,3] -> the same shape and dtype (module
    docstring).  tables: uint8 [2,64], row-major, entries >= 1, in place of quant_tables(quality)
    (a file's own: jpeg_parse(data).quant).  dtype: the working integer type, np.int64 or np.int32."""
    from .jpeg import _roundtrip
    a, single = _images(img_u8, "dejpeg_ref", dtype)
    tables = check_dejpeg(quality, tables, "dejpeg_ref")
    acc = np.zeros(a.shape, dtype)
    for dy in range(8):
        for dx in range(8):
            s = np.pad(a, ((0, 0), (dy, 0), (dx, 0), (0, 0)), mode="edge")
            acc += _roundtrip(s, tables, dtype)[:, dy:, dx:]
    out = ((acc + 32) >> 6).astype(np.uint8)
    return out[0] if single else out


# ---------------------------------------------------------------------------
# device code below: torch and the library are imported on use
# ---------------------------------------------------------------------------
MAX_PLANS = 8   # plans kept over all filters, least recently used first out (metrics._lru)
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


def bm3d(x, sigma=25, search=21, group=16, out=None):
    """A dense uint8 NHWC device tensor [n,h,w,3] -> stage 1 of BM3D, equal to `bm3d_ref` bit for
    bit.  `out` as in `median3`.  The uint32 accumulators (num and den, 24 bytes a pixel) are kept
    with the output buffers; a repeated call allocates nothing, does no host sync and can be
    captured in a graph."""
    import torch
    from . import ops
    from .metrics import _lru
    sigma, search, group = check_bm3d(sigma, search, group)
    out = _device_pair(x, out, "bm3d")
    if x.shape[0] == 0:
        return out
    ws = _lru(_plans, ("bm3d sums",) + tuple(x.shape[:3]) + (x.device,),
              lambda: torch.empty(2 * x.numel(), dtype=torch.int32, device=x.device), MAX_PLANS)
    return ops.bm3d(x, out, ws, sigma, search, group)


def bm3d_wiener(x, pilot, sigma=25, search=21, group=16, out=None):
    """Dense uint8 NHWC device tensors [n,h,w,3], the noisy frame and a pilot estimate of the clean
    one (stage 1's output, or any other: a network's) -> stage 2 of BM3D, equal to
    `bm3d_wiener_ref` bit for bit.  `out` as in `median3`, and never the pilot either (the plan keeps
    a third buffer for the call whose two inputs are its first two).  The accumulators are the ones
    `bm3d` keeps; a repeated call allocates nothing, does no host sync and can be captured."""
    import torch
    from . import ops
    from .metrics import _lru
    sigma, search, group = check_bm3d(sigma, search, group, "bm3d_wiener")
    if not isinstance(pilot, torch.Tensor) or pilot.dtype != torch.uint8 or not isinstance(x, torch.Tensor) \
            or pilot.shape != x.shape or pilot.device != x.device or not pilot.is_contiguous():
        raise ValueError(f"bm3d_wiener: the pilot must be a dense uint8 tensor like the input, got "
                         f"{getattr(pilot, 'dtype', type(pilot))} {tuple(getattr(pilot, 'shape', ()))}")
    if out is pilot:
        raise ValueError("bm3d_wiener: out must not be the pilot")
    given = out is not None
    out = _device_pair(x, out, "bm3d_wiener")
    if x.shape[0] == 0:
        return out
    if not given and out.data_ptr() == pilot.data_ptr():
        bufs = _plans[("bm3d_wiener",) + tuple(x.shape[:3]) + (x.device,)]
        while len(bufs) < 3:
            bufs.append(torch.empty_like(x))
        out = next(b for b in bufs if b.data_ptr() not in (x.data_ptr(), pilot.data_ptr()))
    ws = _lru(_plans, ("bm3d sums",) + tuple(x.shape[:3]) + (x.device,),
              lambda: torch.empty(2 * x.numel(), dtype=torch.int32, device=x.device), MAX_PLANS)
    return ops.bm3d_wiener(x, pilot, out, ws, sigma, search, group)


def bm3d2(x, sigma=25, search=21, group=16, out=None):
    """A dense uint8 NHWC device tensor [n,h,w,3] -> both stages of BM3D, equal to `bm3d2_ref` bit
    for bit: `bm3d` into a pilot buffer kept with the plans, then `bm3d_wiener`.  `out` as in
    `median3`; a repeated call allocates nothing, does no host sync and can be captured."""
    import torch
    from .metrics import _lru
    sigma, search, group = check_bm3d(sigma, search, group, "bm3d2")
    out = _device_pair(x, out, "bm3d2")
    if x.shape[0] == 0:
        return out
    pilot = _lru(_plans, ("bm3d2 pilot",) + tuple(x.shape[:3]) + (x.device,), lambda: torch.empty_like(x), MAX_PLANS)
    return bm3d_wiener(x, bm3d(x, sigma, search, group, out=pilot), sigma, search, group, out=out)


def dejpeg(x, quality=50, tables=None, out=None):
    """A dense uint8 NHWC device tensor [n,h,w,3] -> its shift-averaged re-application at `quality`
    (or with the uint8 [2,64] `tables`), equal to `dejpeg_ref` bit for bit.  `out` as in `median3`.
    One launch, no workspace; the 128 table bytes ride in the kernel's arguments, so there is no
    device table to upload or keep: a repeated call allocates nothing, does no host sync and can be
    captured in a graph."""
    from . import ops
    tables = check_dejpeg(quality, tables)
    out = _device_pair(x, out, "dejpeg")
    return ops.dejpeg(x, out, tables) if x.shape[0] else out
