"""The classical filters' definitions (dgan/filters.py): median3_ref against scipy, nlm_ref's
32-bit working type against the 64-bit one, the weight table, and the argument errors.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest

SIGMA = {3: 1.0, 10: 5.0, 30: 15.0, 40: 15.0}   # the noise a strength h is meant for
COMBOS = [(t, s, h) for t, s in ((3, 7), (5, 11), (7, 21)) for h in (3, 10, 30)]


def noisy(h, w, sigma, seed=0):
    """uint8 [h,w,3]: a smooth pattern (waves, a ramp) plus Gaussian noise of `sigma`."""
    rng = np.random.Generator(np.random.PCG64(1000 * h + w + seed))
    y, x = np.mgrid[0:h, 0:w]
    g = np.stack([128 + 100 * np.sin(x / 5.0) * np.cos(y / 7.0), 40 + 2.5 * x + 0 * y, 200 - 1.5 * y - x], -1)
    return np.clip(np.rint(g + sigma * rng.standard_normal(g.shape)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("size", [(1, 1), (1, 9), (9, 1), (3, 4), (17, 23)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_median3_ref_equals_scipy(size):
    import scipy.ndimage as ndi
    from dgan.filters import median3_ref
    a = np.stack([noisy(*size, 15.0), np.random.default_rng(1).integers(0, 256, size + (3,), dtype=np.uint8)])
    got = median3_ref(a)
    assert got.dtype == np.uint8 and got.shape == a.shape
    for i in range(2):
        assert np.array_equal(got[i], ndi.median_filter(a[i], size=(3, 3, 1), mode="nearest"))
    assert np.array_equal(median3_ref(a[0]), got[0])


@pytest.mark.parametrize("size", [(1, 1), (2, 30), (17, 23)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_nlm_ref_int32_equals_int64_and_acts_on_the_image(size):
    from dgan.filters import nlm_ref
    for t, s, h in COMBOS:
        a = noisy(*size, SIGMA[h])
        got = nlm_ref(a, h, t, s, dtype=np.int64)
        assert got.dtype == np.uint8 and got.shape == a.shape
        assert np.array_equal(got, nlm_ref(a, h, t, s, dtype=np.int32)), (t, s, h)
        assert np.array_equal(got, nlm_ref(a[None], h, t, s)[0])
        if min(size) >= 16:
            assert (got != a).any(axis=-1).mean() >= 0.25, (t, s, h)


@pytest.mark.parametrize("value", [0, 77, 255])
def test_a_flat_frame_comes_back_unchanged(value):
    from dgan.filters import median3_ref, nlm_ref
    a = np.full((2, 9, 12, 3), value, np.uint8)
    assert np.array_equal(median3_ref(a), a) and np.array_equal(nlm_ref(a, 10, 5, 9), a)


@pytest.mark.parametrize("h", [1, 3, 10, 30, 40])
def test_nlm_table(h):
    from dgan.filters import nlm_table
    W = nlm_table(h)
    assert W[0] == 16384 and W[-1] == 0 and (W[:-1] > 0).all() and (np.diff(W) <= 0).all()
    assert abs(len(W) - (10.4 * h * h + 2)) <= 0.01 * h * h + 1
    if h == 10:
        assert len(W) == 1041
    i = np.arange(len(W))
    assert np.array_equal(W, np.floor(16384 * np.exp(-i / float(h * h)) + 0.5))


def test_bad_arguments_raise():
    from dgan.filters import median3_ref, nlm_ref, nlm_table
    a = noisy(8, 8, 5.0)
    for f in (median3_ref, nlm_ref):
        with pytest.raises(ValueError, match="uint8"):
            f(a.astype(np.float32))
        with pytest.raises(ValueError, match="uint8"):
            f(a[..., :1])
        with pytest.raises(ValueError, match="empty"):
            f(np.zeros((0, 8, 3), np.uint8))
    for h in (0, 41, 10.0, None, True):
        with pytest.raises(ValueError, match="h must"):
            nlm_table(h)
    for kw, name in (({"template": 4}, "template"), ({"template": 9}, "template"), ({"search": 8}, "search"),
                     ({"search": 23}, "search"), ({"search": 1}, "search"), ({"h": 0}, "h must")):
        with pytest.raises(ValueError, match=name):
            nlm_ref(a, **kw)
    with pytest.raises(ValueError, match="dtype"):
        nlm_ref(a, dtype=np.int16)


def test_the_baseline_flags_are_checked_before_anything_runs():
    from evaluate import baseline_args
    flags = dict(baseline="nlm", nlm_h=10, nlm_template=7, nlm_search=21)
    assert baseline_args(SimpleNamespace(**flags)) == {"h": 10, "template": 7, "search": 21}
    assert baseline_args(SimpleNamespace(**dict(flags, baseline="median3"))) == {}
    for bad, name in ((dict(nlm_h=41), "h must"), (dict(nlm_template=4), "template"), (dict(nlm_search=22), "search"),
                      (dict(baseline=None, nlm_h=5), "need --baseline nlm")):
        with pytest.raises(ValueError, match=name):
            baseline_args(SimpleNamespace(**dict(flags, **bad)))
