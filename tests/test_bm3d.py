"""The BM3D definition (dgan/filters.py bm3d_ref): its uint32 / int32 working types against int64,
batches, flat frames, that it denoises at all, and the argument errors.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest

from test_filters import noisy

KINDS = ("noisy", "random", "stripes")


def frame(kind, h, w, sigma):
    """uint8 [h,w,3]: the smooth pattern plus noise; uniform random bytes (few candidates pass the
    match bound: m takes 1, 2, 4); stripes of period 3 (many candidates tie at D = 0: idx decides)."""
    if kind == "noisy":
        return noisy(h, w, float(sigma))
    if kind == "random":
        return np.random.default_rng(h * 100 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return np.broadcast_to(np.array([20, 130, 240], np.uint8)[np.arange(w) % 3][None, :, None], (h, w, 3)).copy()


@pytest.mark.parametrize("size", [(1, 1), (2, 30), (17, 23), (40, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_bm3d_ref_uint32_equals_int64(size):
    from dgan.filters import bm3d_ref
    combos = [(5, 3, 2), (25, 7, 16), (40, 21, 16), (25, 21, 2), (5, 21, 16), (40, 3, 16)]
    for sigma, search, group in combos:
        for kind in KINDS:
            a = frame(kind, *size, sigma)
            got = bm3d_ref(a, sigma, search, group, dtype=np.int64)
            assert got.dtype == np.uint8 and got.shape == a.shape
            assert np.array_equal(got, bm3d_ref(a, sigma, search, group, dtype=np.uint32)), (sigma, search, group, kind)


def test_a_batch_equals_its_single_images_and_den_is_positive():
    from dgan.filters import bm3d_ref, bm3d_sums
    imgs = np.stack([frame(kind, 17, 23, 25) for kind in KINDS])
    got = bm3d_ref(imgs, 25, 7, 8)
    for i in range(3):
        assert np.array_equal(got[i], bm3d_ref(imgs[i], 25, 7, 8))
    assert bm3d_sums(imgs, 25, 7, 8)[1].min() >= 1


@pytest.mark.parametrize("value", [0, 77, 255])
def test_a_flat_frame_comes_back_unchanged(value):
    from dgan.filters import bm3d_ref
    a = np.full((2, 9, 12, 3), value, np.uint8)
    assert np.array_equal(bm3d_ref(a), a)


def test_bm3d_ref_denoises():
    """A sanity condition, not a quality bar (the margin over nlm_ref: DESIGN.md)."""
    from dgan.filters import bm3d_ref
    a, clean = noisy(48, 64, 25.0), noisy(48, 64, 0.0).astype(np.float64)
    got = bm3d_ref(a)
    assert (got != a).any(axis=-1).mean() >= 0.25
    assert np.mean((got - clean) ** 2) < np.mean((a - clean) ** 2)   # a higher PSNR against the clean frame


def test_bad_arguments_raise():
    from dgan.filters import bm3d_ref, check_bm3d
    a = noisy(8, 8, 5.0)
    for kw, name in (({"sigma": 0}, "sigma"), ({"sigma": 41}, "sigma"), ({"sigma": 2.5}, "sigma"), ({"search": 8}, "search"),
                     ({"search": 23}, "search"), ({"group": 3}, "group"), ({"group": 32}, "group")):
        with pytest.raises(ValueError, match=name):
            bm3d_ref(a, **kw)
        with pytest.raises(ValueError, match=name):
            check_bm3d(**dict(dict(sigma=25, search=21, group=16), **kw))
    for bad in (a.astype(np.float32), a[..., :1]):
        with pytest.raises(ValueError, match="uint8"):
            bm3d_ref(bad)
    with pytest.raises(ValueError, match="dtype"):
        bm3d_ref(a, dtype=np.int32)
    assert check_bm3d(25, 21, 16) == (25, 21, 16)


def test_the_bm3d_flags_are_checked_before_anything_runs():
    from evaluate import baseline_args
    flags = dict(baseline="bm3d", nlm_h=10, nlm_template=7, nlm_search=21, bm3d_sigma=9, bm3d_search=7, bm3d_group=8)
    assert baseline_args(SimpleNamespace(**flags)) == {"sigma": 9, "search": 7, "group": 8}
    assert baseline_args(SimpleNamespace(baseline="bm3d", nlm_h=10, nlm_template=7, nlm_search=21)) == {
        "sigma": 25, "search": 21, "group": 16}
    for bad, name in ((dict(bm3d_sigma=41), "sigma"), (dict(bm3d_search=4), "search"), (dict(bm3d_group=5), "group"),
                      (dict(baseline="nlm"), "need --baseline bm3d"), (dict(nlm_h=5), "need --baseline nlm")):
        with pytest.raises(ValueError, match=name):
            baseline_args(SimpleNamespace(**dict(flags, **bad)))
