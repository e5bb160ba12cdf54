"""The definitions of BM3D's second stage (dgan/filters.py bm3d_wiener_ref, bm3d2_ref): their uint32 /
int32 working types against int64, batches, flat frames, that the second stage improves on the
first, and the argument errors.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest

from test_bm3d import KINDS, frame
from test_filters import noisy

COMBOS = [(1, 3, 2), (25, 7, 16), (40, 21, 16), (1, 21, 8)]


@pytest.mark.parametrize("size", [(1, 1), (2, 30), (17, 23)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_both_references_uint32_equal_int64(size):
    from dgan.filters import bm3d2_ref, bm3d_wiener_ref
    for sigma, search, group in COMBOS:
        for kind in KINDS:
            a, pilot = frame(kind, *size, sigma), frame("noisy", *size, 3)
            got = bm3d_wiener_ref(a, pilot, sigma, search, group, dtype=np.int64)
            assert got.dtype == np.uint8 and got.shape == a.shape
            assert np.array_equal(got, bm3d_wiener_ref(a, pilot, sigma, search, group, dtype=np.uint32)), (sigma, kind)
            assert np.array_equal(bm3d2_ref(a, sigma, search, group, dtype=np.int64),
                                  bm3d2_ref(a, sigma, search, group, dtype=np.uint32)), (sigma, search, group, kind)


def test_a_batch_equals_its_single_images():
    from dgan.filters import bm3d2_ref, bm3d_wiener_ref
    imgs = np.stack([frame(kind, 17, 23, 25) for kind in KINDS])
    pilots = imgs[::-1].copy()
    got, both = bm3d_wiener_ref(imgs, pilots, 25, 7, 8), bm3d2_ref(imgs, 25, 7, 8)
    for i in range(3):
        assert np.array_equal(got[i], bm3d_wiener_ref(imgs[i], pilots[i], 25, 7, 8))
        assert np.array_equal(both[i], bm3d2_ref(imgs[i], 25, 7, 8))


@pytest.mark.parametrize("value", [0, 7, 77, 255])
def test_a_flat_frame_comes_back_unchanged(value):
    from dgan.filters import bm3d2_ref, bm3d_wiener_ref
    f = np.full((2, 9, 12, 3), value, np.uint8)
    assert np.array_equal(bm3d_wiener_ref(f, f), f) and np.array_equal(bm3d2_ref(f), f)


def test_the_second_stage_improves_on_the_first():
    """A sanity condition with no margin set (the figures: DESIGN.md, BM3D, second stage)."""
    from dgan.filters import bm3d2_ref, bm3d_ref
    a, clean = noisy(48, 64, 25.0), noisy(48, 64, 0.0).astype(np.float64)
    assert np.mean((bm3d2_ref(a) - clean) ** 2) < np.mean((bm3d_ref(a) - clean) ** 2)


def test_bad_arguments_raise():
    from dgan.filters import bm3d2_ref, bm3d_wiener_ref
    a = noisy(8, 8, 5.0)
    for pilot in (a[:7], a[None], np.stack([a, a])):
        with pytest.raises(ValueError, match="pilot"):
            bm3d_wiener_ref(a, pilot)
    for kw, name in (({"sigma": 0}, "sigma"), ({"sigma": 41}, "sigma"), ({"search": 8}, "search"), ({"group": 32}, "group"),
                     ({"dtype": np.int32}, "dtype")):
        with pytest.raises(ValueError, match=name):
            bm3d_wiener_ref(a, a, **kw)
        with pytest.raises(ValueError, match=name):
            bm3d2_ref(a, **kw)
    with pytest.raises(ValueError, match="uint8"):
        bm3d_wiener_ref(a, a.astype(np.float32))


def test_the_bm3d_flags_go_with_bm3d2_too():
    from evaluate import baseline_args
    flags = dict(baseline="bm3d2", nlm_h=10, nlm_template=7, nlm_search=21, bm3d_sigma=9, bm3d_search=7, bm3d_group=8)
    assert baseline_args(SimpleNamespace(**flags)) == {"sigma": 9, "search": 7, "group": 8}
    for bad, name in ((dict(bm3d_sigma=41), "sigma"), (dict(bm3d_group=5), "group"),
                      (dict(baseline="median3"), "need --baseline bm3d"), (dict(nlm_h=5), "need --baseline nlm")):
        with pytest.raises(ValueError, match=name):
            baseline_args(SimpleNamespace(**dict(flags, **bad)))
