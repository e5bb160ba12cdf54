"""The fp64 numpy references of dgan/metrics.py (no GPU, no library): ssim_ref against an
independent restatement, the closed forms of tiny and constant images, the error cases, and the
file pairing of evaluate.py."""
import numpy as np
import pytest


def _restated_ssim(a, b, max_val):
    """tf.image.ssim's defaults restated differently: one depthwise 2-D convolution with the
    11 x 11 outer-product window (torch fp64) and var = E[x^2] - mu^2, per term."""
    import torch
    import torch.nn.functional as F
    i = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(i * i) / (2 * 1.5 ** 2))
    g = g / g.sum()
    C = a.shape[-1]
    win = torch.outer(g, g)[None, None].repeat(C, 1, 1, 1)
    x = torch.from_numpy(np.asarray(a, np.float64)).permute(0, 3, 1, 2)
    y = torch.from_numpy(np.asarray(b, np.float64)).permute(0, 3, 1, 2)
    E = lambda t: F.conv2d(t, win, groups=C)
    mx, my = E(x), E(y)
    vx, vy, cxy = E(x * x) - mx * mx, E(y * y) - my * my, E(x * y) - mx * my
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    s = ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    return s.mean(dim=(1, 2, 3)).numpy()


def test_ssim_ref_equals_an_independent_restatement():
    from dgan.metrics import ssim_ref
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)
    got, want = ssim_ref(a, b), _restated_ssim(a, b, 255.0)
    print("ssim_ref", got, "restated", want)
    assert got.shape == (2,) and got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-12
    assert 0.0 < got.min() and got.max() < 1.0 and got[0] != got[1]
    # fp32 images on [0, 1]
    af, bf = (a / 255.0).astype(np.float32), (b / 255.0).astype(np.float32)
    assert np.abs(ssim_ref(af, bf, 1.0) - _restated_ssim(af, bf, 1.0)).max() <= 1e-12


def test_an_11x11_image_is_the_single_window_formula():
    from dgan.metrics import gaussian_taps, ssim_ref
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (11, 11, 1), dtype=np.uint8)
    b = rng.integers(0, 256, (11, 11, 1), dtype=np.uint8)
    g = gaussian_taps()
    assert abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and abs(g[5] / g[4] - np.exp(1 / 4.5)) < 1e-15
    W = np.outer(g, g)
    x, y = a[..., 0].astype(np.float64), b[..., 0].astype(np.float64)
    mx, my = (W * x).sum(), (W * y).sum()
    vx, vy, cxy = (W * x * x).sum() - mx * mx, (W * y * y).sum() - my * my, (W * x * y).sum() - mx * my
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    want = (2 * mx * my + c1) / (mx * mx + my * my + c1) * (2 * cxy + c2) / (vx + vy + c2)
    got = ssim_ref(a, b)
    assert np.ndim(got) == 0 and abs(got - want) <= 1e-12


def test_identical_images_give_exactly_one_and_inf():
    from dgan.metrics import psnr_ref, ssim_ref
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (2, 24, 40, 3), dtype=np.uint8)
    assert np.array_equal(ssim_ref(a, a.copy()), np.ones(2))
    assert np.all(np.isposinf(psnr_ref(a, a.copy())))
    f = rng.uniform(-1, 1, (1, 16, 16, 3)).astype(np.float32)
    assert ssim_ref(f, f.copy(), 2.0)[0] == 1.0 and np.isposinf(psnr_ref(f, f.copy(), 2.0)[0])


@pytest.mark.parametrize("va,vb", [(255, 254), (200, 100), (0, 255)])
def test_two_constant_images_give_the_closed_forms(va, vb):
    """cs = 1 (no variance, no covariance), l from the two constants, PSNR = 20 log10(255 / d)."""
    from dgan.metrics import psnr_ref, ssim_ref
    a = np.full((1, 16, 19, 3), va, np.uint8)
    b = np.full((1, 16, 19, 3), vb, np.uint8)
    c1 = (0.01 * 255) ** 2
    l = (2.0 * va * vb + c1) / (va * va + vb * vb + c1)
    assert abs(ssim_ref(a, b)[0] - l) <= 1e-12
    assert abs(psnr_ref(a, b)[0] - 20 * np.log10(255.0 / abs(va - vb))) <= 1e-12


def test_error_cases():
    from dgan.metrics import psnr_ref, ssim_ref
    z = np.zeros((1, 10, 32, 3), np.uint8)
    with pytest.raises(ValueError, match="smaller than"):
        ssim_ref(z, z)
    with pytest.raises(ValueError, match="smaller than"):
        ssim_ref(np.zeros((32, 10, 3), np.uint8), np.zeros((32, 10, 3), np.uint8))
    psnr_ref(z, z)   # (PSNR has no window)
    with pytest.raises(ValueError, match="shapes differ"):
        ssim_ref(np.zeros((1, 16, 16, 3), np.uint8), np.zeros((1, 16, 17, 3), np.uint8))
    with pytest.raises(ValueError, match="shapes differ"):
        psnr_ref(np.zeros((1, 16, 16, 3), np.uint8), np.zeros((2, 16, 16, 3), np.uint8))
    for fn in (psnr_ref, ssim_ref):
        with pytest.raises(ValueError, match="dtype"):
            fn(np.zeros((1, 16, 16, 3), np.int32), np.zeros((1, 16, 16, 3), np.int32), 255)
        with pytest.raises(ValueError, match="dtype"):
            fn(np.zeros((1, 16, 16, 3), np.uint8), np.zeros((1, 16, 16, 3), np.float32), 255)
        with pytest.raises(ValueError, match="max_val is required"):
            fn(np.zeros((1, 16, 16, 3), np.float32), np.zeros((1, 16, 16, 3), np.float32))


def test_device_metrics_fail_loudly_without_device_tensors():
    import torch
    from dgan import metrics, ops
    a = torch.zeros((1, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(ops.DGError, match="device"):
        metrics.psnr(a, a)
    with pytest.raises(ops.DGError, match="device"):
        metrics.ssim(a, a)
    with pytest.raises(ValueError, match="max_val is required"):
        metrics.ssim(a.float(), a.float())


def test_workspace_queries_and_argument_errors_need_no_gpu():
    """The shape checks of the C entry points run before anything is launched."""
    import ctypes
    from dgan import _lib, ops
    assert ops.ssim_workspace_bytes(2, 11, 11, 3) == 2 * 8                     # one tile per image
    assert ops.ssim_workspace_bytes(1, 96, 130, 3) == 6 * 4 * 8                # 86 x 120 map in 16 x 32 tiles
    assert ops.ssim_workspace_bytes(0, 64, 64, 3) == 0
    with pytest.raises(ops.DGError, match="h, w >= 11"):
        ops.ssim_workspace_bytes(1, 10, 64, 3)
    with pytest.raises(ops.DGError, match="bad shape"):
        ops.ssim_workspace_bytes(-1, 64, 64, 3)
    L = _lib.lib()
    assert L.dg_ssim_u8(1, 64, 10, 3, None, None, 255.0, None, None, 0, None) == 1   # DG_ERR_ARG
    assert b"h, w >= 11" in L.dg_last_error_string()
    assert L.dg_ssim_u8(1, 64, 64, 3, None, None, 255.0, None, None, 0, None) == 1
    assert b"NULL tensor" in L.dg_last_error_string()
    assert L.dg_u8_err_sums(-1, 10, None, None, None, None) == 1
    assert L.dg_u8_err_sums(0, 10, None, None, None, None) == 0                     # n == 0: a no-op
    assert L.dg_ssim_f32(0, 64, 64, 3, None, None, 0.5, 0.5, 1.0, None, None, 0, None) == 0
    assert L.dg_f32_err_sums(1, 10, None, None, None, None, 0, None) == 1
    nb = ctypes.c_size_t()
    assert L.dg_err_sums_workspace_size(3, 1 << 20, ctypes.byref(nb)) == 0 and nb.value % (3 * 16) == 0 and nb.value > 0


def test_pairing_by_stem():
    from evaluate import pair_by_stem, summarize
    assert pair_by_stem(["b.png", "a.jpg"], ["a.png", "b.bmp"]) == [("a", "a.jpg", "a.png"), ("b", "b.png", "b.bmp")]
    assert pair_by_stem([], []) == []
    with pytest.raises(ValueError, match=r"c\.png has no target"):
        pair_by_stem(["a.png", "c.png"], ["a.png"])
    with pytest.raises(ValueError, match=r"d\.png has no image"):
        pair_by_stem(["a.png"], ["a.png", "d.png"])
    with pytest.raises(ValueError, match="share the stem"):
        pair_by_stem(["a.png", "a.jpg"], ["a.png"])
    s = summarize([{"name": "a", "psnr": 20.0, "ssim": 0.5}, {"name": "b", "psnr": 40.0, "ssim": 0.7}])
    assert s["mean"] == {"psnr": 30.0, "ssim": 0.6} and len(s["images"]) == 2   # the mean of the dB values


def test_evaluate_refuses_bad_pairs_by_name(tmp_path):
    """A size mismatch and an image smaller than the SSIM window end the run with the file's name,
    before anything touches the device."""
    from PIL import Image
    import evaluate
    for sub in ("n1", "c1", "n2", "c2"):
        (tmp_path / sub).mkdir()
    Image.fromarray(np.zeros((10, 20, 3), np.uint8), "RGB").save(tmp_path / "n1" / "tiny.png")
    Image.fromarray(np.zeros((10, 20, 3), np.uint8), "RGB").save(tmp_path / "c1" / "tiny.png")
    with pytest.raises(SystemExit, match=r"tiny\.png is 20x10: smaller than the 11x11 SSIM window"):
        evaluate.main(["--image_dir", str(tmp_path / "n1"), "--target_dir", str(tmp_path / "c1")])
    Image.fromarray(np.zeros((16, 20, 3), np.uint8), "RGB").save(tmp_path / "n2" / "a.png")
    Image.fromarray(np.zeros((16, 21, 3), np.uint8), "RGB").save(tmp_path / "c2" / "a.png")
    with pytest.raises(SystemExit, match=r"a\.png is 20x16 but its target a\.png is 21x16"):
        evaluate.main(["--image_dir", str(tmp_path / "n2"), "--target_dir", str(tmp_path / "c2")])
