"""The resize definition of dgan/resize.py (no GPU): the 4-tap tables against the dataloader's
interpolation matrices, the fp64 reference's identities and conversions, the library's argument
checks and the centre crop of evaluate_sr.py."""
import numpy as np
import pytest

PAIRS = [(8, 4), (4, 8), (13, 13), (1, 3), (3, 1), (37, 11), (11, 64), (2, 7), (270, 1080), (1080, 270)]


def _matrix(n_in, n_out, method):
    import dataloader
    return (dataloader._bicubic_matrix if method == "bicubic" else dataloader._bilinear_matrix)(n_in, n_out)


@pytest.mark.parametrize("method", ["bicubic", "bilinear"])
def test_taps_scatter_into_the_dataloaders_matrices_bit_for_bit(method):
    from dgan.resize import resize_taps
    for n_in, n_out in PAIRS:
        idx, w = resize_taps(n_in, n_out, method)
        assert idx.shape == (n_out, 4) and idx.dtype == np.int32 and w.shape == (n_out, 4) and w.dtype == np.float64
        assert idx.min() >= 0 and idx.max() <= n_in - 1
        m = np.zeros((n_out, n_in), np.float64)
        for k in range(4):   # (tap order, as the matrices accumulate)
            np.add.at(m, (np.arange(n_out), idx[:, k]), w[:, k])
        want = _matrix(n_in, n_out, method)
        assert m.tobytes() == (want + 0.0).tobytes(), (n_in, n_out)
    with pytest.raises(ValueError, match="method"):
        resize_taps(4, 4, "lanczos")
    with pytest.raises(ValueError, match="at least 1"):
        resize_taps(0, 4)


def test_a_clamped_tap_has_weight_zero():
    from dgan.resize import resize_taps
    for n_in, n_out in PAIRS:
        idx, w = resize_taps(n_in, n_out, "bicubic")
        x = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
        raw = np.floor(x).astype(int)[:, None] + np.arange(-1, 3)[None]
        assert np.all(w[(raw < 0) | (raw >= n_in)] == 0.0)
        assert np.abs(w.sum(1) - 1.0).max() <= 1e-15   # (four weights below 1.2, a few roundings at 2^-53 each)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_same_size_bicubic_is_the_identity(dtype):
    from dgan.resize import resize_ref
    rng = np.random.Generator(np.random.PCG64(1))
    a = (rng.integers(0, 256, (2, 13, 17, 3), dtype=np.uint8) if dtype == np.uint8
         else rng.standard_normal((2, 13, 17, 3)).astype(np.float32))
    out = resize_ref(a, 13, 17)
    assert out.dtype == dtype and out.tobytes() == a.tobytes()
    assert resize_ref(a[0], 13, 17).shape == (13, 17, 3)
    if dtype == np.uint8:   # both conversions keep an integer
        assert np.array_equal(resize_ref(a, 13, 17, mul=1.0, bias=0.5), a)
        assert np.array_equal(resize_ref(a, 13, 17, mul=255.5 / 255.0, bias=0.0), a)


@pytest.mark.parametrize("method", ["bicubic", "bilinear"])
def test_reference_is_within_1e_7_of_the_dataloader(method):
    """Both sides round their fp64 result to fp32: half an ulp below 1 (3e-8) twice, on results
    that stay inside [0, 1] (levels 40 .. 215 leave the cubic's overshoot, under a sixth of the
    range, inside 0 .. 255; above 1 an ulp is twice as large)."""
    import dataloader
    from dgan.resize import resize_ref
    host = dataloader.resize_bicubic if method == "bicubic" else dataloader.resize_bilinear
    rng = np.random.Generator(np.random.PCG64(2))
    worst = 0.0
    for (hi, wi), (ho, wo) in [((37, 53), (11, 64)), ((16, 24), (4, 6)), ((11, 13), (44, 52)), ((3, 2), (1, 1))]:
        u8 = rng.integers(40, 216, (hi, wi, 3), dtype=np.uint8)
        f = u8.astype(np.float32)
        got = resize_ref(f, ho, wo, method).astype(np.float64) / 255.0
        want = host(u8 / 255.0, ho, wo).astype(np.float64)
        worst = max(worst, np.abs(got - want).max())
    print("resize_ref vs dataloader", method, worst)
    assert worst <= 1e-7


@pytest.mark.parametrize("method", ["bicubic", "bilinear"])
def test_a_constant_image_stays_constant(method):
    from dgan.resize import DEGRADE, DISPLAY, resize_ref
    for (hi, wi), (ho, wo) in [((5, 7), (20, 28)), ((20, 28), (5, 7)), ((3, 2), (9, 11)), ((37, 53), (11, 64))]:
        for v in (0, 1, 77, 254, 255):
            a = np.full((hi, wi, 3), v, np.uint8)
            for mul, bias in (DEGRADE, DISPLAY):
                assert np.all(resize_ref(a, ho, wo, method, mul, bias) == v), (hi, wi, ho, wo, v, mul)
        f = resize_ref(np.full((hi, wi, 1), 0.3, np.float32), ho, wo, method)
        assert np.abs(f.astype(np.float64) - np.float32(0.3)).max() <= 1e-7


def test_degrade_conversion_is_tfs_float_to_uint8():
    """A x1 resize with the degrade conversion is dataloader.to_uint8 of the [0, 1] image."""
    import dataloader
    from dgan.resize import DEGRADE, resize_ref
    a = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    assert np.array_equal(resize_ref(a, 16, 16, "bicubic", *DEGRADE), dataloader.to_uint8(a / 255.0))
    assert np.array_equal(resize_ref(a, 16, 16, "bilinear", *DEGRADE), dataloader.to_uint8(a / 255.0))


def test_reference_argument_errors():
    from dgan.resize import resize_ref
    with pytest.raises(ValueError, match="uint8 or float32"):
        resize_ref(np.zeros((4, 4, 3), np.float64), 2, 2)
    with pytest.raises(ValueError, match="uint8 images only"):
        resize_ref(np.zeros((4, 4, 3), np.float32), 2, 2, bias=0.5)
    with pytest.raises(ValueError, match="uint8 or float32"):
        resize_ref(np.zeros((4, 4), np.uint8), 2, 2)


def test_library_entries_check_their_arguments_without_a_gpu():
    from dgan import _lib
    L = _lib.lib()
    none = [None] * 6
    assert L.dg_resize_u8(1, 8, 0, 3, 4, 4, *none, 1.0, 0.5, None) == 1   # DG_ERR_ARG
    assert b"bad shape" in L.dg_last_error_string()
    assert L.dg_resize_f32(1, 8, 8, 3, 4, 0, *none, None) == 1
    assert b"bad shape" in L.dg_last_error_string()
    assert L.dg_resize_u8(-1, 8, 8, 3, 4, 4, *none, 1.0, 0.5, None) == 1
    assert L.dg_resize_u8(1, 8, 8, 0, 4, 4, *none, 1.0, 0.5, None) == 1
    assert L.dg_resize_u8(1, 8, 8, 3, 4, 4, *none, 1.0, 0.5, None) == 1
    assert b"NULL tensor" in L.dg_last_error_string()
    assert L.dg_resize_f32(1, 8, 8, 3, 4, 4, *none, None) == 1
    assert b"NULL tensor" in L.dg_last_error_string()
    assert L.dg_resize_u8(1, 8, 8, 3, 4, 4, *none, float("nan"), 0.5, None) == 1
    assert L.dg_resize_u8(0, 8, 8, 3, 4, 4, *none, 1.0, 0.5, None) == 0   # n == 0: a no-op
    assert L.dg_resize_f32(0, 8, 8, 3, 4, 4, *none, None) == 0
    assert L.dg_version() == 1


def test_device_op_refuses_host_tensors():
    import torch
    from dgan.resize import resize
    with pytest.raises(ValueError, match="device tensor"):
        resize(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 4, 4)
    with pytest.raises(ValueError, match="uint8 or float32"):
        resize(np.zeros((1, 8, 8, 3), np.uint8), 4, 4)


def test_centre_crop_of_evaluate_sr():
    from evaluate_sr import centre_crop
    a = np.arange(97 * 138 * 3, dtype=np.uint32).reshape(97, 138, 3)
    out, box = centre_crop(a, 4)
    assert box == (0, 1, 96, 136) and out.shape == (96, 136, 3) and np.array_equal(out, a[0:96, 1:137])
    out, box = centre_crop(a[:96, :136], 4)
    assert box is None and out.shape == (96, 136, 3)
    out, box = centre_crop(a[:15, :23], 8)
    assert box == (3, 3, 8, 16) and np.array_equal(out, a[3:11, 3:19])
    out, box = centre_crop(a, 1)
    assert box is None and out is a
    out, box = centre_crop(a[:3, :9], 4)
    assert out.shape == (0, 8, 3) and box == (1, 0, 0, 8)
