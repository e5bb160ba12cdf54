"""Tile geometry and the numpy reference staging of image inference (dgan/infer.py): no GPU.

The Denoiser and the GPU tests of dg_u8_stage / dg_u8_unstage both rest on these helpers, so
they are checked here against np.pad itself."""
import numpy as np
import pytest

from dgan.infer import (pad_index, source_tile, stage_ref, tile_geometry, tile_rows, u8_to_unit, unit_to_u8,
                        unstage_ref)

SIZES = [(1, 1), (200, 300), (256, 256), (257, 511), (600, 700)]
MODES = [(None, 0), (256, 0), (256, 32)]   # whole image; T = 256 with margin 0 / 32


@pytest.mark.parametrize("tile,margin", MODES)
@pytest.mark.parametrize("h,w", SIZES)
def test_every_pixel_maps_into_one_tile_interior(h, w, tile, margin):
    g = tile_geometry(h, w, tile, margin)
    assert g.Th % 256 == 0 and g.Tw % 256 == 0
    if tile is None:
        assert (g.gi, g.gj) == (1, 1) and g.Th - h < 256 and g.Tw - w < 256   # no extra 256 on a multiple
        assert g.oy == -((g.Th - h) // 2) and g.ox == -((g.Tw - w) // 2)
    else:
        S = tile - 2 * margin
        assert (g.gi, g.gj) == (-(-h // S), -(-w // S)) and (g.oy, g.ox) == (-margin, -margin)
    for axis, size, T, S, m in ((0, h, g.Th, g.Sh, g.mt), (1, w, g.Tw, g.Sw, g.ml)):
        rows = tile_rows(g, axis)                      # [tiles, T] image coordinates each tile covers
        interior = rows[:, m:m + S]
        # exactly one tile's interior holds each output coordinate ...
        count = (interior[None, :, :] == np.arange(size)[:, None, None]).sum(axis=(1, 2))
        assert (count == 1).all()
        # ... and it is the one the gather picks, at the coordinate it picks
        i, t = source_tile(g, axis)
        assert ((t >= m) & (t < m + S) & (t < T)).all()
        assert (rows[i, t] == np.arange(size)).all()


@pytest.mark.parametrize("pad", ["black", "reflect"])
@pytest.mark.parametrize("tile,margin", MODES)
@pytest.mark.parametrize("h,w", SIZES)
def test_read_indices_are_in_range(h, w, tile, margin, pad):
    g = tile_geometry(h, w, tile, margin)
    for axis, size in ((0, h), (1, w)):
        idx = pad_index(tile_rows(g, axis), size, pad)
        assert (idx < size).all()
        assert (idx >= (-1 if pad == "black" else 0)).all()
        inside = (tile_rows(g, axis) >= 0) & (tile_rows(g, axis) < size)
        assert (idx[inside] == tile_rows(g, axis)[inside]).all()
        if pad == "black":
            assert (idx[~inside] == -1).all()


@pytest.mark.parametrize("size", [1, 2, 3, 5, 7])
def test_reflect_index_is_numpy_reflect(size):
    for before, after in ((0, 0), (1, 2), (4, 13), (13, 6)):
        want = np.pad(np.arange(size), (before, after), mode="reflect")
        got = pad_index(np.arange(-before, size + after), size, "reflect")
        assert (got == want).all(), (size, before, after)


def _image(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("tile,margin", MODES)
@pytest.mark.parametrize("h,w", [(1, 1), (200, 300), (257, 511)])
def test_stage_ref_is_np_pad_then_slices(h, w, tile, margin):
    g = tile_geometry(h, w, tile, margin)
    u8 = _image(2, h, w, seed=h + w)
    # pad widths that cover every tile's reach
    pt, pl = -g.oy, -g.ox
    pb = max(g.oy + (g.gi - 1) * g.Sh + g.Th - h, 0)
    pr = max(g.ox + (g.gj - 1) * g.Sw + g.Tw - w, 0)
    widths = ((0, 0), (pt, pb), (pl, pr), (0, 0))
    unit = u8_to_unit(u8)
    # black: the reference pads the [0, 1] image with zeros before * 2 - 1
    zero_one = u8.astype(np.float32) * np.float32(1.0 / 255.0)
    padded = {"reflect": np.pad(unit, widths, mode="reflect"),
              "black": np.pad(zero_one, widths, mode="constant") * np.float32(2.0) - np.float32(1.0)}
    for pad, full in padded.items():
        got = stage_ref(u8, g, pad).reshape(2, g.gi, g.gj, g.Th, g.Tw, 3)
        for i in range(g.gi):
            for j in range(g.gj):
                y0, x0 = i * g.Sh, j * g.Sw   # (oy + pt == 0)
                want = full[:, y0:y0 + g.Th, x0:x0 + g.Tw, :]
                assert np.array_equal(got[:, i, j], want), (pad, i, j)


def test_conversion_round_trip_is_the_identity_for_all_256_values():
    u8 = np.arange(256, dtype=np.uint8)
    assert np.array_equal(unit_to_u8(u8_to_unit(u8)), u8)
    assert unit_to_u8(np.array([-3.0, 3.0, np.nan, -1.0, 1.0], np.float32)).tolist() == [0, 255, 0, 0, 255]


@pytest.mark.parametrize("tile,margin", MODES)
@pytest.mark.parametrize("h,w", SIZES)
def test_unstage_of_stage_is_the_identity(h, w, tile, margin):
    g = tile_geometry(h, w, tile, margin)
    # every byte value occurs (the first 256 channel values), the rest seeded
    u8 = _image(2, h, w, seed=3)
    flat = u8.reshape(-1)
    k = min(256, flat.size)
    flat[:k] = np.arange(k, dtype=np.uint8)
    for pad in ("black", "reflect"):
        assert np.array_equal(unstage_ref(stage_ref(u8, g, pad), g), u8)


def test_geometry_rejects_bad_arguments():
    for kw in (dict(tile=200), dict(tile=256, margin=128), dict(tile=256, margin=-1), dict(tile=None, margin=8)):
        with pytest.raises(ValueError):
            tile_geometry(300, 300, **kw)
    with pytest.raises(ValueError):
        tile_geometry(0, 10)
    with pytest.raises(ValueError):
        pad_index(np.arange(3), 3, "edge")
