"""The device BM3D second stage (csrc/bm3d_wiener.hip, dgan.filters.bm3d_wiener / bm3d2) against its
integer definition, bit for bit: stage 1's sizes and parameters (plus sigma 1), with pilots that
make groups of every size, hit the energy clamp and tie at D = 0; batches, determinism, `out`; then
Evaluator(baseline="bm3d2"), evaluate.py --baseline bm3d2 and infer.py --post bm3d2 end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_bm3d import frame
from test_bm3d_gpu import PARAMS, SIZES
from test_filters import noisy
from test_filters_gpu import REPO, SENTINEL, _baseline_bars, _same_bits, dev

gpu = pytest.mark.gpu
PARAMS2 = PARAMS + [(1, 11, 4)]   # sigma 1 and 40: the two ends of the Wiener divisor


def pairs(h, w, sigma, search, group):
    """(noisy, pilot), uint8 [4,h,w,3] each: stage 1's output as the pilot (m = 16 where the frame is
    smooth); a noisier pilot (groups of every size); a random pilot (nothing matches: m = 1); a
    period-2 0 / 255 pattern as both (an AC coefficient at the energy clamp, ties at D = 0)."""
    from dgan.filters import bm3d_ref
    a, b = frame("noisy", h, w, sigma), noisy(h, w, 25.0)
    bars = np.broadcast_to(np.array([0, 255], np.uint8)[np.arange(w) % 2][None, :, None], (h, w, 3))
    return (np.stack([a, b, a, bars]),
            np.stack([bm3d_ref(a, sigma, search, group), noisy(h, w, 14.0), frame("random", h, w, sigma), bars]))


@gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bm3d_wiener_equals_the_reference_bit_for_bit(size):
    from dgan.filters import bm3d_wiener, bm3d_wiener_ref
    for sigma, search, group in PARAMS2:
        imgs, pilots = pairs(*size, sigma, search, group)
        x, p = dev(imgs), dev(pilots)
        got, want = bm3d_wiener(x, p, sigma, search, group).cpu().numpy(), bm3d_wiener_ref(imgs, pilots, sigma, search, group)
        assert _same_bits(got, want), (size, sigma, search, group, (got != want).reshape(4, -1).sum(1).tolist())
        assert np.array_equal(x.cpu().numpy(), imgs) and np.array_equal(p.cpu().numpy(), pilots)   # (only read)


@pytest.mark.parametrize("search", [7, 21])
def test_the_noisier_pilot_makes_groups_of_every_size(search):
    """What keeps the case above honest: at 23 x 24 all five instantiations of the filter run."""
    from dgan.filters import bm3d_group_sizes
    assert set(bm3d_group_sizes(noisy(23, 24, 14.0), search, 16)) == {1, 2, 4, 8, 16}


@gpu
@pytest.mark.parametrize("size", [(23, 24), (24, 55), (1, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_bm3d2_equals_the_reference_bit_for_bit(size):
    from dgan.filters import bm3d2, bm3d2_ref
    for sigma, search, group in PARAMS2:
        imgs = np.stack([frame("noisy", *size, sigma), frame("stripes", *size, sigma)])
        got, want = bm3d2(dev(imgs), sigma, search, group).cpu().numpy(), bm3d2_ref(imgs, sigma, search, group)
        assert _same_bits(got, want), (size, sigma, search, group)


@gpu
def test_every_image_of_a_batch_equals_its_own_call_and_two_calls_give_the_same_bits():
    from dgan.filters import bm3d2, bm3d_wiener, bm3d_wiener_ref
    imgs = np.stack([noisy(24, 55, 25.0, seed=k) for k in (1, 2, 3)])
    pilots = np.stack([noisy(24, 55, 14.0, seed=k) for k in (1, 2, 3)])
    x, p = dev(imgs), dev(pilots)
    got = bm3d_wiener(x, p, 25, 11, 8).cpu().numpy()
    assert _same_bits(got, bm3d_wiener_ref(imgs, pilots, 25, 11, 8))
    for i in range(3):
        assert _same_bits(bm3d_wiener(dev(imgs[i:i + 1]), dev(pilots[i:i + 1]), 25, 11, 8).cpu().numpy(), got[i:i + 1]), i
    for call in (lambda: bm3d_wiener(x, p, 25, 11, 8), lambda: bm3d2(x, 25, 11, 8)):
        buf = call()
        first = buf.cpu().numpy()
        before = torch.cuda.memory_allocated()
        again = call()
        assert again is buf and torch.cuda.memory_allocated() == before   # the kept buffers, nothing allocated
        assert _same_bits(again.cpu().numpy(), first)
    first = bm3d_wiener(x, p, 25, 11, 8)
    second = bm3d_wiener(x, first, 25, 11, 8)   # the plan's buffer as the pilot: the result is another one
    assert second.data_ptr() not in (x.data_ptr(), first.data_ptr())
    assert _same_bits(second.cpu().numpy(), bm3d_wiener_ref(imgs, got, 25, 11, 8))


@gpu
def test_out_is_honoured_never_an_input_and_nothing_outside_it_is_written():
    from dgan.filters import bm3d2, bm3d2_ref, bm3d_wiener, bm3d_wiener_ref
    imgs = np.stack([noisy(24, 31, 25.0, seed=k) for k in (4, 5)])
    pilots = np.stack([noisy(24, 31, 14.0, seed=k) for k in (4, 5)])
    x, p, nb = dev(imgs), dev(pilots), imgs.size
    for call, want in ((lambda out: bm3d_wiener(x, p, out=out), bm3d_wiener_ref(imgs, pilots)),
                       (lambda out: bm3d2(x, out=out), bm3d2_ref(imgs))):
        obuf = torch.full((nb + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        out = obuf[1:1 + nb].view(imgs.shape)
        assert call(out) is out and _same_bits(out.cpu().numpy(), want)
        o = obuf.cpu().numpy()
        assert (o[:1] == SENTINEL).all() and (o[1 + nb:] == SENTINEL).all()
    with pytest.raises(ValueError, match="out must not be the input"):
        bm3d_wiener(x, p, out=x)
    with pytest.raises(ValueError, match="out must not be the pilot"):
        bm3d_wiener(x, p, out=p)
    with pytest.raises(ValueError, match="out must not be the input"):
        bm3d2(x, out=x)
    with pytest.raises(ValueError, match="pilot"):
        bm3d_wiener(x, p[:1])
    with pytest.raises(ValueError, match="group"):
        bm3d2(x, group=3)
    assert tuple(bm3d_wiener(x[:0], p[:0]).shape) == (0, 24, 31, 3) and tuple(bm3d2(x[:0]).shape) == (0, 24, 31, 3)


@gpu
def test_the_evaluator_and_the_drivers_take_bm3d2(tmp_path):
    from PIL import Image
    from dgan import filters as F, metrics
    from dgan.infer import Denoiser
    from test_infer_gpu import _trained_w8
    from test_jpeg_gpu import _photo
    clean = _photo(2, 32, 48, 77)
    dirty = np.clip(clean.astype(np.int64) + np.rint(9 * np.random.default_rng(9).standard_normal(clean.shape)), 0,
                    255).astype(np.uint8)
    G = _trained_w8()
    den = Denoiser(G)
    ev = metrics.Evaluator(den, baseline="bm3d2", baseline_args=dict(sigma=9, search=11, group=8))
    got = ev.evaluate(dirty, clean)
    assert tuple(got) == metrics.SCORES + metrics.BASELINE_SCORES
    want = F.bm3d2_ref(dirty, 9, 11, 8)
    assert _same_bits(ev.filtered(den.frame(2, 32, 48)).cpu().numpy(), want)
    _baseline_bars(got["psnr_baseline"], got["ssim_baseline"], want, clean)
    with pytest.raises(ValueError, match="group"):
        metrics.Evaluator(den, baseline="bm3d2", baseline_args=dict(group=5))

    for d, imgs in (("clean", clean), ("noisy", dirty)):
        (tmp_path / d).mkdir()
        for i, name in enumerate(("a", "b")):
            Image.fromarray(imgs[i], "RGB").save(tmp_path / d / f"{name}.png")
    r = subprocess.run([sys.executable, os.path.join(REPO, "denoise-gan_amd", "evaluate.py"), "--target_dir",
                        str(tmp_path / "clean"), "--image_dir", str(tmp_path / "noisy"), "--baseline", "bm3d2",
                        "--bm3d_sigma", "9", "--json", str(tmp_path / "s.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = json.load(open(tmp_path / "s.json"))["images"]
    _baseline_bars(np.array([row["psnr_baseline"] for row in rows]), np.array([row["ssim_baseline"] for row in rows]),
                   F.bm3d2_ref(dirty, 9), clean)
    G.save(str(tmp_path / "gen.npz"))
    r = subprocess.run([sys.executable, os.path.join(REPO, "denoise-gan_amd", "infer.py"), "--image_dir", str(tmp_path / "noisy"),
                        "--output_dir", str(tmp_path / "out"), "--model", str(tmp_path / "gen.npz"), "--post", "bm3d2",
                        "--bm3d_sigma", "9"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.asarray(Image.open(tmp_path / "out" / "a.png").convert("RGB"), np.uint8)
    assert _same_bits(got, F.bm3d2_ref(den.denoise(dirty[0]), 9))
