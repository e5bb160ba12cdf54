"""Image inference on the HIP path (dgan/infer.py, csrc/infer.hip): the staging kernels bit for
bit against their numpy references, dg_bn_fold against fp64, the BN-folded generator forward
against the fp64 oracle on trained-looking weights, and predict / Denoiser / the infer.py
driver end to end."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import p2p_oracle as O

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("tile,margin", [(None, 0), (256, 32)])
@pytest.mark.parametrize("h,w", [(200, 300), (257, 511), (1, 1)])
def test_u8_stage_and_unstage_equal_numpy_bit_for_bit(h, w, tile, margin):
    from dgan import ops
    from dgan.infer import stage_ref, tile_geometry, unstage_ref
    g = tile_geometry(h, w, tile, margin)
    rng = np.random.default_rng(h * 1000 + w)
    u8 = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    nt = 2 * g.gi * g.gj
    d_u8 = torch.from_numpy(u8).cuda()
    for pad in ("black", "reflect"):
        tiles = torch.full((nt, g.Th, g.Tw, 3), 7.0, dtype=torch.float32, device="cuda")
        ops.u8_stage(d_u8, tiles, g, pad)
        assert np.array_equal(tiles.cpu().numpy(), stage_ref(u8, g, pad)), pad
    # unstage: values below -1, above 1 and NaN among ordinary ones
    t = (rng.standard_normal((nt, g.Th, g.Tw, 3)) * 0.8).astype(np.float32)
    flat = t.reshape(-1)
    flat[::97] = np.nan
    flat[5::89] = 3.0
    flat[7::83] = -2.5
    flat[11::79] = 1.0
    flat[13::73] = -1.0
    out = torch.full((2, h, w, 3), 9, dtype=torch.uint8, device="cuda")
    ops.u8_unstage(torch.from_numpy(t).cuda(), out, g)
    assert np.array_equal(out.cpu().numpy(), unstage_ref(t, g))


@gpu
def test_u8_unstage_refuses_a_grid_that_does_not_cover_the_image():
    from dgan import ops
    from dgan.infer import tile_geometry
    g = tile_geometry(300, 300, 256, 32)._replace(gi=1)   # one tile row short
    tiles = torch.zeros((g.gi * g.gj, 256, 256, 3), device="cuda")
    with pytest.raises(ops.DGError):
        ops.u8_unstage(tiles, torch.zeros((1, 300, 300, 3), dtype=torch.uint8, device="cuda"), g)


@gpu
@pytest.mark.parametrize("bias_in", [False, True])
@pytest.mark.parametrize("shape,transpose", [((4, 4, 3, 8), False), ((4, 4, 64, 100), False), ((4, 4, 24, 16), True)])
def test_bn_fold_matches_fp64(shape, transpose, bias_in):
    """relative 1e-6 on w_out, max-abs 1e-6 on bias_out (entries O(1)): a few fp32 ulps of a
    product of three fp32 values."""
    from dgan import ops
    rng = np.random.default_rng(sum(shape) + transpose)
    co = shape[2] if transpose else shape[3]
    w = (rng.standard_normal(shape) * 0.02).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, co).astype(np.float32)
    beta = (rng.standard_normal(co) * 0.2).astype(np.float32)
    mean = (rng.standard_normal(co) * 0.3).astype(np.float32)
    var = rng.uniform(0.5, 2.0, co).astype(np.float32)
    b_in = (rng.standard_normal(co) * 0.1).astype(np.float32) if bias_in else None
    eps = 1e-3
    s = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + np.float64(np.float32(eps)))
    w_ref = w.astype(np.float64) * (s[None, None, :, None] if transpose else s)
    b_ref = beta.astype(np.float64) - mean.astype(np.float64) * s
    if bias_in:
        b_ref = b_ref + b_in.astype(np.float64) * s
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    w_out = torch.full(shape, 5.0, dtype=torch.float32, device="cuda")
    b_out = torch.full((co,), 5.0, dtype=torch.float32, device="cuda")
    ops.bn_fold(dev(w), dev(gamma), dev(beta), dev(mean), dev(var), w_out, b_out, transpose=transpose, eps=eps,
                bias_in=dev(b_in))
    got_w, got_b = w_out.cpu().numpy().astype(np.float64), b_out.cpu().numpy().astype(np.float64)
    rel = np.abs(got_w - w_ref).max() / np.abs(w_ref).max()
    rel_each = (np.abs(got_w - w_ref) / np.maximum(np.abs(w_ref), 1e-30)).max()
    err_b = np.abs(got_b - b_ref).max()
    print(f"bn_fold {shape} transpose={transpose} bias_in={bias_in}: rel {rel:.2e} per-element {rel_each:.2e} "
          f"bias {err_b:.2e}")
    assert rel_each <= 1e-6
    assert err_b <= 1e-6


# ---------------------------------------------------------------------------
# folded forward against the fp64 oracle
# ---------------------------------------------------------------------------
def _tiled(a, H, W):
    return np.ascontiguousarray(np.tile(a, (1, H // a.shape[1], W // a.shape[2], 1)))


@functools.lru_cache(maxsize=None)
def trained_looking(width, H, W):
    """Parameters and moving statistics of a generator that looks trained: with fresh weights and
    moving variance near 1 every activation is tiny and an absolute bar shows nothing.  gamma ~
    U(0.5, 1.5), beta ~ N(0, 0.2), last/bias ~ N(0, 0.1); each BN's moving statistics are spread
    around its batch statistics on four synthetic images (training-mode oracle forward, no
    dropout), the variance floored at a tenth of the layer's mean (without the floor the
    full-width case saturates tanh)."""
    rng = np.random.default_rng(1000 + width)
    params = {k: v.copy() for k, v in O.P2PState(width, seed=5).G.items()}
    for k in params:
        if k.endswith("/gamma"):
            params[k] = rng.uniform(0.5, 1.5, params[k].shape).astype(np.float32)
        elif k.endswith("/beta"):
            params[k] = (rng.standard_normal(params[k].shape) * 0.2).astype(np.float32)
    params["last/bias"] = (rng.standard_normal(params["last/bias"].shape) * 0.1).astype(np.float32)
    x4 = _tiled(O.synthetic_pair(4, 256, seed=11)[0], H, W)
    _, cache = O.generator_forward(params, x4, width, training=True, states=None, drop_rate=0.0)
    downs, ups, _ = O.g_layer_specs(width)
    stats = {name: cache["bn"][li][0] for li, (name, _, _, bn) in enumerate(downs) if bn}
    stats.update({name: cache["up"][u]["bc"] for u, (name, *_) in enumerate(ups)})
    states = {}
    for name, bc in stats.items():
        var = np.maximum(bc["var"], 0.1 * bc["var"].mean())
        states[f"{name}/moving_variance"] = (var * rng.uniform(0.5, 2.0, var.shape)).astype(np.float32)
        states[f"{name}/moving_mean"] = (bc["mu"] + 0.3 * np.sqrt(var) * rng.standard_normal(var.shape)).astype(np.float32)
    return params, states


def _generator(width, params, states):
    from dgan.models import Generator
    g = Generator(width=width)
    g.load_state_dict({**params, **states})
    return g


def _no_bn(monkeypatch):
    from dgan import ops

    def refuse(*a, **k):
        raise AssertionError("the folded forward launched a BatchNorm kernel")

    monkeypatch.setattr(ops, "bn_fwd_infer", refuse)
    monkeypatch.setattr(ops, "bn_fwd_train", refuse)


def _errors(gen, folded, x, params, states, monkeypatch):
    """(err_u, err_f, oracle output, folded output): the max-abs distance from the fp64 oracle of
    the parent's path generator(x, training=False) and of the folded path, on the same inputs."""
    ref, _ = O.generator_forward(params, x, gen.width, training=False, states=states)
    got_u = gen(x, training=False).cpu().numpy()
    with monkeypatch.context() as m:
        _no_bn(m)
        got_f = folded(torch.from_numpy(x).cuda()).cpu().numpy()
    assert got_f.shape == ref.shape
    return float(np.abs(got_u - ref).max()), float(np.abs(got_f - ref).max()), ref, got_f


def _assert_bar(err_u, err_f, what):
    assert err_u < 1e-4, (f"{what}: the EXISTING inference path misses the oracle by {err_u:.3e} (bar 1e-4): the test "
                          f"inputs or generator(x, training=False) are at fault, not the folded path")
    bar = max(1e-5, 2 * err_u)
    assert err_f <= bar, f"{what}: folded path {err_f:.3e} from the oracle > max(1e-5, 2 x {err_u:.3e})"


@gpu
@pytest.mark.parametrize("width,N,H,W", [(8, 1, 256, 512), (8, 3, 256, 256), (4, 2, 512, 256), (1, 1, 256, 256)])
def test_folded_forward_matches_the_oracle(width, N, H, W, monkeypatch):
    """err_f <= max(1e-5, 2 err_u): err_u the parent path's own distance from the oracle, the
    factor 2 for the one fp32 rounding per weight and bias that folding adds (comparable to the
    BN apply it replaces), 1e-5 the existing inference bar (tests/test_step_gpu.py)."""
    from dgan.infer import FoldedGenerator
    params, states = trained_looking(width, H, W)
    gen = _generator(width, params, states)
    folded = FoldedGenerator(gen)
    wmax = folded.max_abs_weight()
    assert wmax < 255.0, f"folded weight {wmax} outside the fp16x3 weight planes' range"
    x = _tiled(O.synthetic_pair(N, 256, seed=12)[0], H, W)
    err_u, err_f, ref, first = _errors(gen, folded, x, params, states, monkeypatch)
    sat = float((np.abs(ref) > 0.999).mean())
    print(f"folded forward width {width} {N}x{H}x{W}: err_u {err_u:.3e} err_f {err_f:.3e} oracle std "
          f"{ref.std():.3f} max {np.abs(ref).max():.3f} saturated {sat:.4f} max |w'| {wmax:.2f}")
    assert ref.std() > 0.05 and sat == 0.0, "the inputs do not look trained (tiny or saturated output)"
    _assert_bar(err_u, err_f, f"width {width} {N}x{H}x{W}")
    # a second forward reuses the kept weight planes and changes nothing
    ws = folded.plan(N, H, W).ws.buf
    assert np.array_equal(folded(torch.from_numpy(x).cuda()).cpu().numpy(), first)
    assert folded.plan(N, H, W).ws.buf is ws   # the pre-sized workspace is never re-allocated


# ---------------------------------------------------------------------------
# predict, refresh
# ---------------------------------------------------------------------------
class Args:
    crop_size = 256
    retrain = 0
    content_loss = 0
    width = 8
    seed = 5


@gpu
def test_predict_and_refresh_follow_the_weights(monkeypatch):
    from dgan.infer import Denoiser
    from pix2pix import Pix2Pix
    m = Pix2Pix(Args())
    G = m.generator
    x, y = O.synthetic_pair(2, 256, seed=1)
    u8 = np.random.default_rng(2).integers(0, 256, (200, 300, 3), dtype=np.uint8)
    den = Denoiser(G)
    before = G.predict(x)
    old = den.denoise(u8)
    old_float = den.folded(torch.from_numpy(x).cuda()).cpu().numpy()
    assert isinstance(before, np.ndarray) and before.shape == x.shape and before.dtype == np.float32
    m.trainer(x.shape).step(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    torch.cuda.synchronize()
    after = G.predict(x)
    assert np.abs(after - before).max() > 0, "predict did not pick up the trained weights"
    params, states = G.arena.export(), G.bn.export()
    ref, _ = O.generator_forward(params, x, 8, training=False, states=states)
    err_u = float(np.abs(G(x, training=False).cpu().numpy() - ref).max())
    err_f = float(np.abs(after - ref).max())
    print(f"predict after one step: err_u {err_u:.3e} err_f {err_f:.3e}")
    _assert_bar(err_u, err_f, "predict")
    # (one image per forward: other GEMM plans and operand scales, the same bar)
    _assert_bar(err_u, float(np.abs(G.predict(x, batch_size=1) - ref).max()), "predict, batch_size 1")
    # a Denoiser keeps the weights it folded until refresh()
    assert np.array_equal(den.denoise(u8), old)
    assert np.array_equal(den.folded(torch.from_numpy(x).cuda()).cpu().numpy(), old_float)
    den.refresh()
    assert np.array_equal(den.folded(torch.from_numpy(x).cuda()).cpu().numpy(), after)
    assert np.array_equal(den.denoise(u8), Denoiser(G).denoise(u8))


# ---------------------------------------------------------------------------
# Denoiser end to end
# ---------------------------------------------------------------------------
def _expected(den, u8):
    """numpy stage -> the Denoiser's own FoldedGenerator on those tiles, in its chunks (idle tiles
    black) -> numpy unstage."""
    from dgan.infer import stage_ref, tile_geometry, unstage_ref
    g = tile_geometry(u8.shape[1], u8.shape[2], den.tile, den.margin)
    tiles = stage_ref(u8, g, den.pad)
    nt = tiles.shape[0]
    B = den.batch if den.tile is not None else min(den.batch, nt)
    padded = np.full((-(-nt // B) * B,) + tiles.shape[1:], -1.0, np.float32)
    padded[:nt] = tiles
    out = np.empty_like(padded)
    for t0 in range(0, padded.shape[0], B):
        out[t0:t0 + B] = den.folded(torch.from_numpy(padded[t0:t0 + B]).cuda()).cpu().numpy()
    return unstage_ref(out[:nt], g)


@functools.lru_cache(maxsize=None)
def _trained_w8():
    params, states = trained_looking(8, 256, 256)
    return _generator(8, params, states)


@gpu
@pytest.mark.parametrize("h,w,kw", [(200, 300, dict()), (300, 520, dict(tile=256, margin=32, batch=4))])
def test_denoise_equals_numpy_staging_around_the_folded_forward(h, w, kw):
    from dgan.infer import Denoiser
    den = Denoiser(_trained_w8(), **kw)
    u8 = np.random.default_rng(h).integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    got = den.denoise(u8)
    assert got.dtype == np.uint8 and got.shape == u8.shape
    want = _expected(den, u8)
    assert np.array_equal(got, want)
    assert len(np.unique(got)) > 16, "a flat output would show nothing"
    one = den.denoise(u8[1])   # [h,w,3] in, [h,w,3] out
    assert one.shape == (h, w, 3) and np.array_equal(one, _expected(den, u8[1:2])[0])


@gpu
def test_graph_replays_equal_eager():
    from dgan.infer import Denoiser
    G = _trained_w8()
    eager, graphed = Denoiser(G), Denoiser(G, graph=True)
    rng = np.random.default_rng(4)
    for k in range(2):
        u8 = rng.integers(0, 256, (1, 200, 300, 3), dtype=np.uint8)
        assert np.array_equal(graphed.denoise(u8), eager.denoise(u8)), k
    assert graphed._frames[(1, 200, 300)].graph is not None


# ---------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------
@gpu
def test_infer_driver_writes_denoised_images(tmp_path):
    from PIL import Image
    from dgan.infer import Denoiser
    G = _trained_w8()
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    rng = np.random.default_rng(6)
    images = {"a.png": rng.integers(0, 256, (120, 200, 3), dtype=np.uint8),
              "b.png": rng.integers(0, 256, (260, 90, 3), dtype=np.uint8)}
    for name, a in images.items():
        Image.fromarray(a, "RGB").save(src / name)
    G.save(str(tmp_path / "gen.npz"))
    r = subprocess.run([sys.executable, os.path.join(REPO, "denoise-gan_amd", "infer.py"), "--image_dir", str(src),
                        "--output_dir", str(dst), "--model", str(tmp_path / "gen.npz")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    den = Denoiser(G)
    for name, a in images.items():
        with Image.open(dst / name) as im:
            got = np.asarray(im.convert("RGB"), np.uint8)
        assert got.shape == a.shape
        assert np.array_equal(got, den.denoise(a)), name
