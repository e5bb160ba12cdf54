"""Super-resolution inference on the HIP path (dgan/sr_infer.py, csrc/infer_sr.hip): the fused
inverted-residual kernel and the activated depthwise conv against their references, the folded
SRGAN / FastSRGAN / autoencoder forwards against the fp64 oracle on trained-looking weights, and
predict / Upscaler / the upscale.py driver end to end.

The bar is the project's inference bar (tests/test_infer_gpu.py::_assert_bar): err_f <= max(1e-5,
2 err_u) and err_u < 1e-4, err_f the new path's max-abs distance from fp64 and err_u that of the
library's existing path on the same inputs.

Measured on one MI355X:
  mbconv, every shape and variant     err_u 1.5e-7 .. 1.3e-6   err_f 5.8e-7 .. 1.6e-6
  the folded networks                 DESIGN.md, Inference, Super-resolution (parity table)
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sr_infer_util import MB_C, MB_E, MB_SHAPES, MB_TILE, builder, mb_inputs, oracle_forward, trained_looking

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _assert_bar(err_u, err_f, what):
    assert err_u < 1e-4, (f"{what}: the EXISTING path misses the reference by {err_u:.3e} (bar 1e-4): the test "
                          f"inputs or the existing path are at fault, not the new one")
    bar = max(1e-5, 2 * err_u)
    assert err_f <= bar, f"{what}: new path {err_f:.3e} from the reference > max(1e-5, 2 x {err_u:.3e})"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _wide(a, ld):
    """a [N,H,W,C] as a channel slice of a wider buffer of pixel stride ld (the rest NaN)."""
    N, H, W, C = a.shape
    buf = torch.full((N, H, W, ld), float("nan"), dtype=torch.float32, device="cuda")
    v = buf[..., 4:4 + C]
    if a is not None:
        v.copy_(_dev(a))
    return buf, v


# ---------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------
def test_tile_constant_matches_the_library():
    from dgan import ops
    assert ops.mbconv_tile() == MB_TILE


@functools.lru_cache(maxsize=None)
def _mb_case(shape):
    """(inputs, device inputs, fp64 reference without the residual, the unfused sequence's output
    without the residual) -- computed once per shape."""
    from dgan import ops
    from dgan.sr_infer import mbconv_ref
    t = mb_inputs(*shape)
    d = {k: _dev(v) for k, v in t.items()}
    ref = mbconv_ref(t["x"], t["w_exp"], t["b_exp"], t["k_dw"], t["b_dw"], t["w_proj"], t["b_proj"])
    N, H, W = shape
    e = torch.empty((N, H, W, MB_E), device="cuda")
    e2 = torch.empty_like(e)
    u = torch.empty((N, H, W, MB_C), device="cuda")
    ops.ConvDesc(N, H, W, MB_C, MB_E, 1, 1, "same").fwd(d["x"], d["w_exp"], e, bias=d["b_exp"], act="relu")
    ops.dwconv3_fwd_act(e, d["k_dw"], e2, bias=d["b_dw"], act="relu")
    ops.ConvDesc(N, H, W, MB_E, MB_C, 1, 1, "same").fwd(e2, d["w_proj"], u, bias=d["b_proj"])
    return t, d, ref, u


@gpu
@pytest.mark.parametrize("variant", ["res", "nores", "strided"])
@pytest.mark.parametrize("shape", MB_SHAPES)
def test_mbconv_matches_fp64(shape, variant):
    from dgan import ops
    t, d, ref, u = _mb_case(shape)
    res = variant != "nores"
    if res:
        ref = ref + t["x"].astype(np.float64)
        u = ops.add(u, d["x"], torch.empty_like(u))
    x, y = d["x"], torch.full(t["x"].shape, float("nan"), device="cuda")
    ybuf = None
    if variant == "strided":
        _, x = _wide(t["x"], 40)
        ybuf, y = _wide(np.zeros_like(t["x"]), 40)
        y.fill_(float("nan"))
    ops.mbconv_fwd(x, d["w_exp"], d["b_exp"], d["k_dw"], d["b_dw"], d["w_proj"], d["b_proj"], y, res=x if res else None)
    got = y.cpu().numpy().astype(np.float64)
    err_f = float(np.abs(got - ref).max())
    err_u = float(np.abs(u.cpu().numpy().astype(np.float64) - ref).max())
    print(f"mbconv {shape} {variant}: err_u {err_u:.3e} err_f {err_f:.3e} ref std {ref.std():.3f} max {np.abs(ref).max():.2f}")
    assert np.isfinite(got).all()
    _assert_bar(err_u, err_f, f"mbconv {shape} {variant}")
    if ybuf is not None:   # nothing written outside the slice
        assert torch.isnan(ybuf[..., :4]).all() and torch.isnan(ybuf[..., 4 + MB_C:]).all()


@gpu
def test_mbconv_refuses_aliasing_and_unsupported_channels():
    from dgan import ops
    t = mb_inputs(1, 5, 7)
    d = {k: _dev(v) for k, v in t.items()}
    a = (d["w_exp"], d["b_exp"], d["k_dw"], d["b_dw"], d["w_proj"], d["b_proj"])
    with pytest.raises(ops.DGError, match=r"rc=1"):
        ops.mbconv_fwd(d["x"], *a, d["x"])
    for C, E, Co in [(16, 96, 16), (32, 200, 32), (32, 224, 32), (32, 192, 64), (64, 192, 32)]:
        assert not ops.mbconv_supported_lib(C, E, Co) and not ops.mbconv_supported(C, E, Co)
        x = torch.zeros((1, 5, 7, C), device="cuda")
        with pytest.raises(ops.DGError, match=r"rc=1"):
            ops.mbconv_fwd(x, torch.zeros((1, 1, C, E), device="cuda"), None, torch.zeros((3, 3, E, 1), device="cuda"),
                           None, torch.zeros((1, 1, E, Co), device="cuda"), None, torch.zeros((1, 5, 7, Co), device="cuda"))
    for E in (32, 96, 192):
        assert ops.mbconv_supported_lib(32, E, 32) and ops.mbconv_supported(32, E, 32)


@gpu
def test_dwconv_act_equals_dwconv_then_act_bit_for_bit():
    from dgan import ops
    rng = np.random.default_rng(7)
    x = _dev(rng.standard_normal((2, 5, 7, 192)).astype(np.float32))
    k = _dev((rng.standard_normal((3, 3, 192, 1)) / 3).astype(np.float32))
    b = _dev((rng.standard_normal(192) * 0.5).astype(np.float32))
    plain = ops.dwconv3_fwd(x, k, torch.empty_like(x), bias=b)
    want = ops.act_fwd(plain, torch.empty_like(x), "relu")
    got = ops.dwconv3_fwd_act(x, k, torch.empty_like(x), bias=b, act="relu")
    assert torch.equal(got, want) and float((want == 0).float().mean()) > 0.2
    assert torch.equal(ops.dwconv3_fwd_act(x, k, torch.empty_like(x), bias=b, act="none"), plain)
    assert torch.equal(ops.dwconv3_fwd_act(x, k, torch.empty_like(x), act="none"),
                       ops.dwconv3_fwd(x, k, torch.empty_like(x)))


# ---------------------------------------------------------------------------
# folded networks against the fp64 oracle
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _network(kind):
    from dgan.graph import GraphNetwork
    graph, params, stats = trained_looking(kind)
    net = GraphNetwork(graph, seed=5)
    net.load_state_dict({**params, **stats})
    return net


def _no_bn(monkeypatch):
    from dgan import ops

    def refuse(*a, **k):
        raise AssertionError("the folded forward launched a BatchNorm kernel")

    monkeypatch.setattr(ops, "bn_fwd_infer", refuse)
    monkeypatch.setattr(ops, "bn_fwd_train", refuse)


@functools.lru_cache(maxsize=None)
def _oracle_case(kind, N, H, W):
    _, params, stats = trained_looking(kind)
    x = np.random.default_rng(N * 100 + H).uniform(-1, 1, (N, H, W, 3)).astype(np.float32)
    ref = oracle_forward(kind, params, stats, x)
    err_u = float(np.abs(_network(kind)(x, training=False).cpu().numpy() - ref).max())
    return x, ref, err_u


@gpu
@pytest.mark.parametrize("kind,N,H,W,fuse", [("fsrgan", 2, 24, 24, True), ("fsrgan", 2, 24, 24, False),
                                             ("fsrgan", 1, 13, 19, True), ("fsrgan", 1, 13, 19, False),
                                             ("srgan", 1, 13, 19, True), ("autoencoder", 1, 32, 64, True)])
def test_folded_forward_matches_the_oracle(kind, N, H, W, fuse, monkeypatch):
    from dgan import ops
    from dgan.sr_infer import FoldedNetwork
    net = _network(kind)
    x, ref, err_u = _oracle_case(kind, N, H, W)
    folded = FoldedNetwork(net, fuse=fuse)
    wmax = folded.max_abs_weight()
    assert wmax < 255.0, f"folded weight {wmax} outside the fp16x3 weight planes' range"
    calls = []
    real = ops.mbconv_fwd
    with monkeypatch.context() as m:
        _no_bn(m)
        m.setattr(ops, "mbconv_fwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        first = folded(_dev(x)).cpu().numpy()
    assert first.shape == ref.shape
    err_f = float(np.abs(first - ref).max())
    sat = float((np.abs(ref) > 0.999).mean())
    print(f"folded {kind} {N}x{H}x{W} fuse={fuse}: err_u {err_u:.3e} err_f {err_f:.3e} oracle std {ref.std():.3f} "
          f"max {np.abs(ref).max():.3f} saturated {sat:.4f} max |w'| {wmax:.2f}")
    assert ref.std() > 0.05 and sat == 0.0, "the inputs do not look trained (tiny or saturated output)"
    assert len(calls) == (5 if kind == "fsrgan" and fuse else 0)
    _assert_bar(err_u, err_f, f"{kind} {N}x{H}x{W} fuse={fuse}")
    # a second forward reuses the kept weight planes and the pre-sized workspace and changes nothing
    ws = folded.plan(N, H, W).ws.buf
    assert np.array_equal(folded(_dev(x)).cpu().numpy(), first)
    assert folded.plan(N, H, W).ws.buf is ws


@gpu
def test_folded_forward_under_mixed_float16():
    """conv_math "fp16": the 3x3 convs round their operands to fp16 (2^-11 relative each) on both
    paths -- the folded one rounds w * s where the parent rounds w, an independent rounding of the
    same size -- and the fused blocks' GEMMs stay exact fp32, so the folded path's distance from the
    fp64 oracle is of the parent's order or smaller: err_f <= 2 err_u."""
    from dgan.graph import GraphNetwork
    from dgan.sr_infer import FoldedNetwork
    graph, params, stats = trained_looking("fsrgan")
    net = GraphNetwork(graph, seed=5)
    net.load_state_dict({**params, **stats})
    net.conv_math = "fp16"
    x, ref, err32 = _oracle_case("fsrgan", 1, 13, 19)
    err_u = float(np.abs(net(x, training=False).cpu().numpy() - ref).max())
    folded = FoldedNetwork(net)
    first = folded(_dev(x)).cpu().numpy()
    err_f = float(np.abs(first - ref).max())
    print(f"fp16 fsrgan 1x13x19: err_u {err_u:.3e} err_f {err_f:.3e} (fp32-accurate parent {err32:.3e})")
    assert err_u < 2e-2 and err_f <= max(1e-5, 2 * err_u)
    assert np.array_equal(folded(_dev(x)).cpu().numpy(), first)


@gpu
def test_predict_follows_set_weights():
    from dgan.graph import GraphNetwork
    from dgan.sr_infer import FoldedNetwork
    graph, params, stats = trained_looking("fsrgan")
    net = GraphNetwork(graph, seed=5)
    net.load_state_dict({**params, **stats})
    x = np.random.default_rng(1).uniform(-1, 1, (2, 13, 19, 3)).astype(np.float32)
    before = net.predict(x)
    assert isinstance(before, np.ndarray) and before.shape == (2, 52, 76, 3) and before.dtype == np.float32
    F = net._folded
    v0 = F.arena.version
    held = FoldedNetwork(net)
    held_out = held(_dev(x)).cpu().numpy()
    assert np.array_equal(held_out, before)
    w = net.get_weights()
    rng = np.random.default_rng(2)
    net.set_weights([a + (0.05 * rng.standard_normal(a.shape)).astype(np.float32) if a.ndim == 4 else a for a in w])
    after = net.predict(x)
    assert F.arena.version == v0 + 1
    assert np.abs(after - before).max() > 1e-3, "predict did not pick up the new weights"
    p2 = {n: a for (n, _), a in zip(net.arena.var_list, net.get_weights())}
    ref = oracle_forward("fsrgan", p2, stats, x)
    err_u = float(np.abs(net(x, training=False).cpu().numpy() - ref).max())
    _assert_bar(err_u, float(np.abs(after - ref).max()), "predict after set_weights")
    _assert_bar(err_u, float(np.abs(net.predict(x, batch_size=1) - ref).max()), "predict, batch_size 1")
    # the same plan, forwarded again: bit for bit; a FoldedNetwork keeps what it folded until refold()
    assert np.array_equal(F(_dev(x)).cpu().numpy(), after)
    assert np.array_equal(held(_dev(x)).cpu().numpy(), held_out)
    held.refold()
    assert np.array_equal(held(_dev(x)).cpu().numpy(), after)


# ---------------------------------------------------------------------------
# Upscaler end to end
# ---------------------------------------------------------------------------
def _expected(up, u8):
    """numpy stage -> the Upscaler's own FoldedNetwork on those tiles, in its chunks (idle tiles
    black) -> numpy unstage on the scaled geometry."""
    from dgan.infer import stage_ref, unstage_ref
    from dgan.sr_infer import scaled
    g = up.geometry(u8.shape[1], u8.shape[2])
    tiles = stage_ref(u8, g, up.pad)
    nt = tiles.shape[0]
    B = up.batch if up.tile is not None else min(up.batch, nt)
    padded = np.full((-(-nt // B) * B,) + tiles.shape[1:], -1.0, np.float32)
    padded[:nt] = tiles
    out = [up.folded(_dev(padded[t0:t0 + B])).cpu().numpy() for t0 in range(0, padded.shape[0], B)]
    return unstage_ref(np.concatenate(out)[:nt], scaled(g, up.scale))


@gpu
@pytest.mark.parametrize("h,w,kw", [(13, 19, dict()), (40, 52, dict(tile=32, margin=10, batch=4))])
def test_upscale_equals_numpy_staging_around_the_folded_forward(h, w, kw):
    from dgan.sr_infer import Upscaler
    up = Upscaler(_network("fsrgan"), 4, **kw)
    u8 = np.random.default_rng(h).integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    got = up.upscale(u8)
    assert got.dtype == np.uint8 and got.shape == (2, 4 * h, 4 * w, 3)
    assert np.array_equal(got, _expected(up, u8))
    assert len(np.unique(got)) > 16, "a flat output would show nothing"
    one = up.upscale(u8[1])
    assert one.shape == (4 * h, 4 * w, 3) and np.array_equal(one, _expected(up, u8[1:2])[0])


@gpu
def test_graph_replays_equal_eager_also_after_refresh():
    from dgan.graph import GraphNetwork
    from dgan.sr_infer import Upscaler
    graph, params, stats = trained_looking("fsrgan")
    net = GraphNetwork(graph, seed=5)
    net.load_state_dict({**params, **stats})
    eager, graphed = Upscaler(net, 4), Upscaler(net, 4, graph=True)
    rng = np.random.default_rng(4)
    outs = []
    for k in range(2):
        u8 = rng.integers(0, 256, (1, 13, 19, 3), dtype=np.uint8)
        outs.append(graphed.upscale(u8))
        assert np.array_equal(outs[-1], eager.upscale(u8)), k
    assert graphed._frames[(1, 13, 19)].graph is not None
    net.set_weights([a * np.float32(0.9) if a.ndim == 4 else a for a in net.get_weights()])
    eager.refresh()
    graphed.refresh()
    got = graphed.upscale(u8)
    assert np.array_equal(got, eager.upscale(u8))
    assert not np.array_equal(got, outs[-1]), "refresh() did not pick up the new weights"


@gpu
def test_autoencoder_upscaler_pads_to_a_multiple_of_32():
    from dgan.sr_infer import Upscaler
    up = Upscaler(_network("autoencoder"), 1, multiple=32)
    u8 = np.random.default_rng(5).integers(0, 256, (30, 45, 3), dtype=np.uint8)
    got = up.upscale(u8)
    assert got.shape == (30, 45, 3) and got.dtype == np.uint8
    assert np.array_equal(got, _expected(up, u8[None])[0])
    with pytest.raises(ValueError):
        Upscaler(_network("fsrgan"), 2).upscale(u8)   # the network scales by 4


@gpu
def test_upscale_driver_writes_x4_images(tmp_path):
    from PIL import Image
    from dgan.sr_infer import Upscaler
    net = _network("fsrgan")
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    rng = np.random.default_rng(6)
    images = {"a.png": rng.integers(0, 256, (12, 20, 3), dtype=np.uint8),
              "b.png": rng.integers(0, 256, (26, 9, 3), dtype=np.uint8)}
    for name, a in images.items():
        Image.fromarray(a, "RGB").save(src / name)
    net.save(str(tmp_path / "gen.npz"))
    r = subprocess.run([sys.executable, os.path.join(REPO, "denoise-gan_amd", "upscale.py"), "--image_dir", str(src),
                        "--output_dir", str(dst), "--model", str(tmp_path / "gen.npz")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    up = Upscaler(net, 4)
    for name, a in images.items():
        with Image.open(dst / name) as im:
            got = np.asarray(im.convert("RGB"), np.uint8)
        assert got.shape == (4 * a.shape[0], 4 * a.shape[1], 3)
        assert np.array_equal(got, up.upscale(a)), name
