"""The device resize (csrc/resize.hip, dgan/resize.py) against the fp64 reference `resize_ref`,
bit for bit: uint8 with both conversions and fp32, both methods, the kernel's tile extents and both
of its paths, batch independence, determinism, bounds, alignment, argument errors and the plan
cache; then SREvaluator, evaluate_sr.py and the training-time baseline end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A
SSIM_BAR = 1e-9   # tests/test_metrics_gpu.py: the fp64 filter bound; PSNR from exact sums to 1e-12 dB

TH, TW = 8, 64    # the kernel's output tile (csrc/resize.hip RTH, RTW)
# (hi, wi) -> (ho, wo); the tile's extents one below, at and one above on both axes; a window of 798
# columns that fits the LDS strip (row stride 799, 8 rows of it 6392 <= 6400 doubles) and one of 802 that
# does not (the kernel's direct path)
SHAPES = [((1, 1), (3, 3)), ((3, 2), (1, 1)), ((5, 7), (5, 7)), ((8, 8), (4, 4)), ((16, 24), (4, 6)),
          ((11, 13), (44, 52)), ((37, 53), (11, 64)),
          ((5, 40), (TH - 1, TW - 1)), ((9, 64), (TH, TW)), ((17, 129), (TH + 1, TW + 1)), ((4, 33), (2 * TH, 2 * TW + 2))]
WINDOWS = [((2, 806), (2, 64)), ((2, 810), (2, 64))]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _input(kind, shape, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == "f32":
        return rng.standard_normal(shape).astype(np.float32)
    return rng.integers(0, 256, shape, dtype=np.uint8)


def _conv(kind):
    from dgan.resize import DEGRADE, DISPLAY
    return {"degrade": DEGRADE, "display": DISPLAY, "f32": (1.0, 0.0)}[kind]


def _same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _check(x, ho, wo, method, kind):
    from dgan.resize import resize, resize_ref
    mul, bias = _conv(kind)
    got = resize(dev(x), ho, wo, method, mul, bias).cpu().numpy()
    want = resize_ref(x, ho, wo, method, mul, bias)
    assert _same_bits(got, want), (x.shape, ho, wo, method, kind, int((got != want).sum()))
    return got


# ---------------------------------------------------------------------------
# kernel
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("method", ["bicubic", "bilinear"])
@pytest.mark.parametrize("shape", SHAPES + WINDOWS, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_resize_equals_the_reference_bit_for_bit(shape, method):
    (hi, wi), (ho, wo) = shape
    for C in (3, 1):
        for k, kind in enumerate(("degrade", "display", "f32")):
            _check(_input(kind, (1, hi, wi, C), 10 * C + k), ho, wo, method, kind)


@gpu
def test_a_window_wider_than_the_strip_takes_the_direct_path_to_the_same_bits():
    """C 40: the 24-column window of (16,24)->(4,6) is 960 elements, more than a strip row holds."""
    for kind in ("degrade", "f32"):
        _check(_input(kind, (2, 16, 24, 40), 5), 4, 6, "bicubic", kind)
        _check(_input(kind, (1, 11, 13, 40), 6), 44, 52, "bilinear", kind)


@gpu
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_near_ties_of_the_x2_round_trip(seed):
    """(46,50) -> (23,25) -> (46,50) with the display conversion: these seeds hold pixels whose
    unrounded value is an exact k + 0.5 or within 4.3e-14 of one, which another summation order
    or a contracted FMA flips."""
    for method in ("bicubic", "bilinear"):
        hr = _input("u8", (1, 46, 50, 3), seed)
        lr = _check(hr, 23, 25, method, "degrade")
        _check(lr, 46, 50, method, "display")
        _check(hr, 23, 25, method, "display")


@gpu
def test_several_blocks_batch_independence_and_determinism():
    """(200,300) -> (50,75) and back, n = 2: partial tiles on both axes; every image of the batch
    equals its own call and a second run gives the same bits."""
    from dgan.resize import resize
    for kind in ("degrade", "f32"):
        x = _input(kind, (2, 200, 300, 3), 21)
        lr = _check(x, 50, 75, "bicubic", kind)
        back = _check(lr, 200, 300, "bicubic", "display" if kind == "degrade" else "f32")
        _check(lr, 200, 300, "bilinear", "display" if kind == "degrade" else "f32")
        mul, bias = _conv(kind)
        for i in range(2):
            assert _same_bits(resize(dev(x[i:i + 1]), 50, 75, "bicubic", mul, bias).cpu().numpy(), lr[i:i + 1])
        mul, bias = _conv("display" if kind == "degrade" else "f32")
        assert _same_bits(resize(dev(lr), 200, 300, "bicubic", mul, bias).cpu().numpy(), back)


@gpu
@pytest.mark.parametrize("kind", ["display", "f32"])
def test_output_stays_inside_its_bounds_and_unaligned_bases_work(kind):
    """The output sits one element into a sentinel-filled buffer, the input one element into
    another: neither 4- nor 16-byte aligned, so the narrow loads and stores run."""
    from dgan.resize import resize, resize_ref
    mul, bias = _conv(kind)
    es = 4 if kind == "f32" else 1
    dt = torch.float32 if kind == "f32" else torch.uint8
    for (hi, wi), (ho, wo) in [((37, 53), (11, 64)), ((11, 13), (44, 52))]:
        x = _input(kind, (2, hi, wi, 3), 31)
        ni, no = x.size, 2 * ho * wo * 3
        ibuf = torch.zeros((ni + 16) * es, dtype=torch.uint8, device="cuda").view(dt)
        xin = ibuf[1:1 + ni].view(x.shape)
        xin.copy_(dev(x))
        obuf = torch.full(((no + 32) * es,), SENTINEL, dtype=torch.uint8, device="cuda")
        out = obuf.view(dt)[1:1 + no].view(2, ho, wo, 3)
        assert xin.data_ptr() % (4 * es) == es and out.data_ptr() % (4 * es) == es and out.is_contiguous()
        got = resize(xin, ho, wo, "bicubic", mul, bias, out=out)
        assert got is out
        assert _same_bits(out.cpu().numpy(), resize_ref(x, ho, wo, "bicubic", mul, bias))
        h = obuf.cpu().numpy()
        assert (h[:es] == SENTINEL).all() and (h[(1 + no) * es:] == SENTINEL).all()


@gpu
def test_bad_arguments_raise_and_launch_nothing():
    from dgan import ops
    from dgan.resize import resize, resize_taps
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((1, 4, 4, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="dense"):
        resize(x[:, :, ::2], 4, 4, out=out)
    with pytest.raises(ValueError, match="dense"):
        resize(x[0], 4, 4)
    with pytest.raises(ValueError, match="uint8 or float32"):
        resize(x.double(), 4, 4)
    with pytest.raises(ValueError, match="uint8 images only"):
        resize(x.float(), 4, 4, bias=0.5)
    with pytest.raises(ValueError, match="method"):
        resize(x, 4, 4, "nearest", out=out)
    with pytest.raises(ValueError, match="out must be"):
        resize(x, 4, 4, out=out.float())
    with pytest.raises(ValueError, match="out must be"):
        resize(x, 4, 5, out=out)
    with pytest.raises(ValueError, match="empty"):
        resize(x, 0, 4)
    with pytest.raises(ValueError, match="must not be the input"):
        resize(x, 8, 8, out=x)
    iy, wy = (dev(t) for t in resize_taps(8, 4))
    with pytest.raises(ops.DGError, match="resize ix"):
        ops.resize(x, out, iy, wy, iy[:3], wy)
    with pytest.raises(ops.DGError, match="resize wy"):
        ops.resize(x, out, iy, wy.float(), iy, wy)
    with pytest.raises(ops.DGError, match="does not match"):
        ops.resize(x, out.float(), iy, wy, iy, wy)
    with pytest.raises(ops.DGError, match="finite"):
        ops.resize(x, out, iy, wy, iy, wy, mul=float("inf"))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


@gpu
def test_plans_stay_bounded_and_a_repeated_call_allocates_nothing():
    from dgan import resize as R
    R.clear_plans()
    x = {w: _input("u8", (1, 12, w, 3), w) for w in range(12, 12 + 12)}
    first = {w: R.resize(dev(x[w]), 6, 2 * w).cpu().numpy().copy() for w in x}
    assert len(R._plans) == R.MAX_PLANS
    last = list(R._plans.values())[-1]
    d23 = dev(x[23])
    buf = R.resize(d23, 6, 46)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    again = R.resize(d23, 6, 46)
    assert again is buf and torch.cuda.memory_allocated() == before and list(R._plans.values())[-1] is last   # reused
    assert np.array_equal(again.cpu().numpy(), first[23])
    assert np.array_equal(R.resize(dev(x[12]), 6, 24).cpu().numpy(), first[12])   # evicted, rebuilt, still right
    assert len(R._plans) == R.MAX_PLANS


# ---------------------------------------------------------------------------
# SREvaluator, evaluate_sr.py, the training driver
# ---------------------------------------------------------------------------
def _network(kind):
    from dgan.graph import GraphNetwork
    from sr_infer_util import trained_looking
    graph, params, stats = trained_looking(kind)
    net = GraphNetwork(graph, seed=5)
    net.load_state_dict({**params, **stats})
    return net


def _hr(n, h, w, seed):
    """Image-like uint8 originals (the clean half of the dataloader's synthetic pairs)."""
    from dataloader import synthetic_pair
    size = -(-max(h, w) // 8) * 8
    y = synthetic_pair(n, size, seed=seed)[1]
    return np.floor((y[:, :h, :w] * 0.5 + 0.5) * 255.0 + 0.5).astype(np.uint8)


def _host_scores(up, hr, method="bicubic", jpeg_quality=None):
    """The four arrays and the low-resolution frame on the host: resize_ref, Upscaler.upscale of
    the reference's low-resolution frame, PSNR from the exact integer sums, ssim_ref."""
    import dataloader
    from dgan.metrics import ssim_ref
    from dgan.resize import DEGRADE, DISPLAY, resize_ref
    n, H, W = hr.shape[:3]
    s = up.scale
    lr = resize_ref(hr, H // s, W // s, method, *DEGRADE)
    if jpeg_quality is not None:
        lr = np.stack([np.rint(dataloader.jpeg_roundtrip(a / 255.0, jpeg_quality).astype(np.float64) * 255.0)
                       .astype(np.uint8) for a in lr])
    out = up.upscale(lr)
    base = resize_ref(lr, H, W, method, *DISPLAY)
    count = float(np.prod(hr.shape[1:]))

    def p(a):
        d = a.astype(np.int64) - hr.astype(np.int64)
        with np.errstate(divide="ignore"):
            return 10.0 * np.log10(255.0 ** 2 / ((d * d).reshape(n, -1).sum(1) / count))
    return {"psnr_bicubic": p(base), "psnr_upscaled": p(out), "ssim_bicubic": ssim_ref(base, hr),
            "ssim_upscaled": ssim_ref(out, hr)}, lr


@gpu
@pytest.mark.parametrize("case", ["whole", "tiled", "autoencoder_jpeg"])
def test_sr_evaluator_equals_host_references(case):
    from dgan import metrics
    from dgan.sr_infer import Upscaler
    hr = _hr(2, 96, 136, 61)
    jpeg = None
    if case == "autoencoder_jpeg":
        up, jpeg = Upscaler(_network("autoencoder"), 1, multiple=32), 75
    else:
        up = Upscaler(_network("fsrgan16"), 4, **(dict(tile=16, margin=4, batch=4) if case == "tiled" else {}))
    ev = metrics.SREvaluator(up, jpeg_quality=jpeg)
    got = ev.evaluate(hr)
    f = up.frame(2, 96 // up.scale, 136 // up.scale)
    low = f.u8_in.cpu().numpy()
    want, lr = _host_scores(up, hr, jpeg_quality=jpeg)
    assert np.array_equal(low, lr)
    assert tuple(got) == metrics.SR_SCORES
    for k in metrics.SR_SCORES:
        err = np.abs(got[k] - want[k]).max()
        print(f"sr evaluator {case} {k}: {got[k]} err {err:.3e}")
        assert got[k].shape == (2,) and got[k].dtype == np.float64
        assert err <= (1e-12 if k.startswith("psnr") else SSIM_BAR), k
    assert np.all(np.isfinite(got["psnr_bicubic"])) and got["ssim_bicubic"][0] != got["ssim_bicubic"][1]
    # a second evaluation allocates no new buffer and returns the same bits; [H,W,3] in, [1] out
    bufs = ev.buffers(hr.shape)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    again = ev.evaluate(hr)
    torch.cuda.synchronize()
    assert all(np.array_equal(again[k], got[k]) for k in got)
    assert torch.cuda.memory_allocated() == before and ev.buffers(hr.shape) is bufs and up.frame(2, *low.shape[1:3]) is f
    assert np.array_equal(bufs[0].cpu().numpy(), hr)
    one = ev.evaluate(hr[1])
    assert all(one[k].shape == (1,) for k in one)
    assert abs(one["psnr_bicubic"][0] - got["psnr_bicubic"][1]) <= 1e-12
    assert abs(one["ssim_bicubic"][0] - got["ssim_bicubic"][1]) <= SSIM_BAR
    if up.scale > 1:
        with pytest.raises(ValueError, match="97x136"):
            ev.evaluate(np.zeros((97, 136, 3), np.uint8))
    with pytest.raises(ValueError, match="8x136"):
        ev.evaluate(np.zeros((8, 136, 3), np.uint8))


@gpu
def test_sr_evaluator_on_a_graph_upscaler_equals_eager_bit_for_bit():
    from dgan import metrics
    from dgan.sr_infer import Upscaler
    net = _network("fsrgan16")
    hr = _hr(2, 96, 136, 62)
    eager = metrics.SREvaluator(Upscaler(net, 4)).evaluate(hr)
    graphed_up = Upscaler(net, 4, graph=True)
    graphed = metrics.SREvaluator(graphed_up).evaluate(hr)
    assert graphed_up._frames[(2, 24, 34)].graph is not None
    for k in metrics.SR_SCORES:
        assert np.array_equal(eager[k], graphed[k]), k


@gpu
def test_evaluate_sr_driver_writes_the_evaluators_numbers(tmp_path):
    from PIL import Image
    from dgan import metrics
    from dgan.sr_infer import Upscaler
    net = _network("fsrgan")
    images = {"a.png": _hr(1, 96, 136, 63)[0], "b.png": _hr(1, 97, 138, 64)[0]}
    (tmp_path / "hr").mkdir()
    for name, a in images.items():
        Image.fromarray(a, "RGB").save(tmp_path / "hr" / name)
    net.save(str(tmp_path / "gen.npz"))
    r = subprocess.run([sys.executable, os.path.join(REPO, "denoise-gan_amd", "evaluate_sr.py"), "--image_dir",
                        str(tmp_path / "hr"), "--model", str(tmp_path / "gen.npz"), "--json", str(tmp_path / "scores.json")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.load(open(tmp_path / "scores.json"))
    ev = metrics.SREvaluator(Upscaler(net, 4))
    assert [row["name"] for row in got["images"]] == ["a.png", "b.png"]
    assert "b.png: cropped to 136x96 at (1, 0)" in r.stdout and "a.png: cropped" not in r.stdout
    for row, a in zip(got["images"], (images["a.png"], images["b.png"][0:96, 1:137])):
        want = ev.evaluate(a)
        for k in metrics.SR_SCORES:
            assert row[k] == float(want[k][0]), (row["name"], k)
        assert f"{row['name']} psnr_bicubic {row['psnr_bicubic']:.4f}" in r.stdout
    for k in metrics.SR_SCORES:
        assert got["mean"][k] == float(np.mean([row[k] for row in got["images"]]))
    assert "mean psnr_bicubic" in r.stdout


def _events(logdir):
    path = os.path.join(logdir, "train_1", "events.jsonl")
    return [json.loads(line) for line in open(path)]


@gpu
def test_sr_driver_logs_the_bicubic_baseline_beside_the_existing_tags(tmp_path, monkeypatch):
    """train_srgan.main with metrics = 1: finite Quality/psnr_bicubic and Quality/ssim_bicubic; the
    two existing tags carry what the helper computed before it knew of `x` (restated here, on the
    same tensors); the arenas end as in a run without metrics."""
    import train_srgan
    from dgan import driver, metrics
    from dgan.models import to_device
    from test_fp16_gpu import _srgan_main_args
    real, before = driver.log_quality, []

    def both(writer, args, gen, y, step, x=None):
        assert x is not None and x.shape[1] * 4 == y.shape[1]
        yd, g = to_device(y, gen.device).contiguous(), gen.contiguous()
        before.append((metrics.psnr(g, yd, max_val=2.0).mean().item(),
                       metrics.ssim(g, yd, max_val=1.0, scale=0.5, shift=0.5).mean().item()))
        real(writer, args, gen, y, step, x=x)

    monkeypatch.setattr(driver, "log_quality", both)
    runs = {}
    for metrics_on in (1, 0):
        a = _srgan_main_args(tmp_path / str(metrics_on), 1, 0)
        a.metrics = metrics_on
        runs[metrics_on] = (train_srgan.main(a), _events(a.logdir))
    torch.cuda.synchronize()
    tags = {e["tag"]: e["value"] for e in runs[1][1] if "value" in e}
    assert np.isfinite(tags["Quality/psnr_bicubic"]) and tags["Quality/psnr_bicubic"] > 0.0, tags
    assert np.isfinite(tags["Quality/ssim_bicubic"]) and -1.0 <= tags["Quality/ssim_bicubic"] <= 1.0, tags
    assert (tags["Quality/psnr"], tags["Quality/ssim"]) == before[0]
    assert not any(e["tag"].startswith("Quality/") for e in runs[0][1])
    for na, nb in ((runs[1][0].generator, runs[0][0].generator), (runs[1][0].discriminator, runs[0][0].discriminator)):
        for t in ("data", "m", "v", "iterations"):
            assert torch.equal(getattr(na.arena, t), getattr(nb.arena, t)), t
