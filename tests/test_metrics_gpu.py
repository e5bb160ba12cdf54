"""Device PSNR / SSIM (csrc/metrics.hip, dgan/metrics.py) against the fp64 numpy references:
exact integer error sums, fp64 SSIM to 1e-9, determinism, bounds, argument errors, and the
Evaluator / evaluate.py / training-driver paths end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The inputs and their products are exact in fp64; only the filter sums round.  A sum of 121
# non-negative terms <= 255^2 errs by at most 121 * 2^-53 * 65025 ~ 1e-9 (typically 1e-10 and
# less), and the variance terms it feeds stand against c2 = 58.5 in the denominators, so a factor
# moves by at most ~2e-11: 1e-9 absolute on the SSIM leaves more than an order of magnitude of
# margin.  (A plain fp32 restatement misses this bar by five orders: 2.7e-4 on the all-255 /
# all-254 pair.)
SSIM_BAR = 1e-9
SENTINEL = 0x5A


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np_sums(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    n = a.shape[0]
    return np.stack([(d * d).reshape(n, -1).sum(1), np.abs(d).reshape(n, -1).sum(1)], 1)


# ---------------------------------------------------------------------------
# error sums
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,h,w", [(3, 1, 1), (2, 7, 13), (2, 200, 300)])
def test_u8_sums_equal_numpy_int64_exactly(n, h, w):
    from dgan import metrics
    rng = np.random.default_rng(n * 100 + h)
    a = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    got = metrics.err_sums(dev(a), dev(b)).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, _np_sums(a, b))


@gpu
def test_u8_sums_above_2_to_32():
    """a = 0, b = 255 on 256 x 256 x 3: SSE 12 784 435 200 > 2^32 (a 32-bit accumulator wraps)."""
    from dgan import metrics
    a, b = np.zeros((1, 256, 256, 3), np.uint8), np.full((1, 256, 256, 3), 255, np.uint8)
    got = metrics.err_sums(dev(a), dev(b)).cpu().numpy()
    assert got.tolist() == [[12784435200, 256 * 256 * 3 * 255]]
    assert np.isclose(metrics.psnr(dev(a), dev(b)).cpu().numpy()[0], 0.0, atol=1e-12)


@gpu
def test_u8_sums_of_tensors_one_byte_into_a_buffer():
    """Neither 16- nor 4-byte aligned: the narrow path, and SSIM's byte loads."""
    from dgan import metrics
    from dgan.metrics import ssim_ref
    rng = np.random.default_rng(9)
    shape = (2, 37, 53, 3)
    count = int(np.prod(shape))
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    b = rng.integers(0, 256, shape, dtype=np.uint8)
    bufa = torch.zeros(count + 16, dtype=torch.uint8, device="cuda")
    bufb = torch.zeros(count + 16, dtype=torch.uint8, device="cuda")
    va, vb = bufa[1:1 + count].view(shape), bufb[1:1 + count].view(shape)
    va.copy_(dev(a))
    vb.copy_(dev(b))
    assert va.data_ptr() % 4 == 1 and va.is_contiguous()
    assert np.array_equal(metrics.err_sums(va, vb).cpu().numpy(), _np_sums(a, b))
    assert np.abs(metrics.ssim(va, vb).cpu().numpy() - ssim_ref(a, b)).max() <= SSIM_BAR


@gpu
def test_f32_sums_match_fp64():
    """Relative 1e-10: differences and squares are exact in fp64 (fp32 inputs), and an fp64 sum
    of n = 2e5 terms errs by at most n * 2^-53 ~ 2e-11 relative."""
    from dgan import metrics
    rng = np.random.default_rng(3)
    a = rng.uniform(-1, 1, (2, 200, 300, 3)).astype(np.float32)
    b = (a + 0.1 * rng.standard_normal(a.shape)).astype(np.float32)
    d = a.astype(np.float64) - b.astype(np.float64)
    want = np.stack([(d * d).reshape(2, -1).sum(1), np.abs(d).reshape(2, -1).sum(1)], 1)
    got = metrics.err_sums(dev(a), dev(b)).cpu().numpy()
    rel = np.abs(got - want) / want
    print("f32 sums rel", rel.max())
    assert got.dtype == np.float64 and rel.max() <= 1e-10
    p = metrics.psnr(dev(a), dev(b), max_val=2.0).cpu().numpy()
    assert np.abs(p - metrics.psnr_ref(a, b, 2.0)).max() <= 1e-9
    # a tiny case: fewer elements than one block has threads
    assert np.array_equal(metrics.err_sums(dev(a[:, :1, :2]), dev(b[:, :1, :2])).cpu().numpy(),
                          np.stack([(d[:, :1, :2] ** 2).reshape(2, -1).sum(1), np.abs(d[:, :1, :2]).reshape(2, -1).sum(1)], 1))


# ---------------------------------------------------------------------------
# SSIM
# ---------------------------------------------------------------------------
def _image_like(n, h, w, seed):
    from dataloader import synthetic_pair
    size = -(-max(h, w) // 8) * 8
    x, y = synthetic_pair(n, size, seed=seed)
    q = lambda v: np.floor((v[:, :h, :w] * 0.5 + 0.5) * 255.0 + 0.5).astype(np.uint8)
    return q(x), q(y)


def _content(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "image":
        return _image_like(shape[0], shape[1], shape[2], seed)
    if kind == "flat":
        return ((200 + rng.integers(-1, 2, shape)).astype(np.uint8), (200 + rng.integers(-1, 2, shape)).astype(np.uint8))
    assert kind == "sat"
    return np.full(shape, 255, np.uint8), np.full(shape, 254, np.uint8)


@gpu
@pytest.mark.parametrize("kind,h,w", [("random", 11, 11), ("random", 11, 64), ("random", 64, 11), ("random", 37, 53),
                                      ("random", 96, 130), ("image", 96, 130), ("flat", 37, 53), ("sat", 11, 64),
                                      ("sat", 96, 130)])
def test_ssim_u8_matches_fp64(kind, h, w):
    from dgan import metrics
    a, b = _content(kind, (2, h, w, 3), h * 131 + w)
    want = metrics.ssim_ref(a, b)
    got = metrics.ssim(dev(a), dev(b)).cpu().numpy()
    err = np.abs(got - want).max()
    print(f"ssim u8 {kind} {h}x{w}: ref {want} err {err:.3e}")
    assert got.dtype == np.float64 and got.shape == (2,)
    assert err <= SSIM_BAR


@gpu
def test_ssim_of_identical_images_is_exactly_one():
    from dgan import metrics
    a = np.random.default_rng(5).integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    assert np.array_equal(metrics.ssim(dev(a), dev(a.copy())).cpu().numpy(), np.ones(2))
    assert np.all(np.isposinf(metrics.psnr(dev(a), dev(a.copy())).cpu().numpy()))
    f = np.random.default_rng(6).uniform(-1, 1, (1, 20, 45, 3)).astype(np.float32)
    assert metrics.ssim(dev(f), dev(f.copy()), max_val=1.0, scale=0.5, shift=0.5).cpu().numpy()[0] == 1.0
    # map sizes whose count c has c * (1.0 / c) != 1.0 in fp64: the mean must divide by the count
    for shape in ((1, 96, 130, 3), (2, 200, 300, 3), (1, 64, 64, 1)):
        c = float((shape[1] - 10) * (shape[2] - 10) * shape[3])
        assert c * (1.0 / c) != 1.0, shape
        a = np.random.default_rng(shape[1]).integers(0, 256, shape, dtype=np.uint8)
        assert np.array_equal(metrics.ssim(dev(a), dev(a.copy())).cpu().numpy(), np.ones(shape[0])), shape
        g = (a.astype(np.float32) / 127.5 - 1.0).astype(np.float32)
        got = metrics.ssim(dev(g), dev(g.copy()), max_val=1.0, scale=0.5, shift=0.5).cpu().numpy()
        assert np.array_equal(got, np.ones(shape[0])), shape


@gpu
def test_each_image_of_a_batch_equals_its_own_call_bit_for_bit():
    from dgan import metrics
    a, b = _content("random", (2, 96, 130, 3), 21)
    b[1] = np.clip(a[1].astype(np.int64) + np.random.default_rng(22).integers(-9, 10, a[1].shape), 0, 255).astype(np.uint8)
    both = metrics.ssim(dev(a), dev(b)).cpu().numpy()
    sums = metrics.err_sums(dev(a), dev(b)).cpu().numpy()
    assert both[0] != both[1]
    for i in range(2):
        one = metrics.ssim(dev(a[i:i + 1]), dev(b[i:i + 1])).cpu().numpy()
        assert one[0] == both[i], i
        assert np.array_equal(metrics.err_sums(dev(a[i:i + 1]), dev(b[i:i + 1])).cpu().numpy()[0], sums[i])
    af, bf = a.astype(np.float32), b.astype(np.float32)
    fboth = metrics.err_sums(dev(af), dev(bf)).cpu().numpy()
    assert np.array_equal(metrics.err_sums(dev(af[1:]), dev(bf[1:])).cpu().numpy()[0], fboth[1])


@gpu
def test_ssim_f32_with_scale_and_shift():
    """A [-1, 1] training pair scored on [0, 1]: values (double)v * 0.5 + 0.5 (exact in fp64)."""
    from dataloader import synthetic_pair
    from dgan import metrics
    x, y = synthetic_pair(2, 64, seed=4)
    x, y = np.ascontiguousarray(x[:, :37, :53]), np.ascontiguousarray(y[:, :37, :53])
    want = metrics.ssim_ref(x.astype(np.float64) * 0.5 + 0.5, y.astype(np.float64) * 0.5 + 0.5, 1.0)
    got = metrics.ssim(dev(x), dev(y), max_val=1.0, scale=0.5, shift=0.5).cpu().numpy()
    print("ssim f32", want, np.abs(got - want).max())
    assert np.abs(got - want).max() <= SSIM_BAR
    assert 0.0 < want.min() < want.max() < 1.0


@gpu
def test_every_metric_is_deterministic():
    from dgan import metrics
    a, b = _content("random", (2, 96, 130, 3), 31)
    af, bf = dev(a.astype(np.float32) / 255), dev(b.astype(np.float32) / 255)
    da, db = dev(a), dev(b)
    calls = [lambda: metrics.err_sums(da, db), lambda: metrics.psnr(da, db), lambda: metrics.ssim(da, db),
             lambda: metrics.err_sums(af, bf), lambda: metrics.psnr(af, bf, max_val=1.0),
             lambda: metrics.ssim(af, bf, max_val=1.0), lambda: metrics.ssim(af, bf, max_val=1.0, scale=2.0, shift=-1.0)]
    for k, f in enumerate(calls):
        first = f().cpu().numpy().copy()
        assert np.array_equal(first, f().cpu().numpy()), k


# ---------------------------------------------------------------------------
# bounds and argument errors
# ---------------------------------------------------------------------------
def _guarded(nbytes, lead=64, tail=64):
    """(whole buffer, the nbytes view `lead` bytes into it), all SENTINEL."""
    buf = torch.full((lead + nbytes + tail,), SENTINEL, dtype=torch.uint8, device="cuda")
    return buf, buf[lead:lead + nbytes]


def _untouched(buf, lead, nbytes):
    h = buf.cpu().numpy()
    return bool((h[:lead] == SENTINEL).all() and (h[lead + nbytes:] == SENTINEL).all())


@gpu
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_outputs_and_workspace_stay_inside_their_bounds(dtype):
    from dgan import metrics, ops
    n, h, w = 2, 37, 53
    a, b = _content("random", (n, h, w, 3), 41)
    if dtype == "f32":
        a, b = a.astype(np.float32), b.astype(np.float32)
    da, db = dev(a), dev(b)
    ws_bytes = ops.ssim_workspace_bytes(n, h, w, 3)
    assert ws_bytes == n * 2 * 2 * 8
    wbuf, ws = _guarded(ws_bytes)
    obuf, out = _guarded(n * 8)
    ops.ssim(da, db, out.view(torch.float64), ws, 255.0)
    assert _untouched(wbuf, 64, ws_bytes) and _untouched(obuf, 64, n * 8)
    assert np.abs(out.view(torch.float64).cpu().numpy() - metrics.ssim_ref(a, b, 255.0)).max() <= SSIM_BAR
    sbuf, sums = _guarded(n * 16)
    if dtype == "u8":
        ops.err_sums(da, db, sums.view(torch.int64).view(n, 2))
        assert np.array_equal(sums.view(torch.int64).view(n, 2).cpu().numpy(), _np_sums(a, b))
    else:
        eb = ops.err_sums_workspace_bytes(n, h * w * 3)
        ebuf, ews = _guarded(eb)
        ops.err_sums(da, db, sums.view(torch.float64).view(n, 2), ews)
        assert _untouched(ebuf, 64, eb)
        assert np.array_equal(sums.view(torch.float64).view(n, 2).cpu().numpy(), _np_sums(a, b).astype(np.float64))
    assert _untouched(sbuf, 64, n * 16)


@gpu
def test_bad_arguments_raise_and_launch_nothing():
    from dgan import metrics, ops
    out = torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    small = torch.zeros((2, 10, 64, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ops.DGError, match="h, w >= 11"):
        ops.ssim(small, small, out, ws, 255.0)
    with pytest.raises(ops.DGError, match="h, w >= 11"):
        metrics.ssim(small, small)
    ok = torch.zeros((2, 96, 130, 3), dtype=torch.uint8, device="cuda")
    need = ops.ssim_workspace_bytes(2, 96, 130, 3)
    with pytest.raises(ops.DGError, match="workspace too small"):
        ops.ssim(ok, ok, out, ws[:need - 8], 255.0)
    okf = ok.float()
    sums = torch.full((2, 2), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(ops.DGError, match="workspace too small"):
        ops.err_sums(okf, okf, sums, ws[:ops.err_sums_workspace_bytes(2, 96 * 130 * 3) - 8])
    with pytest.raises(ops.DGError, match="differ"):
        metrics.psnr(ok, ok[:, :, :64].contiguous())
    with pytest.raises(ops.DGError, match="differ"):
        metrics.ssim(ok, okf, max_val=255.0)
    with pytest.raises(ops.DGError, match="uint8 or float32"):
        metrics.psnr(ok.double(), ok.double(), max_val=1.0)
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0)) and torch.equal(sums, torch.full_like(sums, 7.0))
    assert bool((ws == SENTINEL).all())


# ---------------------------------------------------------------------------
# Evaluator, evaluate.py, the training driver
# ---------------------------------------------------------------------------
def _pair_200x300():
    rng = np.random.default_rng(51)
    clean = _image_like(2, 200, 300, 52)[1]
    noisy = np.clip(clean.astype(np.int64) + np.round(12 * rng.standard_normal(clean.shape)).astype(np.int64), 0,
                    255).astype(np.uint8)
    return noisy, clean


def _host_scores(den, noisy, clean):
    """The four arrays from den.denoise(noisy) on the host: PSNR from the exact integer sums."""
    from dgan.metrics import ssim_ref
    out = den.denoise(noisy)
    count = float(np.prod(noisy.shape[1:]))
    with np.errstate(divide="ignore"):
        p = lambda a: 10.0 * np.log10(255.0 ** 2 / (_np_sums(a, clean)[:, 0] / count))
        return {"psnr_noisy": p(noisy), "psnr_denoised": p(out), "ssim_noisy": ssim_ref(noisy, clean),
                "ssim_denoised": ssim_ref(out, clean)}, out


@gpu
@pytest.mark.parametrize("kw", [dict(), dict(tile=256, margin=32, batch=4)], ids=["whole", "tiled"])
def test_evaluator_equals_host_references(kw):
    """SSIM to 1e-9; PSNR to 1e-12 dB: the sums are exact, and mse, the quotient, log10 and the
    product round four times at 2^-53 relative on values below 100 dB (~ 1e-13)."""
    from dgan import metrics
    from dgan.infer import Denoiser
    from test_infer_gpu import _trained_w8
    G = _trained_w8()
    noisy, clean = _pair_200x300()
    den = Denoiser(G, **kw)
    ev = metrics.Evaluator(den)
    got = ev.evaluate(noisy, clean)
    want, out = _host_scores(den, noisy, clean)
    assert set(got) == set(metrics.SCORES)
    for k in metrics.SCORES:
        err = np.abs(got[k] - want[k]).max()
        print(f"evaluator {k}: {got[k]} err {err:.3e}")
        assert got[k].shape == (2,) and got[k].dtype == np.float64
        assert err <= (1e-12 if k.startswith("psnr") else SSIM_BAR), k
    f = den.run(noisy)
    assert np.array_equal(metrics.err_sums(f.u8_out, dev(clean)).cpu().numpy(), _np_sums(out, clean))
    assert np.array_equal(metrics.err_sums(f.u8_in, dev(clean)).cpu().numpy(), _np_sums(noisy, clean))
    assert got["ssim_noisy"][0] != got["ssim_noisy"][1] and 0 < got["ssim_noisy"].min() < 1
    assert np.all(np.isfinite(got["psnr_denoised"])) and np.all(np.abs(got["ssim_denoised"]) < 1)
    # a second evaluation allocates nothing new and returns the same bits; [h,w,3] in, [1] out
    ref = ev.buffers(noisy.shape)[0]
    again = ev.evaluate(noisy, clean)
    assert all(np.array_equal(again[k], got[k]) for k in got) and ev.buffers(noisy.shape)[0] is ref
    assert np.array_equal(ref.cpu().numpy(), clean)
    one = ev.evaluate(noisy[1], clean[1])
    assert all(one[k].shape == (1,) for k in one) and abs(one["ssim_noisy"][0] - got["ssim_noisy"][1]) <= SSIM_BAR


@gpu
def test_evaluator_on_a_graph_denoiser_equals_eager_bit_for_bit():
    from dgan import metrics
    from dgan.infer import Denoiser
    from test_infer_gpu import _trained_w8
    G = _trained_w8()
    noisy, clean = _pair_200x300()
    eager = metrics.Evaluator(Denoiser(G)).evaluate(noisy, clean)
    graphed_den = Denoiser(G, graph=True)
    graphed = metrics.Evaluator(graphed_den).evaluate(noisy, clean)
    assert graphed_den._frames[(2, 200, 300)].graph is not None
    for k in metrics.SCORES:
        assert np.array_equal(eager[k], graphed[k]), k


@gpu
def test_evaluate_driver_writes_the_evaluators_numbers(tmp_path):
    from PIL import Image
    from dgan import metrics
    from dgan.infer import Denoiser
    from test_infer_gpu import _trained_w8
    G = _trained_w8()
    noisy, clean = _pair_200x300()
    (tmp_path / "noisy").mkdir()
    (tmp_path / "clean").mkdir()
    for i, name in enumerate(("a", "b")):
        Image.fromarray(noisy[i], "RGB").save(tmp_path / "noisy" / f"{name}.png")
        Image.fromarray(clean[i], "RGB").save(tmp_path / "clean" / f"{name}.png")
    G.save(str(tmp_path / "gen.npz"))
    r = subprocess.run([sys.executable, os.path.join(REPO, "denoise-gan_amd", "evaluate.py"), "--image_dir",
                        str(tmp_path / "noisy"), "--target_dir", str(tmp_path / "clean"), "--model",
                        str(tmp_path / "gen.npz"), "--json", str(tmp_path / "scores.json")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.load(open(tmp_path / "scores.json"))
    ev = metrics.Evaluator(Denoiser(G))
    assert [row["name"] for row in got["images"]] == ["a.png", "b.png"]
    for i, row in enumerate(got["images"]):
        want = ev.evaluate(noisy[i], clean[i])
        for k in metrics.SCORES:
            assert row[k] == float(want[k][0]), (i, k)
        assert f"{row['name']} psnr_noisy {row['psnr_noisy']:.4f}" in r.stdout
    for k in metrics.SCORES:
        assert got["mean"][k] == float(np.mean([row[k] for row in got["images"]]))
    assert "mean psnr_noisy" in r.stdout


def _events(logdir):
    path = os.path.join(logdir, "train_1", "events.jsonl")
    return [json.loads(line) for line in open(path)]


@gpu
def test_sr_driver_logs_quality_of_the_upscaled_output(tmp_path):
    """The SR family's generator is the layer-graph executor: its 4x output (32 x 32 from 8 x 8)
    is scored against the high-resolution target by the same helper."""
    import train_srgan
    from test_fp16_gpu import _srgan_main_args
    a = _srgan_main_args(tmp_path, 1, 0)
    a.metrics = 1
    train_srgan.main(a)
    tags = {e["tag"]: e["value"] for e in _events(a.logdir) if "value" in e}
    assert np.isfinite(tags["Quality/psnr"]) and tags["Quality/psnr"] > 0.0, tags
    assert -1.0 <= tags["Quality/ssim"] <= 1.0, tags


@gpu
def test_training_driver_logs_quality_without_touching_the_training_state(tmp_path):
    import train_pix2pix
    from test_boundary_gpu import _main_args
    runs = {}
    for metrics_on in (1, 0):
        a = _main_args(tmp_path / str(metrics_on), 1, 0)
        a.metrics = metrics_on
        runs[metrics_on] = (train_pix2pix.main(a), _events(a.logdir))
    torch.cuda.synchronize()
    tags = {e["tag"]: e["value"] for e in runs[1][1] if "value" in e}
    assert np.isfinite(tags["Quality/psnr"]) and 0.0 < tags["Quality/ssim"] <= 1.0, tags
    assert not any(e["tag"].startswith("Quality/") for e in runs[0][1])
    assert "Generator Losses/gen_total_loss" in {e["tag"] for e in runs[0][1]}
    for na, nb in ((runs[1][0].generator, runs[0][0].generator), (runs[1][0].discriminator, runs[0][0].discriminator)):
        for t in ("data", "m", "v", "iterations"):
            assert torch.equal(getattr(na.arena, t), getattr(nb.arena, t)), t
        for k, v in na.bn.export().items():
            assert np.array_equal(v, nb.bn.export()[k]), k


@gpu
def test_plans_and_evaluator_buffers_stay_bounded():
    """Many image sizes (a directory through evaluate.py) keep at most MAX_PLANS plans and
    MAX_SHAPES clean frames; a kept plan is reused, an evicted one is rebuilt and still right."""
    from dgan import metrics

    class NoDenoiser:
        device = torch.device("cuda")

    metrics.clear_plans()
    a = {w: np.random.default_rng(w).integers(0, 256, (1, 12, w, 3), dtype=np.uint8) for w in range(12, 12 + 12)}
    first = {w: metrics.ssim(dev(a[w]), dev(a[w][:, ::-1].copy())).cpu().numpy().copy() for w in a}
    assert len(metrics._plans) == metrics.MAX_PLANS
    last = list(metrics._plans.values())[-1]
    assert np.array_equal(metrics.ssim(dev(a[23]), dev(a[23][:, ::-1].copy())).cpu().numpy(), first[23])
    assert list(metrics._plans.values())[-1] is last                      # reused
    assert np.array_equal(metrics.ssim(dev(a[12]), dev(a[12][:, ::-1].copy())).cpu().numpy(), first[12])   # rebuilt
    assert len(metrics._plans) == metrics.MAX_PLANS
    ev = metrics.Evaluator(NoDenoiser())
    kept = ev.buffers((1, 12, 12, 3))
    for w in range(13, 13 + ev.MAX_SHAPES - 1):
        ev.buffers((1, 12, w, 3))
    assert ev.buffers((1, 12, 12, 3)) is kept and len(ev._bufs) == ev.MAX_SHAPES
    ev.buffers((1, 12, 99, 3))
    assert len(ev._bufs) == ev.MAX_SHAPES and (1, 12, 13, 3) not in ev._bufs
