"""The device resize of Pillow's convention (csrc/resize_pil.hip, dgan.resize.resize_pil) against
the integer reference `resize_pil_ref`, bit for bit: the five filters, the kernel's tile choices,
plans, `out=`, a captured replay, and SREvaluator(protocol="pil") end to end."""
import numpy as np
import pytest
import torch

from test_resize_pil import FILTERS, RAGGED, SHAPES, STEEP, image

gpu = pytest.mark.gpu
SSIM_BAR = 1e-9   # tests/test_resize_gpu.py, tests/test_metrics_gpu.py: the fp64 filter bound; PSNR to 1e-12 dB



def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@gpu
@pytest.mark.parametrize("shape", SHAPES + [RAGGED, STEEP], ids=lambda s: "%dx%d-%dx%d" % s)
@pytest.mark.parametrize("filter", FILTERS)
def test_resize_pil_equals_the_reference_bit_for_bit(filter, shape):
    from dgan.resize import resize_pil, resize_pil_ref
    hi, wi, h, w = shape
    for C, kind in ((3, "random"), (1, "random"), (3, "extremes")):
        x = image(kind, (2, hi, wi, C), hi + wi + C)
        got = resize_pil(dev(x), h, w, filter)
        want = resize_pil_ref(x, h, w, filter)
        assert got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.from_numpy(want)), (C, kind)


@gpu
def test_a_second_call_and_out_write_the_same_bits_and_allocate_nothing():
    from dgan import resize as R
    R.clear_plans()
    hi, wi, h, w = RAGGED
    x = dev(image("random", (2, hi, wi, 3), 3))
    want = torch.from_numpy(R.resize_pil_ref(x.cpu().numpy(), h, w, "lanczos"))
    first = R.resize_pil(x, h, w, "lanczos")
    out = torch.zeros((2, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    again = R.resize_pil(x, h, w, "lanczos")
    given = R.resize_pil(x, h, w, "lanczos", out=out)
    assert again is first and given is out and torch.cuda.memory_allocated() == before and len(R._plans) == 1
    assert torch.equal(again.cpu(), want) and torch.equal(out.cpu(), want)
    empty = R.resize_pil(x[:0], h, w, "lanczos")
    assert tuple(empty.shape) == (0, h, w, 3)
    R.clear_plans()
    assert not R._plans
    with pytest.raises(ValueError, match="C must be 1 or 3"):
        R.resize_pil(torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device="cuda"), 4, 4)
    with pytest.raises(ValueError, match="filter"):
        R.resize_pil(x, h, w, "nearest")
    with pytest.raises(ValueError, match="must not be the input"):
        R.resize_pil(x, hi, wi, out=x)
    with pytest.raises(ValueError, match="out must be"):
        R.resize_pil(x, h, w, out=out[:1])
    with pytest.raises(ValueError, match="dense"):
        R.resize_pil(x[:, :, ::2], h, w)
    with pytest.raises(ValueError, match="empty"):
        R.resize_pil(x, 0, w)
    with pytest.raises(ValueError, match="too steep"):
        R.resize_pil(torch.zeros((1, 100000, 2, 1), dtype=torch.uint8, device="cuda"), 10, 2)


@gpu
def test_a_captured_replay_equals_eager():
    from dgan.dist import CAPTURE_MODE
    from dgan.resize import resize_pil
    hi, wi, h, w = RAGGED
    x = dev(image("random", (1, hi, wi, 3), 4))
    eager = resize_pil(x, h, w).clone()   # (warm: the plan's tables are uploaded outside the capture)
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode=CAPTURE_MODE):
        resize_pil(x, h, w, out=out)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    x.copy_(dev(image("extremes", (1, hi, wi, 3), 5)))
    g.replay()
    assert torch.equal(out, resize_pil(x, h, w))


@gpu
def test_sr_evaluator_pil_protocol_equals_host_references():
    from dgan import metrics
    from dgan.resize import resize_pil_ref
    from dgan.sr_infer import Upscaler
    from test_resize_gpu import _hr, _network
    hr = _hr(2, 48, 68, 65)
    up = Upscaler(_network("fsrgan16"), 4)
    got = metrics.SREvaluator(up, protocol="pil").evaluate(hr)
    lr = resize_pil_ref(hr, 12, 17)
    assert np.array_equal(up.frame(2, 12, 17).u8_in.cpu().numpy(), lr)
    frames = {"bicubic": resize_pil_ref(lr, 48, 68), "upscaled": up.upscale(lr)}
    for name, a in frames.items():
        d = a.astype(np.int64) - hr.astype(np.int64)
        psnr = 10.0 * np.log10(255.0 ** 2 / ((d * d).reshape(2, -1).sum(1) / float(hr[0].size)))
        errs = (np.abs(got["psnr_" + name] - psnr).max(), np.abs(got["ssim_" + name] - metrics.ssim_ref(a, hr)).max())
        print(f"sr evaluator pil {name}: psnr err {errs[0]:.3e} ssim err {errs[1]:.3e}")
        assert errs[0] <= 1e-12 and errs[1] <= SSIM_BAR, name
    with pytest.raises(ValueError, match="protocol"):
        metrics.SREvaluator(up, protocol="pillow")
