"""dgan.filters.dejpeg on the device (csrc/dejpeg.hip) against `dejpeg_ref`, bit for bit: the shapes
at which the fused kernel can go wrong (its tile is 64 x 64), qualities, foreign tables; then the
buffers, the errors, Evaluator(baseline="dejpeg") and a captured replay."""
import functools

import numpy as np
import pytest
import torch

from test_dejpeg import photo, psnr
from test_jpeg import image

gpu = pytest.mark.gpu
SENTINEL = 0x5A
RAGGED = (2, 37, 70)
# 1x1 .. 3x2: both upsampling rules among the shifts; around a block, an MCU and the 64 x 64 tile
SHAPES = [(1, 1, 1), (1, 2, 3), (1, 3, 2), (1, 8, 8), (1, 15, 17), (1, 16, 16), (1, 17, 33), RAGGED, (1, 65, 66),
          (1, 66, 129)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def frames(kind, n, h, w):
    """uint8 [n,h,w,3], different images: random bytes, or crops of the image-like frame coded at 30."""
    from dgan.jpeg import jpeg_ref
    if kind == "random":
        a = np.stack([image("random", h, w, seed=s) for s in range(n)])
    else:
        a = np.stack([jpeg_ref(photo()[7 * s:7 * s + h, 11 * s:11 * s + w], 30) for s in range(n)])
    a.setflags(write=False)
    return a


@gpu
@pytest.mark.parametrize("kind", ["random", "coded"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dejpeg_equals_the_reference_bit_for_bit(shape, kind):
    from dgan.filters import dejpeg, dejpeg_ref
    a = frames(kind, *shape)
    assert torch.equal(dejpeg(dev(a), 50).cpu(), torch.from_numpy(dejpeg_ref(a, 50)))


@gpu
@pytest.mark.parametrize("kw", [dict(quality=10), dict(quality=95), dict(tables="30 / 80")], ids=str)
def test_qualities_and_foreign_tables_on_the_ragged_shape(kw):
    from dgan.filters import dejpeg, dejpeg_ref
    from dgan.jpeg import quant_tables
    if "tables" in kw:
        kw = dict(tables=np.stack([quant_tables(30)[0], quant_tables(80)[1]]))
    a = frames("coded", *RAGGED)
    assert torch.equal(dejpeg(dev(a), **kw).cpu(), torch.from_numpy(dejpeg_ref(a, **kw)))


@gpu
def test_buffers_and_errors():
    from dgan import ops
    from dgan.filters import dejpeg, dejpeg_ref
    from dgan.jpeg import quant_tables
    a = frames("coded", *RAGGED)
    x = dev(a)
    buf = torch.full((a.size + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[1:1 + a.size].view(a.shape)
    want = dejpeg_ref(a, 50)
    assert dejpeg(x, 50, out=out) is out and np.array_equal(out.cpu().numpy(), want)
    b = buf.cpu().numpy()
    assert (b[:1] == SENTINEL).all() and (b[1 + a.size:] == SENTINEL).all() and np.array_equal(x.cpu().numpy(), a)
    first = dejpeg(x, 50)
    assert dejpeg(x, 50).data_ptr() == first.data_ptr()
    twice = dejpeg(first, 50)
    assert twice.data_ptr() != first.data_ptr() and np.array_equal(twice.cpu().numpy(), dejpeg_ref(want, 50))
    assert tuple(dejpeg(x[:0]).shape) == (0,) + a.shape[1:]
    with pytest.raises(ValueError, match="out must not be the input"):
        dejpeg(x, 50, out=x)
    for bad, match in ((x[:, :, ::2], "dense"), (x.cpu(), "dense"), (x.float(), "uint8")):
        with pytest.raises(ValueError, match=match):
            dejpeg(bad, 50)
    with pytest.raises(ValueError, match="quality"):
        dejpeg(x, 0)
    out.fill_(SENTINEL)
    for tables in (quant_tables(50)[:1], quant_tables(50) * 0):
        with pytest.raises(ops.DGError, match="qtab"):
            ops.dejpeg(x, out, tables)
    with pytest.raises(ops.DGError, match="must not be the input"):
        ops.dejpeg(x, x, quant_tables(50))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


@gpu
def test_evaluator_scores_the_dejpeg_baseline_at_the_quality_it_degraded_with():
    from dgan import metrics
    from dgan.filters import dejpeg_ref
    from dgan.infer import Denoiser
    from dgan.jpeg import jpeg_ref
    from test_infer_gpu import _trained_w8
    clean = np.stack([photo()[:32, :48], photo()[40:72, 50:98]])
    den = Denoiser(_trained_w8())
    coded = jpeg_ref(clean, 50)
    for args, q in ((None, 50), (dict(quality=30), 30)):
        got = metrics.Evaluator(den, baseline="dejpeg", baseline_args=args).evaluate_degraded(clean, 50)
        want = dejpeg_ref(coded, q)
        assert np.abs(got["psnr_baseline"] - [psnr(want[i], clean[i]) for i in range(2)]).max() <= 1e-9
    with pytest.raises(ValueError, match="unknown keys"):
        metrics.Evaluator(den, baseline="dejpeg", baseline_args=dict(sigma=3))
    with pytest.raises(ValueError, match="quality"):
        metrics.Evaluator(den, baseline="dejpeg", baseline_args=dict(quality=0))


@gpu
def test_a_captured_replay_equals_eager():
    from dgan.dist import CAPTURE_MODE
    from dgan.filters import dejpeg, dejpeg_ref
    a, b = frames("coded", *RAGGED), frames("random", *RAGGED)
    x = dev(a)
    out = torch.zeros_like(x)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode=CAPTURE_MODE):
        dejpeg(x, 50, out=out)
    for frame in (a, b, a):
        x.copy_(dev(frame))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), dejpeg_ref(frame, 50))
