"""The device PNG encoder (csrc/png_enc.hip, dgan.png.png_encode) against the numpy definition
`png_encode_ref` (which tests/test_png.py holds decodable and small), byte for byte."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_jpeg import image
from test_png import SIZES, frames, run_streams

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@gpu
@pytest.mark.parametrize("size", SIZES + [(8, 200)], ids=lambda s: f"{s[0]}x{s[1]}")   # 8x200: runs past 258
def test_device_files_equal_the_reference_byte_for_byte(size):
    from dgan.png import png_encode, png_encode_ref
    for kind, a in frames(size):
        got, want = png_encode(dev(a[None])), png_encode_ref(a)
        assert len(got) == 1 and isinstance(got[0], bytes)
        assert got[0] == want, (size, kind, len(got[0]), len(want))


@gpu
@pytest.mark.parametrize("name", ["runs", "crossing", "empty", "fibonacci"])
def test_the_deflate_op_equals_the_reference(name):
    from dgan import ops
    from dgan.png import deflate_ref
    d = run_streams()[name]
    out, sizes = ops.png_deflate(dev(np.frombuffer(d, np.uint8).copy()[None]))
    assert out[0, :int(sizes[0])].cpu().numpy().tobytes() == deflate_ref(d)


@gpu
def test_every_file_of_a_batch_equals_its_own_call():
    from dgan.png import png_encode, png_encode_ref
    imgs = np.stack([image("random", 64, 171, seed=1), image("gradient", 64, 171), image("binary", 64, 171, seed=2)])
    got = png_encode(dev(imgs))
    assert len(got) == 3 and len({len(f) for f in got}) == 3
    for i in range(3):
        assert got[i] == png_encode(dev(imgs[i:i + 1]))[0] == png_encode_ref(imgs[i]), i


@gpu
def test_repeated_calls_and_reused_plans_give_the_same_bytes():
    from dgan import png as P
    P.clear_plans()
    x, other = dev(image("gradient", 17, 33)[None]), dev(image("binary", 64, 171)[None])
    first = P.png_encode(x)
    assert P.png_encode(x) == first
    big = P.png_encode(other)
    assert P.png_encode(x) == first == [P.png_encode_ref(image("gradient", 17, 33))]
    assert P.png_encode(other) == big
    assert len(P._plans) == 2
    assert P.png_encode(x[:0]) == []


@gpu
def test_bad_arguments_raise():
    from dgan.png import png_encode
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="uint8"):
        png_encode(x.float())
    for bad in (x[0], x.cpu(), x[:, :, ::2], x[..., :2].contiguous()):
        with pytest.raises(ValueError, match="dense"):
            png_encode(bad)
    with pytest.raises(ValueError, match="empty"):
        png_encode(x[:, :0])
    for shape in ((1, 1, 65536, 3), (1, 65536, 1, 3)):
        with pytest.raises(ValueError, match="65535"):
            png_encode(torch.zeros(shape, dtype=torch.uint8, device="cuda"))


@gpu
def test_infer_driver_writes_the_device_files(tmp_path):
    """infer.py --format png on a width-8 generator and two images: every <stem>.png decodes to
    exactly the frame the Denoiser returns."""
    from PIL import Image
    from dgan.infer import Denoiser
    from dgan.models import Generator
    G = Generator(width=8)
    G.save(str(tmp_path / "gen.npz"))
    (tmp_path / "in").mkdir()
    images = {"a.png": image("random", 40, 56), "b.png": image("gradient", 33, 17)}
    for name, a in images.items():
        Image.fromarray(a, "RGB").save(tmp_path / "in" / name)
    r = subprocess.run([sys.executable, os.path.join(REPO, "denoise-gan_amd", "infer.py"), "--image_dir",
                        str(tmp_path / "in"), "--output_dir", str(tmp_path / "out"), "--model", str(tmp_path / "gen.npz"),
                        "--format", "png"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path / "out")) == ["a.png", "b.png"]
    den = Denoiser(G)
    for name, a in images.items():
        data = (tmp_path / "out" / name).read_bytes()
        assert b"IDAT\x78\x01" in data[:64]   # this encoder's file, not Pillow's
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), den.denoise(a)), name
