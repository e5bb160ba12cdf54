"""The device JPEG decoder (csrc/jpeg_dec.hip, dgan.jpeg.jpeg_decode) against the numpy definition
`jpeg_decode_ref` (which tests/test_jpeg_decode.py holds equal to Pillow's decoder), bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_jpeg import image
from test_jpeg_decode import SIZES, cases, cut_file, flat_file, pillow_file

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (1,1): a scan shorter than one subsequence; (128,256) binary q100: a scan across three workgroups
# with stuffed bytes, blocks without EOB and ZRL; flat: some 190 four-bit blocks per subsequence,
# which synchronise only from the lane before
CASES = list(cases(SIZES + [(128, 256)]))


@gpu
@pytest.mark.parametrize("size", sorted({name.split("-")[0] for name, _ in CASES}))
def test_device_pixels_equal_the_reference_bit_for_bit(size):
    from dgan.jpeg import jpeg_decode, jpeg_decode_ref
    for name, data in CASES:
        if name.split("-")[0] == size:
            got = jpeg_decode([data])
            assert got.dtype == torch.uint8 and got.is_cuda
            want = jpeg_decode_ref(data)
            assert got.shape == (1,) + want.shape and np.array_equal(got[0].cpu().numpy(), want), name


@gpu
def test_the_longest_case_spans_three_workgroups():
    from dgan.jpeg import DECODE_LANES, DECODE_SUBSEQUENCE, _decode, jpeg_decode_ref, jpeg_parse
    from dgan import ops
    data = dict(CASES)["128x256-binary-q100-opt0"]
    first, end = jpeg_parse(data).scan
    stuffed = data[first:end].count(b"\xff\x00")
    assert stuffed > 100 and end - first - stuffed > 2 * DECODE_SUBSEQUENCE * DECODE_LANES
    assert ops.jpeg_decode_geometry() == (DECODE_SUBSEQUENCE, DECODE_LANES)
    got, rounds = _decode([data], None, None)
    assert np.array_equal(got[0].cpu().numpy(), jpeg_decode_ref(data))
    assert 1 <= rounds <= 2


@gpu
def test_every_image_of_a_batch_equals_its_own_call():
    """Three files of one size with three sets of tables: q10, q90 and q50 with optimised Huffman
    tables; Cb and Cr differ, so a mixed-up chroma path shows."""
    from dgan.jpeg import jpeg_decode, jpeg_decode_ref
    a = image("random", 67, 130)
    a[..., 2] = 255 - a[..., 0]
    files = [pillow_file(a, quality=10), pillow_file(image("gradient", 67, 130), quality=90),
             pillow_file(a, quality=50, optimize=True)]
    got = jpeg_decode(files).cpu().numpy()
    assert got.shape == (3, 67, 130, 3)
    for i, f in enumerate(files):
        assert np.array_equal(got[i], jpeg_decode([f])[0].cpu().numpy()), i
        assert np.array_equal(got[i], jpeg_decode_ref(f)), i
    out = torch.zeros((3, 67, 130, 3), dtype=torch.uint8, device="cuda")
    assert jpeg_decode(files, out=out) is out and np.array_equal(out.cpu().numpy(), got)


@gpu
@pytest.mark.parametrize("quality", [10, 90])
def test_decoding_the_encoders_files_is_the_round_trip(quality):
    from dgan.jpeg import jpeg_decode, jpeg_encode, jpeg_roundtrip
    x = torch.from_numpy(np.stack([image("random", 67, 130), image("gradient", 67, 130)])).cuda()
    assert torch.equal(jpeg_decode(jpeg_encode(x, quality)), jpeg_roundtrip(x, quality))


@gpu
def test_a_plan_serves_a_longer_and_then_a_shorter_scan():
    from dgan import jpeg as J
    J.clear_plans()
    files = [pillow_file(image(kind, 67, 130), quality=q) for kind, q in (("gradient", 50), ("binary", 100), ("random", 10))]
    for f in files + files[:1]:
        assert np.array_equal(J.jpeg_decode([f])[0].cpu().numpy(), J.jpeg_decode_ref(f))
    assert len(J._plans) == 1
    assert J.jpeg_decode([]).shape == (0, 0, 0, 3)


@gpu
def test_bad_files_raise():
    from dgan.jpeg import JpegUnsupported, jpeg_decode
    good = pillow_file(image("random", 67, 130), quality=90)
    with pytest.raises(ValueError, match="file 1: the scan ends"):
        jpeg_decode([good, cut_file(good)])
    with pytest.raises(ValueError, match="file 0"):
        jpeg_decode([cut_file(flat_file())])
    with pytest.raises(ValueError, match="one size"):
        jpeg_decode([good, flat_file()])
    with pytest.raises(JpegUnsupported, match="progressive"):
        jpeg_decode([pillow_file(image("random", 67, 130), progressive=True)])
    with pytest.raises(TypeError, match="bytes"):
        jpeg_decode([np.frombuffer(good, np.uint8)])
    with pytest.raises(ValueError, match="out must be"):
        jpeg_decode([], out=torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda"))
    assert jpeg_decode([good]).shape == (1, 67, 130, 3)   # and the next call is sound


@gpu
def test_infer_driver_decodes_on_the_device(tmp_path):
    """infer.py --decode device on a .jpg and a .png with a width-8 generator writes what
    --decode pillow writes."""
    from PIL import Image
    from dgan.models import Generator
    Generator(width=8).save(str(tmp_path / "gen.npz"))
    (tmp_path / "in").mkdir()
    (tmp_path / "in" / "a.jpg").write_bytes(pillow_file(image("random", 40, 56), quality=90))
    Image.fromarray(image("gradient", 33, 17), "RGB").save(tmp_path / "in" / "b.png")
    outs = {}
    for decode in ("pillow", "device"):
        r = subprocess.run([sys.executable, os.path.join(REPO, "denoise-gan_amd", "infer.py"), "--image_dir",
                            str(tmp_path / "in"), "--output_dir", str(tmp_path / decode), "--model", str(tmp_path / "gen.npz"),
                            "--decode", decode], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[decode] = {f: np.asarray(Image.open(tmp_path / decode / f).convert("RGB")) for f in sorted(os.listdir(tmp_path / decode))}
        assert ("Pillow" in r.stdout) == (decode == "device"), r.stdout
    assert sorted(outs["device"]) == ["a.jpg", "b.png"]
    for f in outs["pillow"]:
        assert np.array_equal(outs["device"][f], outs["pillow"][f]), f
