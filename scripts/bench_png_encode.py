#!/usr/bin/env python3
"""PNG encoder timings on the GPU (not part of bench.py): dgan.png.png_encode (csrc/png_enc.hip) of
uint8 frames of 1080 x 1920, n = 1 and 8, the files' bytes copied to the host, against the host path
it replaces (read the frame back, Pillow's `Image.save(format="PNG")` one image at a time into
memory) on the same frames, next to the forward that makes such a frame (FastSRGAN, 270 x 480 ->
1080 x 1920), and both paths' file sizes.

    python scripts/bench_png_encode.py [--out profiles/png/bench_png_encode.json]

Medians over alternating windows, as scripts/bench_jpeg_encode.py takes them; both paths end on the
host, so their windows hold their synchronising copies.  A difference inside a path's own window
spread is not a difference.  The two paths write different files of the same pixels: the device
file is checked by decoding it.
"""
import argparse
import io
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "denoise-gan_amd"), REPO, os.path.join(REPO, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_infer import alternate  # noqa: E402
from bench_jpeg import frames  # noqa: E402
from bench_metrics import spread  # noqa: E402


def pillow_files(x):
    """The host path: read the device frames back, Pillow writes every file into memory."""
    from PIL import Image
    host = x.cpu().numpy()
    files = []
    for i in range(host.shape[0]):
        buf = io.BytesIO()
        Image.fromarray(host[i], "RGB").save(buf, format="PNG")
        files.append(buf.getvalue())
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_png_encode.py: no GPU (a timing needs the device; there is no fallback)")
    from PIL import Image
    from dgan import _lib, zoo
    from dgan.models import default_device
    from dgan.png import png_encode
    from dgan.sr_infer import Upscaler
    from dgan.sr_models import sr_generator_net

    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "repeats": args.repeats,
           "library": _lib.build_info(), "frames": []}
    h, w = 1080, 1920
    up = Upscaler(sr_generator_net(zoo.fsrgan_generator(), 0, default_device()), 4)
    for n in (1, 8):
        x = torch.from_numpy(frames(n, h, w, 1000 * n + h)).cuda()
        low = up.run(frames(n, h // 4, w // 4, n))
        files = png_encode(x)
        same = all(np.array_equal(np.asarray(Image.open(io.BytesIO(f)).convert("RGB")), a)
                   for f, a in zip(files, x.cpu().numpy()))
        r = spread(alternate({"device": lambda: png_encode(x), "host": lambda: pillow_files(x),
                              "forward": lambda: up.run_frame(low)}, args.window, args.repeats))
        row = dict(r, n=n, h=h, w=w, device_file_decodes_to_the_frame=same, device_file_bytes=[len(f) for f in files],
                   host_file_bytes=[len(f) for f in pillow_files(x)],
                   host_over_device=r["host"]["median_ms"] / r["device"]["median_ms"],
                   device_over_forward=r["device"]["median_ms"] / r["forward"]["median_ms"],
                   what="device = png_encode of the device frames, the files as host bytes; host = read-back and "
                        "Image.save(format='PNG') of each frame into memory; forward = FastSRGAN x4 to the same "
                        "frame size, stage -> forward -> unstage on the device")
        res["frames"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"done": True, "out": args.out}))


if __name__ == "__main__":
    main()
