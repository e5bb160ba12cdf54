#!/usr/bin/env python3
"""JPEG decoder timings on the GPU (not part of bench.py): dgan.jpeg.jpeg_decode (csrc/jpeg_dec.hip)
from the files' bytes on the host to a uint8 device tensor, for n = 1 and 8 frames of 1080 x 1920
written by Pillow at quality 90, 4:2:0, against the host path it replaces (`Image.open().convert("RGB")`
of every file, then one upload) on the same files.

    python scripts/bench_jpeg_decode.py [--out profiles/jpeg/bench_jpeg_decode.json]

Medians over alternating windows, as scripts/bench_jpeg.py takes them; both paths start from host
bytes and end with the frames on the device, synchronised.  A difference inside a path's own
window spread is not a difference.  `rounds`: the synchronisation rounds across workgroups a call
ran (dgan.jpeg._decode).
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

QUALITY = 90


def pillow_frames(files):
    """The host path: Pillow decodes every file, one upload of the stacked frames."""
    from PIL import Image
    host = np.stack([np.asarray(Image.open(io.BytesIO(f)).convert("RGB"), np.uint8) for f in files])
    x = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_jpeg_decode.py: no GPU (a timing needs the device; there is no fallback)")
    from PIL import Image
    from dgan import _lib
    from dgan.jpeg import _decode, jpeg_decode, jpeg_parse

    def device_frames(files):
        return jpeg_decode(files)   # (the status read at its end synchronises)

    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "repeats": args.repeats,
           "quality": QUALITY, "library": _lib.build_info(), "frames": []}
    h, w = 1080, 1920
    for n in (1, 8):
        files = []
        for a in frames(n, h, w, 1000 * n + h):
            buf = io.BytesIO()
            Image.fromarray(a, "RGB").save(buf, format="JPEG", quality=QUALITY, subsampling=2)
            files.append(buf.getvalue())
        x, rounds = _decode(files, None, None)
        same = bool(torch.equal(x, pillow_frames(files)))
        r = spread(alternate({"device": lambda: device_frames(files), "host": lambda: pillow_frames(files)},
                             args.window, args.repeats))
        scans = [jpeg_parse(f).scan for f in files]
        row = dict(r, n=n, h=h, w=w, device_equals_host=same, scan_bytes=[e - s for s, e in scans], rounds=rounds,
                   host_over_device=r["host"]["median_ms"] / r["device"]["median_ms"],
                   what="device = jpeg_decode of the files' bytes to a device tensor (header parse, one pinned "
                        "upload, the kernels, the status read); host = Image.open().convert('RGB') of every file "
                        "and one upload of the frames")
        res["frames"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"done": True, "out": args.out}))


if __name__ == "__main__":
    main()
