#!/usr/bin/env python3
"""JPEG round trip timings on the GPU (not part of bench.py): the device round trip
(csrc/jpeg.hip) of uint8 frames of 270 x 480 and 1080 x 1920, n = 1 and 8, in place, against the
host step it replaces (read the frame back, Pillow's codec one image at a time, upload it again:
SREvaluator codec="pillow") on the same frames, next to the four scores of the same frame.

    python scripts/bench_jpeg.py [--out profiles/jpeg/bench_jpeg.json]

Device-event medians over alternating windows, as scripts/bench_sr_eval.py takes them (the host
step's windows include its synchronising copies): a difference inside a path's own window spread
is not a difference.  Bytes moved are the algorithmic ones of the two launches: the frame read and
the Y / Cb / Cr planes written (3 + 1.5 bytes per pixel), the planes read and the frame written
(1.5 + 3), 3 x the frame in all; GB/s follows from the median.
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
from bench_metrics import spread  # noqa: E402

QUALITY = 50


def frames(n, h, w, seed):
    """Image-like uint8 frames: a smooth random field (16-pixel cells, blended) plus noise of sigma 6."""
    rng = np.random.default_rng(seed)
    gh, gw = h // 16 + 2, w // 16 + 2
    coarse = rng.uniform(0, 255, (n, gh, gw, 3))
    ty, tx = (np.arange(h) / 16.0), (np.arange(w) / 16.0)
    y0, x0 = ty.astype(int), tx.astype(int)
    fy, fx = (ty - y0)[None, :, None, None], (tx - x0)[None, None, :, None]
    a = coarse[:, y0][:, :, x0] * (1 - fy) * (1 - fx) + coarse[:, y0 + 1][:, :, x0] * fy * (1 - fx) \
        + coarse[:, y0][:, :, x0 + 1] * (1 - fy) * fx + coarse[:, y0 + 1][:, :, x0 + 1] * fy * fx
    return np.clip(np.rint(a + 6.0 * rng.standard_normal(a.shape)), 0, 255).astype(np.uint8)


def pillow_step(low, quality):
    """The host step: every image of the device frame `low` through Pillow's codec, in place."""
    from PIL import Image
    host = low.cpu().numpy()
    for i in range(host.shape[0]):
        buf = io.BytesIO()
        Image.fromarray(host[i], "RGB").save(buf, format="JPEG", quality=quality, subsampling=2)
        buf.seek(0)
        host[i] = np.asarray(Image.open(buf).convert("RGB"), np.uint8)
    low.copy_(torch.from_numpy(host))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_jpeg.py: no GPU (a timing needs the device; there is no fallback)")
    from dgan import _lib, metrics
    from dgan.jpeg import jpeg_roundtrip

    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "repeats": args.repeats,
           "quality": QUALITY, "library": _lib.build_info(), "frames": []}
    for h, w in ((270, 480), (1080, 1920)):
        for n in (1, 8):
            clean = frames(n, h, w, 1000 * n + h)
            ref = torch.from_numpy(clean).cuda()
            work = ref.clone()
            out4 = torch.empty((4, n), dtype=torch.float64, device="cuda")

            def restore():
                work.copy_(ref)

            def device():
                restore()
                jpeg_roundtrip(work, QUALITY, out=work)

            def host():
                restore()
                pillow_step(work, QUALITY)

            def four():
                metrics.psnr(work, ref, out=out4[0])
                metrics.psnr(work, ref, out=out4[1])
                metrics.ssim(work, ref, out=out4[2])
                metrics.ssim(work, ref, out=out4[3])

            device()
            on_device = work.cpu().numpy()
            host()
            same = bool(np.array_equal(on_device, work.cpu().numpy()))
            r = spread(alternate({"restore": restore, "device": device, "host": host, "four_scores": four},
                                 args.window, args.repeats))
            dev_ms = r["device"]["median_ms"] - r["restore"]["median_ms"]
            host_ms = r["host"]["median_ms"] - r["restore"]["median_ms"]
            nbytes = 9 * n * h * w
            row = dict(r, n=n, h=h, w=w, device_equals_host=same, device_roundtrip_ms=dev_ms, host_step_ms=host_ms,
                       host_over_device=host_ms / dev_ms, bytes=nbytes, GB_per_s=nbytes / (dev_ms * 1e-3) / 1e9,
                       device_over_four_scores=dev_ms / r["four_scores"]["median_ms"],
                       scores={"psnr": metrics.psnr(work, ref).cpu().numpy().tolist(),
                               "ssim": metrics.ssim(work, ref).cpu().numpy().tolist()},
                       what="device = copy the clean frame into the work buffer, round trip in place; host = the same "
                            "copy, then read-back, Pillow one image at a time, upload; *_ms = their medians less the "
                            "copy's (restore); four_scores = two PSNR and two SSIM of the degraded frame")
            res["frames"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"done": True, "out": args.out}))


if __name__ == "__main__":
    main()
