#!/usr/bin/env python3
"""JPEG artifact removal timings on the GPU (not part of bench.py): the fused shift-averaged
re-application (dgan.filters.dejpeg, csrc/dejpeg.hip) of 1080 x 1920 uint8 frames at quality 50,
n = 1 and 8, against the composition it replaces on the same machine (64 times: the shifted frame by
two index_select, dgan.jpeg.jpeg_roundtrip, crop and accumulate in int32; then (sum + 32) >> 6), and
against the same frame's `Denoiser` forward.  PSNR before / after on the image-like frame of
tests/test_dejpeg.py, device result.

    python scripts/bench_dejpeg.py [--out profiles/dejpeg/bench_dejpeg.json]

Device-event medians over alternating windows, as scripts/bench_jpeg.py takes them: a difference
inside a path's own window spread is not a difference.
"""
import argparse
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

QUALITY = 50


def photo():
    """uint8 [128,128,3]: correlated channels, a stripe pattern and a coloured disk."""
    from dataloader import synthetic_pair
    _, y = synthetic_pair(1, 128, seed=3)
    g = y[0].mean(-1, keepdims=True)
    yy, xx = np.mgrid[0:128, 0:128]
    base = (g * 0.4 + 0.5) * 255 + 0.15 * 255 * y[0] * 0.3
    base = base + (((xx * 0.7 + yy * 0.4) % 37 < 18) * 50 - 25)[..., None]
    base = base + (((xx - 64) ** 2 + (yy - 60) ** 2 < 900)[..., None] * np.array([40, -10, -30]))
    return np.clip(base, 0, 255).astype(np.uint8)


def psnr(a, b):
    return float(10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def composed(x, acc, out, index):
    """The 64 round trips with existing ops and torch: x [n,h,w,3] uint8 -> out.  index[d]: the
    device row / column numbers of a frame shifted by d (max(i - d, 0)), made once outside."""
    from dgan.jpeg import jpeg_roundtrip
    acc.zero_()
    for dy in range(8):
        for dx in range(8):
            s = x.index_select(1, index[0][dy]).index_select(2, index[1][dx]) if dy or dx else x
            acc += jpeg_roundtrip(s, QUALITY)[:, dy:, dx:]
    out.copy_((acc + 32) >> 6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dejpeg.py: no GPU (a timing needs the device; there is no fallback)")
    from dgan import _lib
    from dgan.filters import dejpeg
    from dgan.infer import Denoiser
    from dgan.jpeg import jpeg_roundtrip
    from dgan.models import Generator

    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "repeats": args.repeats,
           "quality": QUALITY, "library": _lib.build_info(), "frames": []}

    img = photo()
    res["psnr_image_like_128"] = {}
    for q in (10, 50):
        coded = jpeg_roundtrip(torch.from_numpy(img[None]).cuda(), q).clone()
        after = dejpeg(coded, q)
        res["psnr_image_like_128"][str(q)] = {"jpeg": psnr(coded.cpu().numpy()[0], img),
                                              "dejpeg": psnr(after.cpu().numpy()[0], img)}
    print(json.dumps(res["psnr_image_like_128"]), flush=True)

    h, w = 1080, 1920
    den = Denoiser(Generator(width=1, seed=5))
    for n in (1, 8):
        x = torch.from_numpy(frames(n, h, w, 1000 * n + h)).cuda()
        out, out2 = torch.empty_like(x), torch.empty_like(x)
        acc = torch.empty(x.shape, dtype=torch.int32, device=x.device)
        index = [[torch.clamp(torch.arange(-d, size, device=x.device), min=0) for d in range(8)] for size in (h, w)]
        same = bool(torch.equal(dejpeg(x, QUALITY, out=out), composed(x, acc, out2, index)))
        fns = {"dejpeg": lambda: dejpeg(x, QUALITY, out=out), "composition": lambda: composed(x, acc, out2, index)}
        if n == 1:
            f = den.run(x.cpu().numpy())
            fns["forward"] = lambda: den._run(f)
        r = spread(alternate(fns, args.window, args.repeats))
        row = dict(r, n=n, h=h, w=w, fused_equals_composition=same)
        row["composition_over_dejpeg"] = r["composition"]["median_ms"] / r["dejpeg"]["median_ms"]
        if n == 1:
            row["dejpeg_over_forward"] = r["dejpeg"]["median_ms"] / r["forward"]["median_ms"]
        res["frames"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"done": True, "out": args.out}))


if __name__ == "__main__":
    main()
