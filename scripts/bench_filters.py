#!/usr/bin/env python3
"""Classical filter timings on the GPU (not part of bench.py): the device 3x3 median and non-local
means (csrc/filters.hip) of 1080 x 1920 uint8 frames, n = 1 and 8; the median's traffic; the NLM
against the host path it replaces (read the frame back, `nlm_ref`, upload: timed once on a
270 x 480 crop and scaled by area) and against the same frame's `Denoiser` forward.

    python scripts/bench_filters.py [--out profiles/filters/bench_filters.json]

Device-event medians over alternating windows, as scripts/bench_jpeg.py takes them: a difference
inside a path's own window spread is not a difference.  The median moves 2 x the frame (read once,
written once; the rows above and below come from cache).  NLM work is counted from the design, in
vector integer instructions per lane (`nlm_lane_ops`): a dot product, an add, a multiply-add, a
shift, a min or a byte extract is one.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "denoise-gan_amd"), REPO, os.path.join(REPO, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_infer import alternate  # noqa: E402
from bench_jpeg import frames  # noqa: E402
from bench_metrics import spread  # noqa: E402

H = 10
SETTINGS = ((7, 21), (3, 7))
TILE, THREADS, SEG, PIX = 32, 256, 8, 4   # csrc/filters.hip NTH = NTW, NT, NSEG, NPIX
# One-off figures, copied into every result file: this script cannot take them again.  The kernel
# once had a second variant that formed the squared differences channel by channel (no dot
# products, no N); both were in one library and alternated in one run of this script on one
# MI355X before the slower one was removed.  Median ms of 1080 x 1920 frames at h = 10.
REMOVED_VARIANT = {
    "what": "one-off: k_nlm with dot products (kept) against channel by channel (removed), same run, same library",
    "n1_t7_s21_ms": {"dot": 0.7929, "plain": 1.0566}, "n8_t7_s21_ms": {"dot": 5.7836, "plain": 7.4547},
    "n1_t3_s7_ms": {"dot": 0.0933, "plain": 0.1103}, "n8_t3_s7_ms": {"dot": 0.6608, "plain": 0.7715}}


def nlm_lane_ops(t):
    """Vector integer instructions per pixel and offset of k_nlm, from its design:
    phase 1, (TILE + t - 1) * TILE / SEG threads: SEG + t - 1 dot products, t - 1 adds for the first
    running sum, 2 per further column; phase 2, every thread: t - 1 + 2 (PIX - 1) for the running
    sums, and per pixel 3 for D = N(p) + N(p+d) - 2 box, 2 for the division by 3 t^2, a min, the
    sum of weights, 3 byte extracts and 3 multiply-adds."""
    p1 = (TILE + t - 1) * (TILE // SEG) * ((SEG + t - 1) + (t - 1) + 2 * (SEG - 1))
    p2 = THREADS * ((t - 1) + 2 * (PIX - 1) + PIX * 13)
    return (p1 + p2) / float(TILE * TILE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_filters.py: no GPU (a timing needs the device; there is no fallback)")
    from dgan import _lib
    from dgan.filters import median3, nlm, nlm_ref
    from dgan.infer import Denoiser
    from dgan.models import Generator

    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "repeats": args.repeats, "nlm_h": H,
           "library": _lib.build_info(), "removed_variant": REMOVED_VARIANT, "frames": []}
    h, w = 1080, 1920

    # the host path on a crop: read-back, nlm_ref, upload
    crop = torch.from_numpy(frames(1, 270, 480, 7)).cuda()
    host = {}
    for t, s in SETTINGS:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        back = torch.from_numpy(nlm_ref(crop.cpu().numpy(), H, t, s)).cuda()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        same = bool(torch.equal(back, nlm(crop, H, t, s)))
        host[f"t{t}_s{s}"] = {"crop_270x480_ms": ms, "scaled_to_1080x1920_ms": ms * (h * w) / (270.0 * 480.0),
                              "device_equals_host": same}
    res["host_nlm"] = host
    print(json.dumps(host), flush=True)

    den = Denoiser(Generator(width=1, seed=5))
    for n in (1, 8):
        x = torch.from_numpy(frames(n, h, w, 1000 * n + h)).cuda()
        out = torch.empty_like(x)
        fns = {"median3": lambda: median3(x, out=out)}
        for t, s in SETTINGS:
            fns[f"nlm_t{t}_s{s}"] = lambda t=t, s=s: nlm(x, H, t, s, out=out)
        if n == 1:
            f = den.run(x.cpu().numpy())
            fns["forward"] = lambda: den._run(f)
        r = spread(alternate(fns, args.window, args.repeats))
        row = dict(r, n=n, h=h, w=w)
        ms = r["median3"]["median_ms"]
        row["median3_bytes"] = 2 * x.numel()
        row["median3_GB_per_s"] = 2 * x.numel() / (ms * 1e-3) / 1e9
        for t, s in SETTINGS:
            k = f"nlm_t{t}_s{s}"
            ms = r[k]["median_ms"]
            ops = nlm_lane_ops(t) * s * s * n * h * w
            row[k + "_lane_ops_per_pixel_offset"] = nlm_lane_ops(t)
            row[k + "_T_lane_ops_per_s"] = ops / (ms * 1e-3) / 1e12
            row[k + "_host_over_device"] = host[f"t{t}_s{s}"]["scaled_to_1080x1920_ms"] * n / ms
            if n == 1:
                row[k + "_over_forward"] = ms / r["forward"]["median_ms"]
        res["frames"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"done": True, "out": args.out}))


if __name__ == "__main__":
    main()
