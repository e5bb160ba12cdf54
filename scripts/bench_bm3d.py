#!/usr/bin/env python3
"""BM3D timings on the GPU (not part of bench.py): the device stage-1 BM3D (csrc/bm3d.hip) of
1080 x 1920 uint8 frames, n = 1 and 8, sigma 25, search 21 and 7, against the host path it replaces
(read the frame back, `bm3d_ref`, upload: timed once on a 270 x 480 crop and scaled by area), against
non-local means (t 7 / s 21 and t 3 / s 7, h = 25) and against the same frame's `Denoiser` forward,
all in one run; and the PSNR of the noisy frame, of `nlm` and of `bm3d` against the clean frame.

    python scripts/bench_bm3d.py [--out profiles/filters/bench_bm3d.json]

The clean frame is scripts/bench_jpeg.py's image-like field (which carries a sigma-6 texture of its
own, so no filter can reach much above 32 dB); the noisy frame adds Gaussian noise of sigma 25.
Device-event medians over alternating windows, as scripts/bench_filters.py takes them: a difference
inside a path's own window spread is not a difference.
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

SIGMA, GROUP = 25, 16
SEARCHES = (21, 7)
NLM = ((7, 21), (3, 7))


def noised(clean, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(clean + SIGMA * rng.standard_normal(clean.shape)), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_bm3d.py: no GPU (a timing needs the device; there is no fallback)")
    from dgan import _lib, metrics
    from dgan.filters import bm3d, bm3d_ref, nlm
    from dgan.infer import Denoiser
    from dgan.models import Generator

    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "repeats": args.repeats, "sigma": SIGMA,
           "group": GROUP, "nlm_h": SIGMA, "library": _lib.build_info(), "frames": []}
    h, w = 1080, 1920

    # the host path on a crop: read-back, bm3d_ref, upload
    crop = torch.from_numpy(noised(frames(1, 270, 480, 7), 8)).cuda()
    host = {}
    for s in SEARCHES:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        back = torch.from_numpy(bm3d_ref(crop.cpu().numpy(), SIGMA, s, GROUP)).cuda()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        same = bool(torch.equal(back, bm3d(crop, SIGMA, s, GROUP)))
        host[f"s{s}"] = {"crop_270x480_ms": ms, "scaled_to_1080x1920_ms": ms * (h * w) / (270.0 * 480.0),
                         "device_equals_host": same}
        print(json.dumps(host), flush=True)
    res["host_bm3d"] = host

    den = Denoiser(Generator(width=1, seed=5))
    for n in (1, 8):
        clean = frames(n, h, w, 1000 * n + h)
        x, ref = torch.from_numpy(noised(clean, n)).cuda(), torch.from_numpy(clean).cuda()
        out = torch.empty_like(x)
        fns = {f"bm3d_s{s}": (lambda s=s: bm3d(x, SIGMA, s, GROUP, out=out)) for s in SEARCHES}
        for t, s in NLM:
            fns[f"nlm_t{t}_s{s}"] = lambda t=t, s=s: nlm(x, SIGMA, t, s, out=out)
        if n == 1:
            f = den.run(x.cpu().numpy())
            fns["forward"] = lambda: den._run(f)
        row = dict(spread(alternate(fns, args.window, args.repeats)), n=n, h=h, w=w)
        for s in SEARCHES:
            k = f"bm3d_s{s}"
            row[k + "_host_over_device"] = host[f"s{s}"]["scaled_to_1080x1920_ms"] * n / row[k]["median_ms"]
            row[k + "_over_nlm_t7_s21"] = row[k]["median_ms"] / row["nlm_t7_s21"]["median_ms"]
            if n == 1:
                row[k + "_over_forward"] = row[k]["median_ms"] / row["forward"]["median_ms"]
        if n == 1:
            psnr = {"noisy": float(metrics.psnr(x, ref).item())}
            for k, fn in fns.items():
                if k != "forward":
                    psnr[k] = float(metrics.psnr(fn(), ref).item())
            row["psnr_db"] = psnr
        res["frames"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"done": True, "out": args.out}))


if __name__ == "__main__":
    main()
