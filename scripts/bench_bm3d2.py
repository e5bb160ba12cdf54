#!/usr/bin/env python3
"""BM3D second-stage timings on the GPU (not part of bench.py): `bm3d_wiener` (csrc/bm3d_wiener.hip,
stage 1's output as the pilot) and `bm3d2` (both stages) of 1080 x 1920 uint8 frames, n = 1 and 8,
sigma 25, group 16, search 21 and 7, against stage 1 (`bm3d`) in the same run, which is the
expectation: stage 2 does the same matching plus two transforms and the divisions.  Also non-local
means (t 7 / s 21 and t 3 / s 7, h = 25), the same frame's `Denoiser` forward, the host path
(`bm3d2_ref`, timed once on a 270 x 480 crop, scaled by area, its output compared with the device's)
and the PSNR of the noisy frame, `nlm`, `bm3d` and `bm3d2` against the clean frame.

    python scripts/bench_bm3d2.py [--out profiles/filters/bench_bm3d2.json]

Frames, noise and method are scripts/bench_bm3d.py's: device-event medians over alternating windows;
a difference inside a path's own window spread is not a difference.
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

import torch  # noqa: E402

from bench_bm3d import GROUP, NLM, SEARCHES, SIGMA, noised  # noqa: E402
from bench_infer import alternate  # noqa: E402
from bench_jpeg import frames  # noqa: E402
from bench_metrics import spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_bm3d2.py: no GPU (a timing needs the device; there is no fallback)")
    from dgan import _lib, metrics
    from dgan.filters import bm3d, bm3d2, bm3d2_ref, bm3d_wiener, nlm
    from dgan.infer import Denoiser
    from dgan.models import Generator

    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "repeats": args.repeats, "sigma": SIGMA,
           "group": GROUP, "nlm_h": SIGMA, "library": _lib.build_info(), "frames": []}
    h, w = 1080, 1920

    # the host path on a crop: read-back, bm3d2_ref, upload
    crop = torch.from_numpy(noised(frames(1, 270, 480, 7), 8)).cuda()
    host = {}
    for s in SEARCHES:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        back = torch.from_numpy(bm3d2_ref(crop.cpu().numpy(), SIGMA, s, GROUP)).cuda()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        same = bool(torch.equal(back, bm3d2(crop, SIGMA, s, GROUP)))
        host[f"s{s}"] = {"crop_270x480_ms": ms, "scaled_to_1080x1920_ms": ms * (h * w) / (270.0 * 480.0),
                         "device_equals_host": same}
        print(json.dumps(host), flush=True)
    res["host_bm3d2"] = host

    den = Denoiser(Generator(width=1, seed=5))
    for n in (1, 8):
        clean = frames(n, h, w, 1000 * n + h)
        x, ref = torch.from_numpy(noised(clean, n)).cuda(), torch.from_numpy(clean).cuda()
        out = torch.empty_like(x)
        pilots = {s: bm3d(x, SIGMA, s, GROUP, out=torch.empty_like(x)) for s in SEARCHES}
        fns = {}
        for s in SEARCHES:
            fns[f"bm3d_wiener_s{s}"] = lambda s=s: bm3d_wiener(x, pilots[s], SIGMA, s, GROUP, out=out)
            fns[f"bm3d2_s{s}"] = lambda s=s: bm3d2(x, SIGMA, s, GROUP, out=out)
            fns[f"bm3d_s{s}"] = lambda s=s: bm3d(x, SIGMA, s, GROUP, out=out)
        for t, s in NLM:
            fns[f"nlm_t{t}_s{s}"] = lambda t=t, s=s: nlm(x, SIGMA, t, s, out=out)
        if n == 1:
            f = den.run(x.cpu().numpy())
            fns["forward"] = lambda: den._run(f)
        row = dict(spread(alternate(fns, args.window, args.repeats)), n=n, h=h, w=w)
        for s in SEARCHES:
            row[f"bm3d_wiener_s{s}_over_bm3d_s{s}"] = row[f"bm3d_wiener_s{s}"]["median_ms"] / row[f"bm3d_s{s}"]["median_ms"]
            row[f"bm3d2_s{s}_host_over_device"] = (host[f"s{s}"]["scaled_to_1080x1920_ms"] * n
                                                   / row[f"bm3d2_s{s}"]["median_ms"])
            if n == 1:
                row[f"bm3d2_s{s}_over_forward"] = row[f"bm3d2_s{s}"]["median_ms"] / row["forward"]["median_ms"]
        if n == 1:
            psnr = {"noisy": float(metrics.psnr(x, ref).item())}
            for k, fn in fns.items():
                if k != "forward" and not k.startswith("bm3d_wiener"):
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
