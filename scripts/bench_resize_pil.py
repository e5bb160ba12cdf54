#!/usr/bin/env python3
"""Timings of the device resize of Pillow's convention on the GPU (not part of bench.py):
`dgan.resize.resize_pil` (csrc/resize_pil.hip) of a 1080 x 1920 frame to a quarter and of a
270 x 480 frame to four times its size, bicubic and lanczos, n = 1 and 8, against the host path it
replaces (read the frame back, `Image.resize` per image, upload) and against the 4-tap
`dgan.resize.resize` of the other convention (another result: its work is the yardstick, not its
pixels).

    python scripts/bench_resize_pil.py [--out profiles/resize/bench_resize_pil.json]

Device-event medians over alternating windows, as scripts/bench_filters.py takes them: a difference
inside a path's own window spread is not a difference.  Every timed device result is first
compared with the host path's, bit for bit.  A call moves the input and the output once
(`bytes`); `taps` counts its multiply-adds from the coefficient tables (the horizontal pass over
every input row the output touches, then the vertical pass).
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

CASES = (("down4", 1080, 1920, 270, 480), ("up4", 270, 480, 1080, 1920))
FILTERS = ("bicubic", "lanczos")


def pillow_step(x, h, w, filter, out):
    """The host path: the device frames x through Pillow's resize into the device frames out."""
    from PIL import Image
    host = x.cpu().numpy()
    res = np.stack([np.asarray(Image.fromarray(a, "RGB").resize((w, h), getattr(Image.Resampling, filter.upper())))
                    for a in host])
    out.copy_(torch.from_numpy(res))
    return out


def taps(hi, wi, h, w, filter):
    """Multiply-adds per channel of one image: both passes, from the tables."""
    from dgan.resize import pil_coeffs
    cx = pil_coeffs(wi, w, filter)[1].astype(np.int64)
    fy, cy, _ = pil_coeffs(hi, h, filter)
    rows = np.zeros(hi, bool)
    for f, c in zip(fy, cy):
        rows[f:f + c] = True
    return int(rows.sum()) * int(cx.sum()) + int(cy.astype(np.int64).sum()) * w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_resize_pil.py: no GPU (a timing needs the device; there is no fallback)")
    from dgan import _lib
    from dgan.resize import DISPLAY, pil_tile, resize, resize_pil

    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "repeats": args.repeats,
           "library": _lib.build_info(), "frames": []}
    for name, hi, wi, h, w in CASES:
        for n in (1, 8):
            x = torch.from_numpy(frames(n, hi, wi, 1000 * n + hi)).cuda()
            out, host_out, tf_out = (torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(3))
            fns = {"tf_4tap_bicubic": lambda: resize(x, h, w, "bicubic", *DISPLAY, out=tf_out)}
            row = {"case": name, "n": n, "hi": hi, "wi": wi, "h": h, "w": w, "bytes": int(x.numel() + out.numel())}
            for f in FILTERS:
                same = bool(torch.equal(resize_pil(x, h, w, f, out=out), pillow_step(x, h, w, f, host_out)))
                row[f + "_device_equals_pillow"] = same
                if not same:
                    sys.exit(f"bench_resize_pil.py: {name} n {n} {f}: the device result differs from Pillow's")
                fns["device_" + f] = lambda f=f: resize_pil(x, h, w, f, out=out)
                fns["pillow_" + f] = lambda f=f: pillow_step(x, h, w, f, host_out)
                row[f + "_taps"] = 3 * n * taps(hi, wi, h, w, f)
            row["tile"] = {f: list(pil_tile(hi, wi, h, w, f)) for f in FILTERS}
            r = spread(alternate(fns, args.window, args.repeats))
            row.update(r)
            for f in FILTERS:
                ms = r["device_" + f]["median_ms"]
                row[f + "_GB_per_s"] = row["bytes"] / (ms * 1e-3) / 1e9
                row[f + "_G_taps_per_s"] = row[f + "_taps"] / (ms * 1e-3) / 1e9
                row[f + "_pillow_over_device"] = r["pillow_" + f]["median_ms"] / ms
                row[f + "_over_tf_4tap"] = ms / r["tf_4tap_bicubic"]["median_ms"]
            res["frames"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"done": True, "out": args.out}))


if __name__ == "__main__":
    main()
