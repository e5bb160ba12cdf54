#!/usr/bin/env python3
"""Super-resolution evaluation timings on the GPU (not part of bench.py): the device resize
(csrc/resize.hip) of a 1080 x 1920 uint8 frame down to 270 x 480 (the degrade) and back (the
display upscale), against the four scores of the same frame and the FastSRGAN x4 Upscaler's
stage -> forward -> unstage in the same run, then `SREvaluator.evaluate` against
`Upscaler.upscale` end to end.

    python scripts/bench_sr_eval.py [--out profiles/sr_eval/bench_sr_eval.json]

Device-event medians over alternating windows, as scripts/bench_metrics.py takes them: a
difference inside a path's own window spread is not a difference.  Bytes moved are the
algorithmic ones (input read once, output written once), GB/s follows from the median.
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
from bench_metrics import spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sr_eval.py: no GPU (a timing needs the device; there is no fallback)")
    from dgan import _lib, metrics, zoo
    from dgan.graph import GraphNetwork
    from dgan.resize import DEGRADE, DISPLAY, resize
    from dgan.sr_infer import Upscaler

    H, W, S = 1080, 1920, 4
    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "repeats": args.repeats,
           "library": _lib.build_info()}
    rng = np.random.default_rng(0)
    hr = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    up = Upscaler(GraphNetwork(zoo.fsrgan_generator(), seed=5), S)
    ev = metrics.SREvaluator(up)
    scores = ev.evaluate(hr)                # (builds every buffer)
    f = up.frame(1, H // S, W // S)         # (the frame: its device uint8 input and output)
    ref, base, out4 = ev.buffers(hr.shape)  # (the uploaded original, the baseline, the scores)

    def degrade():
        resize(ref, H // S, W // S, "bicubic", *DEGRADE, out=f.u8_in)

    def display():
        resize(f.u8_in, H, W, "bicubic", *DISPLAY, out=base)

    def four():
        metrics.psnr(base, ref, out=out4[0])
        metrics.psnr(f.u8_out, ref, out=out4[1])
        metrics.ssim(base, ref, out=out4[2])
        metrics.ssim(f.u8_out, ref, out=out4[3])

    r = spread(alternate({"degrade": degrade, "display": display, "both_resizes": lambda: (degrade(), display()),
                          "four_scores": four, "forward": lambda: up._run(f)}, args.window, args.repeats))
    nbytes = {"degrade": H * W * 3 + (H // S) * (W // S) * 3, "display": (H // S) * (W // S) * 3 + H * W * 3}
    for k, b in nbytes.items():
        r[k]["bytes"] = b
        r[k]["GB_per_s"] = b / (r[k]["median_ms"] * 1e-3) / 1e9
    res["frame_1080x1920_x4"] = dict(
        r, both_resizes_over_four_scores=r["both_resizes"]["median_ms"] / r["four_scores"]["median_ms"],
        resizes_below_four_scores=bool(r["both_resizes"]["median_ms"] < r["four_scores"]["median_ms"]),
        what="device time; degrade = 1080x1920 -> 270x480 uint8 bicubic, display = 270x480 -> 1080x1920; four_scores "
             "= PSNR and SSIM of the baseline and of the upscaled frame; forward = stage -> whole-image folded "
             "FastSRGAN forward -> unstage of the same frame (eager)",
        scores={k: float(v[0]) for k, v in scores.items()})
    print(json.dumps(res["frame_1080x1920_x4"]), flush=True)

    # --- end to end, host copies included -------------------------------------------------------
    low = f.u8_in.cpu().numpy()
    r = spread(alternate({"upscale": lambda: up.upscale(low), "evaluate": lambda: ev.evaluate(hr)}, args.window,
                         args.repeats))
    res["end_to_end_1080x1920"] = dict(r, evaluate_over_upscale=r["evaluate"]["median_ms"] / r["upscale"]["median_ms"],
                                       what="host upload -> device work -> host read-back per call: upscale takes the "
                                            "270x480 frame and returns the 1080x1920 one, evaluate uploads the 1080x1920 "
                                            "original and returns four scalars")
    print(json.dumps(res["end_to_end_1080x1920"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"done": True, "out": args.out}))


if __name__ == "__main__":
    main()
