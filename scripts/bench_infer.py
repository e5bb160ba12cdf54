#!/usr/bin/env python3
"""Inference timings on the GPU (not part of bench.py): the existing path
`generator(x, training=False)` against the BN-folded plan (dgan/infer.py), alternated in one
process, and uint8 -> uint8 frames per second of the Denoiser on a 1080 x 1920 frame.

    python scripts/bench_infer.py [--width 1] [--out profiles/infer/bench_infer.json]

Every figure is device-event time over warmed windows of at least --window seconds; each pair of
paths is timed in alternating windows (--repeats of each), and the spread between a path's own
windows is reported beside its median: a difference inside that spread is not a difference.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "denoise-gan_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def window_ms(fn, iters):
    """Device time per call over `iters` back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns, window_s, repeats, warmup=3):
    """fns: {name: callable}.  -> {name: {median_ms, min_ms, max_ms, iters}} from `repeats`
    alternating windows of each, every window at least window_s long."""
    iters = {}
    for name, fn in fns.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = window_ms(fn, 3)
        iters[name] = max(3, int(np.ceil(window_s * 1e3 / ms)))
    got = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            got[name].append(window_ms(fn, iters[name]))
    return {name: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), iters=iters[name],
                       windows=len(v)) for name, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1, help="filter-count divisor (1: the reference model)")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_infer.py: no GPU (a timing needs the device; there is no fallback)")
    from dgan import _lib
    from dgan.infer import Denoiser, FoldedGenerator
    from dgan.models import Generator

    G = Generator(width=args.width, seed=5)
    folded = FoldedGenerator(G)
    res = {"device": torch.cuda.get_device_name(0), "width": args.width, "window_s": args.window,
           "repeats": args.repeats, "library": _lib.build_info(), "forward": [], "frames": []}
    rng = np.random.default_rng(0)
    for N, H, W in ((1, 256, 256), (16, 256, 256), (1, 1024, 1024)):
        x = torch.from_numpy(rng.uniform(-1, 1, (N, H, W, 3)).astype(np.float32)).cuda()
        plan = folded.plan(N, H, W)
        r = alternate({"unfolded": lambda: G(x, training=False), "folded": lambda: plan.forward(x)}, args.window,
                      args.repeats)
        diff = float((G(x, training=False) - plan.forward(x)).abs().max().item())
        row = dict(shape=[N, H, W], max_abs_diff=diff, **r)
        row["speedup"] = r["unfolded"]["median_ms"] / r["folded"]["median_ms"]
        res["forward"].append(row)
        print(json.dumps(row), flush=True)
    frame = rng.integers(0, 256, (1, 1080, 1920, 3), dtype=np.uint8)
    for label, kw in (("whole", dict()), ("tile256_margin32", dict(tile=256, margin=32))):
        dens = {g: Denoiser(G, graph=g, **kw) for g in (False, True)}
        outs = {g: d.denoise(frame) for g, d in dens.items()}   # (builds the buffers, captures)

        def run(d):
            f = d._frames[(1, 1080, 1920)]
            return (lambda: f.graph.replay()) if f.graph is not None else (lambda: d._run(f))

        r = alternate({"eager": run(dens[False]), "graph": run(dens[True])}, args.window, args.repeats)
        row = dict(mode=label, frame=[1080, 1920], graph_equals_eager=bool(np.array_equal(outs[False], outs[True])),
                   what="device time of stage -> forward -> unstage over static uint8 buffers (no host copy)")
        for k, v in r.items():
            row[k] = dict(v, frames_per_s=1e3 / v["median_ms"])
        res["frames"].append(row)
        print(json.dumps(row), flush=True)
        del dens
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"done": True, "out": args.out}))


if __name__ == "__main__":
    main()
