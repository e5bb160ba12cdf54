#!/usr/bin/env python3
"""Super-resolution inference timings on the GPU (not part of bench.py), by the protocol of
scripts/bench_infer.py: device-event time, the median of --repeats alternating windows of at least
--window seconds, each path's own [min - max] beside it.

    python scripts/bench_upscale.py [--out profiles/infer/bench_upscale.json]

Forward paths, alternated in one process on the same input:
  unfolded   the existing inference path network.plan(N,H,W).forward(x, training=False): the
             reference for time
  folded     FoldedNetwork(fuse=False): BatchNorms folded, blocks unfused
  fused      FoldedNetwork(fuse=True): FastSRGAN's inverted-residual blocks in one kernel each
and the uint8 -> uint8 frame through the Upscaler, whole-image, eager and graph.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_upscale.py: no GPU (a timing needs the device; there is no fallback)")
    from dgan import _lib, ops, zoo
    from dgan.graph import GraphNetwork
    from dgan.sr_infer import FoldedNetwork, Upscaler

    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "repeats": args.repeats,
           "library": _lib.build_info(), "forward": [], "frames": []}
    rng = np.random.default_rng(0)
    nets = {"fsrgan": GraphNetwork(zoo.fsrgan_generator(), seed=5), "srgan": GraphNetwork(zoo.srgan_generator(), seed=5)}
    cases = [("fsrgan", 1, 270, 480), ("fsrgan", 1, 540, 960), ("fsrgan", 8, 64, 64), ("srgan", 1, 270, 480)]
    for arch, N, H, W in cases:
        net = nets[arch]
        x = torch.from_numpy(rng.uniform(-1, 1, (N, H, W, 3)).astype(np.float32)).cuda()
        base = net.plan(N, H, W)
        ws = ops.Workspace(net.device)
        ws.get(base.ws_bytes)
        fns = {"unfolded": lambda: base.forward(x, training=False, ws=ws)}
        plans = {"folded": FoldedNetwork(net, fuse=False).plan(N, H, W)}
        if arch == "fsrgan":
            plans["fused"] = FoldedNetwork(net, fuse=True).plan(N, H, W)
        for k, p in plans.items():
            fns[k] = (lambda p: lambda: p.forward(x))(p)
        r = alternate(fns, args.window, args.repeats)
        ref = base.forward(x, training=False, ws=ws)
        row = dict(arch=arch, shape=[N, H, W], **r)
        for k, p in plans.items():
            row[f"max_abs_diff_{k}"] = float((ref - p.forward(x)).abs().max().item())
            row[f"speedup_{k}"] = r["unfolded"]["median_ms"] / r[k]["median_ms"]
        res["forward"].append(row)
        print(json.dumps(row), flush=True)
        del base, plans, fns
        net._plans.clear()
        torch.cuda.empty_cache()
    for h, w in ((270, 480), (540, 960)):
        frame = rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8)
        ups = {g: Upscaler(nets["fsrgan"], 4, graph=g) for g in (False, True)}
        outs = {g: u.upscale(frame) for g, u in ups.items()}   # (builds the buffers, captures)

        def run(u):
            f = u._frames[(1, h, w)]
            return (lambda: f.graph.replay()) if f.graph is not None else (lambda: u._run(f))

        r = alternate({"eager": run(ups[False]), "graph": run(ups[True])}, args.window, args.repeats)
        row = dict(arch="fsrgan", frame=[h, w], out=[4 * h, 4 * w],
                   graph_equals_eager=bool(np.array_equal(outs[False], outs[True])),
                   what="device time of stage -> fused forward -> unstage over static uint8 buffers (no host copy)")
        for k, v in r.items():
            row[k] = dict(v, frames_per_s=1e3 / v["median_ms"])
        res["frames"].append(row)
        print(json.dumps(row), flush=True)
        del ups
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"done": True, "out": args.out}))


if __name__ == "__main__":
    main()
