#!/usr/bin/env python3
"""bench.py's graph-vs-eager check (graph_vs_eager), repeated in one process: from one snapshot,
one eager step and one replay of the captured graph, ITERS times; every comparison that differs
is printed with the parameters of D.grad / G.grad that differ (count, size, max |difference|).

    python scripts/diag/graph_eager_stress.py [ITERS] [CONTENT 0|1] [twin]

twin: every pix2pix / VGG19 GEMM in bf16x6, as bench.py --full's twin leg.  DG_LIB selects the library."""
import os, sys, types
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(REPO, "denoise-gan_amd"), REPO]
import torch
import bench
import dgan
dgan.build()
from dgan.trainer import restore, snapshot, state_diff
from pix2pix import Pix2Pix
N = int(sys.argv[1]) if len(sys.argv) > 1 else 100
content = int(sys.argv[2]) if len(sys.argv) > 2 else 1
if len(sys.argv) > 3 and sys.argv[3] == "twin":
    from dgan import nets as _n
    _n.P2P_MATH = "bf16x6"
    os.environ["DG_VGG_MATH"] = "bf16x6"
wl = bench.WORKLOADS["pix2pix"]
x_np, y_np = bench.synthetic_batch(wl, wl["batch"], seed=1000)
x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
m = Pix2Pix(bench.Args(crop_size=wl["size"], retrain=0, width=1, seed=1234, dropout_seed=0, identity_loss=1,
                       content_loss=content))
tr = m.trainer(x.shape)
for _ in range(5):
    tr.step(x, y)
torch.cuda.synchronize()
s = torch.cuda.Stream()
s.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(s):
    tr.step(x, y)
torch.cuda.current_stream().wait_stream(s)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    tr.step(x, y)
torch.cuda.synchronize()
s0 = snapshot(tr)
bad_runs = 0
ref = None
for i in range(N):
    restore(tr, s0)
    tr.step(x, y)
    eager = snapshot(tr)
    restore(tr, s0)
    g.replay()
    replay = snapshot(tr)
    torch.cuda.synchronize()
    if ref is None:
        ref = eager
    for tag, a, b in (("eager-vs-replay", eager, replay), ("eager-vs-first", eager, ref), ("replay-vs-first", replay, ref)):
        bad = state_diff(a, b)
        if bad:
            bad_runs += 1
            msg = [f"iter {i} {tag}: {bad}"]
            for net, A in (("D", tr.dA), ("G", tr.gA)):
                k = f"{net}.grad"
                if k in bad:
                    d = (a[k] != b[k]).nonzero().flatten()
                    names = []
                    for name in A.layout:
                        lo = A.offsets[name]; hi = A.end_offset(name)
                        c = int(((d >= lo) & (d < hi)).sum())
                        if c:
                            names.append((name, c, hi - lo, float((a[k][lo:hi] - b[k][lo:hi]).abs().max())))
                    msg.append(f"   {k}: {names}")
            print("\n".join(msg), flush=True)
print(f"lib {os.environ.get('DG_LIB', 'tree')} content {content} {sys.argv[3:]}: {N} iterations, {bad_runs} comparisons differed", flush=True)
