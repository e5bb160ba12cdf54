#!/usr/bin/env python
"""Record what the conv planner decides for every layer geometry the project runs
(tests/plan_snapshot.json), so a planner change shows its effect on every layer in review.

    python scripts/gen_plan_snapshot.py            # rewrite tests/plan_snapshot.json
    python scripts/gen_plan_snapshot.py --check    # compare, exit 1 on a difference

Planning needs no GPU: descriptors are planned at creation.  Child processes plan batches of
geometries under DG_PLAN_DEBUG=1 with every other DG_* variable removed; per geometry and math
(ConvDesc's math=) a record holds the ordered "[dg plan]" lines of planning under that math (a
math= descriptor plans the default math first: those lines, the same as a default descriptor's,
are cut off) and the answers of the plan queries: workspace size, arithmetic and operand-plane
mask of the three ops, plane size and format of x / dy / w, and dg_conv_fwd_pool_ok for the four
activations (compact(): values joined into short strings).  In the file, maths whose records are equal share one entry ("fp32,bf16x6": ...).
tests/test_plan.py test_plan_snapshot regenerates the records and compares them with the file
field by field.
"""
import json
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNAPSHOT = os.path.join(REPO, "tests", "plan_snapshot.json")
MATHS = ("fp32", "bf16x6", "fp16", "f16x3")
ACTS = ("none", "relu", "lrelu", "sigmoid")
PER_CHILD = 24   # geometries per child process (1-2 s of imports each)

P1 = (1, 1, 1, 1)   # ZeroPadding2D() + 'valid'


# Geometries are (N, H, W, Cin, Cout, k, s, padding, transpose), read off dgan/nets.py,
# dgan/sr_models.py, dgan/zoo.py and dgan/infer.py (no model is constructed: that allocates
# on the device).
def unet(N, H, W):
    """pix2pix generator (nets.py g_layer_specs / GeneratorPlan): 8 downs, 7 ups, last."""
    out, h, w = [], H, W
    for ci, co in ((3, 64), (64, 128), (128, 256), (256, 512), (512, 512), (512, 512), (512, 512), (512, 512)):
        out.append((N, h, w, ci, co, 4, 2, "same", False))
        h, w = h // 2, w // 2
    for ci, co in ((512, 512), (1024, 512), (1024, 512), (1024, 512), (1024, 256), (512, 128), (256, 64), (128, 3)):
        out.append((N, h, w, ci, co, 4, 2, "same", True))
        h, w = h * 2, w * 2
    return out


def patchgan(N, S):
    """pix2pix discriminator (nets.py d_layer_specs / DiscriminatorPlan)."""
    return [(N, S, S, 6, 64, 4, 2, "same", False), (N, S // 2, S // 2, 64, 128, 4, 2, "same", False),
            (N, S // 4, S // 4, 128, 256, 4, 2, "same", False), (N, S // 8, S // 8, 256, 512, 4, 1, P1, False),
            (N, S // 8 - 1, S // 8 - 1, 512, 1, 4, 1, P1, False)]


def vgg19(N, S):
    """VGG19 to block5_conv4 (zoo.py vgg19_features): every distinct 3x3 layer."""
    return [(N, S, S, 3, 64, 3, 1, "same", False), (N, S, S, 64, 64, 3, 1, "same", False),
            (N, S // 2, S // 2, 64, 128, 3, 1, "same", False), (N, S // 2, S // 2, 128, 128, 3, 1, "same", False),
            (N, S // 4, S // 4, 128, 256, 3, 1, "same", False), (N, S // 4, S // 4, 256, 256, 3, 1, "same", False),
            (N, S // 8, S // 8, 256, 512, 3, 1, "same", False), (N, S // 8, S // 8, 512, 512, 3, 1, "same", False),
            (N, S // 16, S // 16, 512, 512, 3, 1, "same", False)]


def sr_disc(N, S):
    """The SR family's discriminator (zoo.py sr_discriminator), df 32."""
    out, s, ci = [], S, 3
    for co, st in ((32, 1), (32, 2), (32, 1), (32, 2), (64, 1), (64, 2), (64, 1), (64, 2)):
        out.append((N, s, s, ci, co, 3, st, "same", False))
        s, ci = (s + st - 1) // st, co
    out.append((N, s, s, 64, 1, 1, 1, "same", False))
    return out


def srgan_g(N, S):
    """zoo.py srgan_generator, 4x: input conv, residual / post convs, two upsamplers, 1x1 output."""
    return [(N, S, S, 3, 64, 3, 1, "same", False), (N, S, S, 64, 64, 3, 1, "same", False),
            (N, S, S, 64, 256, 3, 1, "same", False), (N, 2 * S, 2 * S, 64, 256, 3, 1, "same", False),
            (N, 4 * S, 4 * S, 64, 3, 1, 1, "same", False)]


def fsrgan_g(N, S):
    """zoo.py fsrgan_generator (gf 32, expansion 6; the depthwise convs are no conv-engine ops)."""
    return [(N, S, S, 3, 32, 3, 1, "same", False), (N, S, S, 32, 32, 1, 1, "same", False),
            (N, S, S, 32, 192, 1, 1, "same", False), (N, S, S, 192, 32, 1, 1, "same", False),
            (N, S, S, 32, 32, 3, 1, "same", False), (N, S, S, 32, 128, 3, 1, "same", False),
            (N, 2 * S, 2 * S, 32, 128, 3, 1, "same", False), (N, 4 * S, 4 * S, 32, 3, 3, 1, "same", False)]


def autoencoder_g(N, S):
    """zoo.py autoencoder_generator: (Cin, Cout, image size divisor) of conv1 .. conv11."""
    spec = ((3, 32, 1), (32, 32, 1), (32, 44, 2), (44, 56, 4), (56, 76, 8), (76, 100, 16),
            (176, 152, 16), (152, 152, 16), (208, 112, 8), (112, 112, 8), (156, 84, 4), (84, 84, 4),
            (116, 64, 2), (64, 64, 2), (67, 64, 1), (64, 32, 1), (32, 3, 1))
    return [(N, S // d, S // d, ci, co, 3, 1, "same", False) for ci, co, d in spec]


def _cases(rows):
    """(name, N, H, W, Cin, Cout, k, s, padding, transpose, bias) test cases -> geometries."""
    return [tuple(r[1:10]) for r in rows]


# tests/test_conv_gpu.py CASES / HALO_CASES, tests/test_x3_gpu.py X3_CASES and its other layer
# descriptors, tests/test_fused_pool_gpu.py, tests/conv_variants.py CASES (tests/test_boundary_gpu.py
# creates no conv descriptor of its own: its steps run the pix2pix networks above)
TEST_CASES = [
    ("G.down1", 2, 64, 64, 3, 64, 4, 2, "same", False),
    ("G.down2", 2, 32, 32, 64, 128, 4, 2, "same", False),
    ("G.down4", 2, 16, 16, 256, 512, 4, 2, "same", False),
    ("G.down8", 4, 2, 2, 512, 512, 4, 2, "same", False),
    ("G.up1", 4, 1, 1, 512, 512, 4, 2, "same", True),
    ("G.up2", 2, 2, 2, 1024, 512, 4, 2, "same", True),
    ("G.up5", 2, 8, 8, 1024, 256, 4, 2, "same", True),
    ("G.up7", 2, 16, 16, 256, 64, 4, 2, "same", True),
    ("G.last", 2, 32, 32, 128, 3, 4, 2, "same", True),
    ("D.down1", 2, 64, 64, 6, 64, 4, 2, "same", False),
    ("D.conv", 2, 16, 16, 256, 512, 4, 1, P1, False),
    ("D.last", 2, 15, 15, 512, 1, 4, 1, P1, False),
    ("k3s1", 2, 12, 12, 64, 64, 3, 1, "same", False),
    ("k3s2", 2, 12, 12, 32, 64, 3, 2, "same", False),
    ("k1s1", 2, 6, 6, 64, 3, 1, 1, "same", False),
    ("odd", 3, 9, 7, 8, 32, 4, 2, "same", False),
    ("V.b1c1", 2, 37, 45, 3, 64, 3, 1, "same", False),
    ("D.down1.odd", 2, 27, 70, 6, 64, 4, 2, "same", False),
    ("k3s2.c3", 2, 17, 19, 3, 64, 3, 2, "same", False),
    ("G.last.odd", 2, 13, 21, 160, 3, 4, 2, "same", True),
    ("small.wide", 3, 32, 128, 3, 64, 4, 2, "same", False),
    ("small.co128", 1, 64, 64, 6, 128, 4, 2, "same", False),
    ("small.rows", 3, 384, 64, 3, 64, 4, 2, "same", False),
    ("small.valid", 2, 66, 66, 6, 64, 4, 2, "valid", False),
    ("small.tlast", 1, 64, 64, 64, 3, 4, 2, "same", True),
    ("small.k3", 2, 32, 64, 3, 64, 3, 1, "same", False),
    ("small.k3c128", 3, 24, 32, 3, 128, 3, 1, "same", False),
    ("co1.full", 4, 31, 31, 512, 1, 4, 1, P1, False),
    ("co1.s2", 2, 19, 23, 64, 1, 4, 2, "same", False),
    ("co1.k3", 2, 9, 300, 128, 1, 3, 1, "same", False),
    ("co1.c4", 2, 11, 13, 4, 1, 4, 1, P1, False),
    ("tlast.ragged", 2, 13, 21, 128, 3, 4, 2, "same", True),
    ("tlast.big", 1, 64, 64, 128, 3, 4, 2, "same", True),
    ("h.ragged", 4, 40, 36, 64, 128, 3, 1, "same", False),
    ("h.bn64", 2, 16, 16, 256, 64, 3, 1, "same", False),
    ("h.splitk", 2, 8, 8, 512, 512, 3, 1, "same", False),
    ("h.valid", 2, 20, 21, 64, 64, 3, 1, "valid", False),
    ("h.tfpad", 3, 13, 29, 32, 48, 3, 1, P1, False),
    ("h32.ragged", 3, 21, 37, 32, 32, 3, 1, "same", False),
    ("h32.c16", 2, 24, 24, 16, 32, 3, 1, "same", False),
    ("h32.splitk", 2, 8, 8, 256, 32, 3, 1, "same", False),
    ("h2.down", 2, 32, 32, 64, 128, 4, 2, "same", False),
    ("h2.up", 2, 16, 16, 256, 64, 4, 2, "same", True),
    ("h2.ragged", 1, 29, 61, 16, 32, 4, 2, "same", False),
    ("h2.odd", 2, 13, 27, 16, 32, 4, 2, "same", False),
    ("h2.splitk", 1, 13, 27, 32, 512, 4, 2, "same", False),
    ("h2.valid", 2, 14, 28, 32, 64, 4, 2, "valid", False),
    ("h2.tail", 2, 13, 27, 10, 32, 4, 2, "same", False),
    ("g2.ragged", 3, 26, 40, 32, 64, 4, 2, "same", False),
    ("g2.odd", 2, 17, 15, 16, 32, 4, 2, "same", False),
    ("g2.splitk", 2, 8, 8, 512, 512, 4, 2, "same", False),
    ("g2.valid", 2, 20, 22, 32, 64, 4, 2, "valid", False),
    ("h4.pad", 2, 18, 21, 32, 64, 4, 1, P1, False),
    ("h4.same", 3, 11, 17, 16, 32, 4, 1, "same", False),
    ("h4.bn128", 2, 16, 16, 64, 256, 4, 1, P1, False),
    ("x3.b2", 2, 32, 32, 64, 128, 3, 1, "same", False),
    ("x3.bn64", 2, 16, 16, 128, 64, 3, 1, "same", False),
    ("x3.ragged", 3, 21, 37, 64, 128, 3, 1, "same", False),
    ("x3.valid", 2, 20, 22, 32, 64, 3, 1, "valid", False),
    ("x3.c48", 2, 16, 24, 96, 48, 3, 1, "same", False),
    ("x3.up.odd", 2, 9, 7, 64, 32, 4, 2, "same", True),
    ("x3.deep", 4, 4, 4, 512, 512, 4, 2, "same", False),
    ("x3.deep.up", 4, 2, 2, 1024, 512, 4, 2, "same", True),
    ("x3.patch", 2, 18, 21, 64, 128, 4, 1, P1, False),
    ("x3.patch.valid", 2, 34, 27, 256, 96, 4, 1, "valid", False),
    ("pool.c64", 16, 64, 64, 32, 64, 3, 1, "same", False),
    ("pool.c128", 16, 64, 64, 32, 128, 3, 1, "same", False),
    ("pool.n8", 8, 64, 64, 32, 128, 3, 1, "same", False),
    ("pool.no12", 4, 12, 12, 64, 64, 3, 1, "same", False),
    ("pool.nos2", 8, 64, 64, 64, 128, 4, 2, "same", False),
    ("pool.b1c2like", 8, 64, 64, 64, 64, 3, 1, "same", False),
    ("pool.b5like", 16, 16, 16, 512, 512, 3, 1, "same", False),
    # tests/conv_variants.py CASES (those not listed above)
    ("v.gemm.tail", 2, 9, 7, 10, 32, 3, 1, "same", False),
    ("v.gemm.k4s2", 2, 8, 8, 32, 32, 4, 2, "same", False),
    ("v.halo3", 2, 9, 17, 32, 64, 3, 1, "same", False),
    ("v.h2.up", 2, 7, 14, 64, 32, 4, 2, "same", True),
    ("v.small.c3", 1, 8, 64, 3, 64, 4, 2, "same", False),
    ("v.small.c6", 1, 8, 64, 6, 64, 4, 2, "same", False),
    ("v.small.k3", 1, 4, 32, 3, 64, 3, 1, "same", False),
    ("v.co1.s2", 2, 9, 11, 64, 1, 4, 2, "same", False),
    ("v.narrow.px", 1, 64, 64, 64, 3, 1, 1, "same", False),
    ("v.narrow.dgrad", 2, 9, 7, 4, 16, 3, 2, "same", False),
    ("v.direct.c3", 2, 9, 13, 3, 64, 3, 1, "same", False),
    ("v.direct.c6", 2, 10, 14, 6, 64, 4, 2, "same", False),
    ("v.tlast", 1, 5, 9, 128, 3, 4, 2, "same", True),
    ("v.recast.dgrad", 2, 5, 7, 160, 3, 4, 2, "same", True),
    ("v.ntile", 2, 9, 11, 3, 32, 3, 1, "same", False),
]


def geometries():
    """Every distinct geometry, in a fixed order."""
    g = []
    # pix2pix bs16 (bench.py): G over [x; y] and D over [real; fake] at 2N = 32, D's fake half and
    # the generator's first layer at N = 16; VGG19 at 256^2 (sr_trainer.ContentLoss): one forward
    # over [generated; target] at 2N, or the two halves' forwards at N (ContentLoss(split=True),
    # what the pix2pix trainer builds), and the backward through the generated half at N
    g += unet(32, 256, 256) + patchgan(32, 256) + patchgan(16, 256) + [(16, 256, 256, 3, 64, 4, 2, "same", False)]
    g += vgg19(32, 256) + vgg19(16, 256)
    # SRGAN 24 -> 96 bs32: D over the generated and real batches (N, and both at 2N), VGG19 as above
    g += srgan_g(32, 24) + sr_disc(64, 96) + sr_disc(32, 96) + vgg19(64, 96) + vgg19(32, 96)
    # FastSRGAN 128 -> 512 bs8
    g += fsrgan_g(8, 128) + sr_disc(16, 512) + sr_disc(8, 512) + vgg19(16, 512) + vgg19(8, 512)
    # autoencoder 64^2 bs4
    g += autoencoder_g(4, 64) + sr_disc(8, 64) + sr_disc(4, 64) + vgg19(8, 64) + vgg19(4, 64)
    # full-width inference (dgan/infer.py): one 256^2 image, 1080 x 1920 padded to 1280 x 2048
    g += unet(1, 256, 256) + unet(1, 1280, 2048)
    g += _cases(TEST_CASES)
    seen, out = set(), []
    for t in g:
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


CHILD = r"""
import ctypes, json, os, sys
sys.path[:0] = [sys.argv[1]]
from dgan import ops
from dgan.ops import ConvDesc
geoms, maths, acts = eval(sys.argv[2])
out = []
for gi, (N, H, W, ci, co, k, s, pad, tr) in enumerate(geoms):
    os.write(2, f"[snap] {gi} default\n".encode())
    ConvDesc(N, H, W, ci, co, k, s, pad, tr)
    for m in maths:
        os.write(2, f"[snap] {gi} {m}\n".encode())
        d = ConvDesc(N, H, W, ci, co, k, s, pad, tr, math=m)
        rec = {"ws": list(d.ws), "arith": [d.op_arith(op) for op in range(3)], "planes": list(d.plane_mask),
               "size": [d.plane_bytes(t) for t in (ops.TENSOR_X, ops.TENSOR_DY, ops.TENSOR_W)],
               "format": [d.plane_format(t) for t in (ops.TENSOR_X, ops.TENSOR_DY, ops.TENSOR_W)],
               "pool": [int(d.pool_fusable(a)) for a in acts]}
        out.append([gi, m, rec])
os.write(2, b"[snap] end\n")
print(json.dumps(out))
"""


def key(geom):
    N, H, W, ci, co, k, s, pad, tr = geom
    p = pad if isinstance(pad, str) else "p" + "".join(map(str, pad))
    return f"{'convT' if tr else 'conv'} N{N} {H}x{W} {ci}->{co} k{k} s{s} {p}"


def record(geoms=None):
    """{geometry key: {math: record}} from fresh child processes."""
    geoms = geometries() if geoms is None else geoms
    env = {k: v for k, v in os.environ.items() if not k.startswith("DG_")}
    env["DG_PLAN_DEBUG"] = "1"
    snap = {}
    for i in range(0, len(geoms), PER_CHILD):
        chunk = geoms[i:i + PER_CHILD]
        r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(REPO, "denoise-gan_amd"),
                            repr((chunk, MATHS, ACTS))], capture_output=True, text=True, env=env, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-4000:])
        lines, cur = {}, None
        for line in r.stderr.splitlines():
            if line.startswith("[snap] "):
                cur = line[len("[snap] "):]
                lines[cur] = []
            elif line.startswith("[dg plan] ") and cur is not None:
                lines[cur].append(line[len("[dg plan] "):])
        for gi, m, rec in json.loads(r.stdout.strip().splitlines()[-1]):
            first, both = lines[f"{gi} default"], lines[f"{gi} {m}"]
            if both[:len(first)] != first:
                raise RuntimeError(f"{key(chunk[gi])} [{m}]: the descriptor's first plan is not the default one")
            rec["plan"] = both[len(first):]
            snap.setdefault(key(chunk[gi]), {})[m] = compact(rec)
    return snap


GEMM_LINE = re.compile(r"mode (\d) M=(\d+) N=(\d+) K=(\d+) -> (\w+) cfg (\d+) splits (\d+) ph (\d+) ptiles (\d+)")


def compact(rec):
    """A record as short strings (nothing dropped): the three ops' (or tensors', activations')
    values joined by spaces, and each GEMM / halo plan line "mode m M= N= K= -> name cfg c splits
    s ph p ptiles t" as "m MxNxK name c s p t"; the other plan lines stay as printed."""
    out = {f: " ".join(map(str, v)) for f, v in rec.items() if f != "plan"}
    out["plan"] = [GEMM_LINE.sub(r"\1 \2x\3x\4 \5 \6 \7 \8 \9", line) if GEMM_LINE.fullmatch(line) else line
                   for line in rec["plan"]]
    return out


def pack(snap):
    """File form: the maths of a geometry whose records are equal share one "m1,m2" entry."""
    out = {}
    for k, per in snap.items():
        groups = []
        for m in MATHS:
            for g in groups:
                if per[g[0]] == per[m]:
                    g.append(m)
                    break
            else:
                groups.append([m])
        out[k] = {",".join(g): per[g[0]] for g in groups}
    return out


def unpack(packed):
    return {k: {m: rec for ms, rec in per.items() for m in ms.split(",")} for k, per in packed.items()}


def differences(want, got):
    """Field-by-field differences between two snapshots, as readable strings."""
    out = []
    for k in sorted(set(want) | set(got)):
        if k not in want or k not in got:
            out.append(f"{k}: {'not in the file' if k not in want else 'not planned'}")
            continue
        for m in MATHS:
            a, b = want[k].get(m, {}), got[k].get(m, {})
            for f in sorted(set(a) | set(b)):
                if a.get(f) != b.get(f):
                    out.append(f"{k} [{m}] {f}: file {a.get(f)} planned {b.get(f)}")
    return out


def main():
    snap = record()
    if "--check" in sys.argv:
        with open(SNAPSHOT) as f:
            diff = differences(unpack(json.load(f)), snap)
        print("\n".join(diff) if diff else f"{len(snap)} geometries match")
        return 1 if diff else 0
    packed = pack(snap)
    with open(SNAPSHOT, "w") as f:
        f.write("{\n" + ",\n".join(
            json.dumps(k) + ": {\n" + ",\n".join(f"  {json.dumps(m)}: {json.dumps(r, separators=(',', ':'))}"
                                                 for m, r in packed[k].items()) + "\n}"
            for k in sorted(packed)) + "\n}\n")
    print(f"wrote {len(snap)} geometries to {os.path.relpath(SNAPSHOT, REPO)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
