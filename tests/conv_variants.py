"""Shared pieces of tests/test_conv_variants_gpu.py: one small layer per conv kernel family and
arithmetic, the plans each must reach, the channel-slice layouts the C ABI documents
(include/dgan.h: "activations carry an explicit pixel stride ld*"), the fp64 references and the
layouts run_engine refuses by design.

Cases are (N, H, W, Cin, Cout, k, s, padding, transpose), ConvDesc's leading arguments."""
import math
import zlib

import torch

from torch_ref import conv2d_ref, conv2d_transpose_ref

P1 = (1, 1, 1, 1)   # ZeroPadding2D() + 'valid'

CASES = {
    # implicit-GEMM tiles: an input gradient with N = Cin = 10 columns (the epilogues' scalar
    # tail, the scalar split-K reduce), and a 4x4 stride-2 layer whose forward is split 8 ways
    "gemm.tail": (2, 9, 7, 10, 32, 3, 1, "same", False),
    "gemm.k4s2": (2, 8, 8, 32, 32, 4, 2, "same", False),
    # halo kernels: 3x3 stride 1; the stride-2 4x4 input gradient in four sub-pixel phases -- odd
    # H and W (phases of 7/6 x 14/13), a 15 x 31 phase grid on 8 x 16 patches, 'valid', split-K,
    # a 10-column tail, the ConvT forward -- and the stride-1 4x4 input gradient
    "halo3": (2, 9, 17, 32, 64, 3, 1, "same", False),
    "h2.odd": (2, 13, 27, 16, 32, 4, 2, "same", False),
    "h2.ragged": (1, 29, 61, 16, 32, 4, 2, "same", False),
    "h2.valid": (2, 14, 28, 32, 64, 4, 2, "valid", False),
    "h2.splitk": (1, 13, 27, 32, 512, 4, 2, "same", False),
    "h2.tail": (2, 13, 27, 10, 32, 4, 2, "same", False),
    "h2.up": (2, 7, 14, 64, 32, 4, 2, "same", True),
    "h4": (3, 11, 17, 16, 32, 4, 1, "same", False),
    # small-Cin MFMA kernels (conv_small.hip)
    "small.c3": (1, 8, 64, 3, 64, 4, 2, "same", False),
    "small.c6": (1, 8, 64, 6, 64, 4, 2, "same", False),
    "small.k3": (1, 4, 32, 3, 64, 3, 1, "same", False),
    # single-output-channel kernels (conv_co1.hip)
    "co1.c4": (2, 11, 13, 4, 1, 4, 1, P1, False),
    "co1.s2": (2, 9, 11, 64, 1, 4, 2, "same", False),
    # narrow VALU kernels (conv.hip), the fused ConvT(3) forward (conv_tlast.hip), the GEMM recast
    "narrow.fwd": (2, 6, 6, 64, 3, 1, 1, "same", False),
    "narrow.px": (1, 64, 64, 64, 3, 1, 1, "same", False),
    "narrow.dgrad": (2, 9, 7, 4, 16, 3, 2, "same", False),
    "direct.c3": (2, 9, 13, 3, 64, 3, 1, "same", False),
    "direct.c6": (2, 10, 14, 6, 64, 4, 2, "same", False),
    "tlast": (1, 5, 9, 128, 3, 4, 2, "same", True),
    "recast.dgrad": (2, 5, 7, 160, 3, 4, 2, "same", True),
    "ntile": (2, 9, 11, 3, 32, 3, 1, "same", False),
}

# the arithmetics each case runs under (ConvDesc's math=): the split-precision kernels where the
# case reaches them; the fp32-only families under fp32, and under bf16x6 where their recast's
# 1x1 GEMM then runs bf16x6
_SPLIT = ("bf16x6", "f16x3")
CASE_MATHS = {
    "gemm.tail": ("fp32", "bf16x6", "fp16"), "gemm.k4s2": ("fp32", "bf16x6", "f16x3", "fp16"),
    "halo3": ("bf16x6", "f16x3", "fp16"),
    "h2.odd": _SPLIT, "h2.ragged": _SPLIT, "h2.valid": _SPLIT, "h2.splitk": _SPLIT,
    "h2.tail": ("bf16x6",), "h2.up": ("bf16x6",), "h4": _SPLIT,
    "small.c3": ("fp32",), "small.c6": ("fp32",), "small.k3": ("fp32",),
    "co1.c4": ("fp32",), "co1.s2": ("fp32", "bf16x6"),
    "narrow.fwd": ("fp32",), "narrow.px": ("fp32",), "narrow.dgrad": ("fp32",),
    "direct.c3": ("fp32",), "direct.c6": ("fp32",), "tlast": ("fp32",),
    "recast.dgrad": ("fp32", "bf16x6"), "ntile": ("fp32",),
}
CASE_MATH = [(c, m) for c in CASES for m in CASE_MATHS[c]]

# what forces an arithmetic at these small shapes (the planner keeps small GEMMs on fp32 tiles)
MATH_ENV = {"fp32": {}, "bf16x6": {"DG_FORCE_X6CFG": "0"}, "f16x3": {"DG_FORCE_X3": "1"}, "fp16": {}}
PLAN_ENV = ("DG_PLAN_DISABLE", "DG_FORCE_X6CFG", "DG_FORCE_X3", "DG_FORCE_X3CFG", "DG_FORCE_SPLITS", "DG_CONV_MATH",
            "DG_XCD_NG")

# layouts of an activation-like tensor of C channels: (first channel, extra pixel stride) of the
# slice inside a wider buffer.  L1 keeps 16-byte alignment (ld % 4 == 0); L2 is the
# discriminator's channels 3:6 of an ld 6 buffer: a base 12 bytes off, an odd ld
LAYOUTS = {"L0": (0, 0), "L1": (4, 8), "L2": (3, 5)}
# (operand layout, output layout) of fwd / bwd_data; (x layout, dy layout) of bwd_filter
PAIRS = (("L0", "L0"), ("L1", "L1"), ("L2", "L2"), ("L2", "L0"), ("L0", "L2"))
BETAS = (0.0, 1.0, -0.5)
FWD_ACTS = (("none", 0.0), ("lrelu", 0.3), ("relu", 0.0), ("tanh", 0.0), ("sigmoid", 0.0))
MASK_ACTS = (("none", 0.0), ("relu", 0.0), ("lrelu", 0.2), ("tanh", 0.0), ("sigmoid", 0.0))

OPS = ("fwd", "bwd_data", "bwd_filter")


def op_mode(case, op):
    """The engine mode (0 FWD, 1 DGRAD, 2 WGRAD) DG_PLAN_DEBUG prints for a layer op: a
    transposed layer's forward is the input-gradient engine and its input gradient the forward's."""
    i = OPS.index(op)
    return i if not CASES[case][8] or i == 2 else 1 - i


# ---------------------------------------------------------------------------------------------
# Plans.  Per (case, math): the DG_PLAN_DEBUG lines of planning under that math, in order (the
# forward, the input gradient, the filter gradient of the layer; a recast's 1x1 GEMM prints in
# its op's place; NARROW / NARROW_DIRECT plans and a narrow op's row-segment filter gradient
# print nothing).  A planner change that moves a case off its family fails here.
# ---------------------------------------------------------------------------------------------
def _g(mode, M, N, K, name, cfg, splits, ph=0, ptiles=0):
    """A GEMM plan's line (cfg: its row of the arithmetic's tile table)."""
    return f"mode {mode} M={M} N={N} K={K} -> {name} cfg {cfg} splits {splits} ph {ph} ptiles {ptiles}"


def _h(mode, M, N, K, name, bn, splits):
    """A halo plan's line (the cfg printed is its BN; 8-row patches, one patch per block)."""
    return _g(mode, M, N, K, name, bn, splits, 8, 1)


def _s(mode, M, N, K, what):
    """co1 / small / ntile"""
    return f"mode {mode} M={M} N={N} K={K} -> {what}"


PLANS = {
    ("gemm.tail", "fp32"): [_g(0, 126, 32, 90, "fp32", 3, 1), _g(1, 126, 10, 288, "fp32", 6, 4),
                            _g(2, 90, 32, 126, "fp32", 3, 1)],
    ("gemm.tail", "bf16x6"): [_g(0, 126, 32, 90, "fp32", 3, 1), _h(1, 126, 10, 288, "x6h", 32, 1),
                              _g(2, 90, 32, 126, "fp32", 3, 1)],
    ("gemm.tail", "fp16"): [_g(0, 126, 32, 90, "fp32", 3, 1), _g(1, 126, 10, 288, "f16", 3, 1),
                            _g(2, 90, 32, 126, "fp32", 3, 1)],
    ("gemm.k4s2", "fp32"): [_g(0, 32, 32, 512, "fp32", 6, 8), _g(1, 32, 32, 128, "fp32", 3, 1),
                            _g(2, 512, 32, 32, "fp32", 3, 1)],
    ("gemm.k4s2", "bf16x6"): [_g(0, 32, 32, 512, "x6", 0, 8), _g(1, 32, 32, 128, "x6", 0, 2),
                              _g(2, 512, 32, 32, "x6", 0, 1)],
    ("gemm.k4s2", "f16x3"): [_g(0, 32, 32, 512, "x3", 3, 4), _g(1, 32, 32, 128, "x3", 3, 1),
                             _g(2, 512, 32, 32, "x3", 3, 1)],
    ("gemm.k4s2", "fp16"): [_g(0, 32, 32, 512, "f16", 3, 1), _g(1, 32, 32, 128, "f16", 3, 1),
                            _g(2, 512, 32, 32, "f16", 3, 1)],
    ("halo3", "bf16x6"): [_h(0, 306, 64, 288, "x6h", 64, 1), _h(1, 306, 32, 576, "x6h", 32, 2),
                          _g(2, 288, 64, 306, "x6", 0, 4)],
    ("halo3", "f16x3"): [_h(0, 306, 64, 288, "x3h", 64, 1), _g(1, 306, 32, 576, "x3", 3, 4, 0, 1),
                         _g(2, 288, 64, 306, "x3", 3, 1)],
    ("halo3", "fp16"): [_h(0, 306, 64, 288, "f16h", 64, 1), _h(1, 306, 32, 576, "f16h", 32, 1),
                        _g(2, 288, 64, 306, "f16", 3, 1)],
    ("h2.odd", "bf16x6"): [_g(0, 196, 32, 256, "x6", 0, 4), _h(1, 196, 16, 128, "x6h2", 64, 1),
                           _g(2, 256, 32, 196, "x6", 0, 2)],
    ("h2.odd", "f16x3"): [_g(0, 196, 32, 256, "fp32", 6, 4), _h(1, 196, 16, 128, "x3h2", 64, 1),
                          _g(2, 256, 32, 196, "fp32", 3, 1)],
    ("h2.ragged", "bf16x6"): [_g(0, 465, 32, 256, "x6", 0, 4), _h(1, 465, 16, 128, "x6h2", 64, 1),
                              _g(2, 256, 32, 465, "x6", 0, 4)],
    ("h2.ragged", "f16x3"): [_g(0, 465, 32, 256, "fp32", 6, 4), _h(1, 465, 16, 128, "x3h2", 64, 1),
                             _g(2, 256, 32, 465, "fp32", 6, 4)],
    ("h2.valid", "bf16x6"): [_g(0, 156, 64, 512, "x6", 0, 8), _h(1, 196, 32, 256, "x6h2", 64, 2),
                             _g(2, 512, 64, 156, "x6", 0, 2)],
    ("h2.valid", "f16x3"): [_g(0, 156, 64, 512, "x3", 3, 4), _h(1, 196, 32, 256, "x3h2", 64, 1),
                            _g(2, 512, 64, 156, "x3", 3, 1)],
    ("h2.splitk", "bf16x6"): [_g(0, 98, 512, 512, "x6", 0, 8), _h(1, 98, 32, 2048, "x6h2", 64, 16),
                              _g(2, 512, 512, 98, "x6", 0, 1)],
    ("h2.splitk", "f16x3"): [_g(0, 98, 512, 512, "x3", 2, 4), _h(1, 98, 32, 2048, "x3h2", 64, 8),
                             _g(2, 512, 512, 98, "x3", 3, 1)],
    ("h2.tail", "bf16x6"): [_g(0, 196, 32, 160, "fp32", 3, 1), _h(1, 196, 10, 128, "x6h2", 64, 1),
                            _g(2, 160, 32, 196, "fp32", 3, 1)],
    # (a transposed layer plans its forward -- the input-gradient engine, mode 1 -- first)
    ("h2.up", "bf16x6"): [_h(1, 196, 32, 256, "x6h2", 64, 2), _g(0, 196, 64, 512, "x6", 0, 8),
                          _g(2, 512, 64, 196, "x6", 0, 2)],
    ("h4", "bf16x6"): [_g(0, 561, 32, 256, "x6", 0, 4), _h(1, 561, 16, 512, "x6h4", 64, 1),
                       _g(2, 256, 32, 561, "x6", 0, 8)],
    ("h4", "f16x3"): [_g(0, 561, 32, 256, "fp32", 6, 4), _h(1, 561, 16, 512, "x6h4", 64, 1),
                      _g(2, 256, 32, 561, "fp32", 6, 8)],
    # (no mode 1 line: the NARROW_DIRECT input gradient)
    ("small.c3", "fp32"): [_s(0, 128, 64, 48, "small splits 1"), _s(2, 48, 64, 128, "small splits 4")],
    ("small.c6", "fp32"): [_s(0, 128, 64, 96, "small splits 1"), _s(2, 96, 64, 128, "small splits 4")],
    ("small.k3", "fp32"): [_s(0, 128, 64, 27, "small splits 1"), _s(2, 27, 64, 128, "ntile blocks 4")],
    # (co1.c4's forward, Ci 4, is k_narrow_fwd: no line; co1.s2's is the recast's 1x1 GEMM over
    # the 198 input pixels, one column per tap)
    ("co1.c4", "fp32"): [_s(1, 286, 4, 16, "co1"), _s(2, 64, 1, 240, "co1")],
    ("co1.s2", "fp32"): [_g(0, 198, 16, 64, "fp32", 3, 1), _s(1, 60, 64, 4, "co1"), _s(2, 1024, 1, 60, "co1")],
    ("co1.s2", "bf16x6"): [_g(0, 198, 16, 64, "x6", 0, 1), _s(1, 60, 64, 4, "co1"), _s(2, 1024, 1, 60, "co1")],
    # (no mode 0 / mode 2 lines: k_narrow_fwd / k_narrow_fwd_px, k_narrow_wgrad)
    ("narrow.fwd", "fp32"): [_g(1, 72, 64, 3, "fp32", 6, 1)],
    ("narrow.px", "fp32"): [_g(1, 4096, 64, 3, "fp32", 6, 1)],
    # (no mode 1 line: k_narrow_dgrad; k_direct_dgrad for direct.*)
    ("narrow.dgrad", "fp32"): [_g(0, 40, 16, 36, "fp32", 3, 1), _g(2, 36, 16, 40, "fp32", 3, 1)],
    ("direct.c3", "fp32"): [_g(0, 234, 64, 27, "fp32", 3, 1), _s(2, 27, 64, 234, "ntile blocks 18")],
    ("direct.c6", "fp32"): [_g(0, 70, 64, 96, "fp32", 3, 1), _g(2, 96, 64, 70, "fp32", 3, 1)],
    ("tlast", "fp32"): ["mode 1 -> tlast", _g(0, 45, 128, 48, "fp32", 3, 1), _g(2, 48, 128, 45, "fp32", 3, 1)],
    # (the layer forward -- engine mode 1, Ci 3, Co 160 -- prints its recast's 1x1 forward GEMM:
    # 70 pixels x 48 = 16 taps x 3 channels, K 160)
    ("recast.dgrad", "fp32"): [_g(0, 70, 48, 160, "fp32", 3, 1), _g(0, 70, 160, 48, "fp32", 3, 1),
                               _g(2, 48, 160, 70, "fp32", 3, 1)],
    ("recast.dgrad", "bf16x6"): [_g(0, 70, 48, 160, "x6", 0, 2), _g(0, 70, 160, 48, "fp32", 3, 1),
                                 _g(2, 48, 160, 70, "fp32", 3, 1)],
    ("ntile", "fp32"): [_g(0, 198, 32, 27, "fp32", 3, 1), _s(2, 27, 32, 198, "ntile blocks 18")],
}

# What each case is there for: (case, math) -> {engine mode: kernel name of its line, or None: the
# mode prints no line}; "N10": that line's GEMM has 10 columns (the epilogues' tail columns)
_N, _T = None, "N10"
FAMILY = {
    ("gemm.tail", "fp32"): {0: "fp32", 1: ("fp32", _T), 2: "fp32"},
    ("gemm.tail", "bf16x6"): {1: ("x6h", _T)}, ("gemm.tail", "fp16"): {1: ("f16", _T)},
    ("gemm.k4s2", "fp32"): {0: "fp32"}, ("gemm.k4s2", "bf16x6"): {0: "x6", 1: "x6", 2: "x6"},
    ("gemm.k4s2", "f16x3"): {0: "x3", 1: "x3", 2: "x3"}, ("gemm.k4s2", "fp16"): {0: "f16", 1: "f16", 2: "f16"},
    ("halo3", "bf16x6"): {0: "x6h", 1: "x6h"}, ("halo3", "f16x3"): {0: "x3h"}, ("halo3", "fp16"): {0: "f16h", 1: "f16h"},
    ("h2.odd", "bf16x6"): {1: "x6h2"}, ("h2.odd", "f16x3"): {1: "x3h2"},
    ("h2.ragged", "bf16x6"): {1: "x6h2"}, ("h2.ragged", "f16x3"): {1: "x3h2"},
    ("h2.valid", "bf16x6"): {1: "x6h2"}, ("h2.valid", "f16x3"): {1: "x3h2"},
    ("h2.splitk", "bf16x6"): {1: "x6h2"}, ("h2.splitk", "f16x3"): {1: "x3h2"},
    ("h2.tail", "bf16x6"): {1: ("x6h2", _T)}, ("h2.up", "bf16x6"): {1: "x6h2"},
    ("h4", "bf16x6"): {1: "x6h4"}, ("h4", "f16x3"): {1: "x6h4"},
    ("small.c3", "fp32"): {0: "small", 1: _N, 2: "small"}, ("small.c6", "fp32"): {0: "small", 1: _N, 2: "small"},
    ("small.k3", "fp32"): {0: "small", 1: _N, 2: "ntile"},
    ("co1.c4", "fp32"): {0: _N, 1: "co1", 2: "co1"},
    ("co1.s2", "fp32"): {0: "fp32", 1: "co1", 2: "co1"}, ("co1.s2", "bf16x6"): {0: "x6", 1: "co1", 2: "co1"},
    ("narrow.fwd", "fp32"): {0: _N, 2: _N}, ("narrow.px", "fp32"): {0: _N, 2: _N},
    ("narrow.dgrad", "fp32"): {1: _N}, ("direct.c3", "fp32"): {1: _N, 2: "ntile"}, ("direct.c6", "fp32"): {1: _N},
    ("tlast", "fp32"): {1: "tlast"},
    ("recast.dgrad", "fp32"): {1: _N, 0: "fp32"}, ("recast.dgrad", "bf16x6"): {1: _N, 0: "x6"},
    ("ntile", "fp32"): {2: "ntile"},
}


def plan_lines(err):
    return [line[len("[dg plan] "):] for line in err.splitlines() if line.startswith("[dg plan] ")]


def plan_desc(case, math_mode, monkeypatch, capfd):
    """The case's descriptor planned under math_mode, and the plan lines of that planning (a
    math= descriptor plans the default math first: those lines are cut off)."""
    from dgan.ops import ConvDesc
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in MATH_ENV[math_mode].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("DG_PLAN_DEBUG", "1")
    capfd.readouterr()
    ConvDesc(*CASES[case])
    first = plan_lines(capfd.readouterr().err)
    d = ConvDesc(*CASES[case], math=math_mode)
    both = plan_lines(capfd.readouterr().err)
    assert both[:len(first)] == first, f"{case}: the descriptor's first plan is not the default one"
    return d, both[len(first):]


def mode_lines(lines, mode):
    return [ln for ln in lines if ln.startswith(f"mode {mode} ")]


def kernel_of(line):
    return line.split("-> ")[1].split()[0]


# ---------------------------------------------------------------------------------------------
# References: fp64 on the CPU, once per case (and once more with the GEMM operands rounded to
# fp16, what math="fp16" computes)
# ---------------------------------------------------------------------------------------------
_REFS = {}


def reference(case, d, rounded=False):
    """x, w, bias, dy as fp32 CPU tensors (the values the device gets) and, in fp64, the layer's
    linear output y (no bias), dx, dw and dbias for them."""
    key = (case, rounded)
    if key in _REFS:
        return _REFS[key]
    N, H, W, Cin, Cout, k, s, _, T = CASES[case]
    g = torch.Generator().manual_seed(zlib.crc32(case.encode()))
    q = (lambda t: t.half().float()) if rounded else (lambda t: t)
    x = q(torch.randn(N, H, W, Cin, generator=g))
    w = q(torch.randn(*d.weight_shape, generator=g) * 0.05)
    b = torch.randn(Cout, generator=g)
    dy = q(torch.randn(*d.out_shape, generator=g))
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    y = conv2d_transpose_ref(xr, wr, s, d.pads, (d.Ho, d.Wo)) if T else conv2d_ref(xr, wr, s, d.pads)
    assert tuple(y.shape) == d.out_shape
    y.backward(dy.double())
    r = {"x": x, "w": w, "b": b, "dy": dy, "y": y.detach(), "dx": xr.grad, "dw": wr.grad,
         "db": dy.double().sum(dim=(0, 1, 2)),
         # reduction lengths of the three ops (test_conv_gpu.test_conv_layer's)
         "K": {"fwd": k * k * (Cout if T else Cin), "bwd_data": k * k * Cout, "bwd_filter": N * d.Ho * d.Wo}}
    _REFS[key] = r
    return r


def act_ref(v, act, alpha):
    if act == "lrelu":
        return torch.where(v > 0, v, alpha * v)
    if act == "relu":
        return v.clamp_min(0)
    if act == "tanh":
        return torch.tanh(v)
    if act == "sigmoid":
        return torch.sigmoid(v)
    return v


def mask_ref(z, act, alpha):
    """act'(.) through the activation's output z (fp64)."""
    if act == "lrelu":
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, alpha))
    if act == "relu":
        return (z > 0).to(z.dtype)
    if act == "tanh":
        return 1 - z * z
    if act == "sigmoid":
        return z * (1 - z)
    return torch.ones_like(z)


def rms(t):
    return float(t.pow(2).mean().sqrt())


# ---------------------------------------------------------------------------------------------
# Channel slices
# ---------------------------------------------------------------------------------------------
class Slice:
    """A [..., C] tensor as channels [c0 : c0 + C] of a device buffer of pixel stride C + extra
    (dense for L0), the rest of the buffer random; `unchanged_outside()` compares it bit for bit
    with a copy taken at construction, `unchanged()` the whole buffer."""

    def __init__(self, values, layout):
        c0, extra = LAYOUTS[layout]
        C = values.shape[-1]
        self.buf = torch.randn(*values.shape[:-1], C + extra, device="cuda")
        self.view = self.buf[..., c0:c0 + C]
        self.view.copy_(values)
        self.saved = self.buf.clone()
        self.c0, self.C = c0, C

    @staticmethod
    def _bits(t):
        return t.contiguous().view(torch.int32)

    def unchanged_outside(self):
        a, b = self.buf, self.saved
        return (torch.equal(self._bits(a[..., :self.c0]), self._bits(b[..., :self.c0])) and
                torch.equal(self._bits(a[..., self.c0 + self.C:]), self._bits(b[..., self.c0 + self.C:])))

    def unchanged(self):
        return torch.equal(self._bits(self.buf), self._bits(self.saved))


def close(got, ref, K, what, math_mode):
    """The project's bars: test_conv_gpu._close for fp32 / bf16x6 / f16x3; 2e-5 max |ref| against
    the rounded-operand reference for fp16 (tests/test_fp16_gpu.py)."""
    import test_conv_gpu
    if math_mode == "fp16":
        err = float((got.double().cpu() - ref).abs().max())
        scale = float(ref.abs().max())
        assert err <= 2e-5 * scale, f"{what}: max abs {err:.3e} vs scale {scale:.3e}"
    else:
        test_conv_gpu._close(got, ref, K, what)


# ---------------------------------------------------------------------------------------------
# Refusals
# ---------------------------------------------------------------------------------------------
# Layouts run_engine refuses by design with DG_ERR_ARG, each resting on one argument check of
# csrc/conv.hip (message fragment, where).  Only L2 -- a base 12 bytes off 16-byte alignment,
# an odd pixel stride -- is ever refused, and only on fp32 plans whose loaders are 16-byte only:
VEC = ("vector path needs lda%4==0 and 16B-aligned A",
       "run_gemm, conv.hip:1578: an fp32 GEMM whose A loader is 16-byte only (pl.vec: the reduction channels "
       "are a multiple of the tile's BK)")
LDB = ("must be multiples of 4",
       "run_gemm, conv.hip:1576: the fp32 filter-gradient GEMM reads its B operand (the conv view's output "
       "gradient) as float4 rows: ldb % 4 (and, :1579, a 16-byte aligned B)")
RECAST = ("recast path needs lda%4==0 and 16B-aligned A",
          "run_engine, conv.hip:1391: the recast's 1x1 GEMM reads the layer operand with 16-byte loads")
CO1W = ("Co == 1 filter gradient needs ldx % 4 == 0 and 16B-aligned x",
        "run_engine, conv.hip:1398: k_co1_wgrad loads x as float4")
# (case, math, op) -> {tensor of the call: the check that refuses it in L2}.  A call is refused
# exactly when one of the named tensors is in L2 (bwd_data_masked follows bwd_data).  In a
# transposed layer's filter gradient the layer's x is the conv view's output gradient (B).
REFUSALS = {
    ("gemm.tail", "fp32", "bwd_data"): {"dy": VEC},
    ("gemm.tail", "fp32", "bwd_filter"): {"dy": LDB},
    ("gemm.tail", "bf16x6", "bwd_filter"): {"dy": LDB},
    ("gemm.tail", "fp16", "bwd_filter"): {"dy": LDB},
    ("gemm.k4s2", "fp32", "fwd"): {"x": VEC},
    ("gemm.k4s2", "fp32", "bwd_data"): {"dy": VEC},
    ("gemm.k4s2", "fp32", "bwd_filter"): {"x": VEC, "dy": LDB},
    ("h2.odd", "f16x3", "fwd"): {"x": VEC},
    ("h2.odd", "f16x3", "bwd_filter"): {"x": VEC, "dy": LDB},
    ("h2.ragged", "f16x3", "fwd"): {"x": VEC},
    ("h2.ragged", "f16x3", "bwd_filter"): {"x": VEC, "dy": LDB},
    ("h2.tail", "bf16x6", "bwd_filter"): {"dy": LDB},
    ("h4", "f16x3", "fwd"): {"x": VEC},
    ("h4", "f16x3", "bwd_filter"): {"x": VEC, "dy": LDB},
    ("co1.c4", "fp32", "bwd_filter"): {"x": CO1W},
    ("co1.s2", "fp32", "fwd"): {"x": RECAST},
    ("co1.s2", "fp32", "bwd_filter"): {"x": CO1W},
    ("co1.s2", "bf16x6", "fwd"): {"x": RECAST},
    ("co1.s2", "bf16x6", "bwd_filter"): {"x": CO1W},
    ("narrow.dgrad", "fp32", "bwd_filter"): {"x": VEC, "dy": LDB},
    ("direct.c6", "fp32", "bwd_filter"): {"dy": LDB},
    ("tlast", "fp32", "bwd_filter"): {"x": LDB},
    ("recast.dgrad", "fp32", "fwd"): {"x": RECAST},
    ("recast.dgrad", "fp32", "bwd_filter"): {"x": LDB},
    ("recast.dgrad", "bf16x6", "fwd"): {"x": RECAST},
    ("recast.dgrad", "bf16x6", "bwd_filter"): {"x": LDB},
}


def refusal(case, math_mode, op, layouts):
    """The checks that refuse this call: layouts = {"x": L, "dy": L} of its operands."""
    rule = REFUSALS.get((case, math_mode, "bwd_data" if op.startswith("bwd_data") else op), {})
    return [chk for t, chk in rule.items() if layouts.get(t) == "L2"]
