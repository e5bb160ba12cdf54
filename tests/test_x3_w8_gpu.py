"""The 8-wave fp16x3 implicit-GEMM tiles (csrc/conv_tiles.h DG_TILES_X3 rows 4 and 5: 256 x 128
and 128 x 256 on a 4 x 2 / 2 x 4 wave grid) and their two-half K loop (csrc/conv_x6.hip
ktile_w8: waves 0-3 and 4-7 half a K-tile apart on three LDS buffers), forced at small shapes
-- the planner picks these tiles only at full-width layers, so otherwise only the step tests
reach them.  DG_FORCE_X3 / DG_FORCE_X3CFG / DG_FORCE_SPLITS are read when a descriptor is planned.

Paths, by the smallest shapes that reach them (nk = K-tiles of 32 per split):
  * filter gradient (K = N Ho Wo pixels): nk 1, 2, 3, even (4, 8, 14, 16) and odd (7) counts,
    a ragged last K-tile (K = 442) and a last split shorter than the others (4, 4, 4, 2);
  * N ragged against 256 and 128 (Co 96, 288); M ragged (3x3 filter gradient, M = 9 Ci = 288:
    the planner admits 3x3 filter gradients to the fp16x3 GEMM, its 3x3 forward goes to the
    halo kernel and its input gradient -- Ci 32 -- stays on the GEMM with 5, 5, 5, 3 K-tiles);
  * all three MODEs: the forward of the 4x4 stride-2 cases, the input gradient of the deep
    4 x 4 image (the halo rule leaves it on the GEMM; its filter gradient is one half-filled
    K-tile), a ConvT whose forward is the input-gradient GEMM and whose input gradient the
    forward GEMM.

Per case: the fp64 bar of test_conv_gpu.test_conv_layer, and y / dx / dw bit-identical to the
same layer on the 4-wave 128 x 128 tile (cfg 0: the lock-step loop, same BK, same K order) at
the same DG_FORCE_SPLITS."""
import re

import pytest
import torch

from dgan import ops
import test_conv_gpu   # (as a module: importing test_conv_layer by name would collect its cases here again)

gpu = pytest.mark.gpu

# (name, N, H, W, Cin, Cout, k, s, padding, transpose, bias)
DOWN = ("w8.down", 2, 32, 32, 64, 128, 4, 2, "same", False, False)
NK3 = ("w8.nk3", 2, 24, 32, 64, 128, 4, 2, "same", False, False)
KRAG = ("w8.kragged", 2, 34, 26, 64, 128, 4, 2, "same", False, True)
CO96 = ("w8.co96", 2, 32, 32, 64, 96, 4, 2, "same", False, True)
CO288 = ("w8.co288", 2, 32, 32, 64, 288, 4, 2, "same", False, False)
M288 = ("w8.m288", 2, 16, 16, 32, 64, 3, 1, "same", False, False)
DEEP = ("w8.deep", 4, 4, 4, 512, 512, 4, 2, "same", False, False)
UPODD = ("w8.up.odd", 2, 9, 7, 64, 32, 4, 2, "same", True, True)

# (case, DG_FORCE_SPLITS, GEMM modes that must run the forced tile: 0 FWD, 1 DGRAD, 2 WGRAD)
W8_CASES = [
    (DOWN, 16, (0, 2)),    # filter gradient nk 1 (forward nk 2)
    (DOWN, 8, (0, 2)),     # nk 2
    (NK3, 4, (0, 2)),      # nk 3
    (DOWN, 2, (0, 2)),     # nk 8
    (DOWN, 1, (0, 2)),     # nk 16, no split-K
    (KRAG, 2, (0, 2)),     # nk 7, ragged last K-tile
    (KRAG, 4, (0, 2)),     # nk 4, 4, 4, 2
    (KRAG, 1, (0, 2)),     # nk 14
    (CO96, 2, (0, 2)),
    (CO288, 2, (0, 2)),
    (M288, 1, (1, 2)),
    (M288, 4, (1, 2)),     # input gradient nk 5, 5, 5, 3
    (DEEP, 1, (0, 1, 2)),
    (UPODD, 2, (0, 1, 2)),
]
IDS = [f"{c[0]}-s{s}" for c, s, _ in W8_CASES]


def _wgrad_nk(case, splits):
    """K-tiles per split of the case's filter-gradient GEMM (conv_plan.hip choose_tiles)."""
    _, N, H, W, Cin, Cout, k, s, padding, transpose, _ = case
    Ho, Wo = (H, W) if transpose or s == 1 else ((H + s - 1) // s, (W + s - 1) // s)
    K = N * Ho * Wo
    ktiles = (K + 31) // 32
    per = (ktiles + splits - 1) // splits
    n = (ktiles + per - 1) // per
    return [min(per, ktiles - i * per) for i in range(n)], K


def test_w8_cases_cover_the_k_loop_paths():
    nks, ragged, short_last = set(), False, False
    for case, splits, _ in W8_CASES:
        nk, K = _wgrad_nk(case, splits)
        nks.update(nk)
        ragged |= K % 32 != 0
        short_last |= len(nk) > 1 and nk[-1] < nk[0]
    assert {1, 2, 3} <= nks
    assert any(n >= 5 and n % 2 == 0 for n in nks) and any(n >= 5 and n % 2 == 1 for n in nks)
    assert ragged and short_last


def _plans(err):
    """{mode: (kernel, cfg, splits)} of the DG_PLAN_DEBUG lines (the last per mode)."""
    out = {}
    for line in err.splitlines():
        m = re.match(r"\[dg plan\] mode (\d) .* -> (\S+) cfg (\d+) splits (\d+)", line)
        if m:
            out[int(m.group(1))] = (m.group(2), int(m.group(3)), int(m.group(4)))
    return out


def _rand(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).cuda()


def _run(case, capfd):
    """y, dx, dw of the layer as the environment plans it, and its plans."""
    name, N, H, W, Cin, Cout, k, s, padding, transpose, has_bias = case
    capfd.readouterr()
    d = ops.ConvDesc(N, H, W, Cin, Cout, k, s, padding, transpose, math="f16x3")
    plans = _plans(capfd.readouterr().err)
    x, w, dy = _rand((N, H, W, Cin), 31), _rand(d.weight_shape, 32, 0.05), _rand(d.out_shape, 33)
    b = _rand((Cout,), 34) if has_bias else None
    y, dx, dw = torch.empty(d.out_shape, device="cuda"), torch.empty_like(x), torch.empty_like(w)
    d.fwd(x, w, y, bias=b)
    d.bwd_data(dy, w, dx)
    d.bwd_filter(x, dy, dw)
    torch.cuda.synchronize()
    return (y, dx, dw), plans


_REF = {}   # (case name, splits) -> the cfg 0 results, computed once for both 8-wave tiles


@gpu
@pytest.mark.parametrize("cfg", [5, 4])
@pytest.mark.parametrize("case,splits,modes", W8_CASES, ids=IDS)
def test_w8_tile_matches_fp64_and_the_4wave_tile(case, splits, modes, cfg, monkeypatch, capfd):
    monkeypatch.delenv("DG_PLAN_DISABLE", raising=False)
    monkeypatch.setenv("DG_FORCE_X3", "1")
    monkeypatch.setenv("DG_FORCE_SPLITS", str(splits))
    monkeypatch.setenv("DG_PLAN_DEBUG", "1")
    key = (case[0], splits)
    if key not in _REF:
        monkeypatch.setenv("DG_FORCE_X3CFG", "0")
        _REF[key] = _run(case, capfd)
    ref, ref_plans = _REF[key]
    monkeypatch.setenv("DG_FORCE_X3CFG", str(cfg))
    got, plans = _run(case, capfd)
    nk, _ = _wgrad_nk(case, splits)
    for mode in modes:
        assert plans.get(mode, ("", -1, 0))[:2] == ("x3", cfg), f"{case[0]}: mode {mode} planned {plans.get(mode)}"
        assert ref_plans[mode][0] == "x3" and ref_plans[mode][1] == 0 and ref_plans[mode][2] == plans[mode][2]
    assert plans[2][2] == len(nk), f"{case[0]}: filter gradient planned {plans[2]}, expected {len(nk)} splits"
    test_conv_gpu.test_conv_layer(case, "f16x3")
    for what, a, b in zip(("y", "dx", "dw"), got, ref):
        assert torch.equal(a, b), f"{case[0]} cfg {cfg} splits {splits}: {what} differs from the 4-wave tile"
