"""The conv engine as its C ABI documents it (include/dgan.h dg_conv_fwd / _bwd_data /
_bwd_data_masked / _bwd_filter) and as the networks call it, one small layer per kernel family
and arithmetic (conv_variants.CASES): channel slices of wider buffers through ld* -- aligned
(L1) and 12 bytes off 16-byte alignment with an odd pixel stride (L2), operand and output
independently -- beta accumulation on all three ops and on dbias, the five fused forward
activations with and without bias, the five act'(z) gradient masks, and the mask over the
accumulated sum on the split-precision plans.

Every case first asserts, from DG_PLAN_DEBUG, the plan it is there for (conv_variants.PLANS /
FAMILY): the kernels' epilogues pick their vector / scalar / tail branches at run time from
exactly these inputs, so a case that silently moved to another kernel would test nothing.

Per variant: the result against the fp64 CPU reference of the same operation at the project's
bars (conv_variants.close; dbias: 1e-6 max_c sum |dy|); with beta 0 the output is pre-filled
with NaN and must come back finite (0 * C is never read); everything in the surrounding buffers
outside the written slice, and every operand buffer, is bit-equal to a copy taken before the
call.  Layouts the engine refuses by design are listed in conv_variants.REFUSALS: such a call
must raise DG_ERR_ARG and leave its outputs untouched; a refusal outside the table fails."""
import zlib

import pytest
import torch

import conv_variants as V

gpu = pytest.mark.gpu
IDS = [f"{c}-{m}" for c, m in V.CASE_MATH]


def _planned(case, math_mode, monkeypatch, capfd):
    """The descriptor, its plan lines (asserted), the references."""
    d, lines = V.plan_desc(case, math_mode, monkeypatch, capfd)
    assert lines == V.PLANS[(case, math_mode)], f"{case} [{math_mode}] planned {lines}"
    for mode, want in V.FAMILY[(case, math_mode)].items():
        got = V.mode_lines(lines, mode)
        if want is None:
            assert not got, f"{case} [{math_mode}]: mode {mode} should print no plan line, printed {got}"
            continue
        name, tail = want if isinstance(want, tuple) else (want, None)
        assert got and V.kernel_of(got[0]) == name, f"{case} [{math_mode}]: mode {mode} planned {got}, expected {name}"
        if tail:
            assert " N=10 " in got[0], f"{case} [{math_mode}]: mode {mode} has no tail columns: {got[0]}"
    ref = V.reference(case, d, rounded=math_mode == "fp16")
    torch.manual_seed(zlib.crc32(f"{case}/{math_mode}".encode()))
    return d, lines, ref


def _prefill(res, beta):
    """(what the output holds before the call, the expected result): randn x rms(result) and
    result + beta * prefill in fp64; NaN for beta 0."""
    if beta == 0.0:
        return torch.full(res.shape, float("nan")), res
    pre = (torch.randn(res.shape) * V.rms(res)).float()
    return pre, res + beta * pre.double()


def _call(case, math_mode, op, layouts, outs, what, fn):
    """Run fn; True if it ran, False if it was refused as the table says (outputs untouched)."""
    from dgan._lib import DGError
    hit = V.refusal(case, math_mode, op, layouts)
    try:
        fn()
    except DGError as e:
        torch.cuda.synchronize()
        assert hit, f"{what}: refused, but not in the refusal table: {e}"
        assert "rc=1" in str(e) and any(chk[0] in str(e) for chk in hit), f"{what}: refused otherwise: {e}"
        for o in outs:
            assert o.unchanged(), f"{what}: refused, yet the output buffer changed"
        return False
    torch.cuda.synchronize()
    assert not hit, f"{what}: ran, but the refusal table expects DG_ERR_ARG ({hit[0][1]})"
    return True


def _settled(what, operands, outs):
    for t in operands:
        assert t.unchanged(), f"{what}: an operand buffer changed"
    for o in outs:
        assert o.unchanged_outside(), f"{what}: wrote outside the output slice"
        assert bool(torch.isfinite(o.view).all()), f"{what}: non-finite output (beta * C read at beta 0?)"


def _fwd(case, math_mode, d, ref, w, lx, ly, beta, bias, act, alpha):
    what = f"{case} [{math_mode}] fwd x {lx} y {ly} beta {beta} bias {int(bias)} act {act}"
    res = V.act_ref(ref["y"] + ref["b"].double() if bias else ref["y"], act, alpha)
    pre, want = _prefill(res, beta)
    x, y = V.Slice(ref["x"], lx), V.Slice(pre, ly)
    b = ref["b"].cuda() if bias else None
    if not _call(case, math_mode, "fwd", {"x": lx}, [y], what,
                 lambda: d.fwd(x.view, w, y.view, bias=b, act=act, alpha=alpha, beta=beta)):
        return False
    _settled(what, [x], [y])
    V.close(y.view, want, ref["K"]["fwd"], what, math_mode)
    return True


def _mask_z(shape, act, alpha):
    """A valid output of the activation, fp32: relu about half exact zeros, tanh inside (-1, 1),
    sigmoid inside (0, 1)."""
    z = V.act_ref(torch.randn(shape), act, alpha).float()
    if act == "relu":
        assert 0.3 < float((z == 0).float().mean()) < 0.7
    if act == "tanh":
        assert float(z.abs().max()) < 1.0
    if act == "sigmoid":
        assert 0.0 < float(z.min()) and float(z.max()) < 1.0
    return z


def _bwd_data(case, math_mode, d, ref, w, ldy, ldx, beta, mask=None, masked_sum=False):
    act, alpha = mask if mask else (None, 0.0)
    op = "bwd_data" if not mask else ("bwd_data_masked_sum" if masked_sum else "bwd_data_masked")
    what = f"{case} [{math_mode}] {op} dy {ldy} dx {ldx} beta {beta} act {act}"
    res = ref["dx"]
    z = None
    if mask:
        zv = _mask_z(res.shape, act, alpha)
        z = V.Slice(zv, ldx)
        mf = V.mask_ref(zv.double(), act, alpha)
    if masked_sum:      # dx = act'(z) * (dL/dx + beta * dx)
        pre = (torch.randn(res.shape) * V.rms(res)).float()
        want = mf * (res + beta * pre.double())
    else:               # dx = dL/dx * act'(z) + beta * dx
        pre, want = _prefill(res * mf if mask else res, beta)
    dy, dx = V.Slice(ref["dy"], ldy), V.Slice(pre, ldx)
    if masked_sum:
        fn = lambda: d.bwd_data_masked_sum(dy.view, w, dx.view, z.view, act, alpha=alpha, beta=beta)
    elif mask:
        fn = lambda: d.bwd_data_masked(dy.view, w, dx.view, z.view, act, alpha=alpha, beta=beta)
    else:
        fn = lambda: d.bwd_data(dy.view, w, dx.view, beta=beta)
    if not _call(case, math_mode, op, {"dy": ldy}, [dx], what, fn):
        return False
    _settled(what, [dy] + ([z] if mask else []), [dx])
    V.close(dx.view, want, ref["K"]["bwd_data"], what, math_mode)
    return True


def _bwd_filter(case, math_mode, d, ref, lx, ldy, beta):
    what = f"{case} [{math_mode}] bwd_filter x {lx} dy {ldy} beta {beta}"
    pre_w, want_w = _prefill(ref["dw"], beta)
    pre_b, want_b = _prefill(ref["db"], beta)
    x, dy = V.Slice(ref["x"], lx), V.Slice(ref["dy"], ldy)
    dw, db = V.Slice(pre_w, "L0"), V.Slice(pre_b.float(), "L0")
    if not _call(case, math_mode, "bwd_filter", {"x": lx, "dy": ldy}, [dw, db], what,
                 lambda: d.bwd_filter(x.view, dy.view, dw.view, dbias=db.view, beta=beta)):
        return False
    _settled(what, [x, dy], [dw, db])
    V.close(dw.view, want_w, ref["K"]["bwd_filter"], what, math_mode)
    # a column sum of random-sign terms can cancel: scale by sum |dy| instead of |sum|
    err = float((db.view.double().cpu() - want_b).abs().max())
    assert err <= 1e-6 * float(ref["dy"].double().abs().sum(dim=(0, 1, 2)).max()), f"{what}: dbias {err:.3e}"
    return True


@gpu
@pytest.mark.parametrize("case,math_mode", V.CASE_MATH, ids=IDS)
def test_conv_layouts_and_beta(case, math_mode, monkeypatch, capfd):
    """layout x beta on the three ops (the forward with bias, the filter gradient with dbias)."""
    d, _, ref = _planned(case, math_mode, monkeypatch, capfd)
    w = ref["w"].cuda()
    ran = []
    for la, lb in V.PAIRS:
        for beta in V.BETAS:
            ran.append(_fwd(case, math_mode, d, ref, w, la, lb, beta, True, "none", 0.0))
            ran.append(_bwd_data(case, math_mode, d, ref, w, la, lb, beta))
            ran.append(_bwd_filter(case, math_mode, d, ref, la, lb, beta))
    # 5 layout pairs x 3 betas x 3 ops; the dense and the aligned-slice calls are never refused
    assert len(ran) == 45 and sum(ran) >= 18 and all(ran[:18]), ran


# the cases whose input gradient runs a split-precision plan: bwd_data_masked_sum applies
MASKED_SUM = {(c, m) for c, m in V.CASE_MATH if m != "fp32" and
              c in ("gemm.tail", "gemm.k4s2", "halo3", "h2.odd", "h2.ragged", "h2.valid", "h2.splitk", "h2.tail", "h2.up",
                    "h4")}


def _nondense(case, math_mode, op, tensor):
    """L2 where the op takes it, else L1 (conv_variants.REFUSALS)."""
    return "L1" if V.refusal(case, math_mode, op, {tensor: "L2"}) else "L2"


@gpu
@pytest.mark.parametrize("case,math_mode", V.CASE_MATH, ids=IDS)
def test_conv_epilogues_and_masks(case, math_mode, monkeypatch, capfd):
    """The forward epilogue (bias on / off x five activations; a transposed layer's runs on the
    input-gradient kernels) and the gradient masks (five activations, z in all three layouts,
    beta 0 and 1; the mask over the accumulated sum on the split-precision plans)."""
    d, lines, ref = _planned(case, math_mode, monkeypatch, capfd)
    w = ref["w"].cuda()
    ran = []
    for lay in ("L0", _nondense(case, math_mode, "fwd", "x")):
        for bias in (True, False):
            for act, alpha in V.FWD_ACTS:
                ran.append(_fwd(case, math_mode, d, ref, w, lay, lay, 0.0, bias, act, alpha))
    nd = _nondense(case, math_mode, "bwd_data", "dy")
    for ldy, ldx in (("L0", "L0"), ("L1", "L1"), (nd, "L2")):
        for mask in V.MASK_ACTS:
            for beta in (0.0, 1.0):
                ran.append(_bwd_data(case, math_mode, d, ref, w, ldy, ldx, beta, mask=mask))
    # (the layouts above avoid the refusal table: every one of these runs)
    assert len(ran) == 50 and all(ran), ran
    split = d.op_arith("bwd_data") != "fp32"
    if split:
        assert V.kernel_of(V.mode_lines(lines, V.op_mode(case, "bwd_data"))[0]) != "fp32"
        for lay in ("L1", "L2"):
            for mask in (("relu", 0.0), ("tanh", 0.0)):
                assert _bwd_data(case, math_mode, d, ref, w, lay, lay, 1.0, mask=mask, masked_sum=True)
    assert split == ((case, math_mode) in MASKED_SUM), f"{case} [{math_mode}]: bwd_data runs {d.op_arith('bwd_data')}"


@gpu
def test_refusal_table_exempts_no_dense_or_aligned_layout():
    """The table's cap: only (case, math, op) triples that exist, only checks this file cites, and
    -- by construction of conv_variants.refusal -- only L2 operands; L0 and L1 always run."""
    for (case, math_mode, op), rule in V.REFUSALS.items():
        assert (case, math_mode) in V.PLANS and op in V.OPS
        assert set(rule) <= ({"x"} if op == "fwd" else {"dy"} if op == "bwd_data" else {"x", "dy"})
        assert all(chk in (V.VEC, V.LDB, V.RECAST, V.CO1W) for chk in rule.values())
    for case, math_mode in V.CASE_MATH:
        for op in V.OPS + ("bwd_data_masked", "bwd_data_masked_sum"):
            for lay in ("L0", "L1"):
                assert not V.refusal(case, math_mode, op, {"x": lay, "dy": lay})
