"""The optimizer, loss-scale, staging and element-wise kernels (csrc/runtime.hip, and the
small kernels dgan.ops reaches in layers.hip / bn.hip / conv_x6.hip) called directly, each
against a plain fp64 (or exact fp32) restatement on the CPU.

The training-step tests reach these kernels only at the workload's shapes and behind Adam's
sign-like normalisation; here every loop of k_adam, the loss-scale state machine at its floor
and guard, the capped grid-stride tails, pixel strides wider than the channel count and the
exact-tie cases are driven on purpose.

Tolerances: Adam against oracle.p2p_oracle.adam_update as test_adam_kernel_matches_keras_adam
(m 1e-5 / 1e-9, v 3e-5 / 1e-12, p 2.5e-7 / 1e-7); the scheduled Adam's p as
test_adam_exponential_decay (1e-6 of the scale); element-wise kernels 1e-6 of the scale;
copies, one-multiplication kernels, the loss-scale state and the fp16 conversion bit for bit.
"""
import numpy as np
import pytest
import torch

from oracle import p2p_oracle as O
from oracle import sr_oracle as S

gpu = pytest.mark.gpu
DEV = "cuda"
SENT = 777.0          # sentinel of padding columns and of the floats after a buffer's end

ADAM_TOL = {"m": (1e-5, 1e-9), "v": (3e-5, 1e-12), "p": (2.5e-7, 1e-7)}


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    """The tensor's bytes as integers (nan-safe, -0.0 != 0.0)."""
    a = _np(t) if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same_bits(got, want, what=""):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g.ravel() != w.ravel())
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first at flat index {bad[0]}"


def _close(got, ref, rtol, atol=0.0, what=""):
    """max |got - ref| <= atol + rtol * max |ref| (tests/test_sr_gpu.py _close)."""
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = ref.detach().double().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite result"
    err = np.abs(got - ref).max() if got.size else 0.0
    scale = np.abs(ref).max() if ref.size else 0.0
    assert err <= atol + rtol * scale, f"{what}: max abs err {err:.3e} vs scale {scale:.3e}"


def _tail_view(n, fill=0.0, extra=8, dtype=torch.float32):
    """(buffer of n + extra elements whose last `extra` hold SENT, its first n as a contiguous view)."""
    buf = torch.full((n + extra,), fill, dtype=dtype, device=DEV)
    buf[n:] = SENT
    return buf, buf[:n]


def _tail_ok(buf, n, what=""):
    assert bool((buf[n:] == SENT).all()), f"{what}: wrote past the end"


def _padded2(rows, C, ld, off=0, fill=SENT):
    """([rows, ld] buffer of `fill`, its channel slice [:, off:off+C])."""
    buf = torch.full((rows, ld), fill, dtype=torch.float32, device=DEV)
    return buf, buf[:, off:off + C]


def _pad_ok(buf, C, off=0, what=""):
    keep = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
    keep[off:off + C] = False
    assert bool((buf[..., keep] == SENT).all()), f"{what}: padding columns written"


def _adam_inputs(rng, n):
    """The draws of test_adam_kernel_matches_keras_adam: gradient magnitudes over e^-20 .. 1."""
    p = rng.standard_normal(n, dtype=np.float32)
    g = rng.standard_normal(n, dtype=np.float32) * np.exp(rng.uniform(-20, 0, n).astype(np.float32))
    m = rng.standard_normal(n, dtype=np.float32) * np.float32(1e-3)
    v = rng.random(n, dtype=np.float32) * np.float32(1e-5)
    return p, g, m, v


def _adam_close(got, ref, what):
    for k in ("m", "v", "p"):
        rtol, atol = ADAM_TOL[k]
        a = got[k].double()                      # np.allclose's |a - b| <= atol + rtol |b|, on the device
        b = torch.from_numpy(np.ascontiguousarray(ref[k])).to(a.device).double()
        ratio = (a - b).abs() / (atol + rtol * b.abs())
        i = int(ratio.argmax())
        worst = float(ratio[i])
        print(f"{what} {k}: worst err/tol {worst:.3f}")
        assert bool(torch.isfinite(a).all()) and worst <= 1.0, \
            f"{what} {k}[{i}]: got {float(a[i])!r} want {float(b[i])!r} (rtol {rtol}, atol {atol})"


# -------------------------------------------------------------------------
# 1. Adam: the unrolled float4 loop, the single-group loop and the scalar tail
# -------------------------------------------------------------------------
# dg_adam launches min(cdiv(n/4 + 1, 256), ADAM_GRID_CAP) blocks of 256 lanes over n/4 float4
# groups, and k_adam's first loop takes ADAM_UNROLL groups per lane and round.
ADAM_GRID_CAP, ADAM_BLOCK, ADAM_UNROLL = 4096, 256, 4
HYPER = dict(lr=2e-4, b1=0.5, b2=0.999, eps=1e-7)


@gpu
def test_adam_all_three_loops_match_oracle_and_chunked_calls():
    """One call on n floats where every loop of k_adam runs, against the fp64 oracle; then the
    same inputs in chunks that stay in the single-group loop, which must give the same bits."""
    from dgan import ops
    # Below the cap the stride is at least n/4 + 1 lanes, so every lane owns at most one group
    # and the unrolled loop (i + 3 * stride < n/4) cannot run.  At the cap the stride is
    # 4096 * 256 lanes: lane i enters the unrolled loop iff i + 3 * stride < n/4.  With
    # n/4 = 3 * stride + 1000, lanes 0..999 take one unrolled round (4 groups), every other lane
    # takes the single-group loop three times, and n % 4 = 3 elements fall to the scalar tail.
    stride = ADAM_GRID_CAP * ADAM_BLOCK
    n = 4 * ((ADAM_UNROLL - 1) * stride + 1000) + 3
    assert n == 12586915
    n4 = n // 4
    rng = np.random.default_rng(101)
    p, g, m, v = _adam_inputs(rng, n)
    t = 7
    it = torch.tensor([t - 1], dtype=torch.int32, device=DEV)
    bufs = {k: _tail_view(n) for k in "pgmv"}
    for k, a in zip("pgmv", (p, g, m, v)):
        bufs[k][1].copy_(torch.from_numpy(a))
    d = {k: bufs[k][1] for k in "pgmv"}
    ops.adam(d["p"], d["g"], d["m"], d["v"], HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], it)
    rp, rm, rv = O.adam_update(p, g.astype(np.float64), m, v, t, **HYPER)
    torch.cuda.synchronize()
    for k in "pmv":
        _tail_ok(bufs[k][0], n, f"adam {k}")
    assert torch.equal(d["g"].view(torch.int32), _dev(g).view(torch.int32)), "adam wrote g"
    _adam_close(d, dict(p=rp, m=rm, v=rv), "adam n=12586915")

    # path check: the update is element-wise, so chunks on float4 boundaries, each small enough
    # that its grid is not capped (chunk/4 + 1 <= 4096 * 256: one group per lane at most), run
    # the single-group loop only and must reproduce the one-call result bit for bit
    chunk = 4_000_000
    assert chunk % 4 == 0 and chunk // 4 + 1 <= stride
    c = {k: _dev(a) for k, a in zip("pgmv", (p, g, m, v))}
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        ops.adam(c["p"][lo:hi], c["g"][lo:hi], c["m"][lo:hi], c["v"][lo:hi], HYPER["lr"], HYPER["b1"],
                 HYPER["b2"], HYPER["eps"], it)
    torch.cuda.synchronize()
    for k in "pmv":
        same = c[k][:4 * n4].view(torch.int32) == d[k][:4 * n4].view(torch.int32)
        nbad = int((~same).sum())
        first = int(torch.nonzero(~same)[0]) if nbad else -1
        assert nbad == 0, f"adam {k}: {nbad} float4-part elements differ between one call and chunks, first {first}"
    _adam_close({k: c[k][4 * n4:] for k in "pmv"}, dict(p=rp[4 * n4:], m=rm[4 * n4:], v=rv[4 * n4:]),
                "adam chunked tail")


@gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_adam_tiny_sizes(n):
    """Tail only (1, 3), exactly one float4 group (4), one group plus tail (5)."""
    from dgan import ops
    rng = np.random.default_rng(110 + n)
    p, g, m, v = _adam_inputs(rng, n)
    t = 3
    it = torch.tensor([t - 1], dtype=torch.int32, device=DEV)
    bufs = {k: _tail_view(n) for k in "pgmv"}
    for k, a in zip("pgmv", (p, g, m, v)):
        bufs[k][1].copy_(torch.from_numpy(a))
    d = {k: bufs[k][1] for k in "pgmv"}
    ops.adam(d["p"], d["g"], d["m"], d["v"], HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], it)
    torch.cuda.synchronize()
    rp, rm, rv = O.adam_update(p, g.astype(np.float64), m, v, t, **HYPER)
    for k in "pgmv":
        _tail_ok(bufs[k][0], n, f"adam n={n} {k}")
    _adam_close(d, dict(p=rp, m=rm, v=rv), f"adam n={n}")


# -------------------------------------------------------------------------
# 2. adam_sched: continuous ExponentialDecay, grad_scale
# -------------------------------------------------------------------------
SCHED = dict(lr=1e-3, steps=100000, rate=0.1, b1=0.9, b2=0.999, eps=1e-7)


def _sched_inputs(rng, n):
    """test_adam_exponential_decay's draws with p shrunk to 0.03: the check is 1e-6 of max |p|,
    and a step under the decayed rate (3e-6 at iteration 250001) has to stand above that.  No
    smaller: fp32 leaves 1e-5 relative in the first steps' 1 - beta2^t, so a step must stay
    below a tenth of max |p| (steps reach 1.3e-3 at iteration 0)."""
    p, g = rng.standard_normal(n) * 0.03, rng.standard_normal(n) * 1e-3
    m, v = rng.standard_normal(n) * 1e-4, rng.uniform(0, 1e-6, n)
    return [a.astype(np.float32) for a in (p, g, m, v)]


def _sched_ref(p, g, m, v, it, staircase, grad_scale=1.0):
    lr = S.exp_decay(SCHED["lr"], it, SCHED["steps"], SCHED["rate"], staircase)
    f = lambda a: a.astype(np.float64)   # noqa: E731
    return S.adam_update(f(p), grad_scale * f(g), f(m), f(v), it + 1, lr, SCHED["b1"], SCHED["b2"], SCHED["eps"])


def _run_sched(ops, p, g, m, v, it, staircase, grad_scale=1.0):
    dp, dg, dm, dv = (_dev(a) for a in (p, g, m, v))
    itd = torch.tensor([it], dtype=torch.int32, device=DEV)
    ops.adam_sched(dp, dg, dm, dv, SCHED["lr"], SCHED["steps"], SCHED["rate"], staircase, SCHED["b1"], SCHED["b2"],
                   SCHED["eps"], itd, grad_scale=grad_scale)
    torch.cuda.synchronize()
    return dp, dm, dv


@gpu
@pytest.mark.parametrize("it", [0, 1, 99999, 100000, 250001])
def test_adam_sched_continuous_decay(it):
    from dgan import ops
    rng = np.random.default_rng(120)
    n = 1027   # one ragged float4 bulk and a three-element tail
    p, g, m, v = _sched_inputs(rng, n)
    dp, dm, dv = _run_sched(ops, p, g, m, v, it, staircase=False)
    rp, rm, rv = _sched_ref(p, g, m, v, it, staircase=False)
    _close(dp, rp, 1e-6, what=f"adam_sched p it={it}")
    assert np.allclose(_np(dm), rm, rtol=ADAM_TOL["m"][0], atol=ADAM_TOL["m"][1])
    assert np.allclose(_np(dv), rv, rtol=ADAM_TOL["v"][0], atol=ADAM_TOL["v"][1])
    if it in (99999, 250001):
        # the staircase rate differs here by far more than the tolerance resolves
        sp = _sched_ref(p, g, m, v, it, staircase=True)[0]
        assert np.abs(sp - rp).max() > 100 * 1e-6 * np.abs(rp).max()


@gpu
def test_adam_sched_grad_scale():
    from dgan import ops
    rng = np.random.default_rng(121)
    n = 1027
    p, g, m, v = _sched_inputs(rng, n)
    dp, dm, dv = _run_sched(ops, p, g, m, v, 41, staircase=False, grad_scale=0.25)
    rp, rm, rv = _sched_ref(p, g, m, v, 41, staircase=False, grad_scale=0.25)
    _close(dp, rp, 1e-6, what="adam_sched p grad_scale")
    assert np.allclose(_np(dm), rm, rtol=ADAM_TOL["m"][0], atol=ADAM_TOL["m"][1])
    assert np.allclose(_np(dv), rv, rtol=ADAM_TOL["v"][0], atol=ADAM_TOL["v"][1])
    up = _sched_ref(p, g, m, v, 41, staircase=False)[0]      # the unscaled gradient moves p elsewhere
    assert np.abs(up - rp).max() > 100 * 1e-6 * np.abs(rp).max()


# -------------------------------------------------------------------------
# 3. adam_ls / counter_add_ls: the step under a dynamic loss scale
# -------------------------------------------------------------------------
def _ls_state(scale, good, flag):
    return torch.tensor([scale, good, flag, SENT], dtype=torch.float32, device=DEV)


LS_ADAM = dict(lr=2e-4, steps=100000, rate=0.1, staircase=False, b1=0.5, b2=0.999, eps=1e-7)


def _adam_ls(ops, d, it, ls, grad_scale):
    h = LS_ADAM
    ops.adam_ls(d["p"], d["g"], d["m"], d["v"], h["lr"], h["steps"], h["rate"], h["staircase"], h["b1"], h["b2"],
                h["eps"], it, ls, grad_scale=grad_scale)


@gpu
def test_adam_ls_skips_the_step_on_a_cleared_flag():
    from dgan import ops
    rng = np.random.default_rng(130)
    n = 2051
    p, g, m, v = _adam_inputs(rng, n)
    g[5], g[n - 1] = np.inf, np.nan     # what clears the flag in a real step
    d = {k: _dev(a) for k, a in zip("pgmv", (p, g, m, v))}
    it = torch.tensor([6], dtype=torch.int32, device=DEV)
    ls = _ls_state(2.0 ** 15, 2.0, 0.0)
    ls0 = ls.clone()
    _adam_ls(ops, d, it, ls, 0.5)
    ops.counter_add_ls(it, ls)
    torch.cuda.synchronize()
    for k, a in zip("pgmv", (p, g, m, v)):
        _same_bits(d[k], a, f"skipped step {k}")
    assert int(it.item()) == 6
    _same_bits(ls, ls0, "loss-scale state")


@gpu
@pytest.mark.parametrize("scale", [2.0 ** 15, 1.0])
def test_adam_ls_unscales_like_adam_sched(scale):
    """Flag set: the scaled gradient G = g * S steps exactly as adam_sched steps g (a power of
    two unscales exactly), within the oracle's tolerances of 0.5 * g; the counter rises."""
    from dgan import ops
    rng = np.random.default_rng(131)
    n = 2051
    p, g, m, v = _adam_inputs(rng, n)
    G = g * np.float32(scale)
    # g * S neither overflows nor goes subnormal, so G / S gives g back exactly
    tiny = np.finfo(np.float32).tiny
    assert np.isfinite(G).all() and (np.abs(G[G != 0]) >= tiny).all() and (np.abs(g[g != 0]) >= 4 * tiny).all()
    assert np.array_equal(G / np.float32(scale), g)
    t = 7
    h = LS_ADAM
    a = {k: _dev(x) for k, x in zip("pgmv", (p, G, m, v))}
    it = torch.tensor([t - 1], dtype=torch.int32, device=DEV)
    ls = _ls_state(scale, 1.0, 1.0)
    ls0 = ls.clone()
    _adam_ls(ops, a, it, ls, 0.5)
    b = {k: _dev(x) for k, x in zip("pgmv", (p, g, m, v))}
    ops.adam_sched(b["p"], b["g"], b["m"], b["v"], h["lr"], h["steps"], h["rate"], h["staircase"], h["b1"], h["b2"],
                   h["eps"], it, grad_scale=0.5)
    torch.cuda.synchronize()
    for k in "pmv":
        _same_bits(a[k], b[k], f"adam_ls vs adam_sched {k}")
    _same_bits(a["g"], G, "adam_ls g (read only)")
    lr = S.exp_decay(h["lr"], t - 1, h["steps"], h["rate"], h["staircase"])
    rp, rm, rv = O.adam_update(p, 0.5 * g.astype(np.float64), m, v, t, lr=lr, b1=h["b1"], b2=h["b2"], eps=h["eps"])
    _adam_close(a, dict(p=rp, m=rm, v=rv), f"adam_ls S={scale}")
    ops.counter_add_ls(it, ls)
    torch.cuda.synchronize()
    assert int(it.item()) == t
    _same_bits(ls, ls0, "loss-scale state")


# -------------------------------------------------------------------------
# 4. loss_scale_update: Keras DynamicLossScale
# -------------------------------------------------------------------------
def _keras_dynamic_loss_scale(scale, good, finite, period, mult):
    """tf.keras mixed_precision DynamicLossScale.update on fp32 state: finite gradients count a
    good step and, at `period` of them, multiply the scale (kept when the product is not
    finite) and restart the count; non-finite ones divide it, not below 1, and restart."""
    scale, mult, good = np.float32(scale), np.float32(mult), np.float32(good)
    if finite:
        if good + np.float32(1) >= np.float32(period):
            with np.errstate(over="ignore"):
                grown = np.float32(scale * mult)
            if np.isfinite(grown):
                scale = grown
            good = np.float32(0)
        else:
            good = np.float32(good + np.float32(1))
    else:
        scale = np.float32(max(np.float32(scale / mult), np.float32(1)))
        good = np.float32(0)
    return scale, good


def _follow(ops, scale, flags, period=3, mult=2.0):
    """Run the flag sequence; after every call the device state equals the restatement's, the flag
    is re-armed and ls[3] is as it was.  Returns the (scale, good) trace."""
    ls = _ls_state(scale, 0.0, 1.0)
    sc, good = np.float32(scale), np.float32(0)
    trace = []
    for i, flag in enumerate(flags):
        ls[2] = float(flag)
        ops.loss_scale_update(ls, period=period, multiplier=mult)
        sc, good = _keras_dynamic_loss_scale(sc, good, bool(flag), period, mult)
        got = _np(ls)
        want = np.array([sc, good, 1.0, SENT], np.float32)
        assert np.array_equal(_bits(got), _bits(want)), f"call {i} (flag {flag}): got {got} want {want}"
        trace.append((float(sc), float(good)))
    return trace


@gpu
def test_loss_scale_grows_after_period_good_steps_and_halves_on_a_bad_one():
    from dgan import ops
    tr = _follow(ops, 8.0, [1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 0])
    assert tr[:3] == [(8.0, 1.0), (8.0, 2.0), (16.0, 0.0)]          # exactly `period` good steps
    assert tr[3:6] == [(16.0, 1.0), (16.0, 2.0), (8.0, 0.0)]         # a bad step halves and zeroes `good`
    assert tr[6:9] == [(8.0, 1.0), (8.0, 2.0), (16.0, 0.0)]
    assert tr[9:] == [(8.0, 0.0), (4.0, 0.0)]


@gpu
def test_loss_scale_stops_at_one():
    from dgan import ops
    tr = _follow(ops, 4.0, [0, 0, 0, 0, 0, 1, 0])
    assert [s for s, _ in tr] == [2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]


@gpu
def test_loss_scale_growth_guard_at_the_top_of_the_range():
    from dgan import ops
    tr = _follow(ops, 2.0 ** 127, [1, 1, 1, 1, 0])
    assert tr == [(2.0 ** 127, 1.0), (2.0 ** 127, 2.0), (2.0 ** 127, 0.0), (2.0 ** 127, 1.0), (2.0 ** 126, 0.0)]


@gpu
def test_loss_scale_multiplier_one_and_a_half():
    from dgan import ops
    tr = _follow(ops, 1000.0, [1, 1, 1, 0, 0, 1, 1, 1] + [0] * 20, mult=1.5)
    assert tr[2] == (1500.0, 0.0) and tr[3] == (1000.0, 0.0)
    assert tr[-1] == (1.0, 0.0)


@gpu
@pytest.mark.parametrize("period,mult", [(0, 2.0), (-1, 2.0), (3, 1.0), (3, 0.5)])
def test_loss_scale_update_rejects_bad_arguments(period, mult):
    from dgan import ops
    from dgan._lib import DGError
    ls = _ls_state(8.0, 0.0, 1.0)
    ls0 = ls.clone()
    with pytest.raises(DGError):
        ops.loss_scale_update(ls, period=period, multiplier=mult)
    torch.cuda.synchronize()
    _same_bits(ls, ls0, "loss-scale state")


# -------------------------------------------------------------------------
# 5. check_finite
# -------------------------------------------------------------------------
CF_GRID_CAP = 2048   # dg_check_finite caps its grid at 2048 blocks of 256 lanes


@gpu
def test_check_finite_finds_a_lone_bad_value_anywhere():
    """More than one round of the capped grid plus a ragged end; one bad value in the first
    round's first / last lane, the second round's first lane, or the last element."""
    from dgan import ops
    lanes = CF_GRID_CAP * 256
    n = 2 * lanes + 77
    rng = np.random.default_rng(150)
    g = _dev(rng.standard_normal(n))
    ls0 = _ls_state(1024.0, 2.0, 1.0)
    ls = ls0.clone()
    ops.check_finite(g, ls)
    torch.cuda.synchronize()
    _same_bits(ls, ls0, "finite input")
    cleared = ls0.clone()
    cleared[2] = 0.0
    for idx in (0, lanes - 1, lanes, n - 1):
        for bad in (float("nan"), float("inf"), float("-inf")):
            keep = float(g[idx])
            g[idx] = bad
            ls = ls0.clone()
            ops.check_finite(g, ls)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(ls), _bits(cleared)), f"{bad} at {idx}: state {_np(ls)}"
            g[idx] = keep
    ls = ls0.clone()
    ops.check_finite(g, ls)                       # restored: finite again
    torch.cuda.synchronize()
    _same_bits(ls, ls0, "restored input")


@gpu
def test_check_finite_keeps_the_flag_on_finite_extremes():
    from dgan import ops
    lanes = CF_GRID_CAP * 256
    n = 2 * lanes + 77
    rng = np.random.default_rng(151)
    g = rng.standard_normal(n).astype(np.float32)
    fmax = np.finfo(np.float32).max
    extremes = np.array([fmax, -fmax, 1e-45, -1e-45, 1e-39, np.finfo(np.float32).tiny, -0.0, 0.0], np.float32)
    for at in (0, lanes - 4, lanes, n - extremes.size):
        g[at:at + extremes.size] = extremes
    gd = _dev(g)
    ls0 = _ls_state(1024.0, 2.0, 1.0)
    ls = ls0.clone()
    ops.check_finite(gd, ls)
    torch.cuda.synchronize()
    _same_bits(ls, ls0, "finite extremes")
    ls = ls0.clone()
    ls[2] = 0.0                                   # an earlier arena already cleared the flag
    was = ls.clone()
    ops.check_finite(gd, ls)
    torch.cuda.synchronize()
    _same_bits(ls, was, "cleared flag stays cleared")


@gpu
def test_check_finite_one_and_no_element():
    from dgan import ops
    ls0 = _ls_state(4.0, 1.0, 1.0)
    for value, flag in ((0.5, 1.0), (float("inf"), 0.0), (float("nan"), 0.0)):
        ls = ls0.clone()
        ops.check_finite(torch.tensor([value], dtype=torch.float32, device=DEV), ls)
        torch.cuda.synchronize()
        want = ls0.clone()
        want[2] = flag
        _same_bits(ls, want, f"n=1 value {value}")
    for flag in (1.0, 0.0):
        ls = ls0.clone()
        ls[2] = flag
        was = ls.clone()
        ops.check_finite(torch.empty(0, dtype=torch.float32, device=DEV), ls)
        torch.cuda.synchronize()
        _same_bits(ls, was, "n=0")


# -------------------------------------------------------------------------
# 6. scale_by
# -------------------------------------------------------------------------
@gpu
def test_scale_by_is_one_fp32_multiplication():
    from dgan import ops
    from dgan._lib import DGError
    n = 8192 * 256 + 333      # past the 8192-block grid, ragged
    rng = np.random.default_rng(160)
    x = (rng.standard_normal(n) * np.exp(rng.uniform(-10, 10, n))).astype(np.float32)
    buf, xd = _tail_view(n)
    xd.copy_(torch.from_numpy(x))
    ls = _ls_state(3.7, 5.0, 1.0)
    ls0 = ls.clone()
    ops.scale_by(xd, ls)
    torch.cuda.synchronize()
    _same_bits(xd, x * _np(ls0)[0], "scale_by")      # one multiplication is correctly rounded
    _tail_ok(buf, n, "scale_by")
    _same_bits(ls, ls0, "loss-scale state")
    with pytest.raises(DGError):
        ops.scale_by(xd[::2], ls)


# -------------------------------------------------------------------------
# 7. fill, channel_concat, accumulate, act_bwd
# -------------------------------------------------------------------------
@gpu
def test_fill():
    from dgan import ops
    n = 8192 * 256 + 5
    buf, t = _tail_view(n, fill=-3.0)
    ops.fill(t, 1.5)
    torch.cuda.synchronize()
    assert bool((t == 1.5).all())
    _tail_ok(buf, n, "fill")


@gpu
@pytest.mark.parametrize("ca,cb", [(3, 3), (1, 5), (64, 67)])
def test_channel_concat_on_padded_buffers(ca, cb):
    from dgan import ops
    npix = 777
    rng = np.random.default_rng(170 + ca)
    abuf, a = _padded2(npix, ca, ca + 2, off=1)
    bbuf, b = _padded2(npix, cb, cb + 3)
    obuf, out = _padded2(npix, ca + cb, ca + cb + 5, off=2)
    a.copy_(_dev(rng.standard_normal((npix, ca))))
    b.copy_(_dev(rng.standard_normal((npix, cb))))
    a0, b0 = abuf.clone(), bbuf.clone()
    ops.channel_concat(a, b, out)
    torch.cuda.synchronize()
    assert torch.equal(out, torch.cat([a, b], dim=1))
    _pad_ok(obuf, ca + cb, off=2, what="concat out")
    assert torch.equal(abuf, a0) and torch.equal(bbuf, b0)


def _layout(kind, rng):
    """(src, dst buffer, dst view) of the float4-eligible dense layout (C = 8) or of the padded
    one (C = 3 in NHWC buffers with pixel stride 7)."""
    if kind == "dense8":
        shape, ld = (300, 8), 8
    else:
        shape, ld = (2, 5, 7, 3), 7
    C = shape[-1]
    sbuf = torch.full(shape[:-1] + (ld,), SENT, dtype=torch.float32, device=DEV)
    dbuf = sbuf.clone()
    src, dst = sbuf[..., :C], dbuf[..., :C]
    src.copy_(_dev(rng.standard_normal(shape)))
    return src, dbuf, dst, C


@gpu
@pytest.mark.parametrize("kind", ["dense8", "padded3"])
@pytest.mark.parametrize("beta", [0.0, 1.0, 0.5])
def test_accumulate(kind, beta):
    """dst = src + beta * dst; beta 0 overwrites, as every `beta` output of the library does
    (k_accumulate does not read dst then): a dst of nan must come out finite."""
    from dgan import ops
    rng = np.random.default_rng(171)
    src, dbuf, dst, C = _layout(kind, rng)
    if beta == 0.0:
        dst.fill_(float("nan"))
        ref = src.double().cpu()
    else:
        dst.copy_(_dev(rng.standard_normal(tuple(dst.shape))))
        ref = src.double().cpu() + beta * dst.double().cpu()
    src0 = src.clone()
    ops.accumulate(src, dst, beta=beta)
    torch.cuda.synchronize()
    _close(dst, ref, 1e-6, what=f"accumulate beta={beta}")
    if dbuf.shape[-1] > C:
        _pad_ok(dbuf, C, what="accumulate dst")
    assert torch.equal(src, src0)


ACTS = {"none": lambda x: x, "linear": lambda x: x, None: lambda x: x, "lrelu": lambda x: S.lrelu(x, 0.3),
        "leaky_relu": lambda x: S.lrelu(x, 0.3), "relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}


@gpu
@pytest.mark.parametrize("kind", ["dense8", "padded3"])
@pytest.mark.parametrize("act", list(ACTS))
def test_act_bwd(kind, act):
    """dy = dz * act'(z), the derivative taken from the activation's OUTPUT z (include/dgan.h):
    torch fp64 autograd of z = act(x), the kernel given z.  Exact zeros of z included (ReLU /
    LeakyReLU: gradient 0 / alpha at 0; tanh at x = 0; sigmoid underflowed to 0)."""
    from dgan import ops
    rng = np.random.default_rng(172)
    zsrc, dybuf, dy, C = _layout(kind, rng)
    x = rng.standard_normal(tuple(zsrc.shape)) * 2
    flat = x.reshape(-1)
    flat[[0, 5, flat.size - 1]] = -1000.0 if act == "sigmoid" else 0.0
    dz = rng.standard_normal(x.shape)
    xt = torch.tensor(x, requires_grad=True)
    zt = ACTS[act](xt)
    ref = torch.autograd.grad(zt, xt, torch.tensor(dz))[0]
    assert int((zt == 0).sum()) >= 3
    zsrc.copy_(_dev(zt.detach().numpy()))
    dzd = _dev(dz)
    ops.act_bwd(dzd, zsrc, dy, act, alpha=0.3)
    torch.cuda.synchronize()
    _close(dy, ref, 1e-6, what=f"act_bwd {act}")
    if dybuf.shape[-1] > C:
        _pad_ok(dybuf, C, what="act_bwd dy")


# -------------------------------------------------------------------------
# 8. to_f16
# -------------------------------------------------------------------------
@gpu
def test_to_f16_rounds_to_nearest_even():
    from dgan import ops
    from dgan._lib import DGError
    n = 8 * 1031
    rng = np.random.default_rng(180)
    x = (rng.standard_normal(n) * np.exp(rng.uniform(-20, 12, n))).astype(np.float32)   # subnormal .. overflow
    e = 2.0 ** -11     # half an fp16 ulp at 1
    special = np.array([
        # ties at 1 and their neighbours
        1 + e, 1 + 3 * e, -(1 + e), -(1 + 3 * e), 1 + e + 2.0 ** -23, 1 + e - 2.0 ** -24,
        65504.0, -65504.0, 65519.9, 65520.0, -65519.9, -65520.0, 0.0, -0.0, np.inf, -np.inf,
        # rounding into the fp16 subnormals, inside them (ties to even, to zero), an fp32 subnormal
        2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -14 - 2.0 ** -26,
        2.0 ** -24, 2.0 ** -25, -(2.0 ** -25), 3 * 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 2.0 ** -26, 1e-30, -1e-30,
        5 * 2.0 ** -25, 1023.5 * 2.0 ** -24, 1e-40,
    ], np.float64).astype(np.float32)
    assert special[0] == np.float32(1 + e)      # the ties are fp32 numbers
    x[3:3 + special.size] = special
    x[n - special.size:] = special[::-1]
    x[1000] = np.nan
    src = _dev(x)
    buf, dst = _tail_view(n, dtype=torch.float16)
    ops.to_f16(src, dst)
    torch.cuda.synchronize()
    want = torch.from_numpy(x).half().numpy()
    got = _np(dst)
    assert np.isnan(got[1000]) and np.isnan(want[1000])
    fin = np.ones(n, bool)
    fin[1000] = False
    bad = np.flatnonzero(_bits(got)[fin] != _bits(want)[fin])
    assert bad.size == 0, (f"{bad.size} differ; first: x={x[fin][bad[0]]!r} got {got[fin][bad[0]]!r} "
                           f"want {want[fin][bad[0]]!r}")
    _tail_ok(buf, n, "to_f16")
    _same_bits(src, x, "to_f16 src")
    with pytest.raises(DGError):
        ops.to_f16(torch.zeros(12, device=DEV), torch.zeros(12, dtype=torch.float16, device=DEV))


# -------------------------------------------------------------------------
# 9. weight_bound_in
# -------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", [(3, 3, 5, 7), (1, 1, 64, 3), (3, 3, 67, 64)], ids=lambda s: "x".join(map(str, s)))
def test_weight_bound_in(shape):
    """max over input channels of sum |w| over taps and output channels, into one float of a
    per-conv vector (the graph executor's gwb[i:i+1]) whose stale value must not survive."""
    from dgan import ops
    rng = np.random.default_rng(190 + shape[2])
    w = (rng.standard_normal(shape) * 0.05).astype(np.float32)
    w[..., shape[2] // 2, :] *= 3.0                 # the maximum sits at an inner input channel
    gwb = torch.tensor([SENT, 1e9, SENT], dtype=torch.float32, device=DEV)
    ops.weight_bound_in(_dev(w), gwb[1:2])
    torch.cuda.synchronize()
    ref = np.abs(w.astype(np.float64)).sum(axis=(0, 1, 3)).max()
    got = _np(gwb)
    assert got[0] == SENT and got[2] == SENT
    assert abs(float(got[1]) - ref) <= 1e-6 * ref, (got[1], ref)
