"""dg_p2p_loss (csrc/loss.hip) called directly: the eight loss values and the five gradients
against oracle.p2p_oracle.losses_and_grads, at shapes the pix2pix step never has.

Images are integer multiples of 1/256 in [-1, 1]: every difference the kernel forms (target -
gen, its row and column differences, ident - target) is then exact in fp32, so kernel and fp64
oracle take the same sign decisions by construction and exact ties (sign(0) = 0 in the L1, TV
and identity gradients) occur and are forced.  H = 1 / W = 1 reach the TV edge branches, C != 3
and channel slices of wider buffers the stride handling, 64 * 256 + 5 logits the second round of
the logit grid, and +-40 / +-100 the saturated BCE.

Tolerances as test_gan_loss_set_matches_oracle and
test_generator_and_discriminator_loss_match_oracle: the eight values rtol 2e-6 / atol 1e-8;
dgen and dident 1e-5 of their scale; logit gradients 1e-6 of their scale; a second call on the
same inputs returns the same bits (fixed grid, ordered final sum).
"""
import numpy as np
import pytest
import torch

from oracle import p2p_oracle as O

gpu = pytest.mark.gpu
DEV = "cuda"
SENT = 777.0

# gan, l1, l2, tv, identity, content (ops.p2p_loss order); dyadic, so fp32 holds them exactly
WEIGHTS = (0.75, 1.25, 0.5, 2.0 ** -9, 0.875, 1.5)
W_ORACLE = dict(zip(("gan", "l1", "l2", "tv", "identity", "content"), WEIGHTS))
CONTENT = 0.25
SHAPES = [(1, 1, 1, 1), (2, 1, 7, 3), (2, 6, 1, 3), (3, 5, 7, 4), (2, 9, 11, 3)]
GRADS = ("dgen", "dident", "dlogit_real_d", "dlogit_fake_d", "dlogit_fake_g")
ORACLE_NAME = dict(dgen="dgen", dident="dident", dlogit_real_d="dzr_d", dlogit_fake_d="dzf_d", dlogit_fake_g="dzf_g")


def _close(got, ref, rtol, atol=0.0, what=""):
    """max |got - ref| <= atol + rtol * max |ref| (tests/test_sr_gpu.py _close)."""
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite"
    err = np.abs(got - ref).max()
    scale = np.abs(ref).max()
    assert err <= atol + rtol * scale, f"{what}: max abs err {err:.3e} vs scale {scale:.3e}"


def _images(rng, shape):
    """gen, tgt, ident on the 1/256 grid, with forced ties."""
    B, H, W, C = shape
    gen, tgt, ident = (rng.integers(-256, 257, shape).astype(np.float64) / 256 for _ in range(3))
    if B * H * W >= 4:
        gen.reshape(-1, C)[1] = tgt.reshape(-1, C)[1]          # d = 0: sign(0) in the L1 gradient
        ident.reshape(-1, C)[2] = tgt.reshape(-1, C)[2]        # identity tie
    if W > 1:
        gen[B - 1, H - 1] = tgt[B - 1, H - 1] - 0.25           # a row of constant d: horizontal TV ties
    if H > 1:
        gen[0, 0:2] = tgt[0, 0:2] - 0.5                        # two such rows: vertical ties as well
    return gen, tgt, ident


def _logits(rng, n):
    z = (rng.standard_normal((2, n)) * 3).astype(np.float32)
    sat = np.array([40.0, -40.0, 100.0, -100.0], np.float32)
    k = min(4, n)
    z[0, :k], z[1, n - k:] = sat[:k], sat[:k][::-1]
    z[0, n - 1], z[1, 0] = 0.0, 0.0
    return z[0].copy(), z[1].copy()


def _slice_of(shape, ld, off, values=None):
    """([B,H,W,ld] buffer of SENT, its channel slice [off, off+C)), the slice holding `values`."""
    B, H, W, C = shape
    buf = torch.full((B, H, W, ld), SENT, dtype=torch.float32, device=DEV)
    view = buf[..., off:off + C]
    if values is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(values, np.float32)).to(DEV))
    return buf, view


def _pad_ok(buf, C, off, what):
    keep = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
    keep[off:off + C] = False
    assert bool((buf[..., keep] == SENT).all()), f"{what}: padding columns written"


class _Case:
    """Inputs on the device, dense or as channel slices of wider buffers, and the oracle's answer."""

    def __init__(self, shape, nlog, seed, strided):
        B, H, W, C = self.shape = shape
        rng = np.random.default_rng(seed)
        self.gen, self.tgt, self.ident = _images(rng, shape)
        self.zr, self.zf = _logits(rng, nlog)
        # the trainer's layout: gen is the second half of the 2C-wide D(fake) input [x | G(x)]
        lay = dict(gen=(2 * C, C), tgt=(C + 3, 1), ident=(C + 5, 2), dgen=(2 * C + 1, C), dident=(C + 2, 1))
        if not strided:
            lay = {k: (C, 0) for k in lay}
        self.lay = lay
        self.buf, self.view = {}, {}
        for k, vals in (("gen", self.gen), ("tgt", self.tgt), ("ident", self.ident), ("dgen", None), ("dident", None)):
            self.buf[k], self.view[k] = _slice_of(shape, *lay[k], values=vals)
        self.inputs0 = {k: self.buf[k].clone() for k in ("gen", "tgt", "ident")}
        self.zrd, self.zfd = (torch.from_numpy(z).to(DEV) for z in (self.zr, self.zf))
        self.content = torch.tensor([CONTENT], dtype=torch.float32, device=DEV)

    def oracle(self, ident=True, content=True):
        return O.losses_and_grads(self.gen, self.tgt, self.ident if ident else None, self.zr.astype(np.float64),
                                  self.zf.astype(np.float64), w=W_ORACLE, content=CONTENT if content else 0.0)

    def run(self, ident=True, content=True, absent=()):
        """One call; returns (out[8], {gradient name: tensor or None}), out sitting between sentinels."""
        from dgan import ops
        C = self.shape[-1]
        for k in ("dgen", "dident"):
            self.view[k].fill_(-5.0)
        obuf = torch.full((12,), SENT, dtype=torch.float32, device=DEV)
        out = obuf[2:10]
        g = dict(dgen=self.view["dgen"], dident=self.view["dident"] if ident else None)
        for k in GRADS[2:]:
            g[k] = torch.full((self.zr.size + 4,), SENT, dtype=torch.float32, device=DEV)
        for k in absent:
            g[k] = None
        ops.p2p_loss(self.view["gen"], self.view["tgt"], self.zrd, self.zfd, out,
                     ident=self.view["ident"] if ident else None, weights=WEIGHTS,
                     content=self.content if content else None,
                     **{k: (None if t is None else t[:self.zr.size] if k in GRADS[2:] else t) for k, t in g.items()})
        torch.cuda.synchronize()
        assert bool((obuf[:2] == SENT).all()) and bool((obuf[10:] == SENT).all()), "wrote around out[8]"
        for k in ("gen", "tgt", "ident"):
            assert torch.equal(self.buf[k], self.inputs0[k]), f"input {k} changed"
        for k in ("dgen", "dident"):
            _pad_ok(self.buf[k], C, self.lay[k][1], k)
        res = {}
        for k, t in g.items():
            if t is not None and k in GRADS[2:]:
                assert bool((t[self.zr.size:] == SENT).all()), f"{k}: wrote past the end"
                t = t[:self.zr.size]
            res[k] = None if t is None else t.clone()
        return out.clone(), res


def _check(case, out, grads, ident=True, content=True):
    vals, ref = case.oracle(ident=ident, content=content)
    got = out.double().cpu().numpy()
    print("values", got.tolist())
    assert np.isfinite(got).all(), got
    assert np.allclose(got, np.array(vals), rtol=2e-6, atol=1e-8), (got, vals)
    for k, t in grads.items():
        if t is None:
            continue
        r = ref[ORACLE_NAME[k]]
        if k in ("dgen", "dident"):
            _close(t, r, 1e-5, what=k)
        else:
            _close(t, r.reshape(-1), 1e-6, what=k)


@gpu
@pytest.mark.parametrize("shape,nlog", list(zip(SHAPES, (17, 64 * 256 + 5, 17, 64 * 256 + 5, 17))),
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_p2p_loss_on_channel_slices_matches_oracle(shape, nlog):
    """Every tensor a channel slice of a wider buffer (gen the second half of a 2C-wide one, as
    the trainer lays it out); a second call gives the same bits; dense buffers give them too."""
    case = _Case(shape, nlog, seed=200 + 10 * shape[1] + shape[2], strided=True)
    out, grads = case.run()
    _check(case, out, grads)
    out2, grads2 = case.run()
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    for k in GRADS:
        assert torch.equal(grads[k].view(torch.int32), grads2[k].view(torch.int32)), k
    dense = _Case(shape, nlog, seed=200 + 10 * shape[1] + shape[2], strided=False)
    out3, grads3 = dense.run()
    assert torch.equal(out.view(torch.int32), out3.view(torch.int32))
    for k in GRADS:
        assert torch.equal(grads[k].contiguous().view(torch.int32), grads3[k].contiguous().view(torch.int32)), k


@gpu
def test_p2p_loss_without_identity_and_without_content():
    case = _Case((3, 5, 7, 4), 17, seed=260, strided=True)
    full, gfull = case.run()
    _check(case, full, gfull)
    out, grads = case.run(ident=False)
    assert float(out[7]) == 0.0 and grads["dident"] is None
    _check(case, out, grads, ident=False)
    assert bool((case.view["dident"] == -5.0).all()), "dident written without ident"
    out, grads = case.run(content=False)
    assert float(out[4]) == 0.0
    assert float(full[4]) == WEIGHTS[5] * CONTENT
    _check(case, out, grads, content=False)
    for k in GRADS:                                     # the content term has no gradient here
        assert torch.equal(grads[k].view(torch.int32), gfull[k].view(torch.int32)), k


@gpu
@pytest.mark.parametrize("absent", GRADS)
def test_p2p_loss_each_gradient_output_is_optional(absent):
    """Leaving one gradient out changes nothing else: the values and the other four keep their bits."""
    case = _Case((3, 5, 7, 4), 64 * 256 + 5, seed=270, strided=True)
    full, gfull = case.run()
    _check(case, full, gfull)
    out, grads = case.run(absent=(absent,))
    assert grads[absent] is None
    if absent in ("dgen", "dident"):
        assert bool((case.view[absent] == -5.0).all()), f"{absent} written though absent"
    assert torch.equal(out.view(torch.int32), full.view(torch.int32))
    for k in GRADS:
        if k != absent:
            assert torch.equal(grads[k].contiguous().view(torch.int32), gfull[k].contiguous().view(torch.int32)), k
