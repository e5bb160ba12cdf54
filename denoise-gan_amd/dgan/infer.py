"""Image inference with the pix2pix generator (the reference's infer.py:40-68 and
infer_video.py:138-159): a U-Net whose BatchNorms are folded into the conv weights, and a
`Denoiser` that pads or tiles uint8 images of any size around it.

At inference BatchNorm is `y * s + (beta - mean * s)` with `s = gamma / sqrt(var + eps)`
constant, so it folds exactly into the preceding conv's kernel and bias (dg_bn_fold).  The
folded network is 16 conv calls -- bias and activation in the conv epilogue, each output written
straight into its concat buffer -- and no BN kernel.  The folded kernels change only in
`refold()`, so their operand planes are kept across forwards like a frozen network's
(`FoldedArena.frozen` / `.version`, PlaneBuf.stamp: dgan/graph.py).

The geometry and the numpy reference implementations of the uint8 staging (`tile_geometry`,
`stage_ref`, `unstage_ref`) are pure Python: the tests and the `Denoiser` share them.
"""
from collections import namedtuple

import numpy as np

PADS = ("black", "reflect")
MODEL_MULTIPLE = 256   # 8 stride-2 blocks (dgan/nets.py GeneratorPlan)

# Tile (i, j) row ty reads image row oy + i*Sh + ty; output pixel y comes from tile
# i = clamp((y - oy - mt) // Sh, 0, gi - 1), tile row y - (oy + i*Sh): the tile whose interior
# rows [mt, mt + Sh) hold it (columns alike, include/dgan.h dg_u8_stage / dg_u8_unstage).
TileGeometry = namedtuple("TileGeometry", "h w Th Tw Sh Sw oy ox gi gj mt ml")


def _up(v, m):
    return -(-v // m) * m


def tile_geometry(h, w, tile=None, margin=0):
    """Whole-image mode (tile None): one tile per image, (h, w) rounded up to a multiple of 256
    and centred (infer_video.py:140 resize_with_crop_or_pad; an exact multiple gets no extra
    256, unlike the reference).  Tile mode: T x T tiles whose interiors of S = T - 2*margin
    cover the image, ceil(h/S) x ceil(w/S) of them, the first starting `margin` outside it."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"empty image {h}x{w}")
    if tile is None:
        if margin:
            raise ValueError("margin applies to tile mode only")
        Th, Tw = _up(h, MODEL_MULTIPLE), _up(w, MODEL_MULTIPLE)
        return TileGeometry(h, w, Th, Tw, Th, Tw, -((Th - h) // 2), -((Tw - w) // 2), 1, 1, 0, 0)
    T, margin = int(tile), int(margin)
    if T < MODEL_MULTIPLE or T % MODEL_MULTIPLE:
        raise ValueError(f"tile must be a multiple of {MODEL_MULTIPLE}, got {T}")
    if not 0 <= margin < T / 2:
        raise ValueError(f"margin must satisfy 0 <= margin < tile/2, got {margin}")
    S = T - 2 * margin
    return TileGeometry(h, w, T, T, S, S, -margin, -margin, -(-h // S), -(-w // S), margin, margin)


def pad_index(r, size, pad):
    """Source indices of image coordinates r (any integers) along an axis of `size`: r itself
    inside; outside -1 for "black", and for "reflect" j = r mod p, j >= size ? p - j : j with
    p = 2 (size - 1) (0 when size == 1) -- np.pad(mode="reflect") for any pad width."""
    if pad not in PADS:
        raise ValueError(f"pad must be one of {PADS}, got {pad!r}")
    r = np.asarray(r, dtype=np.int64)
    inside = (r >= 0) & (r < size)
    if pad == "black":
        return np.where(inside, r, -1)
    if size == 1:
        return np.zeros_like(r)
    p = 2 * (size - 1)
    j = np.mod(r, p)
    return np.where(inside, r, np.where(j >= size, p - j, j))


def tile_rows(g, axis):
    """[tiles, T] image coordinates read by each tile along axis 0 (rows) or 1 (columns)."""
    T, S, o, n = (g.Th, g.Sh, g.oy, g.gi) if axis == 0 else (g.Tw, g.Sw, g.ox, g.gj)
    return o + np.arange(n)[:, None] * S + np.arange(T)[None, :]


def source_tile(g, axis):
    """(tile index, tile coordinate) of every output coordinate along an axis."""
    size, S, o, n, m = (g.h, g.Sh, g.oy, g.gi, g.mt) if axis == 0 else (g.w, g.Sw, g.ox, g.gj, g.ml)
    y = np.arange(size)
    i = np.clip((y - o - m) // S, 0, n - 1)
    return i, y - (o + i * S)


def u8_to_unit(u8):
    """infer_video.py:139-143 in fp32: convert_image_dtype (u8 * (1/255)), then * 2 - 1."""
    return (u8.astype(np.float32) * np.float32(1.0 / 255.0)) * np.float32(2.0) - np.float32(1.0)


def unit_to_u8(v):
    """infer_video.py:149-159 in fp32: clip(v * 0.5 + 0.5, 0, 1) * 255, NaN -> 0 -- rounded to
    nearest (+ 0.5, floor) where the reference truncates: u8_to_unit rounds a*2 - 1 at the spacing
    of 1.0, and truncation would then return 47 of the 256 byte values one level darker."""
    v = np.asarray(v, np.float32)
    t = v * np.float32(0.5) + np.float32(0.5)
    t = np.where(np.isnan(t), np.float32(0.0), np.clip(t, np.float32(0.0), np.float32(1.0))).astype(np.float32)
    return np.floor(t * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)


def stage_ref(u8, g, pad="black"):
    """numpy dg_u8_stage: uint8 [n,h,w,3] -> fp32 tiles [n*gi*gj,Th,Tw,3]."""
    u8 = np.asarray(u8)
    n = u8.shape[0]
    assert u8.dtype == np.uint8 and u8.shape[1:] == (g.h, g.w, 3), u8.shape
    ri, ci = pad_index(tile_rows(g, 0), g.h, pad), pad_index(tile_rows(g, 1), g.w, pad)   # [gi,Th], [gj,Tw]
    unit = u8_to_unit(u8)
    t = unit[:, np.maximum(ri, 0)[:, None, :, None], np.maximum(ci, 0)[None, :, None, :], :]  # [n,gi,gj,Th,Tw,3]
    outside = (ri < 0)[:, None, :, None] | (ci < 0)[None, :, None, :]
    t = np.where(outside[None, ..., None], np.float32(-1.0), t)
    return np.ascontiguousarray(t.reshape(n * g.gi * g.gj, g.Th, g.Tw, 3), dtype=np.float32)


def unstage_ref(tiles, g):
    """numpy dg_u8_unstage: fp32 tiles [n*gi*gj,Th,Tw,3] -> uint8 [n,h,w,3]."""
    tiles = np.asarray(tiles, np.float32)
    n = tiles.shape[0] // (g.gi * g.gj)
    t = tiles.reshape(n, g.gi, g.gj, g.Th, g.Tw, 3)
    i, ty = source_tile(g, 0)
    j, tx = source_tile(g, 1)
    return unit_to_u8(t[:, i[:, None], j[None, :], ty[:, None], tx[None, :], :])


# ---------------------------------------------------------------------------
# the folded U-Net (device code below: torch and the library are imported on use, so the
# geometry above needs neither)
# ---------------------------------------------------------------------------
class FoldedArena:
    """Every layer's folded kernel at the generator arena's offsets, plus one bias per layer.
    `frozen` / `version` / `wplanes`: the frozen-network protocol of dgan/graph.py -- weight
    planes split from version v are reused until the version changes."""
    frozen = True

    def __init__(self, arena, layers):
        import torch
        self.offsets, self.shapes, self.device = arena.offsets, arena.shapes, arena.device
        self.data = torch.zeros(arena.numel, dtype=torch.float32, device=arena.device)
        self.bias_off = {}
        off = 0
        for name, co in layers:
            self.bias_off[name] = (off, co)
            off += _up(co, arena.ALIGN)
        self.bias_data = torch.zeros(off, dtype=torch.float32, device=arena.device)
        self.version = 0
        self.wplanes = {}

    def param(self, name):
        o, shape = self.offsets[name], self.shapes[name]
        return self.data[o:o + int(np.prod(shape))].view(shape)

    def bias(self, layer):
        o, co = self.bias_off[layer]
        return self.bias_data[o:o + co]


class FoldedGenerator:
    """The generator's inference network with every BatchNorm folded into its conv."""

    def __init__(self, generator):
        from .nets import g_layer_specs
        self.generator = generator
        self.width, self.device = generator.width, generator.device
        self.downs, self.ups, self.last = g_layer_specs(generator.width)
        # (layer, transpose, Cout, has BN) in forward order
        self.layers = ([(n, False, co, bn) for n, _, co, bn in self.downs] + [(n, True, co, True) for n, _, co, _ in self.ups]
                       + [(self.last[0], True, self.last[2], False)])
        self.arena = FoldedArena(generator.arena, [(n, co) for n, _, co, _ in self.layers if n != "down1"])
        self._plans = {}
        self.refold()

    def refold(self):
        """Fold the generator's current weights and moving statistics: 14 dg_bn_fold calls, the two
        layers without BN copied; kept weight planes are split again by the next forward."""
        from . import ops
        from .nets import BN_EPS
        G, A = self.generator, self.arena
        for name, transpose, co, bn in self.layers:
            w = G.arena.param(f"{name}/kernel")
            if bn:
                ops.bn_fold(w, G.arena.param(f"{name}/gamma"), G.arena.param(f"{name}/beta"), G.bn.mean[name],
                            G.bn.var[name], A.param(f"{name}/kernel"), A.bias(name), transpose=transpose, eps=BN_EPS)
            else:
                A.param(f"{name}/kernel").copy_(w)
        A.bias("last").copy_(G.arena.param("last/bias"))
        A.version += 1

    def max_abs_weight(self):
        """max |folded weight| (synchronises).  The fp16x3 GEMMs scale weight planes by a static
        2^8 (include/dgan.h DG_MATH_F16X3), which holds |w| < 255."""
        return float(self.arena.data.abs().max().item())

    def plan(self, N, H, W):
        key = (N, H, W)
        if key not in self._plans:
            self._plans[key] = FoldedPlan(self, N, H, W)
        return self._plans[key]

    def __call__(self, x, out=None):
        """x: fp32 NHWC device tensor, H and W multiples of 256 -> the tanh output (the plan's own
        buffer unless `out` is given)."""
        N, H, W, _ = x.shape
        return self.plan(N, H, W).forward(x, out)


class FoldedPlan:
    """The folded forward for one input shape: the concat buffers, z8, an output, a pre-sized
    workspace and the conv descriptors.  A forward allocates nothing and never synchronises."""

    def __init__(self, folded, N, H, W):
        import torch
        from . import ops
        from .nets import P2P_MATH
        from .ops import ConvDesc
        if H % MODEL_MULTIPLE or W % MODEL_MULTIPLE:
            raise ValueError(f"pix2pix generator needs H, W divisible by {MODEL_MULTIPLE}, got {H}x{W}")
        self.folded, self.N, self.H, self.W = folded, N, H, W
        dev = folded.device
        downs, ups, last = folded.downs, folded.ups, folded.last
        self.descs = []
        h, w = H, W
        for name, ci, co, _ in downs:
            d = ConvDesc(N, h, w, ci, co, 4, 2, "same", math=P2P_MATH)
            h, w = d.Ho, d.Wo
            self.descs.append(d)
        self.z8 = torch.empty((N, h, w, downs[7][2]), dtype=torch.float32, device=dev)
        self.cat = []
        for u, (name, ci, co) in enumerate([t[:3] for t in ups] + [last]):
            d = ConvDesc(N, h, w, ci, co, 4, 2, "same", transpose=True, math=P2P_MATH)
            h, w = d.Ho, d.Wo
            self.descs.append(d)
            if u < 7:
                self.cat.append(torch.empty((N, h, w, co + downs[6 - u][2]), dtype=torch.float32, device=dev))
        for d, (name, *_) in zip(self.descs, folded.layers):
            d.label = f"Gf.{name}"
        self.out = torch.empty(self.descs[-1].out_shape, dtype=torch.float32, device=dev)
        self.ws = ops.Workspace(dev)
        self.ws.get(max(d.ws[ops.OP_FWD] for d in self.descs))
        # weight planes: one buffer per layer and layout of the NETWORK, shared by its plans
        A = folded.arena
        self.planes = []
        for d, (name, *_) in zip(self.descs, folded.layers):
            P = None
            if d.plane_mask[ops.OP_FWD] & ops.TENSOR_W:
                lay = ops.weight_layout(d)
                key = (name,) + lay
                if key not in A.wplanes:
                    A.wplanes[key] = ops.PlaneBuf(lay[1], dev, lay[0])
                P = ops.ConvPlanes(w=A.wplanes[key])
            self.planes.append(P)

    def _current(self, P):
        """P's weight planes as of the arena's version (dgan/graph.py _stale_w)."""
        if P is not None and P.w.stamp != self.folded.arena.version:
            P.w.stamp = self.folded.arena.version
            P.w.ready = False
        return P

    def forward(self, x, out=None):
        from .nets import ALPHA
        F = self.folded
        A = F.arena
        out = self.out if out is None else out
        h = x
        for l, (name, ci, co, bn) in enumerate(F.downs):
            z = self.z8 if l == 7 else self.cat[6 - l][..., F.ups[6 - l][2]:]
            self.descs[l].fwd(h, A.param(f"{name}/kernel"), z, bias=A.bias(name) if bn else None, act="lrelu",
                              alpha=ALPHA, ws=self.ws, planes=self._current(self.planes[l]))
            h = z
        for u, (name, ci, co, _) in enumerate(F.ups):
            self.descs[8 + u].fwd(h, A.param(f"{name}/kernel"), self.cat[u][..., :co], bias=A.bias(name), act="relu",
                                  ws=self.ws, planes=self._current(self.planes[8 + u]))
            h = self.cat[u]
        self.descs[15].fwd(h, A.param("last/kernel"), out, bias=A.bias("last"), act="tanh", ws=self.ws,
                           planes=self._current(self.planes[15]))
        return out


def predict(generator, x, batch_size=None):
    """Keras `model.predict` (infer.py:60): numpy in, numpy out, on the folded path with the
    generator's current weights (refolded on every call)."""
    import torch
    from .models import to_device
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 4 or x.shape[-1] != 3:
        raise ValueError(f"predict expects [N,H,W,3], got {x.shape}")
    F = getattr(generator, "_folded", None)
    if F is None:
        F = generator._folded = FoldedGenerator(generator)
    else:
        F.refold()
    n = x.shape[0]
    bs = min(int(batch_size or 32), max(n, 1))
    out = np.empty(x.shape, np.float32)
    for i in range(0, n, bs):
        xb = to_device(x[i:i + bs], generator.device)
        out[i:i + bs] = F(xb).cpu().numpy()
    torch.cuda.synchronize(generator.device)
    return out


class _Frame:
    """Buffers of one (n, h, w): static uint8 input / output, the tile buffers (the last chunk
    filled up with idle tiles) and, with graph=True, the captured launch sequence."""
    __slots__ = ("g", "u8_in", "u8_out", "tin", "tout", "nt", "graph")


class Denoiser:
    """uint8 images of any size through the folded generator.

    tile None: whole-image mode (one padded tile per image); tile T: T x T tiles with `margin`
    pixels of context on each side, `batch` tiles per forward.  pad: "black" (the reference's zero
    pad) or "reflect".  graph: capture stage -> forward -> unstage once per (n, h, w)."""

    def __init__(self, generator, tile=None, margin=0, pad="black", batch=8, graph=False):
        if pad not in PADS:
            raise ValueError(f"pad must be one of {PADS}, got {pad!r}")
        if int(batch) < 1:
            raise ValueError("batch must be at least 1")
        tile_geometry(256, 256, tile, margin)   # (validates tile / margin)
        self.tile, self.margin, self.pad, self.batch, self.graph = tile, int(margin), pad, int(batch), bool(graph)
        self.folded = FoldedGenerator(generator)
        self.device = generator.device
        self._frames = {}

    def refresh(self):
        """Refold after the generator's weights or moving statistics changed.  The weight planes a
        captured graph reads are split again here, by one eager forward per captured plan."""
        self.folded.refold()
        for f in self._frames.values():
            if f.graph is not None:
                self._run(f)

    def _frame(self, n, h, w):
        import torch
        key = (n, h, w)
        if key in self._frames:
            return self._frames[key]
        f = _Frame()
        f.g = g = tile_geometry(h, w, self.tile, self.margin)
        f.nt = n * g.gi * g.gj
        B = self._chunk(f)
        dev = self.device
        f.u8_in = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
        f.u8_out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
        f.tin = torch.full((_up(f.nt, B), g.Th, g.Tw, 3), -1.0, dtype=torch.float32, device=dev)   # idle tiles: black
        f.tout = torch.empty_like(f.tin)
        f.graph = None
        self.folded.plan(B, g.Th, g.Tw)
        if self.graph:
            from .dist import CAPTURE_MODE
            s = torch.cuda.Stream(device=dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                self._run(f)   # (warm: the weight planes are split outside the capture)
            torch.cuda.current_stream(dev).wait_stream(s)
            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
                self._run(f)
            torch.cuda.synchronize(dev)
            f.graph = graph
        self._frames[key] = f
        return f

    def _chunk(self, f):
        """Tiles per forward: `batch` in tile mode (one plan for every image size), in whole-image
        mode at most the images there are (the plan is per padded size anyway)."""
        return self.batch if self.tile is not None else min(self.batch, f.nt)

    def _run(self, f):
        """stage -> forward per chunk -> unstage, all on the current stream."""
        from . import ops
        B = self._chunk(f)
        ops.u8_stage(f.u8_in, f.tin[:f.nt], f.g, self.pad)
        plan = self.folded.plan(B, f.g.Th, f.g.Tw)
        for t0 in range(0, f.tin.shape[0], B):
            plan.forward(f.tin[t0:t0 + B], f.tout[t0:t0 + B])
        ops.u8_unstage(f.tout[:f.nt], f.u8_out, f.g)

    def frame(self, n, h, w):
        """The buffers of n images of h x w (made, and with graph=True captured, on first use)."""
        return self._frame(n, h, w)

    def run_frame(self, f):
        """Denoise what the frame's `u8_in` holds into its `u8_out` on the current stream (a replay
        of the captured graph where there is one); returns the frame."""
        if f.graph is not None:
            f.graph.replay()
        else:
            self._run(f)
        return f

    def run(self, images):
        """Upload uint8 numpy images [n,h,w,3] (n >= 1) and denoise them on the current stream
        without reading anything back: the frame whose device buffers `u8_in` / `u8_out` hold the
        input and the result until the next call on the same shape (dgan/metrics.py Evaluator)."""
        import torch
        f = self._frame(*images.shape[:3])
        f.u8_in.copy_(torch.from_numpy(np.ascontiguousarray(images)))
        if f.graph is not None:
            f.graph.replay()
        else:
            self._run(f)
        return f

    def denoise(self, images):
        """uint8 [n,h,w,3] or [h,w,3] (numpy or torch) -> the same shape, uint8 numpy."""
        import torch
        a = images.cpu().numpy() if isinstance(images, torch.Tensor) else np.asarray(images)
        if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.shape[-1] != 3:
            raise ValueError(f"denoise expects uint8 [n,h,w,3] or [h,w,3], got {a.dtype} {a.shape}")
        single = a.ndim == 3
        if single:
            a = a[None]
        if a.shape[0] == 0:
            return a.copy()
        out = self.run(a).u8_out.cpu().numpy()
        return out[0] if single else out
