"""Inference with the SRGAN / FastSRGAN / autoencoder generators (the reference's
infer_video.py:73-159, whose default model is the FastSRGAN x4 generator): a graph rewrite that
folds every BatchNorm into the conv before it and fuses FastSRGAN's inverted-residual blocks into
one kernel each, a `FoldedNetwork` that runs the rewritten graph, and an `Upscaler` that takes
uint8 images of any size through it.

Rewrite rules (`fold_graph`):
  conv -> bn       one conv with a bias (also where the conv had none) carrying the BN's activation;
  dwconv -> bn     one dwconv carrying the BN's activation (dg_dwconv3_fwd_act);
  conv 1x1 + ReLU -> dwconv + ReLU -> conv 1x1 [-> add with the first conv's input]
                   one `mbconv` node (dg_mbconv_fwd) when the kernel takes the channel counts;
  everything else  unchanged.
A BN folds only when it is the conv's sole consumer and the conv has no activation of its own.

`fold_graph`, `fold_params_ref`, `mbconv_ref` and the geometry are pure Python and numpy: the CPU
tests and the device code share them, and none of them touches the library.

Tile margins that cover the receptive field, in low-resolution pixels, read off the graphs (each
3x3 layer before the upsamplers adds 1; after the first pixel shuffle a 3x3 adds 1/2, after the
second 1/4):
  FastSRGAN (6 blocks)   conv2d 1 + 6 depthwise convs 6 + conv2d_post 1 + deconv_0 1 + deconv_1 1/2
                         + conv2d_out 1/4 -> 10
  SRGAN (16 blocks)      conv2d 1 + 32 block convs 32 + conv2d_post 1 + deconv_0 1 + deconv_1 1/2
                         (conv2d_out is 1x1) -> 36
The autoencoder's five pools give it a receptive field of several hundred pixels: tile it with a
margin as large as the tile allows, or run whole images.
"""
import os

import numpy as np

from .graph import Graph
from .infer import PADS, TileGeometry, _up
from .ops import mbconv_supported as _mbconv_ok


def _is_none(act):
    return act in (None, "none", "linear")


# ---------------------------------------------------------------------------
# graph rewrite
# ---------------------------------------------------------------------------
def _layer_vars(graph):
    out = {}
    for name, shape, init in graph.vars:
        out.setdefault(name.rsplit("/", 1)[0], []).append((name, shape, init))
    return out


def _clone(dst, n, ins, lvars, recipe=None):
    """Node n of another graph, with its variables, onto dst."""
    for name, shape, init in lvars.get(n.name, ()):
        dst._var(name, shape, init)
        if recipe is not None:
            recipe[name] = {"op": "copy", "src": name}
    if n.kind == "bn":
        dst.bn_layers[n.name] = n.out.C
    return dst._node(n.kind, n.name, ins, n.out.C, **n.attrs)


def _fold(graph):
    """conv -> bn and dwconv -> bn become one node each; returns (graph, recipe)."""
    cons = graph.consumers()
    lvars = _layer_vars(graph)
    out = Graph(graph.name, in_ch=graph.input.C)
    tmap = {graph.input.id: out.input}
    recipe = {}
    done = set()
    for n in graph.nodes[1:]:
        if n.idx in done:
            continue
        ins = [tmap[t.id] for t in n.ins]
        cs = cons[n.out.id]
        b = cs[0] if len(cs) == 1 and cs[0].kind == "bn" else None
        if (n.kind in ("conv", "dwconv") and b is not None and n.out.id != graph.output.id
                and _is_none(n.attrs.get("act"))):
            kname = f"{n.name}/kernel" if n.kind == "conv" else f"{n.name}/depthwise_kernel"
            for name, shape, init in lvars[n.name]:
                if name == kname:
                    out._var(name, shape, init)
            out._var(f"{n.name}/bias", (n.out.C,), ("zeros",))
            eps = float(b.attrs["eps"])
            recipe[kname] = {"op": "scale", "src": kname, "bn": b.name, "eps": eps, "axis": 3 if n.kind == "conv" else 2}
            recipe[f"{n.name}/bias"] = {"op": "shift", "src": f"{n.name}/bias" if n.attrs["bias"] else None,
                                        "bn": b.name, "eps": eps}
            attrs = dict(n.attrs, bias=True, act=b.attrs["act"], alpha=b.attrs["alpha"])
            tmap[b.out.id] = out._node(n.kind, n.name, ins, n.out.C, **attrs)
            done.add(b.idx)
        else:
            tmap[n.out.id] = _clone(out, n, ins, lvars, recipe)
    out.set_output(tmap[graph.output.id])
    return out, recipe


def _fuse(graph):
    """conv 1x1 + ReLU -> dwconv + ReLU -> conv 1x1 [-> add with the first conv's input] of a
    folded graph becomes one mbconv node; the variables keep their names."""
    cons = graph.consumers()
    lvars = _layer_vars(graph)
    out = Graph(graph.name, in_ch=graph.input.C)
    tmap = {graph.input.id: out.input}
    done = set()

    def only(t, kind):
        cs = cons[t.id]
        return cs[0] if len(cs) == 1 and cs[0].kind == kind and t.id != graph.output.id else None

    def pointwise(n, act):
        a = n.attrs
        return (n.kind == "conv" and a["k"] == 1 and a["s"] == 1 and a["bias"]
                and (a["act"] == act if act else _is_none(a["act"])))

    for n in graph.nodes[1:]:
        if n.idx in done:
            continue
        ins = [tmap[t.id] for t in n.ins]
        d = only(n.out, "dwconv") if pointwise(n, "relu") else None
        p = only(d.out, "conv") if d is not None and d.attrs["bias"] and d.attrs.get("act") == "relu" else None
        if p is not None and pointwise(p, None) and _mbconv_ok(n.ins[0].C, n.out.C, p.out.C):
            a = only(p.out, "add")
            x = n.ins[0]
            if a is not None and {t.id for t in a.ins} != {p.out.id, x.id}:
                a = None
            prefix = os.path.commonprefix([n.name, d.name, p.name])
            t = out.mbconv(ins[0], n.out.C, p.out.C, n.name, d.name, p.name, res=a is not None, name=prefix + "mbconv")
            tmap[(a or p).out.id] = t
            done.update(m.idx for m in (d, p, a) if m is not None)
        else:
            tmap[n.out.id] = _clone(out, n, ins, lvars)
    out.set_output(tmap[graph.output.id])
    return out


def fold_graph(graph, fuse=True):
    """The inference form of a Graph -> (folded graph, recipe).  recipe[v], for every variable v
    of the folded graph, says what it is made of:
      {"op": "copy",  "src": name}                                  the source variable itself
      {"op": "scale", "src": kernel, "bn": layer, "eps", "axis"}    kernel * s along `axis`
      {"op": "shift", "src": bias or None, "bn": layer, "eps"}      beta + (bias - moving_mean) * s
    with s = gamma / sqrt(moving_variance + eps) of BN layer `bn`."""
    g, recipe = _fold(graph)
    if fuse:
        g = _fuse(g)
    return g, recipe


def fold_params_ref(recipe, params, stats):
    """numpy fp64 reference of the fold: params the source variables, stats the moving statistics
    ("<bn>/moving_mean", "<bn>/moving_variance") -> the folded variables."""
    f64 = lambda a: np.asarray(a, np.float64)   # noqa: E731
    out = {}
    for name, r in recipe.items():
        if r["op"] == "copy":
            out[name] = f64(params[r["src"]]).copy()
            continue
        b = r["bn"]
        s = f64(params[f"{b}/gamma"]) / np.sqrt(f64(stats[f"{b}/moving_variance"]) + r["eps"])
        if r["op"] == "scale":
            w = f64(params[r["src"]])
            shape = [1] * w.ndim
            shape[r["axis"]] = -1
            out[name] = w * s.reshape(shape)
        else:
            bias = f64(params[r["src"]]) if r["src"] else 0.0
            out[name] = f64(params[f"{b}/beta"]) + (bias - f64(stats[f"{b}/moving_mean"])) * s
    return out


def mbconv_ref(x, w_exp, b_exp, k_dw, b_dw, w_proj, b_proj, res=None, mask=True):
    """numpy fp64 reference of dg_mbconv_fwd: x [N,H,W,C], w_exp [C,E], k_dw [3,3,E], w_proj [E,Co].
    mask False is the WRONG border rule (a zero-padded x expanded, relu(b_exp) in the halo)."""
    f64 = lambda a: np.asarray(a, np.float64)   # noqa: E731
    x = f64(x)
    N, H, W, C = x.shape
    E = w_exp.shape[-1]
    xp = np.zeros((N, H + 2, W + 2, C))
    xp[:, 1:-1, 1:-1] = x
    e = np.maximum(xp @ f64(w_exp).reshape(C, E) + f64(b_exp), 0.0)
    if mask:
        e[:, 0] = e[:, -1] = 0.0
        e[:, :, 0] = e[:, :, -1] = 0.0
    k = f64(k_dw).reshape(3, 3, E)
    d = np.zeros((N, H, W, E)) + f64(b_dw)
    for i in range(3):
        for j in range(3):
            d += e[:, i:i + H, j:j + W] * k[i, j]
    y = np.maximum(d, 0.0) @ f64(w_proj).reshape(E, -1) + f64(b_proj)
    return y if res is None else y + f64(res)


# ---------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------
def sr_tile_geometry(h, w, multiple=1, tile=None, margin=0):
    """The input-side TileGeometry.  Whole-image mode (tile None): one tile, (h, w) rounded up to
    `multiple` and centred -- no padding at all when multiple is 1.  Tile mode: T x T tiles,
    T % multiple == 0, 0 <= margin < T/2 (dgan.infer.tile_geometry without the 256 rule)."""
    h, w, multiple = int(h), int(w), int(multiple)
    if h < 1 or w < 1:
        raise ValueError(f"empty image {h}x{w}")
    if multiple < 1:
        raise ValueError(f"multiple must be at least 1, got {multiple}")
    if tile is None:
        if margin:
            raise ValueError("margin applies to tile mode only")
        Th, Tw = _up(h, multiple), _up(w, multiple)
        return TileGeometry(h, w, Th, Tw, Th, Tw, -((Th - h) // 2), -((Tw - w) // 2), 1, 1, 0, 0)
    T, margin = int(tile), int(margin)
    if T < 1 or T % multiple:
        raise ValueError(f"tile must be a positive multiple of {multiple}, got {T}")
    if not 0 <= margin < T / 2:
        raise ValueError(f"margin must satisfy 0 <= margin < tile/2, got {margin}")
    S = T - 2 * margin
    return TileGeometry(h, w, T, T, S, S, -margin, -margin, -(-h // S), -(-w // S), margin, margin)


def scaled(g, s):
    """The output-side geometry of a network that scales by s: every length and offset times s, the
    tile counts as they are."""
    s = int(s)
    if s < 1:
        raise ValueError(f"scale must be at least 1, got {s}")
    return TileGeometry(g.h * s, g.w * s, g.Th * s, g.Tw * s, g.Sh * s, g.Sw * s, g.oy * s, g.ox * s, g.gi, g.gj,
                        g.mt * s, g.ml * s)


def unstage_ok(g):
    """dg_u8_unstage's validity conditions (csrc/infer.hip): every output pixel reads inside its
    tile.  They are linear in the lengths, so they hold for scaled(g, s) whenever they hold for g."""
    return (g.mt >= 0 and g.ml >= 0 and g.mt + g.Sh <= g.Th and g.ml + g.Sw <= g.Tw
            and g.oy + g.mt <= 0 and g.ox + g.ml <= 0
            and g.h - 1 - g.oy - (g.gi - 1) * g.Sh < g.Th and g.w - 1 - g.ox - (g.gj - 1) * g.Sw < g.Tw)


# ---------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------
class SRPlan:
    """The folded forward for one input shape: a GraphPlan over the folded arena, a pre-sized
    workspace and an output buffer.  A forward allocates nothing and never synchronises."""

    def __init__(self, folded, N, H, W):
        import torch
        from . import ops
        from .graph import GraphPlan
        net = folded.network
        self.plan = GraphPlan(folded.graph, N, H, W, folded.arena, net.bn, folded.device, train=False,
                              math=net.conv_math)
        self.out_shape = self.plan.out_shape
        self.out = torch.empty(self.out_shape, dtype=torch.float32, device=folded.device)
        self.ws = ops.Workspace(folded.device)
        self.ws.get(max([d.ws[ops.OP_FWD] for d in self.plan.desc.values()] + [0]))

    def forward(self, x, out=None):
        return self.plan.forward(x, training=False, out=self.out if out is None else out, ws=self.ws)


class FoldedNetwork:
    """A GraphNetwork's inference form on the device: the folded graph over a second, frozen arena
    (`frozen` / `version`: the weight-plane protocol of dgan/graph.py _stale_w, as
    dgan.infer.FoldedArena) that `refold()` fills from the network's current weights."""

    def __init__(self, network, fuse=True):
        from .nets import Arena
        self.network, self.device, self.fuse = network, network.device, bool(fuse)
        self.graph, self.recipe = fold_graph(network.graph, fuse=fuse)
        A = self.arena = Arena(self.graph.var_list(), self.device, self.graph.layout_order())
        A.grad = A.m = A.v = None   # (never trained)
        A.frozen, A.version = True, 0
        self._plans = {}
        self.refold()

    def refold(self):
        """Fold the network's current weights and moving statistics: one dg_bn_fold per folded conv
        or dwconv (a [3,3,C,1] depthwise kernel is taps 9, Cin 1, Cout C in memory), plain copies
        for everything else; kept weight planes are split again by the next forward."""
        from . import ops
        src, bn, A = self.network.arena, self.network.bn, self.arena
        for name, r in self.recipe.items():
            if r["op"] == "copy":
                A.param(name).copy_(src.param(r["src"]))
            elif r["op"] == "scale":
                layer = name.rsplit("/", 1)[0]
                rb = self.recipe[f"{layer}/bias"]
                w, wo = src.param(r["src"]), A.param(name)
                if r["axis"] == 2:
                    C = w.shape[2]
                    w, wo = w.view(3, 3, 1, C), wo.view(3, 3, 1, C)
                b = r["bn"]
                ops.bn_fold(w, src.param(f"{b}/gamma"), src.param(f"{b}/beta"), bn.mean[b], bn.var[b], wo,
                            A.param(f"{layer}/bias"), eps=r["eps"],
                            bias_in=src.param(rb["src"]) if rb["src"] else None)
        A.version += 1

    def max_abs_weight(self):
        """max |folded weight| (synchronises); the fp16x3 weight planes hold |w| < 255."""
        return float(self.arena.data.abs().max().item())

    def plan(self, N, H, W):
        key = (N, H, W, self.network.conv_math)
        if key not in self._plans:
            self._plans[key] = SRPlan(self, N, H, W)
        return self._plans[key]

    def __call__(self, x, out=None):
        """x: fp32 NHWC device tensor -> the network's output (the plan's own buffer unless `out`)."""
        N, H, W, _ = x.shape
        return self.plan(N, H, W).forward(x, out)


def predict(network, x, batch_size=None):
    """Keras `model.predict`: numpy in, numpy out, on the folded path with the network's current
    weights (refolded on every call)."""
    import torch
    from .models import to_device
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 4 or x.shape[-1] != network.graph.input.C:
        raise ValueError(f"predict expects [N,H,W,{network.graph.input.C}], got {x.shape}")
    F = getattr(network, "_folded", None)
    if F is None:
        F = network._folded = FoldedNetwork(network)
    else:
        F.refold()
    n = x.shape[0]
    bs = min(int(batch_size or 32), max(n, 1))
    out = None
    for i in range(0, n, bs):
        xb = to_device(x[i:i + bs], network.device)
        yb = F(xb).cpu().numpy()
        if out is None:
            out = np.empty((n,) + yb.shape[1:], np.float32)
        out[i:i + bs] = yb
    torch.cuda.synchronize(network.device)
    return out if out is not None else np.empty((0,) + x.shape[1:], np.float32)


class _Frame:
    """Buffers of one (n, h, w): static uint8 input / output, the tile buffers (the last chunk
    filled up with idle tiles) and, with graph=True, the captured launch sequence."""
    __slots__ = ("g", "go", "u8_in", "u8_out", "tin", "tout", "nt", "graph")


class Upscaler:
    """uint8 images of any size through a folded SR-family generator, uint8 out at `scale` x.

    scale: the network's (SRGAN 2 or 4, FastSRGAN 4, autoencoder 1); multiple: what the network's
    input sizes must divide by (1; the autoencoder's five pools 32).  tile None: whole-image mode;
    tile T: T x T tiles with `margin` pixels of context, `batch` tiles per forward (module
    docstring: the margins that cover the receptive fields).  graph: capture stage -> forward ->
    unstage once per (n, h, w)."""

    def __init__(self, network, scale, multiple=1, tile=None, margin=0, pad="black", batch=8, graph=False,
                 fuse=True):
        if pad not in PADS:
            raise ValueError(f"pad must be one of {PADS}, got {pad!r}")
        if int(batch) < 1:
            raise ValueError("batch must be at least 1")
        scaled(sr_tile_geometry(1, 1, multiple, tile, margin), scale)   # (validates them)
        self.scale, self.multiple = int(scale), int(multiple)
        self.tile, self.margin, self.pad, self.batch, self.graph = tile, int(margin), pad, int(batch), bool(graph)
        self.folded = FoldedNetwork(network, fuse=fuse)
        self.device = network.device
        self._frames = {}

    def refresh(self):
        """Refold after the network's weights or moving statistics changed.  The weight planes a
        captured graph reads are split again here, by one eager forward per captured plan."""
        self.folded.refold()
        for f in self._frames.values():
            if f.graph is not None:
                self._run(f)

    def geometry(self, h, w):
        return sr_tile_geometry(h, w, self.multiple, self.tile, self.margin)

    def frame(self, n, h, w):
        """The buffers of n images of h x w (made, and with graph=True captured, on first use)."""
        import torch
        key = (n, h, w)
        if key in self._frames:
            return self._frames[key]
        f = _Frame()
        f.g = g = self.geometry(h, w)
        f.go = go = scaled(g, self.scale)
        f.nt = n * g.gi * g.gj
        B = self._chunk(f)
        dev = self.device
        plan = self.folded.plan(B, g.Th, g.Tw)
        if tuple(plan.out_shape) != (B, go.Th, go.Tw, 3):
            raise ValueError(f"the network maps {g.Th}x{g.Tw} tiles to {tuple(plan.out_shape[1:3])}, not scale "
                             f"{self.scale}")
        f.u8_in = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
        f.u8_out = torch.empty((n, go.h, go.w, 3), dtype=torch.uint8, device=dev)
        f.tin = torch.full((_up(f.nt, B), g.Th, g.Tw, 3), -1.0, dtype=torch.float32, device=dev)   # idle tiles: black
        f.tout = torch.empty((f.tin.shape[0], go.Th, go.Tw, 3), dtype=torch.float32, device=dev)
        f.graph = None
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
        """Tiles per forward: `batch` in tile mode, in whole-image mode at most the images there are."""
        return self.batch if self.tile is not None else min(self.batch, f.nt)

    def _run(self, f):
        """stage -> forward per chunk -> unstage, all on the current stream."""
        from . import ops
        B = self._chunk(f)
        ops.u8_stage(f.u8_in, f.tin[:f.nt], f.g, self.pad)
        plan = self.folded.plan(B, f.g.Th, f.g.Tw)
        for t0 in range(0, f.tin.shape[0], B):
            plan.forward(f.tin[t0:t0 + B], f.tout[t0:t0 + B])
        ops.u8_unstage(f.tout[:f.nt], f.u8_out, f.go)

    def run(self, images):
        """Upload uint8 numpy images [n,h,w,3] (n >= 1) and upscale them on the current stream
        without reading anything back: the frame whose device buffers `u8_in` / `u8_out` hold the
        input and the result until the next call on the same shape."""
        import torch
        f = self.frame(*images.shape[:3])
        f.u8_in.copy_(torch.from_numpy(np.ascontiguousarray(images)))
        return self.run_frame(f)

    def run_frame(self, f):
        """Upscale what the frame's `u8_in` holds into its `u8_out` on the current stream (a replay
        of the captured graph where there is one); returns the frame."""
        if f.graph is not None:
            f.graph.replay()
        else:
            self._run(f)
        return f

    def upscale(self, images):
        """uint8 [n,h,w,3] or [h,w,3] (numpy or torch) -> uint8 numpy [n, h*scale, w*scale, 3]."""
        import torch
        a = images.cpu().numpy() if isinstance(images, torch.Tensor) else np.asarray(images)
        if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.shape[-1] != 3:
            raise ValueError(f"upscale expects uint8 [n,h,w,3] or [h,w,3], got {a.dtype} {a.shape}")
        single = a.ndim == 3
        if single:
            a = a[None]
        if a.shape[0] == 0:
            return np.empty((0, a.shape[1] * self.scale, a.shape[2] * self.scale, 3), np.uint8)
        out = self.run(a).u8_out.cpu().numpy()
        return out[0] if single else out
