"""Inputs shared by tests/test_sr_infer.py (CPU) and tests/test_sr_infer_gpu.py: trained-looking
SR-family generators, the fused block's test tensors and the fp64 oracle forwards."""
import functools

import numpy as np
import torch

from oracle import sr_oracle as S

MB_TILE = 16   # the output tile of dg_mbconv_fwd (the GPU test checks it against dg_mbconv_tile)
T = MB_TILE
MB_SHAPES = [(1, 1, 1), (1, 5, 7), (1, T, T), (2, T + 1, 2 * T + 1), (1, 2 * T + 8, 3 * T + 2)]
MB_C, MB_E = 32, 192


def builder(kind):
    from dgan import zoo
    return {"fsrgan": lambda: zoo.fsrgan_generator(),
            "fsrgan16": lambda: zoo.fsrgan_generator(gf=16),
            "srgan": lambda: zoo.srgan_generator(n_blocks=2),
            "autoencoder": lambda: zoo.autoencoder_generator()}[kind]()


def _t64(d):
    return {k: torch.tensor(np.asarray(v, np.float64)) for k, v in d.items()}


def _bn_stats(stats):
    st = S.BNStats()
    for k, v in stats.items():
        layer, what = k.rsplit("/", 1)
        (st.mean if what == "moving_mean" else st.var)[layer] = np.asarray(v, np.float64)
    return st


def oracle_forward(kind, params, stats, x, training=False, bn_stats=None):
    """The fp64 oracle's generator output (numpy) on numpy parameters."""
    P = _t64(params)
    xt = torch.tensor(np.asarray(x, np.float64))
    st = bn_stats if bn_stats is not None else _bn_stats(stats)
    with torch.no_grad():
        if kind.startswith("fsrgan"):
            y = S.fsrgan_generator(P, xt, st, gf=16 if kind == "fsrgan16" else 32, training=training)
        elif kind == "srgan":
            y = S.srgan_generator(P, xt, st, n_blocks=2, training=training)
        else:
            y = S.autoencoder_generator(P, xt)
    return y.numpy()


@functools.lru_cache(maxsize=None)
def trained_looking(kind, H=16, W=16):
    """(graph, params, stats) of a generator that looks trained, by the recipe of
    tests/test_infer_gpu.py::trained_looking: gamma ~ U(0.5, 1.5), beta ~ N(0, 0.2), conv biases ~
    N(0, 0.1), and each BN's moving statistics spread around its batch statistics on four random
    images (a training-mode oracle forward), the variance floored at a tenth of the layer's mean."""
    from dgan.graph import init_graph_variables
    graph = builder(kind)
    rng = np.random.default_rng(sum(map(ord, kind)))
    params = init_graph_variables(graph, 5)
    for k in params:
        if k.endswith("/gamma"):
            params[k] = rng.uniform(0.5, 1.5, params[k].shape).astype(np.float32)
        elif k.endswith("/beta"):
            params[k] = (rng.standard_normal(params[k].shape) * 0.2).astype(np.float32)
        elif k.endswith("/bias"):
            params[k] = (rng.standard_normal(params[k].shape) * 0.1).astype(np.float32)
    if kind == "autoencoder":
        # (he_normal weights on white noise drive the output tanh into saturation, where every
        # path agrees whatever it computes: a tenth of the last kernel keeps |output| below 1)
        params["conv11/kernel"] = params["conv11/kernel"] * np.float32(0.1)
    stats = {}
    if graph.bn_layers:
        x4 = rng.uniform(-1, 1, (4, H, W, 3))
        st = S.BNStats()
        oracle_forward(kind, params, None, x4, training=True, bn_stats=st)
        # the oracle keeps only the updated moving statistics (from 0 / 1): undo the update
        mom = {n.name: n.attrs["momentum"] for n in graph.nodes if n.kind == "bn"}
        for name in graph.bn_layers:
            m = mom[name]
            mu = st.mean[name] / (1 - m)
            var = np.maximum((st.var[name] - m) / (1 - m), 1e-12)
            var = np.maximum(var, 0.1 * var.mean())
            stats[f"{name}/moving_variance"] = (var * rng.uniform(0.5, 2.0, var.shape)).astype(np.float32)
            stats[f"{name}/moving_mean"] = (mu + 0.3 * np.sqrt(var) * rng.standard_normal(var.shape)).astype(np.float32)
    return graph, params, stats


def mb_inputs(N, H, W, seed=0):
    """The fused block's test tensors: x ~ N(0,1), W_exp ~ N(0, 1/sqrt(32)), k_dw ~ N(0, 1/3), W_proj ~
    N(0, 1/sqrt(192)), biases ~ N(0, 0.5)."""
    rng = np.random.default_rng(1000 * N + 100 * H + W + seed)
    f = lambda a: a.astype(np.float32)   # noqa: E731
    return dict(x=f(rng.standard_normal((N, H, W, MB_C))),
                w_exp=f(rng.standard_normal((1, 1, MB_C, MB_E)) / np.sqrt(MB_C)),
                b_exp=f(rng.standard_normal(MB_E) * 0.5),
                k_dw=f(rng.standard_normal((3, 3, MB_E, 1)) / 3.0),
                b_dw=f(rng.standard_normal(MB_E) * 0.5),
                w_proj=f(rng.standard_normal((1, 1, MB_E, MB_C)) / np.sqrt(MB_E)),
                b_proj=f(rng.standard_normal(MB_C) * 0.5))


def mb_oracle(t, res):
    """conv -> relu -> dwconv3 -> relu -> conv (+ x) with the oracle's layers, fp64."""
    P = _t64(t)
    h = torch.relu(S.conv(P["x"], P["w_exp"], P["b_exp"]))
    h = torch.relu(S.dwconv3(h, P["k_dw"], P["b_dw"]))
    h = S.conv(h, P["w_proj"], P["b_proj"])
    return (h + P["x"] if res else h).numpy()
