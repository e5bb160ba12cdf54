"""Super-resolution inference, the parts that need no GPU (dgan/sr_infer.py): the graph rewrite's
node counts, the fold algebra in fp64 against the oracle, the fused block's numpy reference and
its border rule, and the tile geometry of the Upscaler."""
from collections import Counter

import numpy as np
import pytest

from sr_infer_util import MB_SHAPES, builder, mb_inputs, mb_oracle, oracle_forward, trained_looking


def _kinds(g):
    return Counter(n.kind for n in g.nodes[1:])


# ---------------------------------------------------------------------------
# fold_graph
# ---------------------------------------------------------------------------
def test_fsrgan_folds_and_fuses_five_blocks():
    from dgan.sr_infer import fold_graph
    g, recipe = fold_graph(builder("fsrgan"))
    k = _kinds(g)
    assert k["bn"] == 0 and k["mbconv"] == 5 and k["dwconv"] == 1
    # conv, prelu, dw, conv, add, 5 mbconv, conv, add, 2 x (conv, prelu), conv
    assert [n.kind for n in g.nodes[1:]] == (["conv", "prelu", "dwconv", "conv", "add"] + ["mbconv"] * 5
                                             + ["conv", "add"] + ["conv", "prelu"] * 2 + ["conv"])
    assert len(g.nodes) - 1 == 17
    assert all(n.attrs["res"] and n.attrs["E"] == 192 for n in g.nodes if n.kind == "mbconv")
    assert set(recipe) == {v for v, _ in g.var_list()}
    assert g.output.node.attrs["act"] == "tanh"


def test_fsrgan_unfused_keeps_six_depthwise_convs_with_relu():
    from dgan.sr_infer import fold_graph
    g, recipe = fold_graph(builder("fsrgan"), fuse=False)
    k = _kinds(g)
    assert k["bn"] == 0 and k["mbconv"] == 0 and k["dwconv"] == 6
    assert all(n.attrs["act"] == "relu" and n.attrs["bias"] for n in g.nodes if n.kind == "dwconv")
    assert set(recipe) == {v for v, _ in g.var_list()}


def test_srgan_folds_every_bn_and_every_conv_gets_a_bias():
    from dgan.sr_infer import fold_graph
    src = builder("srgan")
    g, recipe = fold_graph(src)
    assert _kinds(g)["bn"] == 0
    convs = [n for n in g.nodes if n.kind == "conv"]
    assert len(convs) == sum(n.kind == "conv" for n in src.nodes) and all(n.attrs["bias"] for n in convs)
    names = {v for v, _ in g.var_list()}
    assert all(f"{n.name}/bias" in names for n in convs)
    assert recipe["conv2d/bias"]["src"] is None and recipe["conv2d/bias"]["bn"] == "batch_normalization"
    assert [n.attrs["act"] for n in convs if n.name == "block_0_conv1"] == ["relu"]


def test_autoencoder_passes_through_unchanged():
    from dgan.sr_infer import fold_graph
    src = builder("autoencoder")
    g, recipe = fold_graph(src)
    assert [(n.kind, n.name, n.attrs) for n in g.nodes] == [(n.kind, n.name, n.attrs) for n in src.nodes]
    assert g.var_list() == src.var_list()
    assert all(r == {"op": "copy", "src": v} for v, r in recipe.items())


def test_unsupported_channel_counts_stay_unfused_but_folded():
    from dgan.sr_infer import fold_graph
    g, _ = fold_graph(builder("fsrgan16"))
    k = _kinds(g)
    assert k["mbconv"] == 0 and k["bn"] == 0 and k["dwconv"] == 6


def test_existing_graphs_carry_no_depthwise_activation():
    g = builder("fsrgan")
    assert all(n.attrs["act"] is None for n in g.nodes if n.kind == "dwconv")


def test_a_training_plan_refuses_inference_nodes():
    torch = pytest.importorskip("torch")
    from dgan.graph import GraphPlan
    from dgan.sr_infer import fold_graph
    g, _ = fold_graph(builder("fsrgan"))
    with pytest.raises(ValueError):
        GraphPlan(g, 1, 8, 8, None, None, torch.device("cpu"), train=True)


# ---------------------------------------------------------------------------
# fold algebra, fp64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fsrgan", "srgan"])
def test_folded_parameters_reproduce_the_oracle(kind):
    """oracle(params, moving statistics, training=False) == oracle(folded params, identity BN) to
    1e-12.  Identity BN: gamma 1, beta 0, variance 1 - eps (scale exactly 1), mean 0 -- or, for a
    conv the oracle gives no bias (SRGAN's use_bias=False convs), mean = -(folded bias), which is
    how the bias the fold creates reaches a network that has no slot for it."""
    from dgan.sr_infer import fold_graph, fold_params_ref
    graph, params, stats = trained_looking(kind)
    _, recipe = fold_graph(graph, fuse=False)
    folded = fold_params_ref(recipe, params, stats)
    assert all(v.dtype == np.float64 for v in folded.values())
    p2, s2 = dict(folded), {}
    for n in graph.nodes:
        if n.kind != "bn":
            continue
        C = n.out.C
        p2[f"{n.name}/gamma"], p2[f"{n.name}/beta"] = np.ones(C), np.zeros(C)
        s2[f"{n.name}/moving_variance"] = np.full(C, 1.0 - n.attrs["eps"])
        src = n.ins[0].node
        assert src.kind in ("conv", "dwconv")
        s2[f"{n.name}/moving_mean"] = np.zeros(C) if src.attrs["bias"] else -folded[f"{src.name}/bias"]
    x = np.random.default_rng(3).uniform(-1, 1, (2, 13, 19, 3))
    want = oracle_forward(kind, params, stats, x)
    got = oracle_forward(kind, p2, s2, x)
    err = np.abs(got - want).max()
    print(f"{kind}: fold algebra max error {err:.2e}, output std {want.std():.3f} max {np.abs(want).max():.3f}")
    assert want.std() > 0.05 and np.abs(want).max() < 0.9999
    assert err <= 1e-12


def test_fold_params_ref_scales_the_depthwise_axis():
    from dgan.sr_infer import fold_graph, fold_params_ref
    graph, params, stats = trained_looking("fsrgan")
    _, recipe = fold_graph(graph)
    r = recipe["block_1_depthwise/depthwise_kernel"]
    assert r["op"] == "scale" and r["axis"] == 2 and r["bn"] == "block_1_depthwise_BN"
    f = fold_params_ref(recipe, params, stats)
    s = params["block_1_depthwise_BN/gamma"].astype(np.float64) / np.sqrt(
        stats["block_1_depthwise_BN/moving_variance"].astype(np.float64) + 1e-3)
    k = params["block_1_depthwise/depthwise_kernel"].astype(np.float64)
    assert np.array_equal(f["block_1_depthwise/depthwise_kernel"], k * s[None, None, :, None])


# ---------------------------------------------------------------------------
# the fused block's reference and its border rule
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", MB_SHAPES)
@pytest.mark.parametrize("res", [True, False])
def test_mbconv_ref_equals_the_oracle_layers(shape, res):
    from dgan.sr_infer import mbconv_ref
    t = mb_inputs(*shape)
    got = mbconv_ref(t["x"], t["w_exp"], t["b_exp"], t["k_dw"], t["b_dw"], t["w_proj"], t["b_proj"],
                     res=t["x"] if res else None)
    want = mb_oracle(t, res)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("shape", MB_SHAPES)
def test_the_inputs_can_see_the_wrong_border_rule(shape):
    """Expanding a zero-padded x (relu(b_exp) in the halo) instead of masking the depthwise input
    changes border pixels by more than 1e-2 and no interior pixel at all."""
    from dgan.sr_infer import mbconv_ref
    t = mb_inputs(*shape)
    a = [t[k] for k in ("x", "w_exp", "b_exp", "k_dw", "b_dw", "w_proj", "b_proj")]
    diff = np.abs(mbconv_ref(*a, mask=False) - mbconv_ref(*a)).max(axis=-1)
    assert float((t["b_exp"] > 0).mean()) > 0.3
    assert np.all(diff[:, 1:-1, 1:-1] == 0.0)
    border = np.ones(diff.shape, bool)
    border[:, 1:-1, 1:-1] = False
    assert diff[border].max() > 1e-2
    for n in range(shape[0]):   # every edge of every image
        for edge in (diff[n, 0], diff[n, -1], diff[n, :, 0], diff[n, :, -1]):
            assert edge.max() > 1e-2


# ---------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------
GEOM = [(h, w, m, kw) for (h, w) in [(1, 1), (13, 19), (270, 480)] for m in (1, 32)
        for kw in (dict(), dict(tile=32, margin=10))]


@pytest.mark.parametrize("h,w,multiple,kw", GEOM)
@pytest.mark.parametrize("s", [1, 2, 4])
def test_scaled_geometry_satisfies_the_unstage_conditions(h, w, multiple, kw, s):
    from dgan.sr_infer import scaled, sr_tile_geometry, unstage_ok
    g = sr_tile_geometry(h, w, multiple, **kw)
    assert g.Th % multiple == 0 and g.Tw % multiple == 0
    if multiple == 1 and not kw:
        assert (g.Th, g.Tw, g.oy, g.ox) == (h, w, 0, 0)   # no padding at all
    assert unstage_ok(g)
    go = scaled(g, s)
    assert unstage_ok(go)
    assert (go.h, go.w, go.Th, go.gi, go.gj) == (h * s, w * s, g.Th * s, g.gi, g.gj)


@pytest.mark.parametrize("h,w,multiple,kw", [c for c in GEOM if c[0] < 100])
@pytest.mark.parametrize("pad", ["black", "reflect"])
def test_round_trip_through_a_nearest_upsampler_repeats_the_image(h, w, multiple, kw, pad):
    from dgan.infer import stage_ref, unstage_ref
    from dgan.sr_infer import scaled, sr_tile_geometry
    s = 4
    g = sr_tile_geometry(h, w, multiple, **kw)
    u8 = np.random.default_rng(h + w).integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    tiles = stage_ref(u8, g, pad)
    up = tiles.repeat(s, axis=1).repeat(s, axis=2)   # the stand-in network
    got = unstage_ref(up, scaled(g, s))
    assert got.shape == (2, h * s, w * s, 3)
    assert np.array_equal(got, u8.repeat(s, axis=1).repeat(s, axis=2))


@pytest.mark.parametrize("kw", [dict(multiple=0), dict(multiple=32, tile=48), dict(tile=0), dict(tile=32, margin=16),
                                dict(tile=32, margin=-1), dict(margin=4), dict(multiple=32, tile=16)])
def test_bad_geometry_raises(kw):
    from dgan.sr_infer import sr_tile_geometry
    with pytest.raises(ValueError):
        sr_tile_geometry(40, 52, **kw)


def test_bad_scale_and_empty_image_raise():
    from dgan.sr_infer import scaled, sr_tile_geometry
    with pytest.raises(ValueError):
        scaled(sr_tile_geometry(4, 4), 0)
    with pytest.raises(ValueError):
        sr_tile_geometry(0, 4)
