"""The A-GCN* and S-TR* models without a GPU: the literal oracle (tests/mod_family_oracle.py) against the reference's own AGcnMod
and STrMod (tests/golden/g16_agcn_mod.npz, g17_str_mod.npz), the folded diagonal graph conv against the literal one, state_dict
layouts and their maps, the geometry and guards the models take from StGcnMod / CoStGcnMod, and CoAGcnMod's native plan: the host
queries that decide it and the executor's launches against the Python engine's."""
import pytest
import torch

import _bootstrap
from oracle import stgcn_oracle as o
from tests import mod_family_oracle as fo
from tests import mod_oracle as mo
from tests import test_mod_cpu as tm
from tests import trace_fixture as tf
from tests.helpers import max_err

pkg = _bootstrap.load()
MODELS = {"agcn": (fo.g16, pkg.agcn.AGcnMod, pkg.agcn.CoAGcnMod), "str": (fo.g17, pkg.str.STrMod, pkg.str.CoSTrMod)}


# ---- oracle against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["ntu", "kin"])
@pytest.mark.parametrize("model", ["agcn", "str"])
def test_literal_oracle_equals_the_reference(model, tag):
    """The tolerance tests/test_mod_cpu.py uses for g15 (1e-4) on the logits and on the layer 1 / 5 / 8 / 10 taps."""
    a, sd, x = MODELS[model][0](tag)
    assert sum(v.numel() for k, v in sd.items() if "running" not in k and "num_batches" not in k) == int(a["nparams"])
    taps = {}
    with torch.no_grad():
        logits = fo.mod_forward(x, sd, taps=taps)
    assert max_err(logits, a["logits"]) <= 1e-4
    for i in (1, 5, 8, 10):
        assert tuple(taps[f"layer{i}"].shape) == tuple(a[f"layer{i}_shape"])
        assert max_err(taps[f"layer{i}"].reshape(-1)[::97], a[f"layer{i}_sub"]) <= 1e-4
        assert float(a[f"layer{i}_absmax"]) <= 32.0                   # O(1) activations: an absolute tolerance means something
    assert tuple(taps["layer10"].shape) == (2 * x.shape[0], 256, x.shape[2] - 80, x.shape[3])


@pytest.mark.parametrize("tag", ["ntu", "kin"])
def test_folded_diagonal_graph_conv_equals_the_literal_one(tag):
    """The plain graph conv of oracle/stgcn_oracle.py on diag(s_i) against the literal forward, layer by layer on the literal
    stack's own activations (identity and conv gcn_residual, 3 to 256 channels) and through the whole model: within 1e-5.  The
    softmax row sums differ from 1 by at most (V - 1) ulp, 1.5e-6 relative."""
    a, sd, x = fo.g16(tag)
    taps = {}
    with torch.no_grad():
        lit = fo.mod_forward(x, sd, taps=taps)
        h = o.stgcn_pre(x, sd)
        for i in range(10):
            p = f"layers.layer{i + 1}.gcn."
            want, got = fo.adaptive_graph_conv_mod(h, sd, p), fo.folded_graph_conv_mod(h, sd, p)
            assert max_err(got, want) <= 1e-5 * max(1.0, float(want.abs().max())), i + 1
            h = taps[f"layer{i + 1}"]
        folded = fo.mod_forward(x, sd, gcn=fo.folded_graph_conv_mod)
    assert max_err(folded, lit) <= 1e-5
    # the embedding convs do not reach the output
    alt = {k: (v * 3.0 + 0.25 if ".a_conv." in k or ".b_conv." in k else v) for k, v in sd.items()}
    with torch.no_grad():
        assert max_err(fo.mod_forward(x, alt), lit) <= 1e-5


def test_fold_builds_the_diagonal_ell():
    a, sd, _ = fo.g16("ntu")
    net = pkg.agcn.AGcnMod(pkg.ntu_graph().A, (3, 88, 25, 2), 60)
    net.load_state_dict(sd, strict=True)
    for i in (1, 5, 10):
        g = net.layers[f"layer{i}"].gcn
        assert type(g) is pkg.agcn.AdaptiveGraphConvolutionMod and pkg.blocks.is_plain_graph_conv(g)
        f, p = g._fold(), f"layers.layer{i}.gcn."
        assert f["ell_w"] == 1 and f["ell_cnt_host"].tolist() == [1, 1, 1]
        assert f["ell_src"].dtype == torch.int32 and torch.equal(f["ell_src"], torch.arange(25, dtype=torch.int32).repeat(3, 1).unsqueeze(-1))
        s64 = 1.0 + (sd[p + "A"].double() + sd[p + "graph_attn"].double()).sum(-1)
        assert f["ell_val"].shape == (3, 25, 1) and torch.equal(f["ell_val"][:, :, 0], s64.float()) and torch.equal(fo.row_sums(sd, p), s64.float())
        plain = pkg.fold.fold_graph_conv({k[len(p):]: v for k, v in sd.items() if k.startswith(p)})
        assert torch.equal(f["w"], plain["w"]) and torch.equal(f["bias"], plain["bias"]) and f["res_mode"] == plain["res_mode"]
        assert not any(k.startswith(("w_embed", "a_sum")) for k in f)


# ---- state dicts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["agcn", "str"])
def test_state_dicts_load_strictly_in_both_directions(model):
    load, clip_name, co_name = MODELS[model]
    a, sd, _ = load("ntu")
    A = pkg.ntu_graph().A
    clip = clip_name(A, (3, 88, 25, 2), 60)
    assert set(clip.state_dict().keys()) == {str(k) for k in a["sd_keys"]}
    assert {k: tuple(v.shape) for k, v in clip.state_dict().items()} == {str(k): tuple(eval(str(s))) for k, s in zip(a["sd_keys"], a["sd_shapes"])}
    clip.load_state_dict(sd, strict=True)
    co = co_name(A, (3, 88, 25, 2), 60)
    co.load_state_dict(co.map_state_dict(clip.state_dict()), strict=True)
    back = {k.replace("0.1.", "").replace("0.0.residual", "residual"): v for k, v in co.state_dict().items()}
    assert back.keys() == clip.state_dict().keys() and all(torch.equal(back[k], v) for k, v in clip.state_dict().items())
    clip2 = clip_name(A, (3, 88, 25, 2), 60)
    clip2.load_state_dict(back, strict=True)
    assert all(torch.equal(v, clip2.state_dict()[k]) for k, v in clip.state_dict().items())
    padded = {"agcn": pkg.CoAGcn, "str": pkg.CoSTr}[model](A, (3, 88, 25, 2), 60)
    assert set(co.state_dict().keys()) == set(padded.state_dict().keys())      # the reference's continual container layout


# ---- geometry, routing and guards ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["agcn", "str"])
def test_geometry_routing_and_guards_are_stgcn_mods(model):
    _, clip_name, co_name = MODELS[model]
    A = pkg.ntu_graph().A
    for t in (300, 150, 88):
        co = co_name(A, (3, t, 25, 2), 60)
        assert (co.receptive_field, co.padding, co.stride, co.delay) == (81, 0, 1, 0) == mo.mod_geometry() + (0,)
        assert (co.pool_size, co.pool_padding) == (t - 80, 0) == mo.mod_pool_defaults(t)
        assert [b.delay for b in co.layers.values()] == [8] * 10 and [b.stride for b in co.layers.values()] == [1] * 10
    clip = clip_name(A, (3, 88, 25, 2), 60).eval()
    for net in (clip, co):
        assert [i + 1 for i, b in enumerate(net.layers.values()) if b.wino_valid_res] == [5, 8]
        assert all(b.wino_valid and b.tcn.padding == 0 and b.residual_shrink == 4 for b in net.layers.values())
    for plain in (pkg.StGcnMod(A, (3, 88, 25, 2), 60), pkg.CoStGcnMod(A, (3, 88, 25, 2), 60)):      # left alone
        assert not any(b.wino_valid_res for b in plain.layers.values())
    assert pkg.SpatioTemporalBlock.wino_valid_res is False
    with pytest.raises(ValueError, match="T >= 81"):
        clip(torch.zeros(1, 3, 80, 25, 2))                                       # raised before the device check: nothing launched
    with pytest.raises(ValueError, match="T >= 81"):
        co.eval()(torch.zeros(1, 3, 80, 25, 2))
    with pytest.raises(NotImplementedError):
        clip.set_latency_mode(4)
    with pytest.raises(NotImplementedError):
        co.set_latency_mode(8)
    with pytest.raises(NotImplementedError):
        pkg.set_step_precision(co, "bf16x3")
    pkg.set_precision(clip, "bf16x3")
    with pytest.raises(NotImplementedError):
        clip(torch.zeros(1, 3, 88, 25, 2))
    kinds = [type(b.gcn).__name__ for b in clip.layers.values()]
    assert kinds == (["AdaptiveGraphConvolutionMod"] * 10 if model == "agcn" else ["GraphConvolution"] * 3 + ["GcnUnitAttention"] * 7)


def test_constructors_of_the_plain_mod_models_take_a_graph_conv():
    A = pkg.ntu_graph().A
    made = []

    def factory(ci, co, a, bn_momentum=0.1):
        made.append((ci, co))
        return pkg.GraphConvolution(ci, co, a, bn_momentum)

    pkg.StGcnMod(A, (3, 88, 25, 2), 60, GraphConv=factory)
    pkg.CoStGcnMod(A, (3, 88, 25, 2), 60, CoGraphConv=factory)
    assert made == [(ci, co) for ci, co, _, _ in mo.mod_layer_table(3)] * 2
    assert list(pkg.StGcnMod(A, (3, 88, 25, 2), 60).state_dict()) == list(pkg.StGcnMod(A, (3, 88, 25, 2), 60, GraphConv=None).state_dict())


# ---- native plan -------------------------------------------------------------------------------------------------------------
def test_coagcn_mod_is_a_stack_of_plain_graph_convs_for_the_plan():
    """What ``_build_plan`` asks of every block, and what the executor asks of the structs (csrc/executor.hip): plain graph convs
    whose ELL counts are skeleton-sparse (<= 1 / 1 / 4) -- the fused 64-channel step included -- and no adaptive operands."""
    net = pkg.agcn.CoAGcnMod(pkg.ntu_graph().A, (3, 88, 25, 2), 60).eval()
    cpu = torch.device("cpu")
    assert all(pkg.blocks.is_plain_graph_conv(b.gcn) and not hasattr(b.gcn, "plan_operands") for b in net.layers.values())
    with tf.Recorder(pkg):
        net.use_native_plan = False
        net._bind(1, cpu)
        arr, keep, *_ = net._layer_structs(cpu)
        assert [b._fusable(4, 80, 25) for b in net.layers.values()] == [b._fusable(4, 80, 25) for b in _bound(pkg.CoStGcnMod).layers.values()]
    for i, L in enumerate(arr):
        assert (L.ell_w, list(L.ell_cnt)) == (1, [1, 1, 1]) and L.ell_val and L.ell_src and not L.agcn_inter and not L.agcn_adj
        assert L.res_kind == (0 if i == 0 else 2 if i in (4, 7) else 1) and L.stride == 1
    assert net.__dict__.get("_agcn_adj") is None
    assert not pkg.blocks.is_plain_graph_conv(pkg.str.CoSTrMod(pkg.ntu_graph().A).layers.layer4.gcn)      # CoSTrMod: the Python engine


def _bound(cls):
    net = cls(pkg.ntu_graph().A, (3, 88, 25, 2), 60).eval()
    net.use_native_plan = False
    net._bind(1, torch.device("cpu"))
    return net


def _python_reduced():
    net = pkg.agcn.CoAGcnMod(pkg.ntu_graph().A, pool_size=tm.POOL, pool_padding=tm.POOL_PAD).eval()
    net.use_native_plan = False
    net.set_max_cycle(8)
    calls, out, r_of = tf._drive_model(pkg, net, tm.CYCLES, flush=False), [], iter(tm.CYCLES)
    for c in calls:
        name, a = c[0], c[2:]
        if name == "csk_input_norm_frames_f32":
            out.append(("norm", a[2], [tm._loc(p)[2] for p in a[1]]))
        elif name == "csk_co_block_step_f32":
            out.append(tm._reduce("fused_block", a))
        elif name == "return":
            out.append(("return", next(r_of), a[0] if a[1] else None, a[1], a[2]))
        elif name == "counters":
            counters = a
        else:
            assert name in ("csk_gcn_stage_f32", "csk_tcn_step_f32", "csk_co_head_step_f32"), name   # no embedding / attention launch
            if name == "csk_gcn_stage_f32":
                assert a[7] == 1 and a[8] == 0 and a[9] == 0             # ell_w 1, one adjacency for all segments and frames
            out.append(tm._reduce(name, a))
    return out, counters


def test_native_plan_issues_the_python_engines_launches_for_coagcn_mod():
    """As tests/test_mod_cpu.py for CoStGcnMod: 100 frames from a clean state in cycles of 1, 3 and 4; the executor's launches for a
    "*" stack of plain graph convs (tests/executor_trace_mod_main.cpp) are, launch for launch, the Python engine's for CoAGcnMod --
    the same rings, slots, runs and emission counts, the same returns per cycle, the same counters at the end."""
    native = tm._native_trace()
    got, (want, counters) = tm._native_reduced(native["mod"]), _python_reduced()
    nat, last = [], None
    for g in got:
        if g[0] == "cycle":
            nat.append(("return", g[1], g[3], g[4], g[5]))
            last = g[6]
        else:
            nat.append(g)
    for i, (g, w) in enumerate(zip(nat, want)):
        assert g == w, f"launch {i} differs\n native {g}\n python {w}"
    assert len(nat) == len(want) and list(last) == list(counters)
    assert {"norm", "gcn", "tcn", "fused", "head", "return"} <= {g[0] for g in nat}
    assert sum(g[3] for g in nat if g[0] == "return") == 20
