"""``AdaptiveGraphConvolution`` and the clip drivers launch what they launched before their launch sequences were gathered into
one copy each: every library call of ``forward``, ``forward_framewise`` and ``stage`` -- V = 18 and 25, the channel pairs of
both ``gcn_residual`` kinds and both embedding widths, T = 1 and 5, the fused and the two-launch route, one chunk and chunks of
2 + 2 + 1 frames -- and of the four "input norm, then the ten blocks" drivers, in order, with every number, every allocation's
shape and every view's offset (tests/agcn_routes_fixture.py), against tests/golden/agcn_routes_trace.json, which that module
wrote on the commit before the change.  And the one thing the change adds: every driver refuses a ``data_bn`` that does not
match the input's (C, V, M) before anything is launched.  No GPU."""
import json

import pytest
import torch

import _bootstrap
from tests import agcn_routes_fixture as fx

pkg = _bootstrap.load()
SCENARIOS = fx.scenarios(pkg)


@pytest.fixture(scope="module")
def golden():
    with open(fx.GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_scenarios(golden):
    assert sorted(golden) == sorted(SCENARIOS)
    # 2 joint counts x 3 channel pairs x (2 frame counts x 2 routes x 3 methods + the 2 chunked runs) + 2 kernel runs + 6 drivers
    assert len(golden) == 2 * 3 * (2 * 2 * 3 + 2) + 2 + 6


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_launch_trace_is_the_recorded_one(golden, name):
    got, want = fx.record(SCENARIOS[name]), golden[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: call {i} differs\n got  {g}\n want {w}"
    assert len(got) == len(want), f"{name}: {len(got)} calls, recorded {len(want)}"


def _entries(calls):
    return [c[0] for c in calls]


def test_the_scenarios_reach_every_launch_sequence(golden):
    """What the comparison above is worth: the fixture holds both routes of all three callers, the V = 18 gate of the fused clip
    form, the slack behind the clip form's embeddings, the scratch of each form, the chunks and their views."""
    fused, two = ["csk_agcn_embed_attention_f32", "csk_gcn_stage_f32"], ["csk_conv1x1_f32", "csk_agcn_attention_f32", "csk_gcn_stage_f32"]
    for v in fx.JOINTS:
        for ci, co in fx.CHANNELS:
            inter = co // 4
            for t in fx.FRAMES:
                tag = f"V{v}-{ci}x{co}-T{t}"
                assert _entries(golden[f"forward-{tag}-fused"]) == (fused if v == 18 else two)      # V = 25 keeps the two launches
                assert _entries(golden[f"forward-{tag}-two"]) == two
                for method in ("framewise", "stage"):
                    assert _entries(golden[f"{method}-{tag}-fused"]) == fused and _entries(golden[f"{method}-{tag}-two"]) == two
                # the clip form: embeddings with 4 floats of slack, a 4-range scratch from T = 2 on, none at T = 1
                conv, attention, _ = golden[f"forward-{tag}-two"]
                assert conv[2][2:] == [[fx.N, 6 * inter, t, v], 4 * (fx.N * 6 * inter * t * v + 4)]
                assert attention[4] == (["t2", 0, [fx.N, 3, 4, v, v], 4 * fx.N * 3 * 4 * v * v] if t > 1 else None)
                # the per-frame forms take no scratch, one adjacency per (segment, frame), and say so to the graph conv
                for name in (f"framewise-{tag}-fused", f"stage-{tag}-fused"):
                    embed, stage = golden[name]
                    assert embed[6] is None and embed[12] == 1 and embed[5][2] == [fx.N * t, 3, v, v] and stage[10] == 1
                for name in (f"framewise-{tag}-two", f"stage-{tag}-two"):
                    assert golden[name][1][4] is None and golden[name][1][3][2] == [fx.N * t, 3, v, v] and golden[name][2][10] == 1
            if v == 18:                               # the per-segment fused form: one scratch slice per tile of 128 // 18 frames
                embed, stage = golden[f"forward-V18-{ci}x{co}-T5-fused"]
                assert embed[6][2] == [fx.N, 3, 1, v, v] and embed[12] == 0 and stage[10] == 0
            for route in ("fused", "two"):
                calls = golden[f"framewise-chunked-V{v}-{ci}x{co}-T5-{route}"]
                stages = [c for c in calls if c[0] == "csk_gcn_stage_f32"]
                assert [c[14] for c in stages] == [2, 2, 1]                                          # frames per chunk
                assert [c[1][1] for c in stages] == [0, 2 * v * 4, 4 * v * 4]                        # the views: t0 * V floats into a row
                assert [c[2][1] for c in stages] == [0, 2 * v * 4, 4 * v * 4] and len({c[2][0] for c in stages}) == 1
        assert _entries(golden[f"framewise-kernel-V{v}-64x128-T5"]) == ["csk_agcn_stage_framewise_f32_route", "csk_agcn_stage_framewise_f32"]
    clip = _entries(golden["StGcn.features"])
    assert clip[0] == "csk_input_norm_f32" and clip[1::2] == ["csk_gcn_stage_f32"] * 10 and len(clip) == 21
    assert all(e.startswith("csk_tcn_stage_") for e in clip[2::2])
    assert _entries(golden["CoStGcn._clip_stack"]) == clip
    assert _entries(golden["CoStGcn._prime_chunk"]) == clip + ["csk_co_prime_pack_f32"]
    steps = _entries(golden["CoAGcn.features_clip_as_steps"])
    assert steps[0] == clip[0] and steps.count("csk_agcn_embed_attention_f32") == 10 and "csk_agcn_stage_framewise_f32" not in steps
    assert _entries(golden["CoAGcn._prime_chunk-framewise"]) == steps + ["csk_co_prime_pack_f32"]
    kernel = _entries(golden["CoAGcn.features_clip_as_steps-kernel"])
    assert 0 < kernel.count("csk_agcn_stage_framewise_f32") < 10           # the measured-faster table picks per layer


@pytest.mark.parametrize("name", ["StGcn.features", "CoStGcn._clip_stack", "CoAGcn.features_clip_as_steps", "CoStGcn._prime_chunk"])
def test_a_data_bn_of_the_wrong_width_is_refused_before_any_launch(name):
    """A clip of 18 joints into a model whose data_bn was sized for 25: the shared refusal of ``input_norm``."""
    t = fx.DRIVERS[name][3]
    x = torch.zeros((1, fx.SHAPE[0], t, 18, fx.SHAPE[3]))
    cls, kwargs, call, _, route = fx.DRIVERS[name]
    net, table = fx._model(pkg, getattr(pkg, cls), **kwargs)
    with fx.Recorder(pkg, dict(table, x=x), route) as rec:
        with pytest.raises(RuntimeError, match=r"input \(C,V,M\)=\(3,18,2\) does not match data_bn with 150 channels"):
            call(net, x)
    assert rec.calls == []
