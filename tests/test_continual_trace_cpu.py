"""The continual driver launches what it launched before its arithmetic was gathered into one copy each: every library call
of six scenarios, in order, with every argument (tests/trace_fixture.py), against tests/golden/continual_trace.json; and the
two closed forms of that arithmetic, ``emissions`` and ``ring_runs``, against the scans they replaced.  No GPU."""
import json

import pytest

import _bootstrap
from tests import trace_fixture as tf

pkg = _bootstrap.load()
co = pkg.continual


@pytest.fixture(scope="module")
def golden():
    """{scenario: full call list}, decoded from the fixture's template form (tests/trace_fixture.py: fixture format)."""
    with open(tf.GOLDEN) as f:
        enc = json.load(f)
    return {name: tf.decode(enc, name) for name in enc["scenarios"]}


def test_the_fixture_holds_exactly_the_scenarios(golden):
    assert sorted(golden) == sorted(tf.SCENARIOS)


@pytest.mark.parametrize("name", list(tf.SCENARIOS))
def test_launch_trace_is_the_recorded_one(golden, name):
    got, want = tf.record(name), golden[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: call {i} differs\n got  {g}\n want {w}"
    assert len(got) == len(want), f"{name}: {len(got)} calls, recorded {len(want)}"


def test_the_scenarios_reach_every_launch_path(golden):
    """What the comparison above is worth: the fixture holds fused and two-launch cycles, wrapped slot runs, split-K of both
    convs, the bf16x3 step launcher, conv / identity / no residual, flushes and head steps with and without logits."""
    def names(sc):
        return {(c[0], c[1]) for c in golden[sc]}
    assert ("csk_co_block_step_f32", "") in names("default") and ("csk_co_block_step_f32", "") not in names("fusion_off")
    assert ("csk_gcn_stage_splitk_f32", "") in names("latency")
    assert any(c[0] == "csk_tcn_step_f32" and c[24] > 1 for c in golden["latency"])                   # ksplit
    assert ("csk_tcn_step_bf16x3", "tcn_step_split_launch") in names("bf16x3_step")
    assert all(c[1] == "tcn_step_launch" for sc in golden for c in golden[sc] if c[0] == "csk_tcn_step_f32")
    assert {c[21] for c in golden["default"] if c[0] == "csk_tcn_step_f32"} == {0, 1, 2}              # residual mode
    assert {c[21] for c in golden["block"] if c[0] == "csk_tcn_step_f32"} == {2}
    heads = [c for c in golden["default"] if c[0] == "csk_co_head_step_f32"]
    assert any(c[2] is None for c in heads) and any(c[7] is None for c in heads) and any(c[7] is not None for c in heads)
    assert len({c[12] for c in golden["default"] if c[0] == "csk_gcn_stage_f32"}) > 3                 # slot runs of 1..8 frames


def _scan(s0, r, delay, stride):
    """The scan the closed form replaced, and the count that stood next to it."""
    first = next((s for s in range(s0, s0 + r) if s >= delay and (s - delay) % stride == 0), None)
    return (None, 0) if first is None else (first, (s0 + r - 1 - first) // stride + 1)


def test_emissions_equals_the_scan():
    for s0 in range(41):
        for r in range(1, 9):
            for delay in (0, 4, 8):
                for stride in (1, 2):
                    got = co.emissions(s0, r, delay, stride)
                    assert got == _scan(s0, r, delay, stride), (s0, r, delay, stride)
                    emitting = [s for s in range(s0, s0 + r) if s >= delay and (s - delay) % stride == 0]
                    assert got == ((emitting[0], len(emitting)) if emitting else (None, 0))


@pytest.mark.parametrize("depths", [(5,), (8,), (12,), (16,), (12, 16), (5, 8), (8, 12, 16), (5, 8, 12, 16)])
def test_ring_runs_cover_the_frames_once_and_never_wrap(depths):
    for s0 in range(41):
        for r in range(1, 9):
            runs = list(co.ring_runs(s0, r, *depths))
            covered = [s + j for s, run in runs for j in range(run)]
            assert covered == list(range(s0, s0 + r)), (s0, r, runs)
            for s, run in runs:
                assert run >= 1 and all(s % d + run <= d for d in depths), (s0, r, depths, s, run)
            # as few runs as the rings allow: each run but the last ends on a multiple of some depth
            assert all(any((s + run) % d == 0 for d in depths) for s, run in runs[:-1]), (s0, r, runs)
