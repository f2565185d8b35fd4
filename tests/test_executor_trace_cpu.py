"""The native step executor (csrc/executor.hip) issues the launches it issued before its fused paths and its step arithmetic
were gathered into one copy each: tests/executor_trace_main.cpp links the executor against recording stubs of every entry it
calls and prints every call of seven scenarios with every argument; tests/golden/executor_trace.json is what the executor of
the commit before that change printed.  The C counterpart of tests/test_continual_trace_cpu.py.  No GPU."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "executor_trace.json")
SCENARIOS = ("default", "fusion_off", "latency", "agcn", "ring4", "lone_block", "fail_at_k")


def _hipcc():
    return shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def trace(tmp_path_factory):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc to build the trace program with")
    exe = str(tmp_path_factory.mktemp("executor_trace") / "executor_trace")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "continual-skeletons_amd", "csrc", "executor.hip"),
                           os.path.join(ROOT, "tests", "executor_trace_main.cpp"), "-o", exe])
    return json.loads(subprocess.check_output([exe]))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_scenarios(golden, trace):
    assert sorted(golden) == sorted(SCENARIOS) == sorted(trace)


@pytest.mark.parametrize("name", SCENARIOS)
def test_launch_trace_is_the_recorded_one(golden, trace, name):
    got, want = trace[name], golden[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: call {i} differs\n got  {g}\n want {w}"
    assert len(got) == len(want), f"{name}: {len(got)} calls, recorded {len(want)}"


def test_the_scenarios_reach_every_launch_path(trace):
    """What the comparison above is worth: fused calls of one block and of runs, none with fusion off, both split-K entries,
    the adaptive graph conv pair, wrapped slot runs, head steps with and without logits, the refused 8-frame cycle."""
    def names(sc):
        return {c[0] for c in trace[sc]}
    assert {c[1] for c in trace["default"] if c[0] == "fused"} == {1, 3} and "fused" not in names("fusion_off")
    assert {c[1] for c in trace["lone_block"] if c[0] == "fused"} == {1}
    assert all(c[17] == 1 for c in trace["lone_block"] if c[0] == "fused")          # identity gcn_residual: a lone stackable block
    assert "csk_gcn_stage_splitk_f32" in names("latency") and "fused" not in names("latency")
    assert any(c[0] == "csk_tcn_step_f32" and c[23] > 1 for c in trace["latency"])                  # ksplit
    assert "csk_agcn_embed_attention_f32" in names("agcn") and "fused" not in names("agcn")
    assert len({c[13] for c in trace["default"] if c[0] == "csk_gcn_stage_f32"}) > 3                # slot runs of 1..8 frames
    heads = [c for c in trace["default"] if c[0] == "csk_co_head_step_f32"]
    assert {c[14] for c in heads} == {0, 1}                                                         # emit
    refused = [c for c in trace["ring4"] if c[0] == "cycle" and c[2] != 0]
    assert [c[1:3] for c in refused] == [[8, -1]] and "error" in names("ring4")


def test_a_failing_launch_leaves_no_trace(trace):
    """Every launch k of one cycle failing in turn: the stub's return code comes back, the counters are byte for byte what was
    passed in, and the launches before k are the unfailing run's first k."""
    fails = trace["fail_at_k"]
    assert len(fails) == 18 and [c[1] for c in fails] == list(range(18))
    assert all(c[2:] == [700, 1, 1, c[1]] for c in fails)
