"""The unpadded "*" models without a GPU: the composed oracle (tests/mod_oracle.py) against the reference's own StGcnMod
(tests/golden/g15_stgcn_mod.npz), the step protocol against the clip form, the geometry derived from the layer table, the native
executor's launches for a CoStGcnMod against the Python engine's, and the weight image of the valid Winograd form."""
import json
import os
import re
import shutil
import subprocess

import pytest
import torch

import _bootstrap
from oracle import stgcn_oracle as o
from tests import mod_oracle as mo
from tests import trace_fixture as tf
from tests.helpers import max_err

pkg = _bootstrap.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- oracle against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["ntu", "kin"])
def test_g15_composed_oracle_equals_the_reference_stgcn_mod(tag):
    """The tolerance of tests/test_oracle_golden.py::test_g6_full_stgcn (1e-4) on logits and on the layer 1 / 5 / 8 / 10 taps."""
    a, sd, x = mo.g15(tag)
    assert sum(v.numel() for k, v in sd.items() if "running" not in k and "num_batches" not in k) == int(a["nparams"])
    taps = {}
    with torch.no_grad():
        logits = mo.stgcn_mod_forward(x, sd, taps=taps)
    assert max_err(logits, a["logits"]) <= 1e-4
    for i in (1, 5, 8, 10):
        assert tuple(taps[f"layer{i}"].shape) == tuple(a[f"layer{i}_shape"])
        assert max_err(taps[f"layer{i}"].reshape(-1)[::97], a[f"layer{i}_sub"]) <= 1e-4
    assert tuple(taps["layer10"].shape)[2] == x.shape[2] - 80


def test_step_oracle_equals_clip_oracle_frame_for_frame():
    """tests/test_st_gcn_mod.py:66-90 of the reference: emission s of the stepped stack is the clip stack's frame s - 80; nothing
    is emitted before frame 80."""
    a, sd, x = mo.g15("ntu")
    with torch.no_grad():
        clip = mo.stgcn_mod_features(x, sd)                                       # (N * M, 256, 8, V)
        net = mo.CoStGcnModOracle(sd, pool_size=4, pool_padding=0)
        feats = [net.features_step(x[:, :, s]) for s in range(x.shape[2])]
    assert all(f is None for f in feats[:80]) and all(f is not None for f in feats[80:])
    for s in range(80, x.shape[2]):
        assert max_err(feats[s], clip[:, :, s - 80]) <= 1e-5, s


# ---- geometry ----------------------------------------------------------------------------------------------------------------
def test_geometry_is_derived_from_the_layer_table():
    co, models = pkg.continual, pkg.models
    assert co.co_geometry() == co.co_geometry(3) == (153, 76, 4) == o.co_stgcn_geometry()
    assert co.co_geometry(3, unpadded=True) == (81, 0, 1) == mo.mod_geometry()
    assert models.layer_table(3) == o.layer_table(3)
    assert models.layer_table(3, unpadded=True) == mo.mod_layer_table(3)
    net = pkg.CoStGcnMod(pkg.ntu_graph().A)
    assert (net.receptive_field, net.padding, net.stride, net.delay) == (81, 0, 1, 0)
    assert (net.pool_size, net.pool_padding) == (220, 0) == mo.mod_pool_defaults(300)
    assert [b.delay for b in net.layers.values()] == [8] * 10 and [b.stride for b in net.layers.values()] == [1] * 10
    assert net._cum_delays()[10] == 80 and net._ready_age() == 80 + 219 + 1
    pad = pkg.CoStGcn(pkg.ntu_graph().A)
    assert (pad.receptive_field, pad.padding, pad.stride, pad.pool_size, pad.pool_padding) == (153, 76, 4, 75, 19)


def test_state_dict_keys_are_the_references_and_map():
    a, sd, _ = mo.g15("ntu")
    A = pkg.ntu_graph().A
    clip = pkg.StGcnMod(A, (3, 88, 25, 2), 60)
    assert list(clip.state_dict().keys()) == [str(k) for k in a["sd_keys"]]
    clip.load_state_dict(sd, strict=True)
    co = pkg.CoStGcnMod(A, (3, 88, 25, 2), 60)
    ref_co = pkg.CoStGcn(A, (3, 88, 25, 2), 60)
    assert list(co.state_dict().keys()) == list(ref_co.state_dict().keys())       # the continual container layout (g9_key_map)
    co.load_state_dict(co.map_state_dict(clip.state_dict()), strict=True)
    back = {k.replace("0.1.", "").replace("0.0.residual", "residual"): v for k, v in co.state_dict().items()}
    assert all(torch.equal(back[k], v) for k, v in clip.state_dict().items())


def test_short_clips_and_unbuilt_modes_raise():
    A = pkg.ntu_graph().A
    clip = pkg.StGcnMod(A, (3, 88, 25, 2), 60).eval()
    with pytest.raises(ValueError, match="T >= 81"):
        clip(torch.zeros(1, 3, 80, 25, 2))                                       # raised before the device check: nothing launched
    with pytest.raises(NotImplementedError):
        clip.set_latency_mode(4)
    co = pkg.CoStGcnMod(A, (3, 88, 25, 2), 60).eval()
    with pytest.raises(NotImplementedError):
        co.set_latency_mode(8)
    with pytest.raises(NotImplementedError):
        pkg.set_step_precision(co, "bf16x3")
    assert all(b.step_precision == "f32" and b.split_k == 0 for b in co.layers.values())
    for name in ("AGcnMod", "CoAGcnMod", "STrMod", "CoSTrMod"):
        assert not hasattr(pkg, name)


# ---- weight fold -------------------------------------------------------------------------------------------------------------
def test_valid_form_streams_the_padded_forms_weight_image():
    A = pkg.ntu_graph().A
    torch.manual_seed(3)
    padded = pkg.SpatioTemporalBlock(64, 64, A).eval()
    valid = pkg.SpatioTemporalBlock(64, 64, A, temporal_padding=0).eval()
    with torch.no_grad():
        for prm in padded.tcn.parameters():
            prm.copy_(torch.randn_like(prm))
        padded.tcn.bn.running_var.copy_(torch.rand(64) + 0.5)
    valid.load_state_dict(padded.state_dict(), strict=True)
    wp, wv = padded._fold()["w_wino"], valid._fold()["w_wino"]
    assert wp.shape == wv.shape == (12, 64, 64) and wp.dtype == wv.dtype == torch.float32
    assert wp.numpy().tobytes() == wv.numpy().tobytes()
    s, _ = pkg.fold.bn_affine(valid.tcn.bn.weight.detach(), valid.tcn.bn.bias.detach(), valid.tcn.bn.running_mean, valid.tcn.bn.running_var)
    assert torch.equal(wv, pkg.fold.pack_conv_weight_wino(valid.tcn.t_conv.weight.detach(), s))


# ---- executor trace ----------------------------------------------------------------------------------------------------------
# Both engines in one reduced form: per launch the layer, the ring depths and slots, the run lengths and emission counts -- what
# the delay decides.  (Operand pointers are not compared: the two recorders name them differently, and they do not move.)
N_, M_, V_, P_, POOL, POOL_PAD = 1, 2, 25, 52, 6, 2          # the shape of tests/executor_trace_main.cpp
CH = [3, 64, 64, 64, 64, 128, 128, 128, 256, 256, 256]       # channels in front of layer i / behind layer i - 1
CYCLES = ([1, 3, 4] * 13)[:38]                               # 12 rounds of 8 frames, then 1 + 3: 100 frames


def _loc(ptr):
    """'<ring name>+<bytes>' -> (layer the ring belongs to as an OUTPUT or y ring: 0 = the input ring, slot)."""
    name, off = ptr.rsplit("+", 1)
    m = re.fullmatch(r"(?:L(\d+)|layer(\d+))\.(y|out)", name)
    if name == "xin0":
        layer, kind = 0, "out"
    else:
        layer, kind = (int(m.group(1)) + 1 if m.group(1) is not None else int(m.group(2))), m.group(3)
    c = CH[layer]
    assert int(off) % (c * P_ * 4) == 0
    return layer, kind, int(off) // (c * P_ * 4)


def _reduce(name, a):
    """One launch (arguments in the order of include/cskel.h, ell_cnt as ONE entry) -> comparable tuple."""
    if name == "csk_gcn_stage_f32":
        return ("gcn", _loc(a[0]), _loc(a[1]), a[10], a[11], a[12])
    if name == "csk_tcn_step_f32":
        return ("tcn", _loc(a[0])[0], a[1], a[2], a[3], a[4], a[7], a[8], a[9], a[13], a[14], a[19], a[22])
    if name == "fused_block":
        return ("fused", _loc(a[11])[0], _loc(a[0])[:2], a[1], a[2], a[12], a[13], a[16], a[17], a[19], a[20])
    if name == "csk_co_head_step_f32":
        return ("head", _loc(a[0]), a[10], a[11], a[12], a[13])
    raise AssertionError(name)


def _native_trace():
    hipcc = shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc")
    if not hipcc:
        pytest.skip("no hipcc to build the trace program with")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "executor_trace_mod")
        subprocess.check_call([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "tests"), "-Wno-unused-function",
                               os.path.join(ROOT, "continual-skeletons_amd", "csrc", "executor.hip"),
                               os.path.join(ROOT, "tests", "executor_trace_mod_main.cpp"), "-o", exe])
        return json.loads(subprocess.check_output([exe]))


def _native_reduced(calls):
    out = []
    for c in calls:
        name, a = c[0], c[1:]
        if name == "csk_input_norm_frames_f32":
            r = (len(a) - 9) // 2
            out.append(("norm", r, [_loc(p)[2] for p in a[r: 2 * r]]))
        elif name == "fused":
            n = a[0]
            for k in range(n):
                b = a[4 + 24 * k: 4 + 24 * (k + 1)]
                out.append(_reduce("fused_block", b[:8] + [b[8:11]] + b[11:]))
        elif name == "cycle":
            out.append(("cycle", a[0], a[1], a[2] if a[3] else None, a[3], a[4], a[5:]))
        elif name in ("csk_gcn_stage_f32",):
            out.append(_reduce(name, a[:6] + [a[6:9]] + a[9:]))
        else:
            out.append(_reduce(name, a))
    return out


def _python_reduced():
    net = pkg.CoStGcnMod(pkg.ntu_graph().A, pool_size=POOL, pool_padding=POOL_PAD).eval()
    net.use_native_plan = False
    net.set_max_cycle(8)
    calls, out, r_of = tf._drive_model(pkg, net, CYCLES, flush=False), [], iter(CYCLES)
    for c in calls:
        name, a = c[0], c[2:]
        if name == "csk_input_norm_frames_f32":
            out.append(("norm", a[2], [_loc(p)[2] for p in a[1]]))
        elif name == "csk_co_block_step_f32":
            out.append(_reduce("fused_block", a))
        elif name == "return":                       # (slot, n_feat, n_logits) of the cycle; the counters follow from the launches
            out.append(("return", next(r_of), a[0] if a[1] else None, a[1], a[2]))
        elif name == "counters":
            out.append(("counters", a))
        else:
            out.append(_reduce(name, a))
    return out


def test_native_plan_issues_the_python_engines_launches_for_a_mod_stack():
    """100 frames from a clean state in cycles of 1, 3 and 4: launch for launch the same rings, slots, runs and emission counts;
    per cycle the same features / logits returned; at the end the same counters.  The fused stack call of the executor is compared
    block by block with the Python engine's one-block calls (the same kernels, include/cskel.h: csk_co_stack_step_f32)."""
    native = _native_trace()
    assert native["refused"] == [["set_delays", -1, -1]]
    got, want = _native_reduced(native["mod"]), _python_reduced()
    counters = None
    py = []
    for w in want:                                   # the Python recorder's per-cycle "return" <-> the executor's "cycle" record
        if w[0] == "counters":
            counters = w[1]
        else:
            py.append(w)
    nat = []
    for g in got:
        if g[0] == "cycle":
            assert g[2] == 0
            nat.append(("return", g[1], g[3], g[4], g[5]))
            last = g[6]
        else:
            nat.append(g)
    for i, (g, w) in enumerate(zip(nat, py)):
        assert g == w, f"launch {i} differs\n native {g}\n python {w}"
    assert len(nat) == len(py)
    assert list(last) == list(counters)
    kinds = {g[0] for g in nat}
    assert {"norm", "gcn", "tcn", "fused", "head", "return"} <= kinds
    # the first layer-10 feature comes with frame 80, one per frame from there on; logits from the (POOL - POOL_PAD)-th feature
    feats = sum(g[3] for g in nat if g[0] == "return")
    assert feats == 20 and last[0] == 100 and last[1] == 20
    assert sum(g[4] for g in nat if g[0] == "return") == 20 - (POOL - POOL_PAD - 1)
