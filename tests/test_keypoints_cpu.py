"""Kinetics keypoint intake, the parts that need no GPU: the fixture the reference's own feeder wrote
(tests/golden/g15_keypoints.npz, make_golden_keypoints.py) is admissible and holds the cases it must, the numpy oracle
(tests/keypoint_oracle.py) reproduces it bit for bit and has teeth, and the C ABI and the host layer refuse what they must."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import _bootstrap
from tests import keypoint_oracle as ko
from tests.helpers import GOLDEN

pkg = _bootstrap.load()
keypoints = pkg.keypoints
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("csk_select_people_f32", "csk_select_people_frames_f32")
SAMPLES = (0, 1, 2)


@pytest.fixture(scope="module")
def golden():
    d = np.load(os.path.join(GOLDEN, "g15_keypoints.npz"))
    return {k: d[k] for k in d.files}


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _present(frame):
    """Indices of the people of a (P, V, 3) frame with any non-zero score."""
    return [p for p in range(frame.shape[0]) if frame[p, :, 2].any()]


# ---- the fixture -------------------------------------------------------------------------------------------------------
def test_fixture_is_admissible(golden):
    """In every frame the score sums of the people with any non-zero score are pairwise distinct: ties occur only among
    all-zero people, where every order gives the same output.  All values are multiples of 1/1024 in [0, 1]."""
    for i in SAMPLES:
        k, want = golden[f"s{i}/k"], golden[f"s{i}/want"]
        assert k.dtype == want.dtype == np.float32 and k.shape[1:] == (5, 18, 3) and want.shape == (3, k.shape[0], 18, 2)
        assert k.min() >= 0.0 and k.max() <= 1.0 and np.array_equal(k * 1024, np.round(k * 1024))
        sums = ko.score_sums(k)
        for t in range(k.shape[0]):
            present = _present(k[t])
            assert len({float(sums[t, p]) for p in present}) == len(present), (i, t)
            assert present == list(range(len(present)))                  # OpenPose fills the leading slots


def test_fixture_holds_the_cases_the_intake_can_get_wrong(golden):
    counts, best_slots, swaps, zero_score_xy, neg_zero, x_half = set(), set(), 0, 0, 0, 0
    for i in SAMPLES:
        k, want = golden[f"s{i}/k"], golden[f"s{i}/want"]
        sums = ko.score_sums(k)
        top = []
        for t in range(k.shape[0]):
            present = _present(k[t])
            counts.add(len(present))
            order = ko.order_people(sums[t])
            top.append(tuple(order[:2]) if len(present) >= 2 else None)
            if present:
                best_slots.add(order[0])
            zero_score_xy += int(((k[t, :, :, 2] == 0) & (k[t, :, :, 0] != 0) & (k[t, :, :, 1] != 0)).sum())
            x_half += int(((k[t, :, :, 0] == 0.5) & (k[t, :, :, 2] != 0)).sum())
        swaps += sum(1 for a, b in zip(top, top[1:]) if a and b and a == b[::-1])
        neg_zero += int((np.signbit(want[1]) & (want[1] == 0)).sum())
        assert not (np.signbit(want[0]) & (want[0] == 0)).any()              # x - 0.5 at x == 0.5 is +0.0
    assert counts >= {0, 1, 2, 3, 5} and best_slots & {3, 4} and swaps >= 2
    assert zero_score_xy >= 10 and neg_zero >= 3 and x_half >= 3


# ---- the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", SAMPLES)
def test_oracle_equals_the_reference_bit_for_bit(golden, i):
    got = ko.select_people_clip(golden[f"s{i}/k"][None])[0]
    assert got.dtype == np.float32 and np.array_equal(_bytes(got), _bytes(golden[f"s{i}/want"]))


def test_oracle_has_teeth(golden):
    """Each wrong step changes the bytes: no ranking, the clip's order in place of the frame's, 0.5 - y, no zeroing."""
    k, want = golden["s0/k"], golden["s0/want"]
    unranked = np.where(k[:, :2, :, 2] == 0, np.float32(0), k[:, :2, :, 0] - np.float32(0.5)).transpose(0, 2, 1)      # slots 0 and 1
    assert unranked.shape == want[0].shape and not np.array_equal(unranked, want[0])
    whole_clip = ko.order_people(ko.score_sums(k).sum(axis=0))[:2]
    assert any(ko.order_people(s)[:2] != whole_clip for s in ko.score_sums(k))
    flipped = np.where(k[..., 2] == 0, np.float32(0), np.float32(0.5) - k[..., 1])
    assert not np.signbit(flipped[flipped == 0]).any() and np.signbit(want[1][want[1] == 0]).any()
    kept = ko.select_people_clip(k[None])[0]
    undetected = (k[..., 2] == 0) & k[..., 2].any(axis=-1, keepdims=True)         # score 0 on a person who is there
    assert not kept[:2][:, kept[2] == 0].any() and undetected.sum() >= 10 and (k[..., :2][undetected] != 0).all()


def test_oracle_tie_nan_and_negative_zero_rules():
    assert ko.order_people(np.array([1.0, 2.0, 2.0, 0.5])) == [1, 2, 0, 3]
    assert ko.order_people(np.array([np.nan, 1.0, np.nan, -np.inf, np.inf])) == [4, 1, 3, 0, 2]
    assert ko.order_people(np.array([-0.0, 0.0, -1.0])) == [0, 1, 2]
    k = np.zeros((1, 18, 3), dtype=np.float32)
    k[0, :, :2] = 0.75
    k[0, 0, 2], k[0, 1, 2], k[0, 2, 2] = -0.0, np.nan, 0.5
    out = ko.select_frame(k, 1)
    assert out[0, 0, 0] == 0 and not np.signbit(out[0, 0, 0]) and np.signbit(out[2, 0, 0])       # -0.0 counts as 0 and is kept
    assert out[0, 1, 0] == 0.25 and np.isnan(out[2, 1, 0]) and out[1, 2, 0] == -0.25


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cskel.h")).read()
    declared = set(re.findall(r"\b(csk_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(pkg.native.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in pkg.native.SIGNATURES and hasattr(lib, name), name
        assert len(pkg.native.SIGNATURES[name]) == 8
    assert pkg.native.lib().csk_abi_version() == 16 and "#define CSK_ABI_VERSION 16" in hdr
    assert os.path.exists(os.path.join(ROOT, "continual-skeletons_amd", "csrc", "keypoints.hip"))


def test_entries_refuse_bad_arguments_before_any_launch():
    """Every refusal is decided on the host: the code and a message, and no GPU is needed to get them."""
    lib = pkg.native.lib()
    buf = (ctypes.c_float * 64)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 128          # never dereferenced: every call returns before a launch

    def clip(k=a, out=b, n=1, t=2, p=5, v=18, m=2):
        return lib.csk_select_people_f32(k, out, n, t, p, v, m, None)

    assert clip(k=None) == -1 and b"null pointer" in lib.csk_last_error()
    assert clip(out=None) == -1 and b"null pointer" in lib.csk_last_error()
    assert clip(out=a) == -1 and b"out must not be k" in lib.csk_last_error()
    for dims in (dict(n=0), dict(t=0), dict(p=0), dict(v=0), dict(m=0), dict(n=-1)):
        assert clip(**dims) == -1 and b"bad dims" in lib.csk_last_error(), dims
    for dims in (dict(p=9, m=2), dict(p=2, m=3), dict(p=8, m=9)):
        assert clip(**dims) == -2 and b"M <= P <= 8" in lib.csk_last_error(), dims
    assert clip(v=65) == -2 and b"V <= 64" in lib.csk_last_error()

    src, dst = (ctypes.c_void_p * 8)(*([a] * 8)), (ctypes.c_void_p * 8)(*[b + 512 * i for i in range(8)])

    def frames(s=src, d=dst, r=1, n=1, p=5, v=18, m=2):
        return lib.csk_select_people_frames_f32(s, d, r, n, p, v, m, None)

    assert frames(s=None) == -1 and frames(d=None) == -1 and b"null pointer" in lib.csk_last_error()
    for r in (0, 9, -3):
        assert frames(r=r) == -2 and b"1..8 frames" in lib.csk_last_error()
    for dims in (dict(n=0), dict(p=0), dict(v=0), dict(m=0)):
        assert frames(**dims) == -1 and b"bad dims" in lib.csk_last_error(), dims
    for dims in (dict(p=9), dict(p=1, m=2)):
        assert frames(**dims) == -2 and b"M <= P <= 8" in lib.csk_last_error(), dims
    assert frames(v=65) == -2 and b"V <= 64" in lib.csk_last_error()
    assert frames(s=(ctypes.c_void_p * 8)(a, None), r=2) == -1 and b"null frame" in lib.csk_last_error()
    assert frames(d=src) == -1 and b"buffer of its own" in lib.csk_last_error()
    assert frames(d=(ctypes.c_void_p * 8)(b, b), r=2) == -1 and b"buffer of its own" in lib.csk_last_error()
    with pytest.raises(RuntimeError, match="V <= 64"):
        pkg.native.check(clip(v=65), "csk_select_people_f32")


# ---- the host layer ------------------------------------------------------------------------------------------------------
def _models():
    a25, a18 = pkg.ntu_graph().A, pkg.kinetics_graph().A
    return [pkg.StGcn(a18, (3, 20, 18, 2)), pkg.AGcn(a18, (3, 20, 18, 2)), pkg.STr(a18, (3, 20, 18, 2)),
            pkg.CoStGcn(a18, (3, 300, 18, 2)), pkg.CoAGcn(a18, (3, 300, 18, 2)), pkg.CoSTr(a25, (3, 300, 25, 2)),
            pkg.StGcnMod(a18, (3, 100, 18, 2)), pkg.CoStGcnMod(a18, (3, 100, 18, 2))]


def test_set_keypoint_intake_host_rules():
    for net in _models():
        assert net.keypoint_intake is False and "keypoint_intake" not in net.__dict__           # the class attribute says so
        assert not [k for k in net.__dict__ if k.startswith("_kp")]
        assert keypoints.set_keypoint_intake(net) is net and net.keypoint_intake is True and net.stage("keypoints").people == 5
        assert keypoints.set_keypoint_intake(net, 8) is net and net.stage("keypoints").people == 8
        assert keypoints.set_keypoint_intake(net, people_in=2) is net and net.stage("keypoints").people == 2
        for bad in (1, 9, 0, -1, 2.0, None, True):
            with pytest.raises(ValueError, match="people_in"):
                keypoints.set_keypoint_intake(net, bad)
        assert net.stage("keypoints").people == 2 and net.stage("keypoints").fed_shape(7) == (7, 2, net.input_shape[2], 3)
        assert net.stage("keypoints").fed_shape(7, 4) == (7, 4, 2, net.input_shape[2], 3)
        assert keypoints.set_keypoint_intake(net, enabled=False) is net and net.keypoint_intake is False
    for cls in (pkg.StGcn, pkg.CoStGcn):
        with pytest.raises(ValueError, match="C = 2"):
            keypoints.set_keypoint_intake(cls(pkg.kinetics_graph().A, (2, 300, 18, 2)))
    for wrong in (pkg.GraphConvolution(3, 8, pkg.ntu_graph().A), None, "StGcn"):
        with pytest.raises(TypeError):
            keypoints.set_keypoint_intake(wrong)
    # independent of the other two pre-passes: all three can be on
    net = pkg.set_input_modality(pkg.set_pre_normalization(keypoints.set_keypoint_intake(pkg.CoStGcn(pkg.kinetics_graph().A, (3, 300, 18, 2)))), "bone")
    assert net.keypoint_intake and net.pre_normalization and net.input_modality == "bone"


def test_the_names_live_in_the_module_only():
    for name in ("set_keypoint_intake", "select_people_clip", "KeypointIntake"):
        assert hasattr(keypoints, name) and not hasattr(pkg, name)
    src = open(os.path.join(ROOT, "continual-skeletons_amd", "keypoints.py")).read()
    assert not re.search(r"^\s*(from|import)\s+\S*oracle", src, re.M) and "oracle" not in src


def _stepped(frames):
    net = pkg.CoStGcn(pkg.kinetics_graph().A, (3, 300, 18, 2))
    net._ctr = (ctypes.c_int64 * 22)()
    net._n, net._xin0 = 2, types.SimpleNamespace(device="cpu")     # stands for a bound slab (binding needs a device)
    net.stage("keypoints").bind = lambda n, device, max_cycle: None
    net._frames = frames
    return net


def test_a_model_that_has_stepped_refuses_the_switch():
    net = _stepped(0)
    keypoints.set_keypoint_intake(net)                      # frame counter 0: allowed
    net._frames = 8
    keypoints.set_keypoint_intake(net)                      # no change: allowed
    for change in (dict(enabled=False), dict(people_in=6)):
        with pytest.raises(RuntimeError, match=r"clean_state\(\)"):
            keypoints.set_keypoint_intake(net, **change)
    assert net.keypoint_intake is True and net.stage("keypoints").people == 5


def test_stream_shards_validate_every_shard_before_switching_any():
    shards = object.__new__(pkg.parallel.StreamShards)
    shards.models = [_stepped(0), _stepped(8)]
    with pytest.raises(RuntimeError, match=r"clean_state\(\)"):
        keypoints.set_keypoint_intake(shards)
    assert [m.keypoint_intake for m in shards.models] == [False, False]
    shards.models = [_stepped(0), pkg.CoStGcn(pkg.kinetics_graph().A, (2, 300, 18, 2))]
    with pytest.raises(ValueError, match="C = 2"):
        keypoints.set_keypoint_intake(shards)
    shards.models = [_stepped(0), pkg.GraphConvolution(3, 8, pkg.ntu_graph().A)]
    with pytest.raises(TypeError):
        keypoints.set_keypoint_intake(shards)
    shards.models = [_stepped(0), _stepped(0)]
    with pytest.raises(ValueError, match="people_in"):
        keypoints.set_keypoint_intake(shards, 9)
    assert shards.models[0].keypoint_intake is False
    assert keypoints.set_keypoint_intake(shards, 6) is shards
    assert [(m.keypoint_intake, m.stage("keypoints").people) for m in shards.models] == [(True, 6)] * 2


def test_cpu_tensors_and_wrong_shapes_are_refused_on_the_host():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        keypoints.select_people_clip(torch.zeros(1, 2, 5, 18, 3))
    net = keypoints.set_keypoint_intake(pkg.CoStGcn(pkg.kinetics_graph().A, (3, 300, 18, 2)).eval())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.forward_step(torch.zeros(2, 5, 18, 3))
    with pytest.raises(RuntimeError, match="keypoint history shape"):
        net._check_prime(torch.zeros(2, 3, 80, 18, 2))
