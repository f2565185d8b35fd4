"""Pre-normalisation of raw skeleton frames, the parts that need no GPU: the fixture the reference's own function wrote
(tests/golden/g14_prenorm.npz, make_golden_prenorm.py) is admissible, the numpy oracle (tests/prenorm_oracle.py) reproduces
it and has teeth, its step form equals its clip form, and the C ABI and the host layer refuse what they must."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import _bootstrap
from tests import prenorm_oracle as po
from tests.helpers import GOLDEN

pkg = _bootstrap.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("csk_prenorm_f32", "csk_prenorm_frames_f32")
SHAPES = {"ntu": (3, 3, 6, 25, 2), "kin": (2, 3, 5, 18, 1)}
TAGS = tuple(SHAPES)


@pytest.fixture(scope="module")
def golden():
    d = np.load(os.path.join(GOLDEN, "g14_prenorm.npz"))
    return {k: d[k] for k in d.files}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the fixture -------------------------------------------------------------------------------------------------------
def test_fixture_is_admissible(golden):
    """Shapes, the three kinds of null data the issue asks for, and nothing the reference's padding step would touch: no
    leading or trailing null frame of a present person and no empty sample."""
    for tag in TAGS:
        x, want = golden[f"{tag}/x"], golden[f"{tag}/want"]
        assert x.shape == want.shape == SHAPES[tag] and x.dtype == want.dtype == np.float32
        assert np.abs(want).max() <= 8.0
        for n in range(x.shape[0]):
            assert x[n].any()
            for m in range(x.shape[4]):
                person = x[n, :, :, :, m]
                if person.any():
                    assert person[:, 0].any() and person[:, -1].any(), (tag, n, m)
    x = golden["ntu/x"]
    assert not x[1, :, :, :, 1].any() and x[1, :, :, :, 0].all()                 # an absent second person
    assert not x[0, :, 2, :, 1].any() and x[0, :, 3:, :, 1].all() and x[0, :, :2, :, 1].all()     # a null frame that is not trailing
    assert not x[2, :, 3, 7, 0].any() and x[2, :, 3, 6, 0].all()                 # a null joint of the main body
    null = po.null_mask(x.transpose(0, 2, 1, 3, 4))                             # (N, T, V, M)
    assert int(null.sum()) == 6 * 25 + 25 + 1
    assert not golden["ntu/want"].transpose(0, 2, 1, 3, 4)[np.broadcast_to(null[:, :, None], (3, 6, 3, 25, 2))].any()


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_is_well_conditioned(golden, tag):
    """Both latched angles of every sample in [20, 160] degrees: near 0 or pi the reference's fp32 unit vector moves the
    angle by up to ~3.5e-4 rad and the fixture would measure that, not the arithmetic."""
    ang = po.latched_angles(golden[f"{tag}/x"])
    assert ang.shape == (SHAPES[tag][0], 2) and ang.min() >= 20.0 and ang.max() <= 160.0, ang


# ---- the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_oracle_reproduces_the_reference(golden, tag):
    """Within 1e-6 absolute (one fp32 ulp at |want| ~ 4.9 is 4.8e-7): the reference takes the unit vector in fp32, the
    oracle and the device in fp64, so bit equality is not the contract."""
    got = po.pre_normalize_clip(golden[f"{tag}/x"])
    err = float(np.abs(got.astype(np.float64) - golden[f"{tag}/want"]).max())
    print(f"{tag}: max |oracle - reference| = {err:.3e}, |want| max {np.abs(golden[f'{tag}/want']).max():.3f}")
    assert got.dtype == np.float32 and err <= 1e-6


def _mutant(x, kind):
    """The oracle with one step wrong."""
    out = np.empty_like(x)
    for n in range(x.shape[0]):
        rz, rx, _, _ = po.latch(x[n, :, 1 if kind == "frame1" else 0])
        if kind == "no_rz":
            rz = np.eye(3)
        elif kind == "no_rx":
            rx = np.eye(3)
        elif kind == "rz_transposed":
            rz = rz.T
        for t in range(x.shape[2]):
            out[n, :, t] = po.normalise_frame(x[n, :, t], rz, rx, use_mask=kind != "no_mask",
                                              centre_of=x[n, :, 0] if kind == "centre_frame0" else None)
    return out


@pytest.mark.parametrize("kind", ["no_rz", "no_rx", "rz_transposed", "centre_frame0", "frame1", "no_mask"])
def test_oracle_has_teeth(golden, kind):
    """Each wrong step moves the result by more than 1e-2 on both tags (no_mask: on ntu, the tag with null data) -- four
    orders of magnitude above the tolerance of the parity tests."""
    for tag in TAGS:
        if kind == "no_mask" and tag == "kin":
            continue
        dist = float(np.abs(_mutant(golden[f"{tag}/x"], kind).astype(np.float64) - golden[f"{tag}/want"]).max())
        print(f"{tag} {kind}: {dist:.3f}")
        assert dist > 1e-2, (tag, kind, dist)


@pytest.mark.parametrize("tag", TAGS)
def test_step_oracle_equals_clip_oracle(golden, tag):
    x = golden[f"{tag}/x"]
    clip = po.pre_normalize_clip(x)
    assert np.array_equal(_bits(po.pre_normalize_steps(x)), _bits(clip))
    # a "first frame" at frame 3 of the last stream: from there on it is the clip oracle of x[:, :, 3:]; the others run on
    first = np.zeros(x.shape[:1] + x.shape[2:3], dtype=bool)
    first[:, 0] = first[-1, 3] = True
    steps = po.pre_normalize_steps(x, first)
    late = po.pre_normalize_clip(x[:, :, 3:])
    assert np.array_equal(_bits(steps[-1, :, 3:]), _bits(late[-1])) and np.array_equal(_bits(steps[-1, :, :3]), _bits(clip[-1, :, :3]))
    assert np.array_equal(_bits(steps[:-1]), _bits(clip[:-1])) and not np.array_equal(steps[-1, :, 3:], clip[-1, :, 3:])


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cskel.h")).read()
    declared = set(re.findall(r"\b(csk_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(pkg.native.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in pkg.native.SIGNATURES and hasattr(lib, name), name
    assert len(pkg.native.SIGNATURES["csk_prenorm_f32"]) == 11 and len(pkg.native.SIGNATURES["csk_prenorm_frames_f32"]) == 14
    assert pkg.native.lib().csk_abi_version() == 16
    assert pkg.pre_normalize_clip is pkg.prenorm.pre_normalize_clip and pkg.set_pre_normalization is pkg.prenorm.set_pre_normalization


def test_entries_refuse_bad_arguments_before_any_launch():
    """Every refusal is decided on the host: the code and a message, and no GPU is needed to get them."""
    lib = pkg.native.lib()
    buf = (ctypes.c_float * 64)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 128          # never dereferenced: every call returns before a launch

    def clip(x=a, out=b, n=1, t=2, v=25, m=1, j=(0, 1, 8, 4)):
        return lib.csk_prenorm_f32(x, out, n, t, v, m, *j, None)

    assert clip(x=None) == -1 and b"null pointer" in lib.csk_last_error()
    assert clip(out=None) == -1 and b"null pointer" in lib.csk_last_error()
    assert clip(out=a) == -1 and b"out must not be x" in lib.csk_last_error()
    for dims in (dict(n=0), dict(t=0), dict(v=0), dict(m=0), dict(n=-1)):
        assert clip(**dims) == -1 and b"bad dims" in lib.csk_last_error(), dims
    assert clip(v=1, j=(0, 0, 0, 0)) == -2 and b"V >= 2" in lib.csk_last_error()
    for j in ((25, 1, 8, 4), (0, -1, 8, 4), (0, 1, 25, 4), (0, 1, 8, 99)):
        assert clip(j=j) == -2 and b"outside [0, 25)" in lib.csk_last_error(), j

    src, dst = (ctypes.c_void_p * 8)(*([a] * 8)), (ctypes.c_void_p * 8)(*([b] * 8))
    rot, flags = (ctypes.c_double * 18)(), (ctypes.c_int32 * 4)()

    def frames(s=src, d=dst, r=1, rt=rot, fl=flags, n=1, v=25, m=1, j=(0, 1, 8, 4)):
        return lib.csk_prenorm_frames_f32(s, d, r, rt, fl, 1, n, v, m, *j, None)

    assert frames(s=None) == -1 and frames(d=None) == -1 and b"null pointer" in lib.csk_last_error()
    for r in (0, 9, -3):
        assert frames(r=r) == -2 and b"1..8 frames" in lib.csk_last_error()
    for dims in (dict(n=0), dict(v=0), dict(m=0)):
        assert frames(**dims) == -1 and b"bad dims" in lib.csk_last_error(), dims
    assert frames(v=1, j=(0, 0, 0, 0)) == -2 and b"V >= 2" in lib.csk_last_error()
    for j in ((0, 1, 8, 25), (-1, 1, 8, 4)):
        assert frames(j=j) == -2 and b"outside [0, 25)" in lib.csk_last_error(), j
    assert frames(rt=None) == -1 and b"has_rot" in lib.csk_last_error()
    assert frames(fl=None) == -1 and b"has_rot" in lib.csk_last_error()
    assert frames(s=(ctypes.c_void_p * 8)(a, None), r=2) == -1 and b"null frame" in lib.csk_last_error()
    assert frames(d=src) == -1 and b"buffer of its own" in lib.csk_last_error()
    with pytest.raises(RuntimeError, match="outside"):
        pkg.native.check(clip(j=(0, 1, 8, 25)), "csk_prenorm_f32")


# ---- the host layer ------------------------------------------------------------------------------------------------------
def _models():
    a25, a18 = pkg.ntu_graph().A, pkg.kinetics_graph().A
    return [pkg.StGcn(a25, (3, 20, 25, 2)), pkg.AGcn(a18, (3, 20, 18, 2)), pkg.STr(a25, (3, 20, 25, 2)),
            pkg.CoStGcn(a25, (3, 300, 25, 2)), pkg.CoAGcn(a18, (3, 300, 18, 2)), pkg.CoSTr(a25, (3, 300, 25, 2))]


def test_set_pre_normalization_host_rules():
    for net in _models():
        v = net.input_shape[2]
        assert net.pre_normalization is False and "pre_normalization" not in net.__dict__       # the class attribute says so
        assert not [k for k in net.__dict__ if k.startswith("_pn")]
        assert pkg.set_pre_normalization(net) is net and net.pre_normalization is True and net.stage("prenorm").joints == (0, 1, 8, 4)
        assert pkg.set_pre_normalization(net, True, zaxis=(2, 3), xaxis=[v - 1, 0]) is net and net.stage("prenorm").joints == (2, 3, v - 1, 0)
        for bad in (dict(zaxis=(0, v)), dict(xaxis=(-1, 4)), dict(zaxis=(0,)), dict(xaxis=(1.0, 2)), dict(zaxis=None)):
            with pytest.raises(ValueError):
                pkg.set_pre_normalization(net, True, **bad)
        assert net.stage("prenorm").joints == (2, 3, v - 1, 0)
        assert pkg.set_pre_normalization(net, False) is net and net.pre_normalization is False
    for cls in (pkg.StGcn, pkg.CoStGcn):
        with pytest.raises(ValueError, match="C = 2"):
            pkg.set_pre_normalization(cls(pkg.ntu_graph().A, (2, 300, 25, 2)))
    for wrong in (pkg.GraphConvolution(3, 8, pkg.ntu_graph().A), None, "StGcn"):
        with pytest.raises(TypeError):
            pkg.set_pre_normalization(wrong)
    # the modality is independent of the switch: both can be on, in either order
    net = pkg.set_input_modality(pkg.set_pre_normalization(pkg.CoStGcn(pkg.ntu_graph().A)), "bone_motion")
    assert net.pre_normalization and net.input_modality == "bone_motion"


def _stepped(frames):
    net = pkg.CoStGcn(pkg.ntu_graph().A)
    net._ctr = (ctypes.c_int64 * 22)()
    net._n, net._xin0 = 2, types.SimpleNamespace(device="cpu")     # stands for a bound slab (binding needs a device)
    net.stage("prenorm").bind = lambda n, device, max_cycle: None
    net._frames = frames
    return net


def test_a_model_that_has_stepped_refuses_the_switch():
    """The rule reads the model's own frame counter; a slab that is bound but has not stepped may still change."""
    net = _stepped(0)
    pkg.set_pre_normalization(net)                          # frame counter 0: allowed
    net._frames = 8
    pkg.set_pre_normalization(net)                          # no change: allowed
    for change in (dict(enabled=False), dict(zaxis=(1, 0))):
        with pytest.raises(RuntimeError, match=r"clean_state\(\)"):
            pkg.set_pre_normalization(net, **change)
    assert net.pre_normalization is True and net.stage("prenorm").joints == (0, 1, 8, 4)


def test_stream_shards_validate_every_shard_before_switching_any():
    shards = object.__new__(pkg.parallel.StreamShards)
    shards.models = [_stepped(0), _stepped(8)]
    with pytest.raises(RuntimeError, match=r"clean_state\(\)"):
        pkg.set_pre_normalization(shards)
    assert [m.pre_normalization for m in shards.models] == [False, False]
    shards.models = [_stepped(0), pkg.CoStGcn(pkg.ntu_graph().A, (2, 300, 25, 2))]
    with pytest.raises(ValueError, match="C = 2"):
        pkg.set_pre_normalization(shards)
    shards.models = [_stepped(0), pkg.GraphConvolution(3, 8, pkg.ntu_graph().A)]
    with pytest.raises(TypeError):
        pkg.set_pre_normalization(shards)
    with pytest.raises(ValueError, match="outside"):
        pkg.set_pre_normalization(shards, zaxis=(0, 25))
    assert shards.models[0].pre_normalization is False
    shards.models = [_stepped(0), _stepped(0)]
    assert pkg.set_pre_normalization(shards, xaxis=(9, 5)) is shards
    assert [(m.pre_normalization, m.stage("prenorm").joints) for m in shards.models] == [(True, (0, 1, 9, 5))] * 2
