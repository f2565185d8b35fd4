"""Bone / motion input modalities, the parts that need no GPU: the numpy oracle against what the reference's own scripts
wrote (tests/golden/g13_modalities.npz, make_golden_modalities.py), the parent tables, the C ABI and the host errors."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import _bootstrap
from tests import modality_oracle as mo
from tests.helpers import GOLDEN

pkg = _bootstrap.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("csk_derive_modality_f32", "csk_derive_modality_frames_f32")


@pytest.fixture(scope="module")
def golden():
    d = np.load(os.path.join(GOLDEN, "g13_modalities.npz"))
    return {k: d[k] for k in d.files}


@pytest.mark.parametrize("tag", ["ntu", "kinetics"])
def test_oracle_reproduces_the_reference_scripts_bit_for_bit(golden, tag):
    x, parents = golden[f"{tag}/joint"], golden[f"{tag}/parents"]
    assert x.shape == (2, 3, 6, 25 if tag == "ntu" else 18, 2) and x.dtype == np.float32
    for kind in ("bone", "joint_motion", "bone_motion"):
        got = mo.derive_clip(x, kind, parents)
        assert got.dtype == np.float32 and np.array_equal(got, golden[f"{tag}/{kind}"]), kind
    assert np.count_nonzero(golden[f"{tag}/bone"]) > 0 and not golden[f"{tag}/joint_motion"][:, :, -1].any()
    # the step form is the clip form one frame later: m'[s] = m[s-1], m'[0] = 0
    for kind in ("joint_motion", "bone_motion"):
        steps = mo.derive_steps(x, kind, parents)
        assert np.array_equal(steps[:, :, 1:], golden[f"{tag}/{kind}"][:, :, :-1]) and not steps[:, :, 0].any()
    first = np.zeros((2, 6), dtype=bool)
    first[:, 0] = first[1, 3] = True
    steps = mo.derive_steps(x, "joint_motion", parents, first)
    assert not steps[1, :, 3].any() and np.array_equal(steps[0], mo.derive_steps(x, "joint_motion", parents)[0])


def test_graph_bone_parents_equal_the_reference_tables(golden):
    for tag, g in (("ntu", pkg.ntu_graph()), ("kinetics", pkg.kinetics_graph())):
        assert g.bone_parents.dtype == np.int32 and g.bone_parents.shape == (g.num_node,)
        assert np.array_equal(g.bone_parents, golden[f"{tag}/parents"])
        roots = [v for v in range(g.num_node) if g.bone_parents[v] == v]
        assert roots == ([20] if tag == "ntu" else [0])
        assert np.array_equal(pkg.modality.bone_parents(g.num_node), g.bone_parents)
    assert pkg.Graph([(0, 1)], 2).bone_parents is None


def test_entries_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cskel.h")).read()
    declared = set(re.findall(r"\b(csk_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(pkg.native.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in pkg.native.SIGNATURES and hasattr(lib, name), name
    assert [int(re.search(rf"#define CSK_MODALITY_{n.upper()} (\d)", hdr).group(1)) for n in pkg.modality.MODALITIES] == [0, 1, 2, 3]
    assert pkg.modality.MODE == {"joint": 0, "bone": 1, "joint_motion": 2, "bone_motion": 3}
    assert pkg.native.lib().csk_abi_version() == 16


def test_entries_refuse_bad_arguments_before_any_launch():
    """mode, parent table and r are checked on the host: -2 with a message, and no GPU is needed to get it."""
    lib = pkg.native.lib()
    buf = (ctypes.c_float * 64)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 128          # never dereferenced: every call returns before a launch
    good = (ctypes.c_int32 * 3)(0, 0, 1)
    for mode in (0, 4, -1):
        assert lib.csk_derive_modality_f32(a, b, mode, good, 1, 1, 2, 3, 1, None) == -2 and b"unknown mode" in lib.csk_last_error()
    for bad in ((0, 3, 1), (0, -1, 1)):
        assert lib.csk_derive_modality_f32(a, b, 1, (ctypes.c_int32 * 3)(*bad), 1, 1, 2, 3, 1, None) == -2
        assert b"outside [0, 3)" in lib.csk_last_error()
    assert lib.csk_derive_modality_f32(a, a, 1, good, 1, 1, 2, 3, 1, None) == -1
    assert lib.csk_derive_modality_f32(a, b, 1, None, 1, 1, 2, 3, 1, None) == -1 and b"parent table" in lib.csk_last_error()
    src, dst = (ctypes.c_void_p * 8)(*([a] * 8)), (ctypes.c_void_p * 8)(*([b] * 8))
    flags = (ctypes.c_int32 * 4)()
    for r in (0, 9, -3):
        assert lib.csk_derive_modality_frames_f32(src, dst, r, 2, None, a, flags, 1, 1, 1, 3, 1, None) == -2
        assert b"1..8 frames" in lib.csk_last_error()
    assert lib.csk_derive_modality_frames_f32(src, dst, 1, 7, good, a, flags, 1, 1, 1, 3, 1, None) == -2
    assert lib.csk_derive_modality_frames_f32(src, dst, 1, 3, (ctypes.c_int32 * 3)(0, 5, 1), a, flags, 1, 1, 1, 3, 1, None) == -2
    assert lib.csk_derive_modality_frames_f32(src, dst, 1, 2, None, None, None, 1, 1, 1, 3, 1, None) == -1     # motion without its state
    with pytest.raises(RuntimeError, match="unknown mode"):
        pkg.native.check(lib.csk_derive_modality_f32(a, b, 9, good, 1, 1, 2, 3, 1, None), "csk_derive_modality_f32")


def _models():
    a25, a18 = pkg.ntu_graph().A, pkg.kinetics_graph().A
    return [pkg.StGcn(a25, (3, 20, 25, 2)), pkg.AGcn(a18, (3, 20, 18, 2)), pkg.STr(a25, (3, 20, 25, 2)),
            pkg.CoStGcn(a25, (3, 300, 25, 2)), pkg.CoAGcn(a18, (3, 300, 18, 2)), pkg.CoSTr(a25, (3, 300, 25, 2))]


def test_set_input_modality_host_rules():
    for net in _models():
        assert net.input_modality == "joint"
        for name in ("bone", "joint_motion", "bone_motion", "joint"):
            assert pkg.set_input_modality(net, name) is net and net.input_modality == name
        for bad in ("motion", "Bone", "", None, 1):
            with pytest.raises(ValueError, match="input modality must be one of"):
                pkg.set_input_modality(net, bad)
        assert net.input_modality == "joint"
    with pytest.raises(TypeError):
        pkg.set_input_modality(pkg.GraphConvolution(3, 8, pkg.ntu_graph().A), "bone")
    # a skeleton without a parent table: refused at the call, the model keeps its mode
    odd = pkg.StGcn(np.ones((3, 10, 10)), (3, 20, 10, 2))
    for name in ("bone", "bone_motion"):
        with pytest.raises(ValueError, match="no bone parent table"):
            pkg.set_input_modality(odd, name)
    assert odd.input_modality == "joint"
    # a fresh model is "joint" by default and the class attribute is what says so (constructors keep the reference's signatures)
    assert "input_modality" not in pkg.CoStGcn(pkg.ntu_graph().A).__dict__


def test_a_model_that_has_stepped_refuses_a_change_of_modality():
    """The rule reads the model's own frame counter; a slab that is bound but has not stepped may still change."""
    net = pkg.CoStGcn(pkg.ntu_graph().A)
    net._ctr = (ctypes.c_int64 * 22)()
    net._n, net._xin0 = 2, types.SimpleNamespace(device="cpu")     # stands for a bound slab (binding needs a device)
    net.stage("modality").bind = lambda n, device, max_cycle: None
    pkg.set_input_modality(net, "bone")                      # frame counter 0: allowed
    net._frames = 8
    pkg.set_input_modality(net, "bone")                      # no change: allowed
    with pytest.raises(RuntimeError, match=r"clean_state\(\)"):
        pkg.set_input_modality(net, "joint_motion")
    assert net.input_modality == "bone"


def test_online_ensemble_checks_its_members():
    a = pkg.ntu_graph().A
    def make(**kw):
        return pkg.CoStGcn(a, (3, 300, 25, 2), 60, **{"pool_size": 3, "pool_padding": 1, **kw})
    ens = pkg.fusion.OnlineEnsemble([make(), pkg.set_input_modality(make(), "bone")])
    assert [n.input_modality for n in ens.nets] == ["joint", "bone"] and ens.method == "add"
    with pytest.raises(ValueError, match="pool_size"):
        pkg.fusion.OnlineEnsemble([make(), make(pool_size=4)])
    with pytest.raises(ValueError, match="pool_padding"):
        pkg.fusion.OnlineEnsemble([make(), make(pool_padding=0)])
    with pytest.raises(ValueError, match="num_classes"):
        pkg.fusion.OnlineEnsemble([make(), pkg.CoStGcn(a, (3, 300, 25, 2), 40, pool_size=3, pool_padding=1)])
    with pytest.raises(ValueError, match="2..4"):
        pkg.fusion.OnlineEnsemble([make()])
    with pytest.raises(ValueError, match="2..4"):
        pkg.fusion.OnlineEnsemble([make() for _ in range(5)])
    with pytest.raises(ValueError, match="method"):
        pkg.fusion.OnlineEnsemble([make(), make()], method="mean")
    one, two = make(), make()
    one._n, two._n = 3, 4
    with pytest.raises(ValueError, match="number of streams"):
        pkg.fusion.OnlineEnsemble([one, two])
