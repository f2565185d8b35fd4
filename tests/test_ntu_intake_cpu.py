"""NTU body intake, the parts that need no GPU: the fixture the reference's own functions wrote
(tests/golden/g18_ntu_intake.npz, make_golden_ntu_intake.py) is admissible and reaches every branch, the numpy oracle
(tests/ntu_intake_oracle.py) reproduces it bit for bit, and the C ABI and the host layer refuse what they must."""
import ctypes
import os
import re

import numpy as np
import pytest

import _bootstrap
from tests import ntu_intake_oracle as no
from tests.helpers import GOLDEN

pkg = _bootstrap.load()
ntu_intake, keypoints = pkg.ntu_intake, pkg.keypoints
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "csk_ntu_intake_f32"
FRAMES_OUT = 12
# case -> the oracle's table [(slot, L, frame 0 null)] of the two kept bodies: the branch the case was built to take
PLAN = {
    "order": [(1, 8, False), (3, 8, False)],            # energy order 1, 3, 0, 2: not slot order
    "one": [(0, 6, False), (3, 0, True)],               # the empty slots tie at 0: the highest fills person 1
    "tie": [(3, 7, False), (2, 7, False)],              # slots 1, 2 (duplicates) and 3 (mirrored) tie: the higher slots win
    "empty": [(3, 0, True), (2, 0, True)],
    "compact": [(2, 5, True), (0, 10, False)],          # frames 2, 3, 5, 6, 7 move to the front; 12 = 2 * 5 + 2
    "gap": [(0, 6, False), (1, 8, False)],              # frame 2 null inside, frames 6, 7 null behind
    "tail": [(1, 5, False), (3, 5, False)],             # 12 - 5 = 7 is no multiple of 5
    "one_frame": [(1, 1, False), (3, 0, True)],
    "full": [(1, 12, False), (0, 12, False)],           # T = frames_out: nothing to fill
    "two_lengths": [(0, 7, False), (3, 4, False)],
    "late": [(0, 8, False), (2, 3, True)],              # the second person appears in frame 5
}


@pytest.fixture(scope="module")
def golden():
    d = np.load(os.path.join(GOLDEN, "g18_ntu_intake.npz"))
    return {k: d[k] for k in d.files}


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- the fixture and the oracle ----------------------------------------------------------------------------------------------
def test_fixture_holds_every_case(golden):
    assert {k.split("/")[0] for k in golden} == set(PLAN)
    assert os.path.getsize(os.path.join(GOLDEN, "g18_ntu_intake.npz")) < 256 * 1024
    for case in PLAN:
        bodies = golden[f"{case}/bodies"]
        assert bodies.dtype == np.float32 and bodies.shape[1:] == (4, 25, 3) and bodies.shape[0] <= FRAMES_OUT
        assert bodies.shape[0] <= 10 or case == "full"
        for name in ("want_selected", "want_padded", "want_final"):
            assert golden[f"{case}/{name}"].dtype == np.float32 and golden[f"{case}/{name}"].shape == (3, FRAMES_OUT, 25, 2)
        assert np.isfinite(bodies).all() and np.abs(golden[f"{case}/want_final"]).max() <= 8.0


@pytest.mark.parametrize("case", sorted(PLAN))
def test_oracle_equals_the_reference_bit_for_bit(golden, case):
    bodies = golden[f"{case}/bodies"]
    selected = no.select_only(bodies, FRAMES_OUT, 2)
    padded = no.select_bodies(bodies, FRAMES_OUT, 2)
    assert np.array_equal(_bytes(selected), _bytes(golden[f"{case}/want_selected"]))
    assert np.array_equal(_bytes(padded), _bytes(golden[f"{case}/want_padded"]))
    assert np.array_equal(_bytes(no.select_bodies_clip(bodies[None], FRAMES_OUT, 2)[0]), _bytes(padded))


@pytest.mark.parametrize("case", sorted(PLAN))
def test_fixture_is_admissible_and_takes_its_branch(golden, case):
    """Apart from the designed ties (bit-identical energies) two energies of a clip are at least 1e-6 apart, relatively: no
    fp64 summation order decides a rank.  The oracle's table says which branch the case takes."""
    bodies = golden[f"{case}/bodies"]
    energy = no.energies(bodies)
    assert no.energy_gaps(energy) >= 1e-6
    assert no.plan_clip(bodies, FRAMES_OUT, 2) == PLAN[case]
    if case == "tie":
        assert energy[1] == energy[2] == energy[3] > energy[0] > 0
        assert np.array_equal(bodies[:, 1], bodies[:, 2]) and not np.array_equal(bodies[:, 1], bodies[:, 3])
        want = golden["tie/want_selected"]
        assert np.array_equal(want[:, :7, :, 0], bodies[:, 3].transpose(2, 0, 1))      # the fixture is the authority: slot 3 leads
        assert np.array_equal(want[:, :7, :, 1], bodies[:, 2].transpose(2, 0, 1))
    if case != "full":
        assert not np.array_equal(golden[f"{case}/want_padded"], golden[f"{case}/want_selected"]) or case == "empty"


def test_oracle_rules():
    assert no.order_bodies(np.array([1.0, 2.0, 2.0, 0.5])) == [2, 1, 0, 3]
    assert no.order_bodies(np.array([0.0, 0.0, 0.0, 0.0])) == [3, 2, 1, 0]
    assert no.order_bodies(np.array([np.nan, 1.0, np.nan, 3.0])) == [3, 1, 2, 0]
    present = np.array([0, 1, 0, 1, 1, 0], dtype=bool)
    assert no.source_frames(present, 8)[:2] == (3, True) and no.source_frames(present, 8)[2].tolist() == [1, 3, 4, 1, 3, 4, 1, 3]
    present = np.array([1, 0, 1, 0, 0], dtype=bool)
    assert no.source_frames(present, 7)[:2] == (3, False) and no.source_frames(present, 7)[2].tolist() == [0, 1, 2, 0, 1, 2, 0]
    assert no.source_frames(np.zeros(4, dtype=bool), 6) == (0, True, None)
    b = np.zeros((3, 2, 4, 3), dtype=np.float32)
    b[1, 0] = -0.0                                          # all -0.0: null
    b[2, 1, 3, 1] = np.nan                                  # NaN is not zero
    assert no.null_flags(b).tolist() == [[False, False, False], [False, False, True]]
    x = np.arange(24, dtype=np.float32).reshape(2, 1, 4, 3)
    assert no.energies(x)[0] == pytest.approx(sum(x[:, 0, :, c].astype(np.float64).std() for c in range(3)), rel=1e-12)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cskel.h")).read()
    declared = set(re.findall(r"\b(csk_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(pkg.native.LIB_PATH)
    assert ENTRY in declared and ENTRY in pkg.native.SIGNATURES and hasattr(lib, ENTRY)
    assert len(pkg.native.SIGNATURES[ENTRY]) == 9
    assert pkg.native.lib().csk_abi_version() == 16 and "#define CSK_ABI_VERSION 16" in hdr
    limit = int(re.search(r"#define CSK_NTU_MAX_FRAMES (\d+)", hdr).group(1))
    assert limit == ntu_intake.MAX_FRAMES >= 300
    assert os.path.exists(os.path.join(ROOT, "continual-skeletons_amd", "csrc", "ntu_intake.hip"))


def test_entry_refuses_bad_arguments_before_any_launch():
    """Every refusal is decided on the host: the code and a message, and no GPU is needed to get them."""
    lib = pkg.native.lib()
    buf = (ctypes.c_float * 64)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 128          # never dereferenced: every call returns before a launch

    def call(bodies=a, out=b, n=1, t=2, p=4, v=25, m=2, t_out=300):
        return lib.csk_ntu_intake_f32(bodies, out, n, t, p, v, m, t_out, None)

    assert call(bodies=None) == -1 and b"null pointer" in lib.csk_last_error()
    assert call(out=None) == -1 and b"null pointer" in lib.csk_last_error()
    assert call(out=a) == -1 and b"out must not be bodies" in lib.csk_last_error()
    for dims in (dict(n=0), dict(t=0), dict(p=0), dict(v=0), dict(m=0), dict(t_out=0), dict(n=-1)):
        assert call(**dims) == -1 and b"bad dims" in lib.csk_last_error(), dims
    for dims in (dict(p=9, m=2), dict(p=2, m=3), dict(p=8, m=9)):
        assert call(**dims) == -2 and b"M <= P <= 8" in lib.csk_last_error(), dims
    assert call(v=65) == -2 and b"V <= 64" in lib.csk_last_error()
    for dims in (dict(t=301), dict(t=5, t_out=4), dict(t_out=ntu_intake.MAX_FRAMES + 1)):
        assert call(**dims) == -2 and b"T <= T_out <= 1024" in lib.csk_last_error(), dims
    with pytest.raises(RuntimeError, match="V <= 64"):
        pkg.native.check(call(v=65), ENTRY)


# ---- the host layer ----------------------------------------------------------------------------------------------------------
def _clip_models():
    a25 = pkg.ntu_graph().A
    return [pkg.StGcn(a25, (3, 20, 25, 2)), pkg.AGcn(a25, (3, 20, 25, 2)), pkg.STr(a25, (3, 20, 25, 2)),
            pkg.StGcnMod(a25, (3, 100, 25, 2)), pkg.agcn.AGcnMod(a25, (3, 100, 25, 2)), pkg.str.STrMod(a25, (3, 100, 25, 2))]


def test_set_ntu_intake_host_rules():
    for net in _clip_models():
        assert net.ntu_intake is False and "ntu_intake" not in net.__dict__            # the class attribute says so
        assert not [k for k in net.__dict__ if k.startswith("_ntu")]
        assert ntu_intake.set_ntu_intake(net) is net and net.ntu_intake is True and net.stage("ntu").bodies == 4
        assert ntu_intake.set_ntu_intake(net, bodies_in=8) is net and net.stage("ntu").bodies == 8
        assert ntu_intake.set_ntu_intake(net, True, 2) is net and net.stage("ntu").bodies == 2
        for bad in (1, 9, 0, -1, 2.0, None, True):
            with pytest.raises(ValueError, match="bodies_in"):
                ntu_intake.set_ntu_intake(net, bodies_in=bad)
        assert net.stage("ntu").bodies == 2 and net.ntu_intake is True
        assert ntu_intake.set_ntu_intake(net, enabled=False) is net and net.ntu_intake is False
    with pytest.raises(ValueError, match="C = 2"):
        ntu_intake.set_ntu_intake(pkg.StGcn(pkg.ntu_graph().A, (2, 300, 25, 2)))
    with pytest.raises(ValueError, match="T = 2000"):
        ntu_intake.set_ntu_intake(pkg.StGcn(pkg.ntu_graph().A, (3, 2000, 25, 2)))
    for wrong in (pkg.GraphConvolution(3, 8, pkg.ntu_graph().A), None, "StGcn"):
        with pytest.raises(TypeError, match="no NTU intake"):
            ntu_intake.set_ntu_intake(wrong)
    # independent of the other two pre-passes
    net = pkg.set_input_modality(pkg.set_pre_normalization(ntu_intake.set_ntu_intake(pkg.StGcn(pkg.ntu_graph().A, (3, 20, 25, 2)))), "bone")
    assert net.ntu_intake and net.pre_normalization and net.input_modality == "bone"


def test_the_two_intakes_exclude_each_other_in_either_order():
    net = pkg.StGcn(pkg.ntu_graph().A, (3, 20, 25, 2))
    ntu_intake.set_ntu_intake(net)
    with pytest.raises(ValueError, match="NTU intake is on"):
        keypoints.set_keypoint_intake(net)
    assert net.keypoint_intake is False and net.ntu_intake is True
    keypoints.set_keypoint_intake(net, enabled=False)               # switching the other one off is no conflict
    ntu_intake.set_ntu_intake(net, enabled=False)
    keypoints.set_keypoint_intake(net)
    with pytest.raises(ValueError, match="keypoint intake is on"):
        ntu_intake.set_ntu_intake(net)
    assert net.keypoint_intake is True and net.ntu_intake is False
    ntu_intake.set_ntu_intake(net, enabled=False)
    keypoints.set_keypoint_intake(net, enabled=False)
    assert ntu_intake.set_ntu_intake(net).ntu_intake is True


def test_continual_models_and_shards_are_refused_with_the_reason():
    a25 = pkg.ntu_graph().A
    shards = object.__new__(pkg.parallel.StreamShards)
    shards.models = []
    for model in (pkg.CoStGcn(a25), pkg.CoAGcn(a25), pkg.CoSTr(a25), pkg.CoStGcnMod(a25, (3, 100, 25, 2)), shards):
        with pytest.raises(TypeError, match="looks ahead") as err:
            ntu_intake.set_ntu_intake(model)
        assert "select_bodies_clip" in str(err.value) and "prime_streams" in str(err.value)
        assert not getattr(model, "ntu_intake", False)


def test_the_names_live_in_the_module_only():
    for name in ("set_ntu_intake", "select_bodies_clip", "NtuIntake"):
        assert hasattr(ntu_intake, name) and not hasattr(pkg, name)
    src = open(os.path.join(ROOT, "continual-skeletons_amd", "ntu_intake.py")).read()
    assert "oracle" not in src
    assert ".skeleton" in ntu_intake.__doc__ and "running-energy" in ntu_intake.__doc__         # what is out of scope is said


def test_cpu_tensors_and_wrong_arguments_are_refused_on_the_host():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ntu_intake.select_bodies_clip(torch.zeros(1, 2, 4, 25, 3))
    net = ntu_intake.set_ntu_intake(pkg.StGcn(pkg.ntu_graph().A, (3, 20, 25, 2)).eval())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(2, 10, 4, 25, 3))
