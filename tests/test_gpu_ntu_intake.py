"""NTU body intake on the device: csk_ntu_intake_f32 (csrc/ntu_intake.hip) against what the reference's own functions wrote
(tests/golden/g18_ntu_intake.npz), against the numpy oracle (tests/ntu_intake_oracle.py) at the seams of the kernel, and the clip
models that run it in front of the unchanged path.

The intake rounds nothing -- fp64 energies that decide an order, then a gather -- so every comparison of its output is bit for
bit (``torch.equal`` / uint8 views); the random clips give every body a scale of its own, and the tests assert that their
energies are 1e-6 apart before they trust the oracle's order.  Only the comparison behind the pre-normalisation has a tolerance:
1e-5 absolute at |want| <= 8, the one tests/test_gpu_prenorm.py uses for that arithmetic.
The seams: a wave of the kernel owns the frames t = w mod 16 and loads four of them at a time (64 frames per round), the flag
scan and the gather walk 64 frames / 64 rows at a time, a lane holds the elements l, l + 64, l + 128 of a V * 3 item (V = 3: one
partly filled slot, V = 25: two, V = 64: three) and V * M > 64 needs more than one sweep of an output row."""
import os

import numpy as np
import pytest
import torch

import _bootstrap
from tests import ntu_intake_oracle as no
from tests.helpers import GOLDEN, check_parity, guarded_allocs, randomise_unit_

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native, ntu_intake, keypoints = pkg.native, pkg.ntu_intake, pkg.keypoints
DEV = "cuda:0"
PAD = 1024                      # guard elements on either side of a guarded operand
FRAMES_OUT = 12
CASES = ("order", "one", "tie", "empty", "compact", "gap", "tail", "one_frame", "full", "two_lengths", "late")


def _same_bytes(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


@pytest.fixture(scope="module")
def golden():
    d = np.load(os.path.join(GOLDEN, "g18_ntu_intake.npz"))
    return {k: d[k] for k in d.files}


def _bodies(n, t, p, v, seed):
    """Seeded bodies (N, T, P, V, 3): body p of a clip is offset + scale * normal with a scale of its own (energies well apart),
    present in frames drawn from one of: all, none, a late start, an early end, a gap, a random half."""
    rng = np.random.default_rng(seed)
    b = np.zeros((n, t, p, v, 3), dtype=np.float32)
    for i in range(n):
        scales = 0.5 + 0.25 * rng.permutation(p)
        for q in range(p):
            kind = rng.integers(6) if q else rng.choice([0, 2, 3, 4, 5])       # slot 0 is never empty: no clip is
            lo, hi = sorted(rng.integers(0, t + 1, size=2))
            present = {0: np.ones(t, bool), 1: np.zeros(t, bool), 2: np.arange(t) >= min(lo, t - 1), 3: np.arange(t) <= lo,
                       4: (np.arange(t) < lo) | (np.arange(t) >= hi), 5: rng.random(t) < 0.5}[int(kind)]
            body = (rng.standard_normal(3) + scales[q] * rng.standard_normal((t, v, 3))).astype(np.float32)
            b[i, present, q] = body[present]
    return b


def _oracle(b, frames_out, m):
    for clip in b:
        assert no.energy_gaps(no.energies(clip)) >= 1e-6        # the oracle's order is the kernel's: no rank hangs on rounding
    return no.select_bodies_clip(b, frames_out, m)


def _guarded(shape, values=None):
    """A tensor of ``shape`` in the middle of a buffer whose PAD elements on either side are NaN."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), float("nan"), device=DEV, dtype=torch.float32)
    view = buf[PAD:PAD + n].view(shape)
    if values is not None:
        view.copy_(values)
    return buf, view


def _intact(buf, n):
    return bool(torch.isnan(torch.cat([buf[:PAD], buf[PAD + n:]])).all())


def _entry(bodies, m, frames_out, out=None):
    n, t, p, v, _ = bodies.shape
    out = torch.empty((n, 3, frames_out, v, m), device=DEV, dtype=torch.float32) if out is None else out
    rc = native.lib().csk_ntu_intake_f32(native.ptr(bodies), native.ptr(out), n, t, p, v, m, frames_out, native.stream_of(bodies))
    torch.cuda.synchronize()
    return rc, out


def _run_guarded(b, m, frames_out):
    """The entry on operands between NaN guards -> the output (host); the guards are intact."""
    b = torch.as_tensor(b)
    src_buf, src = _guarded(b.shape, b.to(DEV))
    dst_buf, dst = _guarded((b.shape[0], 3, frames_out, b.shape[3], m))
    rc, got = _entry(src, m, frames_out, out=dst)
    assert rc == 0 and _intact(src_buf, src.numel()) and _intact(dst_buf, dst.numel())
    return got.cpu()


# ---- 1. against the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_select_bodies_clip_equals_what_the_reference_wrote(golden, case):
    bodies, want = torch.from_numpy(golden[f"{case}/bodies"])[None], torch.from_numpy(golden[f"{case}/want_padded"])
    got = _run_guarded(bodies, 2, FRAMES_OUT)
    assert got.shape == (1, 3, FRAMES_OUT, 25, 2) and torch.equal(got[0], want), case
    assert _same_bytes(got[0].numpy(), want.numpy())                            # the sign of zero as well
    with guarded_allocs(pad=PAD) as ga:                                         # the tensor the host layer allocates
        out = ntu_intake.select_bodies_clip(bodies.to(DEV), FRAMES_OUT, 2)
    torch.cuda.synchronize()
    assert ga.count == 1 and torch.equal(out[0].cpu(), want) and _intact(out._base, out.numel())


def test_all_fixture_cases_in_batches_by_length(golden):
    """Clips of one length in one launch, every clip its own workgroup: the same bits as alone."""
    by_t = {}
    for case in CASES:
        by_t.setdefault(golden[f"{case}/bodies"].shape[0], []).append(case)
    assert max(len(v) for v in by_t.values()) >= 2
    for t, cases in by_t.items():
        got = ntu_intake.select_bodies_clip(torch.from_numpy(np.stack([golden[f"{c}/bodies"] for c in cases])).to(DEV), FRAMES_OUT)
        assert _same_bytes(got.cpu().numpy(), np.stack([golden[f"{c}/want_padded"] for c in cases])), t


# ---- 2. the seams against the oracle ---------------------------------------------------------------------------------------------
SEAMS = [  # n, T, P, V, M, frames_out
    (3, 70, 4, 25, 2, 300), (2, 1, 4, 25, 2, 1), (2, 1, 1, 3, 1, 5), (2, 15, 4, 25, 2, 16), (2, 16, 4, 25, 2, 17),
    (2, 17, 4, 3, 2, 64), (2, 63, 4, 25, 2, 64), (2, 64, 4, 25, 2, 64), (2, 65, 8, 25, 2, 130), (2, 64, 1, 3, 1, 65),
    (2, 65, 8, 3, 8, 65), (1, 17, 8, 25, 8, 40), (1, 129, 2, 64, 2, 200), (1, 300, 4, 25, 2, 1024),
]


@pytest.mark.parametrize("n,t,p,v,m,frames_out", SEAMS)
def test_seams_against_the_oracle(n, t, p, v, m, frames_out):
    b = _bodies(n, t, p, v, 100 * t + 10 * p + v)
    got = _run_guarded(b, m, frames_out)
    assert _same_bytes(got.numpy(), _oracle(b, frames_out, m)), (n, t, p, v, m, frames_out)


def test_default_frames_out_is_the_clip_length_and_kept_bodies_two():
    b = _bodies(2, 9, 4, 25, 5)
    got = ntu_intake.select_bodies_clip(torch.from_numpy(b).to(DEV))
    assert got.shape == (2, 3, 9, 25, 2) and _same_bytes(got.cpu().numpy(), _oracle(b, 9, 2))


def test_ties_go_to_the_higher_slot_and_negative_zero_frames_are_null():
    b = np.random.default_rng(9).standard_normal((1, 10, 6, 25, 3)).astype(np.float32)
    b[0, :, 1] = b[0, :, 4]                                 # duplicates: bit-identical energies whatever the slot
    b[0, :, 5] = b[0, :, 4] * np.float32(2.0)               # the leader
    b[0, :, 3] *= np.float32(0.5)
    b[0, :, 0] = 0.0
    b[0, 3:, 2] = -0.0                                      # -0.0 frames are null: slot 2 ends at frame 3
    b[0, :3, 2] = b[0, :3, 4] * np.float32(0.01)
    got = _run_guarded(b, 6, 14)
    assert _same_bytes(got.numpy(), no.select_bodies_clip(b, 14, 6))
    order = no.order_bodies(no.energies(b[0]))
    assert order == [5, 4, 1, 3, 2, 0] and no.energy_gaps(no.energies(b[0])) >= 1e-6
    m2 = order.index(2)
    assert torch.equal(got[0, :, 3:6, :, m2], got[0, :, 0:3, :, m2]) and not torch.signbit(got[0, :, :, :, order.index(0)]).any()


# ---- 3. batch invariance and NaN -------------------------------------------------------------------------------------------------
def test_a_clips_result_does_not_depend_on_its_batch():
    b = _bodies(5, 70, 4, 25, 31)
    whole = _run_guarded(b, 2, 300)
    alone = _run_guarded(b[3:4], 2, 300)
    moved = _run_guarded(np.ascontiguousarray(b[[3, 0, 4]]), 2, 300)
    assert torch.equal(alone[0], whole[3]) and torch.equal(moved[0], whole[3]) and torch.equal(moved[2], whole[4])


def test_a_nan_clip_stays_inside_its_operands_and_leaves_the_other_clips_alone():
    b = _bodies(3, 40, 4, 25, 41)
    clean = _run_guarded(b, 2, 100)
    b[1, 5, 0, 3, 1] = np.nan                               # one coordinate
    b[1, :, 2] = np.nan                                     # a whole body: a NaN energy
    b[1, 0, 3] = np.inf
    got = _run_guarded(b, 2, 100)                           # asserts the guards
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_refused_calls_launch_nothing():
    b = torch.from_numpy(_bodies(2, 6, 4, 25, 51)).to(DEV)
    out = torch.full((2, 3, 8, 25, 2), 3.0, device=DEV)
    for m, frames_out in ((5, 8), (2, 5), (2, 1025)):       # M > P, T_out < T, T_out beyond the limit
        rc, _ = _entry(b, m, frames_out, out=out)
        assert rc == -2 and native.lib().csk_last_error() and bool((out == 3.0).all()), (m, frames_out)
    wide = torch.zeros((1, 1, 2, 65, 3), device=DEV)
    rc, _ = _entry(wide, 2, 8, out=out)
    assert rc == -2 and bool((out == 3.0).all())
    many = torch.zeros((1, 1, 9, 25, 3), device=DEV)
    rc, _ = _entry(many, 2, 8, out=out)
    assert rc == -2 and bool((out == 3.0).all())
    with pytest.raises(ValueError, match="bodies_in"):
        ntu_intake.select_bodies_clip(b, 8, 5)
    with pytest.raises(ValueError, match="frames_out"):
        ntu_intake.select_bodies_clip(b, 5)
    with pytest.raises(ValueError, match="frames_out"):
        ntu_intake.select_bodies_clip(b, 1025)
    with pytest.raises(ValueError, match="integers"):
        ntu_intake.select_bodies_clip(b, 8.0)
    with pytest.raises(RuntimeError, match=r"\(N, T, P, V, 3\)"):
        ntu_intake.select_bodies_clip(b[..., :2].contiguous())
    with pytest.raises(RuntimeError, match="contiguous"):
        ntu_intake.select_bodies_clip(b.transpose(1, 2))


# ---- 5. models -------------------------------------------------------------------------------------------------------------------
def _twins(cls, shape_t, seed=7):
    nets = [cls(pkg.ntu_graph().A, (3, shape_t, 25, 2), 60).eval() for _ in range(2)]
    randomise_unit_(nets[0], seed, attn_scale=1 / 25 if "AGcn" in cls.__name__ else 1.0)
    nets[1].load_state_dict(nets[0].state_dict())
    return [net.to(DEV) for net in nets]


@pytest.mark.parametrize("model,shape_t,t,n", [("StGcn", 20, 13, 2), ("STr", 20, 7, 2), ("AGcnMod", 84, 30, 1)])
def test_clip_model_with_the_switch_on_equals_its_twin_on_the_selected_clip(model, shape_t, t, n):
    cls = getattr(pkg, model, None) or getattr(pkg.agcn, model)
    net, twin = _twins(cls, shape_t)
    assert ntu_intake.set_ntu_intake(net) is net and twin.ntu_intake is False
    bodies = torch.from_numpy(_bodies(n, t, 4, 25, 61)).to(DEV)
    with torch.no_grad():
        selected = ntu_intake.select_bodies_clip(bodies, shape_t, 2)
        got, want = net(bodies), twin(selected)
        assert got.shape == (n, 60) and torch.equal(got, want)
        first_two = torch.zeros_like(selected)
        first_two[:, :, :t] = bodies[:, :, :2].permute(0, 4, 1, 3, 2)           # slots 0 and 1, zero tail: not what the intake feeds
        assert not torch.equal(got, twin(first_two))
        with pytest.raises(RuntimeError, match="body clip"):
            net(selected)
        with pytest.raises(RuntimeError, match="body clip"):
            net(torch.zeros((n, shape_t + 1, 4, 25, 3), device=DEV))
    ntu_intake.set_ntu_intake(net, enabled=False)
    assert net._intake_clip(selected) is selected                               # off: no launch, no allocation, the tensor itself
    with torch.no_grad():
        assert torch.equal(net(selected), want)


@pytest.mark.parametrize("case", CASES)
def test_with_pre_normalisation_the_pre_pass_is_the_references_pipeline(golden, case):
    """set_ntu_intake + set_pre_normalization = read_xyz -> gendata -> pre_normalization: the model's pre-pass output against
    what the reference's function returned."""
    net = pkg.set_pre_normalization(ntu_intake.set_ntu_intake(pkg.StGcn(pkg.ntu_graph().A, (3, FRAMES_OUT, 25, 2)))).eval()
    bodies = torch.from_numpy(golden[f"{case}/bodies"])[None].to(DEV)
    padded = net._intake_clip(bodies)
    assert torch.equal(padded[0].cpu(), torch.from_numpy(golden[f"{case}/want_padded"]))
    got = net.stage("prenorm").clip(padded)
    check_parity(got[0].cpu(), torch.from_numpy(golden[f"{case}/want_final"]), tol=1e-5, ref_cap=8.0, tag=case,
                 what="NTU intake + pre_normalize_clip vs read_xyz + pre_normalization")


def test_switches_refuse_on_device_models_what_they_must():
    net = pkg.StGcn(pkg.ntu_graph().A, (3, 20, 25, 2)).eval().to(DEV)
    ntu_intake.set_ntu_intake(net)
    with pytest.raises(ValueError, match="NTU intake is on"):
        keypoints.set_keypoint_intake(net)
    ntu_intake.set_ntu_intake(net, enabled=False)
    keypoints.set_keypoint_intake(net)
    with pytest.raises(ValueError, match="keypoint intake is on"):
        ntu_intake.set_ntu_intake(net)
    co = pkg.CoStGcn(pkg.ntu_graph().A).eval().to(DEV)
    with pytest.raises(TypeError, match="looks ahead"):
        ntu_intake.set_ntu_intake(co)
