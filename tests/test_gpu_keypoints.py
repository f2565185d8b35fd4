"""Kinetics keypoint intake on the device: the two entries of csrc/keypoints.hip against what the reference's own feeder wrote
(tests/golden/g15_keypoints.npz), against the numpy oracle (tests/keypoint_oracle.py) and against each other, and the models
that run them in front of the unchanged path.

Every comparison is bit for bit (uint8 views / ``torch.equal``): the intake rounds nothing -- one fp32 subtraction that the
oracle performs as well, fp64 sums that decide an order -- and a model with the switch on runs the very kernels its twin
runs on the selected tensor.  The sweep's shapes are the issue's: 260 items is more than one batch of the kernel for every
(P, V) of the sweep (a batch holds 4..32 items) with a partial last batch, V = 25 and the one-float offset take the dword
staging path, V = 64 with P = 8 the largest item."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _bootstrap
from tests import keypoint_oracle as ko
from tests.helpers import GOLDEN, guarded_allocs, randomise_unit_

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native, keypoints = pkg.native, pkg.keypoints
DEV = "cuda:0"
PAD = 1024                      # guard elements on either side of a guarded operand (a multiple of 4: alignment is kept)


def _same_bytes(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def _people(n, t, p, v, seed):
    """Seeded keypoints (N, T, P, V, 3): coordinates and scores uniform in [0, 1), a sixth of the joints undetected (score 0,
    coordinates kept), a fifth of the people absent (all zero), a few exact halves."""
    g = torch.Generator().manual_seed(seed)
    k = torch.rand((n, t, p, v, 3), generator=g)
    k[..., 2] = torch.where(torch.rand((n, t, p, v), generator=g) < 1 / 6, torch.zeros(()), k[..., 2])
    k[..., 0] = torch.where(torch.rand((n, t, p, v), generator=g) < 1 / 16, torch.full((), 0.5), k[..., 0])
    k[..., 1] = torch.where(torch.rand((n, t, p, v), generator=g) < 1 / 16, torch.full((), 0.5), k[..., 1])
    k[torch.rand((n, t, p), generator=g) < 1 / 5] = 0.0
    return k


def _offset(t, words):
    """A device copy of ``t`` whose base lies ``words`` floats behind a fresh allocation's (1: not 16-byte aligned)."""
    buf = torch.empty((t.numel() + words + 4,), device=DEV, dtype=torch.float32)
    view = buf[words:words + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (4 * words) % 16
    return view


def _clip_entry(k, m, out=None):
    n, t, p, v, _ = k.shape
    out = torch.empty((n, 3, t, v, m), device=DEV, dtype=torch.float32) if out is None else out
    rc = native.lib().csk_select_people_f32(native.ptr(k), native.ptr(out), n, t, p, v, m, native.stream_of(k))
    torch.cuda.synchronize()
    return rc, out


def _frames_entry(frames, m, dsts=None, r=None, p=None):
    n, p_, v, _ = frames[0].shape
    dsts = [torch.empty((n, 3, v, m), device=DEV, dtype=torch.float32) for _ in frames] if dsts is None else dsts
    src = (ctypes.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
    dst = (ctypes.c_void_p * len(frames))(*[d.data_ptr() for d in dsts])
    rc = native.lib().csk_select_people_frames_f32(src, dst, len(frames) if r is None else r, n, p_ if p is None else p, v, m,
                                                   native.stream_of(frames[0]))
    torch.cuda.synchronize()
    return rc, dsts


# ---- 1. the entries against the reference ---------------------------------------------------------------------------------
def test_clip_entry_equals_what_the_reference_wrote():
    g = np.load(os.path.join(GOLDEN, "g15_keypoints.npz"))
    for i in range(3):
        k, want = torch.from_numpy(g[f"s{i}/k"])[None], g[f"s{i}/want"]
        got = keypoints.select_people_clip(k.to(DEV), 2)
        assert got.shape == (1, 3, k.shape[1], 18, 2)
        assert _same_bytes(got[0].cpu().numpy(), want), i
        assert int((np.signbit(want[1]) & (want[1] == 0)).sum()) >= 3           # the -0.0 of y == 0.5 is in the comparison


@pytest.mark.parametrize("r", [1, 3, 8])
def test_frames_entry_equals_the_clip_entry(r):
    for n, p, v, m in ((5, 5, 18, 2), (130, 8, 25, 3), (3, 1, 1, 1)):
        k = _people(n, r, p, v, 40 + r + n).to(DEV)
        rc, clip = _clip_entry(k, m)
        rc2, got = _frames_entry([k[:, t].contiguous() for t in range(r)], m)
        assert rc == 0 and rc2 == 0
        assert torch.equal(torch.stack(got, dim=2), clip), (n, p, v, m)


# ---- 2. the sweep against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n,t", [(1, 1), (3, 7), (130, 2)])
def test_sweep_against_the_oracle(n, t, offset):
    cases = 0
    for p in (1, 2, 5, 8):
        for v in (1, 18, 25, 64):
            k = _people(n, t, p, v, 1000 * n + 10 * p + v)
            kd = _offset(k, offset)
            frames = [_offset(k[:, f], offset) for f in range(t)]
            for m in sorted({1, min(2, p), p}):
                want = ko.select_people_clip(k.numpy(), m)
                out = _offset(torch.zeros((n, 3, t, v, m)), offset)
                rc, got = _clip_entry(kd, m, out=out)
                assert rc == 0 and _same_bytes(got.cpu().numpy(), want), (p, v, m)
                rc, got = _frames_entry(frames, m)
                assert rc == 0 and _same_bytes(torch.stack(got, dim=2).cpu().numpy(), want), (p, v, m)
                cases += 1
    assert cases == 4 * (1 + 2 + 3 + 3)


# ---- 3. the order ----------------------------------------------------------------------------------------------------------------
def _order_of(k, m):
    """The people the clip entry kept, read off a marker: joint 0 of person p has x = 0.5 + (p + 1) / 16 and a score."""
    rc, out = _clip_entry(k.to(DEV), m)
    assert rc == 0
    return torch.round(out[:, 0, :, 0, :].cpu() * 16 - 1).to(torch.int64)      # (N, T, M)


def test_exact_ties_among_present_people_resolve_by_index():
    p, v = 6, 18
    k = torch.zeros((1, 3, p, v, 3))
    k[..., 0] = (0.5 + (torch.arange(p) + 1) / 16)[None, None, :, None]
    k[..., 2] = 0.5                                         # every sum is 9.0
    k[0, 1, 4, :, 2] = 0.75                                 # frame 1: person 4 leads, the rest tie
    k[0, 2, 0, :, 2], k[0, 2, 3, :2, 2], k[0, 2, 3, 2:4, 2] = 0.25, 1.0, 0.0     # frame 2: 0 trails; 3 has the same sum from other terms
    got = _order_of(k, p)
    assert got[0, 0].tolist() == [0, 1, 2, 3, 4, 5]
    assert got[0, 1].tolist() == [4, 0, 1, 2, 3, 5]
    assert got[0, 2].tolist() == [1, 2, 3, 4, 5, 0]
    assert _same_bytes(_clip_entry(k.to(DEV), p)[1].cpu().numpy(), ko.select_people_clip(k.numpy(), p))


def test_a_nan_score_sum_goes_last():
    p, v = 4, 18
    k = torch.zeros((2, 1, p, v, 3))
    k[..., 0] = (0.5 + (torch.arange(p) + 1) / 16)[None, None, :, None]
    k[..., 2] = torch.tensor([0.1, 0.2, 0.3, 0.4])[None, None, :, None]
    k[0, 0, 3, 5, 2] = float("nan")                         # the best person gets a NaN score: behind every number
    k[1, 0, 0, 1, 2], k[1, 0, 2, 7, 2] = float("nan"), float("inf")
    k[1, 0, 2, 8, 2] = float("-inf")                        # inf - inf: a NaN sum as well; NaN sums by index
    got = _order_of(k, p)
    assert got[0, 0].tolist() == [2, 1, 0, 3] and got[1, 0].tolist() == [3, 1, 0, 2]
    assert _same_bytes(_clip_entry(k.to(DEV), p)[1].cpu().numpy(), ko.select_people_clip(k.numpy(), p))


def test_negative_zero_scores_count_as_zero():
    k = _people(2, 3, 5, 18, 77)
    k[..., 2] = torch.where(k[..., 2] == 0, torch.full((), -0.0), k[..., 2])
    rc, got = _clip_entry(k.to(DEV), 2)
    got = got.cpu()
    absent = got[:, 2] == 0
    assert rc == 0 and int(absent.sum()) > 10 and bool(torch.signbit(got[:, 2][absent]).all())        # the score itself is kept
    for c in (0, 1):
        assert not got[:, c][absent].any() and not torch.signbit(got[:, c][absent]).any()              # +0.0
    assert _same_bytes(got.numpy(), ko.select_people_clip(k.numpy(), 2))


# ---- 4. operand bounds -----------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("n,p,v,m", [(5, 5, 18, 2), (130, 5, 18, 2), (3, 8, 64, 8), (7, 3, 25, 1), (1, 1, 1, 1)])
def test_both_entries_stay_inside_their_operands(n, p, v, m):
    """k, out and every frame buffer between NaN guards: a write outside an operand breaks a guard, a read outside one brings
    a NaN into a sum or an output.  Outputs are finite and bitwise those of the unguarded run."""
    t = 4
    k = _people(n, t, p, v, 500 + n + p + v).to(DEV)
    rc, plain = _clip_entry(k, m)
    assert rc == 0
    bufs = []

    def guarded(shape, values=None):
        buf, view = _guarded(shape, values)
        bufs.append((buf, view.numel()))
        return view

    rc, got = _clip_entry(guarded(k.shape, k), m, out=guarded(plain.shape))
    assert rc == 0 and torch.isfinite(got).all() and torch.equal(got, plain)
    srcs = [guarded(k[:, f].shape, k[:, f]) for f in range(t)]
    dsts = [guarded((n, 3, v, m)) for _ in range(t)]
    rc, got = _frames_entry(srcs, m, dsts=dsts)
    assert rc == 0 and torch.isfinite(torch.stack(got)).all() and torch.equal(torch.stack(got, dim=2), plain)
    assert len(bufs) == 2 + 2 * t and all(_intact(buf, cnt) for buf, cnt in bufs)
    with guarded_allocs(pad=PAD) as ga:                     # the tensor the host layer allocates, guarded by the helper
        out = keypoints.select_people_clip(k, m)
    torch.cuda.synchronize()
    assert ga.count == 1 and torch.equal(out, plain) and _intact(out._base, out.numel())


def test_refused_calls_launch_nothing():
    k = _people(2, 4, 5, 18, 10).to(DEV)
    out = torch.full((2, 3, 4, 18, 2), 3.0, device=DEV)
    rc, _ = _clip_entry(k, 6, out=out)                      # M > P
    assert rc == -2 and native.lib().csk_last_error() and bool((out == 3.0).all())
    wide = torch.zeros((1, 1, 2, 65, 3), device=DEV)
    rc, _ = _clip_entry(wide, 2, out=out)                   # V > 64
    assert rc == -2 and bool((out == 3.0).all())
    frames = [k[:, t].contiguous() for t in range(4)]
    dsts = [torch.full((2, 3, 18, 2), 3.0, device=DEV) for _ in frames]
    for r, p in ((0, None), (9, None), (None, 9)):
        rc, _ = _frames_entry(frames, 2, dsts=dsts, r=r, p=p)
        assert rc == -2 and all(bool((d == 3.0).all()) for d in dsts), (r, p)
    rc, _ = _frames_entry(frames, 2, dsts=[dsts[0], dsts[1], dsts[0], dsts[3]])
    assert rc == -1 and all(bool((d == 3.0).all()) for d in dsts)
    with pytest.raises(ValueError, match="people_in"):
        keypoints.select_people_clip(k, 6)
    with pytest.raises(RuntimeError, match=r"\(N, T, P, V, 3\)"):
        keypoints.select_people_clip(k[..., :2].contiguous())


# ---- models ------------------------------------------------------------------------------------------------------------------------
def _twins(cls, n_copies, shape_t=300, seed=7, **kw):
    nets = [cls(pkg.kinetics_graph().A, (3, shape_t, 18, 2), 60, **kw).eval() for _ in range(n_copies)]
    randomise_unit_(nets[0], seed, attn_scale=1 / 18 if "AGcn" in cls.__name__ else 1.0)
    for net in nets[1:]:
        net.load_state_dict(nets[0].state_dict())
    return [net.to(DEV) for net in nets]


@pytest.mark.parametrize("model", ["StGcn", "AGcn", "STr"])
def test_clip_model_with_the_switch_on_equals_its_twin_on_the_selected_clip(model):
    net, twin = _twins(getattr(pkg, model), 2, shape_t=20)
    assert keypoints.set_keypoint_intake(net) is net and twin.keypoint_intake is False
    k = _people(2, 20, 5, 18, 11).to(DEV)
    with torch.no_grad():
        selected = keypoints.select_people_clip(k, 2)
        got, want = net(k), twin(selected)
        assert got.shape == (2, 60) and torch.equal(got, want)
        unranked = (k[:, :, :2] - torch.tensor([0.5, 0.5, 0.0], device=DEV)).permute(0, 4, 1, 3, 2).contiguous()
        assert not torch.equal(got, twin(unranked))
        with pytest.raises(RuntimeError, match="keypoint clip"):
            net(selected)


CO = dict(pool_size=3, pool_padding=1)      # tests/test_gpu_stream_reset.py: first logits with frame 81, then every 4 frames
T_SEQ = 96
N = 5


def _sequence(seed, t=T_SEQ, n=N):
    """Keypoint frames (T, N, 5, 18, 3) on the device and the frames of the selected clip (T, N, 3, 18, 2)."""
    key = (seed, t, n)
    if key not in _sequence.cache:
        k = _people(n, t, 5, 18, seed).to(DEV)
        _sequence.cache[key] = (k.permute(1, 0, 2, 3, 4).contiguous(), keypoints.select_people_clip(k, 2).permute(2, 0, 1, 3, 4).contiguous())
    return _sequence.cache[key]


_sequence.cache = {}


def _predictions(net, frames, r, lo=0, hi=None):
    out = []
    hi = len(frames) if hi is None else hi
    for t in range(lo, hi, r):
        cyc = [frames[t + f] for f in range(r)]
        logits = net.forward_cycle(cyc) if r > 1 else [o for o in [net.forward_step(cyc[0])] if o is not None]
        out += [(t + r, o.clone()) for o in logits]
    return out


def _same(a, b):
    return len(a) == len(b) and all(ta == tb and torch.equal(x, y) for (ta, x), (tb, y) in zip(a, b))


@pytest.mark.parametrize("native_plan,r,prepasses", [(True, 4, False), (False, 1, False), (True, 4, True)])
def test_stepping_on_keypoint_frames_equals_the_twin_stepped_on_the_selected_frames(native_plan, r, prepasses):
    """Logits and every ring of the slab, 5 streams.  ``prepasses``: pre-normalisation and the bone-motion modality on in both
    models -- the twin is fed the selected frames, so the intake must have run in front of the other two."""
    net, twin = _twins(pkg.CoStGcn, 2, **CO)
    for m in (net, twin):
        m.use_native_plan = native_plan
        if prepasses:
            pkg.set_input_modality(pkg.set_pre_normalization(m), "bone_motion")
    keypoints.set_keypoint_intake(net)
    raw, selected = _sequence(21)
    got, want = _predictions(net, raw, r), _predictions(twin, selected, r)
    assert len(want) == 4 and _same(got, want)
    assert bool(net.__dict__.get("_plan")) == native_plan
    mine, theirs = net._state_tensors(), twin._state_tensors()
    assert len(mine) == len(theirs) and all(torch.equal(a, b) for a, b in zip(mine, theirs))       # no state of its own
    assert net.state_bytes() == twin.state_bytes() and net.move_signature() == twin.move_signature()
    assert net.scratch_bytes() - twin.scratch_bytes() == 4 * net.max_cycle * N * 3 * 18 * 2
    assert net.stage("keypoints").scratch.shape == (net.max_cycle, N, 3, 18, 2) and twin.stage("keypoints").scratch is None
    with pytest.raises(RuntimeError, match=r"clean_state\(\)"):
        keypoints.set_keypoint_intake(net, enabled=False)
    with pytest.raises(RuntimeError, match="does not match"):
        net.forward_step(selected[0])


def test_a_peek_changes_nothing():
    peeker, twin = _twins(pkg.CoStGcn, 2, **CO)
    for net in (peeker, twin):
        keypoints.set_keypoint_intake(net)
    raw, selected = _sequence(21)
    assert peeker.forward_step(raw[5], update_state=False) is None          # a peek on a fresh slab: binds
    clip_form = raw.permute(1, 0, 2, 3, 4).contiguous()                     # (N, T, P, V, 3)
    n_pred = 0
    for t in range(T_SEQ):
        p1 = None
        if t in (1, 37, 80, 84):
            p1 = peeker.forward_step(raw[t], update_state=False)
            if t in (37, 80):
                ahead = peeker.forward_steps(clip_form[:, t:t + 8].contiguous(), update_state=False)
                assert ahead.shape[2] == (2 if t == 80 else 0)
        got, want = peeker.forward_step(raw[t]), twin.forward_step(raw[t])
        assert (got is None) == (want is None), t
        if want is not None:
            assert torch.equal(got, want), t
            n_pred += 1
            if t in (80, 84):
                assert torch.equal(p1, want), t
    assert n_pred == 4 and all(torch.equal(a, b) for a, b in zip(peeker._state_tensors(), twin._state_tensors()))


def test_forward_steps_and_frame_mode_take_keypoint_clips():
    net, twin = _twins(pkg.CoStGcn, 2, **CO)
    keypoints.set_keypoint_intake(net)
    raw, selected = _sequence(21)
    k = raw[:88].permute(1, 0, 2, 3, 4).contiguous()
    x = selected[:88].permute(1, 2, 0, 3, 4).contiguous()
    with torch.no_grad():
        got, want = net.forward_steps(k), twin.forward_steps(x)
        assert want.shape == (N, 60, 2) and torch.equal(got, want)
        assert torch.equal(net(k, "frame"), twin(x, "frame"))
        assert torch.equal(net(k[:, :40].contiguous(), "clip"), twin(x[:, :, :40].contiguous(), "clip"))


def test_stream_shards_with_the_switch_on():
    def make():
        return _twins(pkg.CoStGcn, 1, **CO)[0]
    shards, twin = pkg.parallel.StreamShards(make, N, 2, DEV), pkg.parallel.StreamShards(make, N, 2, DEV)
    assert keypoints.set_keypoint_intake(shards) is shards and all(m.keypoint_intake for m in shards.models)
    raw, selected = _sequence(21)
    n_pred = 0
    for t in range(0, T_SEQ, 4):
        got, want = shards.forward_cycle(list(raw[t:t + 4])), twin.forward_cycle(list(selected[t:t + 4]))
        assert (got is None) == (want is None), t
        if want is not None:
            assert torch.equal(got, want), t
            n_pred += 1
    assert n_pred == 4 and [m.stage("keypoints").scratch.shape[1] for m in shards.models] == [3, 2]
    assert shards.scratch_bytes() - twin.scratch_bytes() == 4 * 8 * N * 3 * 18 * 2


def test_online_ensemble_with_the_switch_on_every_member():
    nets = _twins(pkg.CoStGcn, 2, **CO) + _twins(pkg.CoStGcn, 2, seed=8, **CO)       # (joint, joint twin, bone, bone twin)
    for net in nets[2:]:
        pkg.set_input_modality(net, "bone")
    for net in (nets[0], nets[2]):
        keypoints.set_keypoint_intake(net)
    ens, twin = pkg.fusion.OnlineEnsemble([nets[0], nets[2]]), pkg.fusion.OnlineEnsemble([nets[1], nets[3]])
    raw, selected = _sequence(21)
    n_pred = 0
    for t in range(0, T_SEQ, 4):
        got, want = ens.forward_cycle(list(raw[t:t + 4])), twin.forward_cycle(list(selected[t:t + 4]))
        assert (got is None) == (want is None), t
        if want is not None:
            assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)), t
            n_pred += len(want)
    assert n_pred == 4


def test_prime_state_on_a_keypoint_history_equals_the_twins_on_the_selected_clip():
    net, twin = _twins(pkg.CoStGcn, 2, **CO)
    keypoints.set_keypoint_intake(net)
    raw, selected = _sequence(21)
    hist_k = raw[:80].permute(1, 0, 2, 3, 4).contiguous()               # (N, 80, 5, 18, 3)
    hist_x = selected[:80].permute(1, 2, 0, 3, 4).contiguous()          # (N, 3, 80, 18, 2)
    got, want = net.prime_state(hist_k), twin.prime_state(hist_x)
    assert torch.equal(got.packed, want.packed) and torch.equal(got.ages, want.ages) and got.signature == want.signature
    with pytest.raises(RuntimeError, match="keypoint history shape"):
        net.prime_state(hist_x)
    # streams primed into a slab at frame 88 continue on keypoint frames as the twin's continue on the selected ones
    assert _same(_predictions(net, raw, 4, 0, 88), _predictions(twin, selected, 4, 0, 88))
    net.prime_streams(hist_k[[1, 3]].contiguous(), [1, 3])
    twin.prime_streams(hist_x[[1, 3]].contiguous(), [1, 3])
    tail = _predictions(twin, selected, 4, 88)
    assert len(tail) == 2 and _same(_predictions(net, raw, 4, 88), tail)
    assert all(torch.equal(a, b) for a, b in zip(net._state_tensors(), twin._state_tensors()))


def test_the_switch_is_off_by_default_and_then_nothing_is_allocated_or_launched():
    net, plain = _twins(pkg.CoStGcn, 2, **CO)
    assert keypoints.set_keypoint_intake(net, enabled=False) is net and net.keypoint_intake is False
    _, selected = _sequence(21)
    cyc = [selected[0], selected[1], selected[2], selected[3]]
    assert _same(_predictions(net, selected, 4, 0, 8), _predictions(plain, selected, 4, 0, 8)) and net.stage("keypoints").frames(cyc) is cyc
    assert net.stage("keypoints").scratch is None and net.scratch_bytes() == plain.scratch_bytes()
    x = selected[:20].permute(1, 2, 0, 3, 4).contiguous()
    assert net._intake_clip(x) is x
    before = net.scratch_bytes()
    net.clean_state()
    keypoints.set_keypoint_intake(net)                  # a bound slab that has not stepped takes the switch and binds its scratch
    assert net.stage("keypoints").scratch.shape == (net.max_cycle, N, 3, 18, 2) and net.scratch_bytes() - before == 4 * net.max_cycle * N * 3 * 18 * 2
    keypoints.set_keypoint_intake(net, enabled=False)
    assert net.stage("keypoints").scratch is None and net.scratch_bytes() == before
