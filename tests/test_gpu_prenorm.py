"""Pre-normalisation of raw skeleton frames on the device: the two entries of csrc/prenorm.hip against what the reference's
own function wrote (tests/golden/g14_prenorm.npz) and against each other, and the models that run them in front of the
unchanged path.

Parity with the reference is within 1e-5 absolute at |want| <= 8: the device and the numpy oracle differ only by fp64 libm
ulps in the 18 matrix entries, i.e. by at most one flipped fp32 rounding per stage (<= ~3 ulp at magnitude 8 ~ 3e-6), and the
oracle is within 1e-6 of the reference (tests/test_prenorm_cpu.py) -- a factor of 10^3 below the smallest distance of a
wrong-on-purpose oracle.  Everything else is ``torch.equal``: the step entry latches through the same device function as
the clip entry, and a model with the switch on runs the very kernels its twin runs on the normalised tensor."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _bootstrap
from tests import prenorm_oracle as po
from tests.helpers import GOLDEN, check_parity, randomise_unit_

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native, prenorm = pkg.native, pkg.prenorm
DEV = "cuda:0"
JOINTS = (0, 1, 8, 4)
PAD = 1024                      # guard elements on either side of a guarded operand (a multiple of 4: alignment is kept)


def _golden(tag):
    g = np.load(os.path.join(GOLDEN, "g14_prenorm.npz"))
    return torch.from_numpy(g[f"{tag}/x"]), torch.from_numpy(g[f"{tag}/want"])


def _raw(n, t, v, m, seed):
    """Seeded standard-normal joints (N, 3, T, V, M) with null data: one null joint of the main body, one null frame of the
    last person of sample 0 (not frame 0), and -- for M = 2 -- an absent second person in the last sample."""
    x = torch.randn((n, 3, t, v, m), generator=torch.Generator().manual_seed(seed))
    x[0, :, min(2, t - 1), 5, 0] = 0.0
    x[0, :, t - 2, :, m - 1] = 0.0
    if m == 2:
        x[n - 1, :, :, :, 1] = 0.0
    return x


def _clip_entry(x, out=None, joints=JOINTS):
    n, _, t, v, m = x.shape
    out = torch.empty(x.shape, device=x.device, dtype=torch.float32) if out is None else out
    rc = native.lib().csk_prenorm_f32(native.ptr(x), native.ptr(out), n, t, v, m, *joints, native.stream_of(x))
    torch.cuda.synchronize()
    return rc, out


def _state(n):
    return torch.zeros((n, 18), device=DEV, dtype=torch.float64), torch.zeros((n,), device=DEV, dtype=torch.int32)


def _frames_entry(frames, rot, flags, update, dsts=None, joints=JOINTS, r=None):
    n, _, v, m = frames[0].shape
    dsts = [torch.empty(frames[0].shape, device=DEV, dtype=torch.float32) for _ in frames] if dsts is None else dsts
    src = (ctypes.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
    dst = (ctypes.c_void_p * len(frames))(*[d.data_ptr() for d in dsts])
    rc = native.lib().csk_prenorm_frames_f32(src, dst, len(frames) if r is None else r, native.ptr(rot), native.ptr(flags), update,
                                             n, v, m, *joints, native.stream_of(frames[0]))
    torch.cuda.synchronize()
    return rc, dsts


def _split(x):
    return [x[:, :, t].contiguous() for t in range(x.shape[2])]


# ---- 1. the clip entry against the reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["ntu", "kin"])
def test_clip_entry_equals_what_the_reference_wrote(tag):
    x, want = _golden(tag)
    got = pkg.pre_normalize_clip(x.to(DEV))
    assert got.shape == x.shape and got.data_ptr() != x.data_ptr()
    err = check_parity(got.cpu(), want, tol=1e-5, ref_cap=8.0, tag=tag, what="pre_normalize_clip vs preprocess.pre_normalization")
    oracle = torch.from_numpy(po.pre_normalize_clip(x.numpy()))
    print(f"{tag}: max |device - reference| = {err:.3e}; max |device - oracle| = {float((got.cpu() - oracle).abs().max()):.3e}")
    rc, again = _clip_entry(x.to(DEV))
    assert rc == 0 and torch.equal(again, got)


def test_null_joints_frames_and_persons_come_out_zero():
    x, _ = _golden("ntu")
    got = pkg.pre_normalize_clip(x.to(DEV)).cpu()
    null = torch.from_numpy(po.null_mask(x.numpy().transpose(0, 2, 1, 3, 4)))             # (N, T, V, M)
    assert int(null.sum()) == 6 * 25 + 25 + 1
    assert not got[1, :, :, :, 1].any() and not got[0, :, 2, :, 1].any() and not got[2, :, 3, 7, 0].any()
    zero = (got == 0).all(dim=1)                                                        # (N, T, V, M): all three channels
    centre = torch.zeros_like(null)
    centre[:, :, 1, 0] = True                               # the centre joint itself is x - x = 0
    assert torch.equal(zero, null | centre)
    assert not torch.signbit(got.permute(0, 2, 1, 3, 4)[null[:, :, None].expand(-1, -1, 3, -1, -1)]).any()      # +0


# ---- 2. the step entry against the clip entry -----------------------------------------------------------------------------
SHAPES = [(3, 25, 2), (2, 18, 1), (3, 25, 1), (5, 18, 1)]       # (N, V, M); 3 * 25 * 1 and 5 * 18 * 1 floats per channel: scalar tails


@pytest.mark.parametrize("n,v,m", SHAPES)
def test_step_entry_equals_the_clip_entry_bit_for_bit(n, v, m):
    """T = 8 frames in cycles of 8, 4 and 1: the first launch latches, the later ones reuse the latch (r = 1: every launch but
    the first).  update = 0 returns the same frames and leaves rot / has_rot bitwise untouched, latched or not."""
    x = _raw(n, 8, v, m, 300 + n + v + m).to(DEV)
    rc, clip = _clip_entry(x)
    assert rc == 0 and torch.isfinite(clip).all()
    want, frames = _split(clip), _split(x)
    final = None
    for r in (8, 4, 1):
        rot, flags = _state(n)
        for t in range(0, 8, r):
            if t in (0, 4):                                  # a peek first: fresh state at 0, latched state at 4
                keep = rot.clone(), flags.clone()
                rc, got = _frames_entry(frames[t:t + r], rot, flags, 0)
                assert rc == 0 and torch.equal(rot, keep[0]) and torch.equal(flags, keep[1]), (r, t)
                assert all(torch.equal(g, w) for g, w in zip(got, want[t:t + r])) and bool(flags.all()) == (t == 4), (r, t)
            rc, got = _frames_entry(frames[t:t + r], rot, flags, 1)
            assert rc == 0 and all(torch.equal(g, w) for g, w in zip(got, want[t:t + r])), (r, t)
            assert bool(flags.all())
        final = rot.clone() if final is None else final
        assert torch.equal(rot, final), r                   # every cycle length latches the same 18 doubles
    # the latched matrices are rotations, and the ones the oracle computes
    rz, rx = final.view(n, 2, 3, 3)[:, 0].cpu(), final.view(n, 2, 3, 3)[:, 1].cpu()
    eye = torch.eye(3, dtype=torch.float64).expand(n, 3, 3)
    assert float((rz @ rz.transpose(1, 2) - eye).abs().max()) < 1e-14 and float((rx @ rx.transpose(1, 2) - eye).abs().max()) < 1e-14
    for i in range(n):
        orz, orx, _, _ = po.latch(x[i, :, 0].cpu().numpy())
        assert np.abs(rz[i].numpy() - orz).max() < 1e-12 and np.abs(rx[i].numpy() - orx).max() < 1e-12
    # the step form on the golden input is the reference's output as well
    gx, gwant = _golden("ntu" if (v, m) == (25, 2) else "kin") if (n, v, m) in ((3, 25, 2), (2, 18, 1)) else (None, None)
    if gx is not None:
        rot, flags = _state(n)
        rc, got = _frames_entry(_split(gx.to(DEV)), rot, flags, 1)
        assert rc == 0
        check_parity(torch.stack(got, dim=2).cpu(), gwant, tol=1e-5, ref_cap=8.0, what="csk_prenorm_frames_f32 vs reference")


def test_a_stream_with_a_clear_flag_latches_from_the_cycle_it_is_in():
    """Flags (1, 0, 1) going into frame 3: stream 1 latches from frame 3 -- the clip entry on x[:, :, 3:] -- while its
    neighbours keep the matrices of frame 0."""
    x = _raw(3, 8, 25, 2, 77).to(DEV)
    clip, late = _clip_entry(x)[1], _clip_entry(x[:, :, 3:].contiguous())[1]
    rot, flags = _state(3)
    frames = _split(x)
    assert _frames_entry(frames[:3], rot, flags, 1)[0] == 0
    flags[1] = 0
    rc, got = _frames_entry(frames[3:], rot, flags, 1)
    got = torch.stack(got, dim=2)
    assert rc == 0 and torch.equal(got[[0, 2]], clip[[0, 2], :, 3:]) and torch.equal(got[1], late[1])
    assert not torch.equal(got[1], clip[1, :, 3:]) and bool(flags.all())


# ---- 3. operand bounds -------------------------------------------------------------------------------------------------------
def _guarded(shape, dtype, values=None):
    """A tensor of ``shape`` in the middle of a buffer whose PAD elements on either side are NaN (int32: -7)."""
    n = int(np.prod(shape))
    fill = -7 if dtype == torch.int32 else float("nan")
    buf = torch.full((n + 2 * PAD,), fill, device=DEV, dtype=dtype)
    view = buf[PAD:PAD + n].view(shape)
    if values is not None:
        view.copy_(values)
    return buf, view


def _intact(buf, n):
    edge = torch.cat([buf[:PAD], buf[PAD + n:]])
    return bool((edge == -7).all()) if buf.dtype == torch.int32 else bool(torch.isnan(edge).all())


@pytest.mark.parametrize("n,v,m", SHAPES)
def test_both_entries_stay_inside_their_operands(n, v, m):
    """x, out, rot, has_rot and every frame buffer between guards: a read outside an operand brings a NaN into the result (or
    into a latched matrix), a write outside one breaks a guard.  Outputs are finite and bitwise those of the unguarded run."""
    x = _raw(n, 4, v, m, 500 + n + v + m).to(DEV)
    rc, plain = _clip_entry(x)
    rot0, flags0 = _state(n)
    rc2, plain_frames = _frames_entry(_split(x), rot0, flags0, 1)
    assert rc == 0 and rc2 == 0
    bufs = []

    def guarded(shape, dtype, values=None):
        buf, view = _guarded(shape, dtype, values)
        bufs.append((buf, view.numel()))
        return view

    out = guarded(x.shape, torch.float32)
    rc, got = _clip_entry(guarded(x.shape, torch.float32, x), out=out)
    assert rc == 0 and torch.isfinite(got).all() and torch.equal(got, plain)
    rot, flags = guarded((n, 18), torch.float64, rot0 * 0), guarded((n,), torch.int32, flags0 * 0)
    srcs = [guarded(f.shape, torch.float32, f) for f in _split(x)]
    dsts = [guarded(f.shape, torch.float32) for f in srcs]
    for update in (0, 1, 1):                                # a peek, the latching launch, a launch that reads the latch
        rc, got = _frames_entry(srcs, rot, flags, update, dsts=dsts)
        assert rc == 0 and all(torch.isfinite(g).all() and torch.equal(g, w) for g, w in zip(got, plain_frames)), update
    assert torch.equal(rot, rot0) and torch.equal(flags, flags0) and torch.isfinite(rot).all()
    assert len(bufs) == 4 + 2 * 4 and all(_intact(buf, k) for buf, k in bufs)


def test_refused_calls_launch_nothing():
    x = _raw(2, 4, 25, 2, 10).to(DEV)
    out = torch.full(x.shape, 3.0, device=DEV)
    for joints in ((0, 25, 8, 4), (0, 1, -1, 4)):
        rc, _ = _clip_entry(x, out=out, joints=joints)
        assert rc == -2 and native.lib().csk_last_error() and bool((out == 3.0).all())
    frames = _split(x)
    dsts = [torch.full(frames[0].shape, 3.0, device=DEV) for _ in frames]
    rot, flags = _state(2)
    for joints, r in (((0, 1, 8, 25), None), (JOINTS, 0), (JOINTS, 9)):
        rc, _ = _frames_entry(frames, rot, flags, 1, dsts=dsts, joints=joints, r=r)
        assert rc == -2 and all(bool((d == 3.0).all()) for d in dsts) and not rot.any() and not flags.any(), (joints, r)
    with pytest.raises(ValueError, match="outside"):
        pkg.pre_normalize_clip(x, zaxis=(0, 25))
    with pytest.raises(RuntimeError, match=r"\(N, 3, T, V, M\)"):
        pkg.pre_normalize_clip(x[:, :2].contiguous())


# ---- models ---------------------------------------------------------------------------------------------------------------------
def _twins(cls, n_copies, shape_t=300, seed=7, **kw):
    nets = [cls(pkg.ntu_graph().A, (3, shape_t, 25, 2), 60, **kw).eval() for _ in range(n_copies)]
    randomise_unit_(nets[0], seed, attn_scale=1 / 25 if "AGcn" in cls.__name__ else 1.0)
    for net in nets[1:]:
        net.load_state_dict(nets[0].state_dict())
    return [net.to(DEV) for net in nets]


@pytest.mark.parametrize("model", ["StGcn", "AGcn", "STr"])
def test_clip_model_with_the_switch_on_equals_its_twin_on_the_normalised_clip(model):
    net, twin = _twins(getattr(pkg, model), 2, shape_t=20)
    assert pkg.set_pre_normalization(net) is net and twin.pre_normalization is False
    x = _raw(2, 20, 25, 2, 11).to(DEV)
    with torch.no_grad():
        got, want, on_raw = net(x), twin(pkg.pre_normalize_clip(x)), twin(x)
        assert torch.equal(got, want) and not torch.equal(got, on_raw)
        pkg.set_input_modality(net, "bone_motion")
        pkg.set_input_modality(twin, "bone_motion")
        assert torch.equal(net(x), twin(pkg.pre_normalize_clip(x)))


def test_continual_model_clip_forward_takes_the_clip_form():
    net, twin = _twins(pkg.CoStGcn, 2, pool_size=3, pool_padding=1)
    pkg.set_pre_normalization(net)
    x = _raw(2, 40, 25, 2, 12).to(DEV)
    with torch.no_grad():
        assert torch.equal(net(x, "clip"), twin(pkg.pre_normalize_clip(x), "clip"))


CO = dict(pool_size=3, pool_padding=1)      # tests/test_gpu_stream_reset.py: first logits with frame 81, then every 4 frames
T_SEQ = 96
N = 5


def _sequence(seed, t=T_SEQ, n=N):
    """Raw joints (N, 3, T, V, M) on the device and the frames of the clip form, (T, N, 3, V, M) both."""
    key = (seed, t, n)
    if key not in _sequence.cache:
        x = _raw(n, t, 25, 2, seed).to(DEV)
        _sequence.cache[key] = (x.permute(2, 0, 1, 3, 4).contiguous(), pkg.pre_normalize_clip(x).permute(2, 0, 1, 3, 4).contiguous())
    return _sequence.cache[key]


_sequence.cache = {}


def _predictions(net, frames, r, lo=0, hi=None, rows=None):
    out = []
    hi = len(frames) if hi is None else hi
    for t in range(lo, hi, r):
        cyc = [frames[t + f] if rows is None else frames[t + f][rows].contiguous() for f in range(r)]
        logits = net.forward_cycle(cyc) if r > 1 else [o for o in [net.forward_step(cyc[0])] if o is not None]
        out += [(t + r, o.clone()) for o in logits]
    return out


def _same(a, b):
    return len(a) == len(b) and all(ta == tb and torch.equal(x, y) for (ta, x), (tb, y) in zip(a, b))


@pytest.mark.parametrize("native_plan,r,modality", [(True, 4, "joint"), (False, 1, "joint"), (True, 1, "bone_motion"), (False, 4, "bone_motion")])
def test_stepping_on_raw_frames_equals_the_twin_stepped_on_the_clip_form(native_plan, r, modality):
    """Logits and features (every ring of the slab), 5 streams; with a modality on top, the twin in that modality fed the
    normalised frames -- so the motion state holds normalised frames."""
    net, twin = _twins(pkg.CoStGcn, 2, **CO)
    for m in (net, twin):
        m.use_native_plan = native_plan
        pkg.set_input_modality(m, modality)
    pkg.set_pre_normalization(net)
    raw, normed = _sequence(21)
    got, want = _predictions(net, raw, r), _predictions(twin, normed, r)
    assert len(want) == 4 and _same(got, want)
    theirs = twin._state_tensors()
    assert all(torch.equal(a, b) for a, b in zip(net._state_tensors()[:len(theirs)], theirs))
    mine = net._state_tensors()[len(theirs):]
    assert len(mine) == 2 and mine[0] is net.stage("prenorm").rot and mine[1] is net.stage("prenorm").flags and bool(net.stage("prenorm").flags.all())
    cyc = [raw[0], raw[1]]
    assert twin.stage("prenorm").scratch is None and twin.stage("prenorm").rot is None and twin.stage("prenorm").reset_jobs() == [] and twin.stage("prenorm").frames(cyc) is cyc
    assert net.state_bytes() - twin.state_bytes() == N * (18 * 8 + 4)
    assert net.scratch_bytes() - twin.scratch_bytes() == 4 * net.max_cycle * N * 3 * 25 * 2
    if modality != "joint":
        assert torch.equal(net.stage("modality").prev, normed[-1])
    with pytest.raises(RuntimeError, match=r"clean_state\(\)"):
        pkg.set_pre_normalization(net, False)


def test_stream_shards_with_the_switch_on():
    def make():
        return _twins(pkg.CoStGcn, 1, **CO)[0]
    shards, twin = pkg.parallel.StreamShards(make, N, 2, DEV), pkg.parallel.StreamShards(make, N, 2, DEV)
    for s in (shards, twin):
        pkg.set_input_modality(s, "bone_motion")
    assert pkg.set_pre_normalization(shards) is shards and all(m.pre_normalization for m in shards.models)
    raw, normed = _sequence(21)
    n_pred = 0
    for t in range(0, T_SEQ, 4):
        got, want = shards.forward_cycle(list(raw[t:t + 4])), twin.forward_cycle(list(normed[t:t + 4]))
        assert (got is None) == (want is None), t
        if want is not None:
            assert torch.equal(got, want), t
            n_pred += 1
    assert n_pred == 4 and [m.stage("prenorm").flags.shape[0] for m in shards.models] == [3, 2]


# ---- state contracts
@pytest.mark.parametrize("native_plan", [True, False])
def test_peeks_do_not_latch_and_snapshots_restore(native_plan):
    peeker, twin = _twins(pkg.CoStGcn, 2, **CO)
    for net in (peeker, twin):
        net.use_native_plan = native_plan
        pkg.set_pre_normalization(net)
    raw, _ = _sequence(21)
    assert peeker.forward_step(raw[5], update_state=False) is None          # a peek on a fresh slab: binds, does not latch
    assert not peeker.stage("prenorm").flags.any() and not peeker.stage("prenorm").rot.any()
    ahead = peeker.forward_steps(raw[8:16].permute(1, 2, 0, 3, 4).contiguous(), update_state=False)
    assert ahead.shape[2] == 0 and not peeker.stage("prenorm").flags.any() and not peeker.stage("prenorm").rot.any()
    n_pred = 0
    for t in range(T_SEQ):
        p1 = None
        if t in (1, 37, 80, 84):
            keep = [s.clone() for s in [t for _, t in peeker.stage("prenorm").state()]]
            p1 = peeker.forward_step(raw[t], update_state=False)
            if t in (37, 80):
                ahead = peeker.forward_steps(raw[t:t + 8].permute(1, 2, 0, 3, 4).contiguous(), update_state=False)
                assert ahead.shape[2] == (2 if t == 80 else 0)
            assert all(torch.equal(a, b) for a, b in zip([t for _, t in peeker.stage("prenorm").state()], keep)) and bool(peeker.stage("prenorm").flags.all()), t
        got, want = peeker.forward_step(raw[t]), twin.forward_step(raw[t])
        assert (got is None) == (want is None), t
        if want is not None:
            assert torch.equal(got, want), t
            n_pred += 1
            if t in (80, 84):
                assert torch.equal(p1, want), t
    assert n_pred == 4 and all(torch.equal(a, b) for a, b in zip(peeker._state_tensors(), twin._state_tensors()))


def test_reset_streams_and_clean_state_make_the_next_frame_a_first_frame():
    """80 frames, reset_streams([1, 3]) (80 = 20 * 4), on to frame 176 in cycles of 4.  Streams 1 and 3 == a fresh
    pre-normalising model fed their frames alone from there on (it latches from frame 80); streams 0, 2 and 4 == the slab that
    was never reset.  Then clean_state() and a second sequence == a fresh model."""
    slab, plain, fresh, fresh2 = _twins(pkg.CoStGcn, 4, **CO)
    for net in (slab, plain, fresh, fresh2):
        pkg.set_pre_normalization(net)
    raw, _ = _sequence(22, t=176)
    assert _same(_predictions(slab, raw, 4, 0, 80), _predictions(plain, raw, 4, 0, 80))
    rot_before = slab.stage("prenorm").rot.clone()
    slab.reset_streams([1, 3])
    assert slab.stage("prenorm").flags.tolist() == [1, 0, 1, 0, 1] and torch.equal(slab.stage("prenorm").rot, rot_before)
    got, want_plain = _predictions(slab, raw, 4, 80), _predictions(plain, raw, 4, 80)
    want_fresh = _predictions(fresh, raw, 4, 80, rows=[1, 3])
    assert len(got) == len(want_plain) == 24 and len(want_fresh) == 4
    for (t, a), (tp, b) in zip(got, want_plain):
        assert t == tp and torch.equal(a[[0, 2, 4]], b[[0, 2, 4]]), t
    tail = got[-len(want_fresh):]
    assert all(t == tf and torch.equal(a[[1, 3]], b) for (t, a), (tf, b) in zip(tail, want_fresh))
    assert any(not torch.equal(a[[1, 3]], b[[1, 3]]) for (_, a), (_, b) in zip(tail, want_plain[-len(tail):]))
    assert torch.equal(slab.stage("prenorm").rot[[1, 3]], fresh.stage("prenorm").rot) and torch.equal(slab.stage("prenorm").rot[[0, 2, 4]], plain.stage("prenorm").rot[[0, 2, 4]])
    slab.clean_state()
    assert not slab.stage("prenorm").flags.any()
    second = raw[60:156]
    assert _same(_predictions(slab, second, 4), _predictions(fresh2, second, 4))


def test_the_switch_is_off_by_default_and_then_nothing_is_allocated_or_launched():
    net, plain = _twins(pkg.CoStGcn, 2, **CO)
    assert pkg.set_pre_normalization(net, False) is net
    raw, _ = _sequence(21)
    cyc = [raw[0], raw[1], raw[2], raw[3]]
    assert _same(_predictions(net, raw, 4, 0, 8), _predictions(plain, raw, 4, 0, 8)) and net.stage("prenorm").frames(cyc) is cyc
    assert net.stage("prenorm").scratch is None and net.stage("prenorm").rot is None and net.stage("prenorm").flags is None and [t for _, t in net.stage("prenorm").state()] == []
    x = raw[:20].permute(1, 2, 0, 3, 4).contiguous()
    assert net.stage("prenorm").clip(x) is x
    net.clean_state()
    pkg.set_pre_normalization(net)                      # a bound slab that has not stepped takes the switch and binds its state
    assert net.stage("prenorm").rot.shape == (N, 18) and net.stage("prenorm").rot.dtype == torch.float64 and net.stage("prenorm").flags.dtype == torch.int32
    assert net.stage("prenorm").scratch.shape == (net.max_cycle, N, 3, 25, 2)
    pkg.set_pre_normalization(net, False)
    assert net.stage("prenorm").rot is None and net.stage("prenorm").scratch is None
