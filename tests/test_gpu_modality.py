"""Bone / motion input modalities on the device: the two entries of csrc/modality.hip against the numpy oracle
(tests/modality_oracle.py) and what the reference's scripts wrote (tests/golden/g13_modalities.npz), and the models that
run them in front of the unchanged path.

Every comparison is ``torch.equal``: the derivation is exactly rounded fp32 subtraction on both sides -- one rounding per
subtraction, in the stated order -- and a model in modality ``m`` then runs the very kernels its twin runs on the
host-derived tensor, so there is no tolerance to choose."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _bootstrap
from tests import modality_oracle as mo
from tests.helpers import GOLDEN, guarded_allocs, randomise_unit_

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native, modality = pkg.native, pkg.modality
DEV = "cuda:0"
DERIVED = ("bone", "joint_motion", "bone_motion")


def _parents(v):
    return modality.bone_parents(v)


def _c_parents(v, table=None):
    return (ctypes.c_int32 * v)(*[int(p) for p in (_parents(v) if table is None else table)])


def _joints(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _clip_entry(x, mode, out=None, parents=None):
    """csk_derive_modality_f32 on a device tensor (N, C, T, V, M) -> (rc, out)."""
    n, c, t, v, m = x.shape
    out = torch.empty(x.shape, device=x.device, dtype=torch.float32) if out is None else out
    rc = native.lib().csk_derive_modality_f32(native.ptr(x), native.ptr(out), mode, _c_parents(v, parents), n, c, t, v, m,
                                              native.stream_of(x))
    torch.cuda.synchronize()
    return rc, out


def _frames_entry(frames, mode, prev, flags, update, dsts=None, parents=None, r=None):
    """csk_derive_modality_frames_f32 on a list of device frames (N, C, V, M) -> (rc, dsts)."""
    n, c, v, m = frames[0].shape
    dsts = [torch.empty(frames[0].shape, device=DEV, dtype=torch.float32) for _ in frames] if dsts is None else dsts
    src = (ctypes.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
    dst = (ctypes.c_void_p * len(frames))(*[d.data_ptr() for d in dsts])
    rc = native.lib().csk_derive_modality_frames_f32(src, dst, len(frames) if r is None else r, mode, _c_parents(v, parents),
                                                     native.ptr(prev), native.ptr(flags), update, n, c, v, m, native.stream_of(frames[0]))
    torch.cuda.synchronize()
    return rc, dsts


# ---- 1. the clip entry -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("v", [25, 18])
@pytest.mark.parametrize("t", [1, 5])
def test_clip_entry_equals_the_oracle(t, v, m):
    """N = 2, C = 3: 150 .. 1500 floats, most of them no multiple of 4 (a scalar tail), frame rows of 25 / 50 / 18 / 36
    floats (4-byte, 8-byte and 16-byte aligned row starts).  Also from a base that is only 4-byte aligned (scalar path)."""
    x = _joints((2, 3, t, v, m), 100 + t + v + m)
    for kind in DERIVED:
        want = torch.from_numpy(mo.derive_clip(x.numpy(), kind, _parents(v)))
        rc, got = _clip_entry(x.to(DEV), modality.MODE[kind])
        assert rc == 0 and torch.equal(got.cpu(), want), kind
        if t == 1 and kind != "bone":
            assert not got.any()
        assert torch.equal(modality.derive_clip(x.to(DEV), kind).cpu(), want), kind
        # the same from / to buffers one float off a 16-byte boundary
        xb, ob = torch.zeros(x.numel() + 1, device=DEV), torch.full((x.numel() + 1,), 7.0, device=DEV)
        xb[1:] = x.flatten().to(DEV)
        rc, _ = _clip_entry(xb[1:].view(x.shape), modality.MODE[kind], out=ob[1:].view(x.shape))
        assert rc == 0 and torch.equal(ob[1:].view(x.shape).cpu(), want) and float(ob[0]) == 7.0, kind
    xd = x.to(DEV)
    assert modality.derive_clip(xd, "joint") is xd          # the input itself: no launch, no allocation


@pytest.mark.parametrize("tag", ["ntu", "kinetics"])
def test_clip_entry_equals_what_the_reference_scripts_wrote(tag):
    g = np.load(os.path.join(GOLDEN, "g13_modalities.npz"))
    x = torch.from_numpy(g[f"{tag}/joint"]).to(DEV)
    for kind in DERIVED:
        rc, got = _clip_entry(x, modality.MODE[kind], parents=g[f"{tag}/parents"])
        assert rc == 0 and np.array_equal(got.cpu().numpy(), g[f"{tag}/{kind}"]), kind


def test_clip_entry_over_many_workgroups():
    """N = 64, T = 20: 384 000 floats, 375 workgroups, rows of 50 floats crossing every 4-float group boundary."""
    x = _joints((64, 3, 20, 25, 2), 5)
    for kind in DERIVED:
        rc, got = _clip_entry(x.to(DEV), modality.MODE[kind])
        assert rc == 0 and torch.equal(got.cpu(), torch.from_numpy(mo.derive_clip(x.numpy(), kind, _parents(25)))), kind


# ---- 2. the step entry -----------------------------------------------------------------------------------------------
def _step_case(n, v, m, seed):
    g = torch.Generator().manual_seed(seed)
    frames = [torch.randn((n, 3, v, m), generator=g) for _ in range(4)]
    prev = torch.randn((n, 3, v, m), generator=g)
    flags = torch.tensor(([1, 0, 1] * n)[:n], dtype=torch.int32)
    return frames, prev, flags


def _step_want(frames, prev, flags, kind, v):
    """Oracle: the sequence [prev, frames...] differenced backwards, frame 0 zeroed for streams without a previous frame."""
    seq = torch.stack([prev] + frames, dim=2).numpy()                      # (N, C, 1 + r, V, M)
    first = np.zeros((seq.shape[0], seq.shape[2]), dtype=bool)
    first[:, 1] = flags.numpy() == 0
    out = mo.derive_steps(seq, kind, _parents(v), first)
    return [torch.from_numpy(np.ascontiguousarray(out[:, :, 1 + i])) for i in range(len(frames))]


@pytest.mark.parametrize("n,v,m", [(3, 25, 2), (3, 18, 2), (3, 25, 1), (9, 25, 2), (19, 18, 1)])
def test_step_entry_equals_the_oracle_and_keeps_its_state_rules(n, v, m):
    """Flags (1, 0, 1, ...): a stream without a previous frame gets 0 for frame 0 and differences from frame 1 on.  r in
    {1, 2, 4}; one 4-frame launch == four 1-frame launches; update = 1 stores the last raw frame and sets every flag,
    update = 0 leaves buffer and flags bitwise untouched.  N = 9 / 19: three / two chunks of streams, the last one partial."""
    frames, prev, flags = _step_case(n, v, m, 40 + n + v + m)
    dev = [f.to(DEV) for f in frames]
    for kind in DERIVED:
        mode, motion = modality.MODE[kind], kind != "bone"
        for r in (1, 2, 4):
            want = _step_want(frames[:r], prev, flags, kind, v)
            for update in (0, 1):
                p, f = prev.to(DEV), flags.to(DEV)
                rc, got = _frames_entry(dev[:r], mode, p, f, update)
                assert rc == 0 and all(torch.equal(a.cpu(), b) for a, b in zip(got, want)), (kind, r, update)
                if update and motion:
                    assert torch.equal(p.cpu(), frames[r - 1]) and torch.equal(f.cpu(), torch.ones(n, dtype=torch.int32))
                else:
                    assert torch.equal(p.cpu(), prev) and torch.equal(f.cpu(), flags), (kind, r, update)
        # four 1-frame launches, each updating, == the one 4-frame launch (outputs and final state)
        p4, f4 = prev.to(DEV), flags.to(DEV)
        rc, got4 = _frames_entry(dev, mode, p4, f4, 1)
        p1, f1 = prev.to(DEV), flags.to(DEV)
        for i in range(4):
            rc1, got1 = _frames_entry(dev[i:i + 1], mode, p1, f1, 1)
            assert rc == 0 and rc1 == 0 and torch.equal(got1[0], got4[i]), (kind, i)
        assert torch.equal(p1, p4) and torch.equal(f1, f4)
    # the bone mode has no state: no buffer, no flags
    rc, got = _frames_entry(dev[:2], modality.MODE["bone"], None, None, 1)
    assert rc == 0 and torch.equal(got[1].cpu(), torch.from_numpy(mo.bone(frames[1].numpy(), _parents(v))))


# ---- 3. operand bounds -------------------------------------------------------------------------------------------------
def test_both_entries_read_inside_their_operands():
    """Every operand between NaN guards (helpers.guarded_allocs): the parent gather (bone) and the next-frame / previous-
    frame reads (motion) are where a read could leave its operand, and a NaN read would show in the difference.  The last
    frame of a clip has no successor and a flag-less stream no predecessor: neither may be read into the result."""
    x = _joints((2, 3, 5, 25, 2), 8)
    frames, prev, flags = _step_case(3, 25, 2, 9)
    plain_clip = {k: _clip_entry(x.to(DEV), modality.MODE[k])[1].cpu() for k in DERIVED}
    plain_step = {k: [d.cpu() for d in _frames_entry([f.to(DEV) for f in frames], modality.MODE[k], prev.to(DEV), flags.to(DEV), 1)[1]]
                  for k in DERIVED}
    with guarded_allocs() as g:
        def guarded(t):
            buf = torch.empty(t.shape, device=DEV, dtype=torch.float32)
            buf.copy_(t)
            return buf
        for kind in DERIVED:
            out = torch.empty(x.shape, device=DEV, dtype=torch.float32)
            rc, got = _clip_entry(guarded(x), modality.MODE[kind], out=out)
            assert rc == 0 and torch.isfinite(got).all() and torch.equal(got.cpu(), plain_clip[kind]), kind
            dsts = [torch.empty(frames[0].shape, device=DEV, dtype=torch.float32) for _ in frames]
            rc, got = _frames_entry([guarded(f) for f in frames], modality.MODE[kind], guarded(prev), flags.to(DEV), 1, dsts=dsts)
            assert rc == 0 and all(torch.isfinite(d).all() and torch.equal(d.cpu(), w) for d, w in zip(got, plain_step[kind])), kind
        assert g.count >= 3 * (2 + 4 + 4 + 1)


# ---- 4. error returns ----------------------------------------------------------------------------------------------------
def test_refused_calls_launch_nothing():
    x = _joints((2, 3, 5, 25, 2), 10).to(DEV)
    out = torch.full(x.shape, 3.0, device=DEV)
    bad_parents = _parents(25).copy()
    bad_parents[7] = 25
    for mode, parents in ((0, None), (4, None), (modality.MODE["bone"], bad_parents), (modality.MODE["bone_motion"], -bad_parents - 1)):
        rc, _ = _clip_entry(x, mode, out=out, parents=parents)
        assert rc == -2 and native.lib().csk_last_error() and bool((out == 3.0).all()), mode
    frames = [x[:, :, i].contiguous() for i in range(4)]
    dsts = [torch.full(frames[0].shape, 3.0, device=DEV) for _ in frames]
    prev, flags = torch.full(frames[0].shape, 5.0, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    for mode, parents, r in ((9, None, None), (modality.MODE["bone"], bad_parents, None), (modality.MODE["joint_motion"], None, 0),
                             (modality.MODE["joint_motion"], None, 9)):
        rc, _ = _frames_entry(frames, mode, prev, flags, 1, dsts=dsts, parents=parents, r=r)
        assert rc == -2 and all(bool((d == 3.0).all()) for d in dsts) and bool((prev == 5.0).all()) and not flags.any(), (mode, r)
    with pytest.raises(RuntimeError, match="outside"):
        modality.derive_clip(x, "bone", parents=bad_parents)


# ---- models -----------------------------------------------------------------------------------------------------------------
def _graph(v):
    return (pkg.ntu_graph() if v == 25 else pkg.kinetics_graph()).A


def _twins(cls, v, n_copies, shape_t=300, seed=7, **kw):
    """``n_copies`` models of one state_dict (randomised: BN statistics, graph attention, every conv) on the device."""
    nets = [cls(_graph(v), (3, shape_t, v, 2), 60, **kw).eval() for _ in range(n_copies)]
    randomise_unit_(nets[0], seed, attn_scale=1 / v if "AGcn" in cls.__name__ else 1.0)
    for net in nets[1:]:
        net.load_state_dict(nets[0].state_dict())
    return [net.to(DEV) for net in nets]


# ---- 5. clip models
@pytest.mark.parametrize("kind", DERIVED)
@pytest.mark.parametrize("model,v", [("StGcn", 25), ("AGcn", 18), ("STr", 25)])
def test_clip_model_in_a_modality_equals_its_twin_on_the_derived_clip(model, v, kind):
    net, twin = _twins(getattr(pkg, model), v, 2, shape_t=20)
    assert pkg.set_input_modality(net, kind) is net and twin.input_modality == "joint"
    x = _joints((2, 3, 20, v, 2), 11)
    want_in = torch.from_numpy(mo.derive_clip(x.numpy(), kind, _parents(v))).to(DEV)
    with torch.no_grad():
        got, want, on_joints = net(x.to(DEV)), twin(want_in), twin(x.to(DEV))
    assert torch.equal(got, want) and not torch.equal(got, on_joints)


@pytest.mark.parametrize("kind", DERIVED)
def test_continual_model_clip_forward_keeps_the_forward_difference(kind):
    net, twin = _twins(pkg.CoStGcn, 25, 2, pool_size=3, pool_padding=1)
    pkg.set_input_modality(net, kind)
    x = _joints((2, 3, 40, 25, 2), 12)
    want_in = torch.from_numpy(mo.derive_clip(x.numpy(), kind, _parents(25))).to(DEV)
    with torch.no_grad():
        assert torch.equal(net(x.to(DEV), "clip"), twin(want_in, "clip"))


# ---- 6. continual models
CO = dict(pool_size=3, pool_padding=1)      # tests/test_gpu_stream_reset.py: first logits with frame 81, then every 4 frames
T_SEQ = 96
N = 3


def _predictions(net, frames, r, lo=0, hi=None, rows=None):
    """Step ``net`` over frames[lo:hi] ((T, N, C, V, M) on the device) in cycles of r -> list of (frame count, logits)."""
    out = []
    hi = len(frames) if hi is None else hi
    for t in range(lo, hi, r):
        cyc = [frames[t + f] if rows is None else frames[t + f][rows].contiguous() for f in range(r)]
        logits = net.forward_cycle(cyc) if r > 1 else [o for o in [net.forward_step(cyc[0])] if o is not None]
        out += [(t + r, o.clone()) for o in logits]
    return out


def _same(a, b):
    return len(a) == len(b) and all(ta == tb and torch.equal(x, y) for (ta, x), (tb, y) in zip(a, b))


def _sequences(v, seed, t=T_SEQ, n=N):
    """Joint frames (T, N, C, V, M) on the host and the three derived step sequences, computed once per skeleton."""
    key = (v, seed, t, n)
    if key not in _sequences.cache:
        x = _joints((t, n, 3, v, 2), seed)
        ncTvm = x.permute(1, 2, 0, 3, 4).numpy()
        der = {k: torch.from_numpy(np.ascontiguousarray(mo.derive_steps(ncTvm, k, _parents(v)).transpose(2, 0, 1, 3, 4))) for k in DERIVED}
        _sequences.cache[key] = (x, der)
    return _sequences.cache[key]


_sequences.cache = {}


@pytest.mark.parametrize("kind", DERIVED)
@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("native_plan", [True, False])
def test_stepping_on_joints_equals_the_twin_stepped_on_host_derived_frames(native_plan, r, kind):
    net, twin = _twins(pkg.CoStGcn, 25, 2, **CO)
    net.use_native_plan = twin.use_native_plan = native_plan
    pkg.set_input_modality(net, kind)
    x, der = _sequences(25, 21)
    got, want = _predictions(net, x.to(DEV), r), _predictions(twin, der[kind].to(DEV), r)
    assert len(want) == 4 and _same(got, want)
    assert (net.__dict__.get("_plan") is not None) == native_plan
    assert (net.stage("modality").prev is not None) == (kind != "bone") and net.stage("modality").scratch is not None and twin.stage("modality").scratch is None
    if kind != "bone":
        assert torch.equal(net.stage("modality").prev, x[-1].to(DEV)) and bool(net.stage("modality").flags.all())


@pytest.mark.parametrize("model,v,native_plan,r", [("CoAGcn", 25, True, 1), ("CoSTr", 25, False, 4)])
def test_sibling_models_step_in_bone_motion(model, v, native_plan, r):
    net, twin = _twins(getattr(pkg, model), v, 2, **CO)
    net.use_native_plan = twin.use_native_plan = native_plan
    pkg.set_input_modality(net, "bone_motion")
    x, der = _sequences(v, 21)
    got, want = _predictions(net, x.to(DEV), r), _predictions(twin, der["bone_motion"].to(DEV), r)
    assert len(want) == 4 and _same(got, want)


# ---- 7. peeks
@pytest.mark.parametrize("kind", ["joint_motion", "bone_motion"])
@pytest.mark.parametrize("native_plan", [True, False])
def test_peeks_leave_every_later_prediction_unchanged(native_plan, kind):
    """forward_step(update_state=False) runs the pre-pass with update = 0; forward_steps(update_state=False) restores the
    previous-frame buffer and the flags with the rest of the slab.  The peeked model goes on like its twin, and a peek's
    own answer is the answer of the real step that follows."""
    peeker, twin = _twins(pkg.CoStGcn, 25, 2, **CO)
    for net in (peeker, twin):
        net.use_native_plan = native_plan
        pkg.set_input_modality(net, kind)
    x, _ = _sequences(25, 21)
    frames = x.to(DEV)
    n_pred = 0
    for t in range(T_SEQ):
        p1 = None
        if t in (0, 1, 37, 80, 84, 85):
            keep = [s.clone() for s in [t for _, t in peeker.stage("modality").state()]] if t else None
            p1 = peeker.forward_step(frames[t], update_state=False)
            if t in (37, 80):
                ahead = peeker.forward_steps(frames[t:t + 8].permute(1, 2, 0, 3, 4).contiguous(), update_state=False)
                assert ahead.shape[2] == (2 if t == 80 else 0)
            if keep:
                assert all(torch.equal(a, b) for a, b in zip([t for _, t in peeker.stage("modality").state()], keep)), t
        got, want = peeker.forward_step(frames[t]), twin.forward_step(frames[t])
        assert (got is None) == (want is None), t
        if want is not None:
            assert torch.equal(got, want), t
            n_pred += 1
            if t in (80, 84):
                assert torch.equal(p1, want), t
    assert n_pred == 4 and all(torch.equal(a, b) for a, b in zip(peeker._state_tensors(), twin._state_tensors()))
    assert sum(s is peeker.stage("modality").prev or s is peeker.stage("modality").flags for s in peeker._state_tensors()) == 2


# ---- 8. resets
@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("native_plan", [True, False])
def test_reset_stream_is_a_fresh_model_and_its_neighbours_run_on(native_plan, r):
    """joint_motion, 80 frames, reset_streams([1]) (80 = 20 * 4), on to frame 176.  Stream 1 == a fresh same-modality model fed
    its frames since the reset alone -- so its first frame after the reset gave motion 0, not a difference against the old
    stream's last frame; streams 0 and 2 == the slab that was never reset.  Then clean_state() and a second sequence == a
    fresh model."""
    slab, plain, fresh, fresh2 = _twins(pkg.CoStGcn, 25, 4, **CO)
    for net in (slab, plain, fresh, fresh2):
        net.use_native_plan = native_plan
        pkg.set_input_modality(net, "joint_motion")
    x, _ = _sequences(25, 22, t=176)
    frames = x.to(DEV)
    head, head_plain = _predictions(slab, frames, 4, 0, 80), _predictions(plain, frames, 4, 0, 80)
    assert _same(head, head_plain) and not head
    slab.reset_streams([1])
    assert slab.stage("modality").flags.tolist() == [1, 0, 1]
    got, want_plain = _predictions(slab, frames, r, 80), _predictions(plain, frames, r, 80)
    want_fresh = _predictions(fresh, frames, r, 80, rows=[1])
    assert len(got) == len(want_plain) == 24 and len(want_fresh) == 4
    for (t, a), (tp, b) in zip(got, want_plain):
        assert t == tp and torch.equal(a[[0, 2]], b[[0, 2]]), t
    tail = got[-len(want_fresh):]
    assert all(t == tf and torch.equal(a[1], b[0]) for (t, a), (tf, b) in zip(tail, want_fresh))
    assert any(not torch.equal(a[1], b[1]) for (_, a), (_, b) in zip(tail, want_plain[-len(tail):]))
    slab.clean_state()
    assert not slab.stage("modality").flags.any() and not slab.stage("modality").prev.any()
    second = frames[60:156]
    assert _same(_predictions(slab, second, r), _predictions(fresh2, second, r))


# ---- 9. the default modality
def test_joint_modality_is_the_untouched_model_and_allocates_nothing():
    net, plain = _twins(pkg.CoStGcn, 25, 2, **CO)
    assert pkg.set_input_modality(net, "joint") is net
    x, _ = _sequences(25, 21)
    frames = x.to(DEV)
    got, want = _predictions(net, frames, 4), _predictions(plain, frames, 4)
    assert len(want) == 4 and _same(got, want)
    for m in (net, plain):
        assert m.stage("modality").scratch is None and m.stage("modality").prev is None and m.stage("modality").flags is None and [t for _, t in m.stage("modality").state()] == []
        assert m.stage("modality").reset_jobs() == []
    cyc = [frames[0], frames[1]]
    assert net.stage("modality").frames(cyc) is cyc                   # the cycle's own list: no launch
    clip, clip_plain = _twins(pkg.StGcn, 25, 2, shape_t=20)
    pkg.set_input_modality(clip, "joint")
    xc = _joints((2, 3, 20, 25, 2), 11).to(DEV)
    with torch.no_grad():
        assert torch.equal(clip(xc), clip_plain(xc)) and clip.stage("modality").clip(xc) is xc
    # a bound model that has stepped refuses the change and names the way out; after clean_state() it takes it
    with pytest.raises(RuntimeError, match=r"clean_state\(\)"):
        pkg.set_input_modality(net, "bone")
    net.clean_state()
    pkg.set_input_modality(net, "bone_motion")
    assert net.stage("modality").prev is not None and net.stage("modality").prev.shape == (N, 3, 25, 2) and net.stage("modality").flags.dtype == torch.int32
    pkg.set_input_modality(net, "bone")
    assert net.stage("modality").prev is None and net.stage("modality").flags is None and net.stage("modality").scratch is not None


# ---- 10. the ensemble
@pytest.mark.parametrize("method", ["add", "maximum"])
def test_online_ensemble_equals_the_fusion_of_its_members_stepped_alone(method):
    joint, bone, joint2, bone2 = _twins(pkg.CoStGcn, 25, 4, **CO)
    for net in (bone, bone2):
        pkg.set_input_modality(net, "bone")
    ens = pkg.fusion.OnlineEnsemble([joint, bone], method=method)
    x, _ = _sequences(25, 21)
    frames = x.to(DEV)
    alone = [_predictions(net, frames, 4) for net in (joint2, bone2)]
    want = [(t, pkg.fusion.aggregate_preds([a, b], method)) for (t, a), (_, b) in zip(*alone)]
    got = []
    for t in range(0, 88, 4):
        fused = ens.forward_cycle([frames[t + f] for f in range(4)])
        got += [(t + 4, o) for o in fused or []]
    for t in range(88, T_SEQ):
        o = ens.forward_step(frames[t])
        got += [(t + 1, o)] if o is not None else []
    assert len(want) == 4 and [t for t, _ in got] == [84, 88, 89, 93] and not ens.streams_ready().logical_not().any()
    assert torch.equal(got[0][1], want[0][1]) and torch.equal(got[1][1], want[1][1])
    assert not torch.equal(alone[0][0][1], alone[1][0][1])
    ens.clean_state()
    again = []
    for t in range(0, T_SEQ, 4):
        again += ens.forward_cycle([frames[t + f] for f in range(4)]) or []
    assert len(again) == 4 and all(torch.equal(a, w) for a, (_, w) in zip(again, want))
    ens.reset_streams([2])
    assert ens.streams_ready().tolist() == [True, True, False]
    other = _twins(pkg.CoStGcn, 25, 1, pool_size=4, pool_padding=1)[0]
    with pytest.raises(ValueError, match="pool_size"):
        pkg.fusion.OnlineEnsemble([joint, other], method=method)
