"""Priming continual streams from buffered history (prime_state / prime_streams, csk_co_prime_pack_f32).

The yardstick is the stream that was STEPPED through the same history: its exported record (3d), job by job, and what it goes on
to predict.  Small states and structural zeros are compared bit for bit; activations within the project's clip-versus-steps
bound (rtol 1e-4, atol 1e-5: tests/test_gpu_continual_parity.py), here per job as max|primed - stepped| <= 1e-4 max|stepped|.
The ratios the record test observes are printed (run with -s); profiles/r20_stream_prime.md holds what was measured."""
import contextlib
import ctypes
import functools

import pytest
import torch

import _bootstrap
from tests.helpers import randomise_unit_

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native = pkg.native
DEV = "cuda:0"
SENTINEL = 0x7FC0BEEF                   # a NaN payload no source holds (the sources' NaNs are filtered against it)


# ---- the kernel alone --------------------------------------------------------------------------------------------------
def _pack(jobs, packed, record, n, m, v):
    arr = (native.PrimeJob * len(jobs))(*jobs)
    native.check(native.lib().csk_co_prime_pack_f32(ctypes.byref(arr), len(jobs), native.ptr(packed), record, n, m, v,
                                                    native.stream_of(packed)), "csk_co_prime_pack_f32")
    torch.cuda.synchronize()


def _bits(shape, g):
    """Random 32-bit patterns (NaN payloads, infinities, denormals, both zeros included), none of them the sentinel."""
    x = torch.randint(-2 ** 31, 2 ** 31, shape, generator=g, dtype=torch.int64).to(torch.int32)
    x[x == torch.tensor(SENTINEL, dtype=torch.int32)] = 1
    x.view(-1)[:: 97] = -4194304 + 5                                               # 0xFFC00005: a negative quiet NaN with a payload
    return x


def _ring_expectation(src, n, m, first, window):
    """(n, window * C * M * V) int32 by indexing: frames first .. first + window - 1 of (n * M, C, T, V), oldest first, rows,
    then the stream's segment m * V + v; frames in front of the clip are +0 bits."""
    nm, c, t, v = src.shape
    s = src.view(n, m, c, t, v)
    out = torch.zeros((n, window, c, m, v), dtype=torch.int32)
    for i in range(window):
        if first + i >= 0:
            out[:, i] = s[:, :, :, first + i].permute(0, 2, 1, 3)
    return out.reshape(n, -1)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("window,place", [(4, "front"), (4, "zero"), (4, "end"), (8, "front"), (8, "zero"), (8, "end")])
@pytest.mark.parametrize("v", [25, 18])
def test_pack_kernel_gathers_the_named_frames_bit_for_bit(v, window, place, lead):
    """Two ring jobs (C = 3 on T_src = 12, C = 64 on T_src = 5: more than one workgroup), a words job and an empty job in one
    launch for 3 streams of M = 2 skeletons.  ``lead`` words in front, an odd record with a gap no job covers and jobs at odd
    offsets put every run on each 4-byte phase, so both store widths and every head / tail length run.  The packed buffer
    equals the indexing gather bit for bit; the sentinel words in front of it, behind it and in every record's gap are intact."""
    n, m = 3, 2
    g = torch.Generator().manual_seed(1000 * v + 10 * window + lead)
    srcs = [_bits((n * m, 3, 12, v), g), _bits((n * m, 64, 5, v), g)]
    words = _bits((n, 37), g)

    def first_of(t_src):
        return min({"front": -3, "zero": 0, "end": t_src - window}[place], t_src - window)

    firsts = [first_of(12), first_of(5)]                                           # T_src = 5 holds a window of 8 at first = -3 only
    sizes = [window * s.shape[1] * m * v for s in srcs]
    gap = 3
    offs = [0, sizes[0] + gap, sizes[0] + gap + sizes[1]]
    record = offs[2] + 37 + 2
    dev = [s.to(DEV) for s in srcs] + [words.to(DEV)]
    jobs = [native.PrimeJob(dev[i].data_ptr(), offs[i], native.PRIME_RING, srcs[i].shape[1], srcs[i].shape[2], firsts[i], window, 0)
            for i in range(2)]
    jobs += [native.PrimeJob(dev[2].data_ptr(), offs[2], native.PRIME_WORDS, 37, 1, 0, 1, 0),
             native.PrimeJob(dev[0].data_ptr(), 1, native.PRIME_RING, 3, 12, 12, 0, 0)]    # an empty window: nothing is written
    buf = torch.full((lead + (n + 2) * record,), SENTINEL, dtype=torch.int32, device=DEV)
    packed = buf[lead + record: lead + (n + 1) * record].view(n, record)
    want = torch.full(buf.shape, SENTINEL, dtype=torch.int32)
    wp = want[lead + record: lead + (n + 1) * record].view(n, record)
    for i in range(2):
        wp[:, offs[i]: offs[i] + sizes[i]] = _ring_expectation(srcs[i], n, m, firsts[i], window)
    wp[:, offs[2]: offs[2] + 37] = words
    _pack(jobs, packed.view(torch.float32), record, n, m, v)
    assert torch.equal(buf.cpu(), want)
    if place == "front":                                                           # the three frames in front of the clip: +0 bits
        assert not bool(packed[:, : 3 * 3 * m * v].any())


@pytest.mark.parametrize("v,c", [(25, 256), (18, 64), (25, 3)])
def test_pool_job_is_the_head_steps_pool(v, c):
    """Pool job over frames -1 .. 2 of a (n * M, C, 5, V) source: entry 0 is +0 bits; the others are within the rounding bound
    of an M * V-term fp32 sum against the fp64 mean -- (M V + 1) 2^-24 mean|x|: M V - 1 additions and one division, each
    within half an ulp of a partial sum no larger than sum|x| -- and bit for bit the ring entry csk_co_head_step_f32 writes
    for the same feature frame (the same summation order, stated in csrc/stream_prime.hip)."""
    n, m, t_src, window, first = 3, 2, 5, 4, -1
    g = torch.Generator().manual_seed(v * c)
    src = (torch.randn((n * m, c, t_src, v), generator=g) * 3.0 + 0.5)
    dev = src.to(DEV)
    record = window * c + 7
    buf = torch.full((1 + (n + 2) * record,), SENTINEL, dtype=torch.int32, device=DEV)
    packed = buf[1 + record: 1 + (n + 1) * record].view(n, record)
    _pack([native.PrimeJob(dev.data_ptr(), 5, native.PRIME_POOL, c, t_src, first, window, 0)], packed.view(torch.float32), record, n, m, v)
    got = packed.cpu()[:, 5: 5 + window * c].view(torch.float32).view(n, window, c)
    host = buf.cpu()
    assert int((host == SENTINEL).sum()) == host.numel() - n * window * c          # nothing but the entries was written
    assert torch.equal(got[:, 0].view(torch.int32), torch.zeros((n, c), dtype=torch.int32))
    s = src.view(n, m, c, t_src, v).double()
    mv, p = m * v, (n * m * v + 3) // 4 * 4
    for i in range(1, window):
        frame = s[:, :, :, first + i]                                              # (n, m, c, v)
        want = frame.mean(dim=(1, 3))
        bound = (mv + 1) * 2.0 ** -24 * frame.abs().mean(dim=(1, 3))
        assert bool(((got[:, i].double() - want).abs() <= bound).all()), (i, float(((got[:, i].double() - want).abs() / bound).max()))
        slot = torch.zeros((c, p), device=DEV)
        slot[:, : n * mv] = frame.float().permute(2, 0, 1, 3).reshape(c, n * mv).to(DEV)    # channel-major ring slot of the frame
        ring = torch.zeros((1, n, c), device=DEV)
        native.check(native.lib().csk_co_head_step_f32(native.ptr(slot), native.ptr(ring), None, None, None, None, n, c, mv, p,
                                                       1, 0, 0, 0, 0, native.stream_of(slot)), "csk_co_head_step_f32")
        assert torch.equal(ring[0].cpu().view(torch.int32), got[:, i].contiguous().view(torch.int32)), i


# ---- models --------------------------------------------------------------------------------------------------------------
def _small_states(net):
    pkg.set_input_modality(net, "bone_motion")
    pkg.set_pre_normalization(net)


def _bone(net):
    pkg.set_input_modality(net, "bone")


SETUPS = {"plain": None, "small": _small_states, "bone": _bone}


def _make(model, graph, sizes, setup="plain", native_plan=True, seed=7):
    """One model per entry of ``sizes`` with the same seeded weights and non-trivial BN statistics, on the device."""
    a = (pkg.ntu_graph() if graph == "ntu" else pkg.kinetics_graph()).A
    v = a.shape[-1]
    cls = {"stgcn": pkg.CoStGcn, "str": pkg.CoSTr}[model]
    nets = [cls(a, (3, 300, v, 2), 60, pool_size=4, pool_padding=0).eval() for _ in sizes]
    randomise_unit_(nets[0], seed)
    for net in nets[1:]:
        net.load_state_dict(nets[0].state_dict())
    for net in nets:
        net.use_native_plan = native_plan
        if SETUPS[setup]:
            SETUPS[setup](net)
    return [net.to(DEV) for net in nets], v


def _frames(t, n, v, seed):
    return torch.rand((t, n, 3, v, 2), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _steps(net, frames, t0, t1, r=4):
    out = []
    for t in range(t0, t1, r):
        out += net._cycle([frames[t + f] for f in range(r)])[2]
    return out


def _history(frames, t):
    """(T, n, C, V, M) frames -> the (n, C, T, V, M) history tensor of the first ``t``."""
    return frames[:t].permute(1, 2, 0, 3, 4).contiguous()


T_MORE = 16


@functools.lru_cache(maxsize=None)
def _stepped(model, graph, setup, t, native_plan=True):
    """Slab A: 3 streams stepped through ``t`` frames of a seeded history, left at frame ``t``; the reference of every test
    below, computed once per configuration and put back by whoever steps it on (``_restored``)."""
    (A,), v = _make(model, graph, (3,), setup, native_plan)
    frames = _frames(t + T_MORE, 3, v, 100 + t)
    _steps(A, frames, 0, t)
    return A, frames, v


@contextlib.contextmanager
def _restored(net):
    tensors = net._state_tensors()
    keep, position = [x.clone() for x in tensors], net._position()
    try:
        yield
    finally:
        for x, k in zip(tensors, keep):
            x.copy_(k)
        net._set_position(position)


def _export_any_age(net, idx):
    """The record of streams that are live in every block but possibly not ready yet (``export_streams`` insists on ready)."""
    return net._export(idx)


SMALL = ("mod_prev", "mod_flags", "pn_rot", "pn_flags")


def _compare_records(net, primed, stepped, t, label):
    """Job by job: small states and the frames in front of the clip bit for bit, exact zeros of the stepped record bit for bit,
    activations within 1e-4 of the job's largest stepped magnitude.  Prints the observed ratio of every job."""
    table = {name: (count, first, window) for name, _, count, first, window in net.prime_table(t)}
    offset, worst = 0, 0.0
    p, s = primed.cpu(), stepped.cpu()
    for name, rows, seg, window in net._move_windows():
        size = rows * seg * window
        a, b = p[:, offset: offset + size], s[:, offset: offset + size]
        if name in SMALL:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (label, name)
            assert bool((b.view(torch.int32) != 0).any()), (label, name, "the stepped state is empty: nothing was compared")
        else:
            count, first, _ = table[name]
            lead = max(0, -first) * (size // window)                                # words of the frames in front of the clip
            assert int(a[:, :lead].view(torch.int32).abs().max() if lead else 0) == 0, (label, name, "leading frames are not +0")
            assert torch.equal(a[:, :lead].view(torch.int32), b[:, :lead].view(torch.int32)), (label, name)
            zero = b == 0
            flips = int((a.view(torch.int32)[zero] != b.view(torch.int32)[zero]).sum())
            scale = float(b.abs().max())
            ratio = float((a - b).abs().max()) / scale if scale else 0.0
            worst = max(worst, ratio)
            print(f"prime-vs-steps {label} T={t} {name}: max|primed-stepped|/max|stepped| = {ratio:.3e} "
                  f"(bound 1e-4), exact zeros {int(zero.sum())}, of them differing {flips}, count {count}, first {first}")
            assert count == 0 or scale > 0, (label, name, "the stepped window is empty: nothing was compared")
            assert flips == 0, (label, name, flips)
            assert ratio <= 1e-4, (label, name, ratio)
        offset += size
    assert offset == net.record_floats()
    return worst


RECORD_CASES = [("stgcn", "ntu", "small", 96), ("stgcn", "ntu", "small", 76), ("stgcn", "kinetics", "plain", 80),
                ("str", "ntu", "plain", 96)]


@pytest.mark.parametrize("model,graph,setup,t", RECORD_CASES, ids=[f"{m}-{g}-{s}-T{t}" for m, g, s, t in RECORD_CASES])
def test_primed_record_equals_the_stepped_streams_record(model, graph, setup, t):
    """Slab A steps the history and exports; ``prime_state`` of the same history must give the same record, job by job.  With
    bone_motion and pre-normalisation on, the previous raw frame, both flags and the latched rotations match bit for bit.  At
    T = 76 the pooling window is empty and layer 10's post-GCN window starts with four zero frames.  The model's continual
    state and position are untouched by ``prime_state``; a fresh, unbound model of the same weights gives the same bits."""
    A, frames, v = _stepped(model, graph, setup, t, native_plan=model == "stgcn")
    x = _history(frames, t)
    before, position = [s.clone() for s in A._state_tensors()], A._position()
    state = A.prime_state(x)
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(A._state_tensors(), before))
    assert A._position() == position
    assert state.ages.tolist() == [t] * 3 and state.signature == A.move_signature() and state.packed.shape == (3, A.record_floats())
    stepped = _export_any_age(A, [0, 1, 2])
    _compare_records(A, state.packed, stepped.packed, t, f"{model}-{graph}-{setup}")
    (fresh,), _ = _make(model, graph, (1,), setup)
    assert fresh._n is None
    alone = fresh.prime_state(x[1:2])                                              # no slab; another batch: the same bits per stream
    assert fresh._n is None and torch.equal(alone.packed.view(torch.int32), state.packed[1:2].view(torch.int32))
    fresh.prime_budget_bytes = 1                                                   # one stream per chunk
    chunked = fresh.prime_state(x)
    assert torch.equal(chunked.packed.view(torch.int32), state.packed.view(torch.int32))


CONT_CASES = [("stgcn", "small", 96, True), ("stgcn", "small", 76, True), ("stgcn", "plain", 96, False), ("str", "plain", 96, False)]


@pytest.mark.parametrize("model,setup,t,native_plan", CONT_CASES,
                         ids=[f"{m}-{s}-T{t}-{'plan' if p else 'python'}" for m, s, t, p in CONT_CASES])
def test_a_primed_stream_continues_as_the_stepped_stream(model, setup, t, native_plan):
    """Slab B (and its twin B') is warmed on other frames to frame 100 -- other slot positions in every ring than a slab at
    frame T -- and ``prime_streams(x[1:2], [1])`` makes its stream 1 the stream that A stepped through x.  Both then step the
    same further frames in cycles of 4: B's logits of stream 1 are allclose (rtol 1e-4, atol 1e-5) to A's, B's streams 0 and 2
    are bit for bit B''s.  The primed stream reports age T; at T = 96 it is ready at once, at T = 76 it is live in every block
    but not ready, and turns ready with the cycle in which the stepped fresh stream first predicts (age 89)."""
    A, frames, v = _stepped(model, "ntu", setup, t, native_plan=model == "stgcn")
    (B, Bt), _ = _make(model, "ntu", (3, 3), setup, native_plan)
    warm = _frames(100 + T_MORE, 3, v, 55)
    for net in (B, Bt):
        _steps(net, warm, 0, 100)
    x = _history(frames, t)
    B.prime_streams(x[1:2], [1])
    assert B.stream_ages().tolist() == [100, t, 100] and B._counters() == Bt._counters()
    ready = A._ready_age()
    assert ready == 89 and B.streams_ready().tolist() == [True, t >= ready, True]
    more = 8 if t >= ready else T_MORE
    compared = 0
    with _restored(A):
        for s in range(0, more, 4):
            cyc_a = [frames[t + s + f] for f in range(4)]
            cyc_bt = [warm[100 + s + f] for f in range(4)]
            cyc_b = []
            for xa, xb in zip(cyc_a, cyc_bt):
                y = xb.clone()
                y[1] = xa[1]
                cyc_b.append(y)
            la, lb, lbt = A._cycle(cyc_a)[2], B._cycle(cyc_b)[2], Bt._cycle(cyc_bt)[2]
            assert len(lb) == len(lbt) == 1                                        # the slab predicts on every stride cycle
            assert torch.equal(lb[0][[0, 2]], lbt[0][[0, 2]]), (s, "the neighbours of the primed stream")
            age = t + s + 4
            assert len(la) == (1 if age >= ready else 0), (s, "the stepped stream")
            assert B.streams_ready().tolist() == [True, age >= ready, True] and B.stream_ages().tolist() == [100 + s + 4, age, 100 + s + 4]
            for a, b in zip(la, lb):
                compared += 1
                assert torch.allclose(b[1], a[1], rtol=1e-4, atol=1e-5), (s, float((b[1] - a[1]).abs().max()))
                assert not torch.equal(b[1], lbt[0][1])                            # ... and it is the primed stream that answers
    assert compared == (2 if t >= ready else 1)


def test_the_record_does_not_depend_on_the_engine():
    """``use_native_plan`` on and off: the primed record is computed by the clip kernels, so it is the same bits, and the two
    slabs -- warmed alike, primed alike -- continue bit for bit alike."""
    A, frames, v = _stepped("stgcn", "ntu", "plain", 96, native_plan=True)
    (P, Q), _ = _make("stgcn", "ntu", (3, 3), "plain", True)
    Q.use_native_plan = False
    warm = _frames(100 + 8, 3, v, 56)
    x = _history(frames, 96)
    for net in (P, Q):
        _steps(net, warm, 0, 100)
    assert P.__dict__.get("_plan") is not None
    assert torch.equal(P.prime_state(x[:1]).packed.view(torch.int32), Q.prime_state(x[:1]).packed.view(torch.int32))
    for net in (P, Q):
        net.prime_streams(x[:2], [2, 0])
    got = [_steps(net, warm, 100, 108) for net in (P, Q)]
    assert len(got[0]) == len(got[1]) == 2 and all(torch.equal(a, b) for a, b in zip(*got))


def test_stream_shards_prime_streams_equals_the_unsharded_slab():
    """2 shards x 2 streams against one slab of 4: global streams 2 (shard 1) and 1 (shard 0) are primed from the same
    histories; every prediction of the next 8 frames is bit for bit the unsharded slab's."""
    A, frames, v = _stepped("stgcn", "ntu", "plain", 96, native_plan=True)
    nets, _ = _make("stgcn", "ntu", (2, 2, 4), "plain", True)
    pool = nets[:2]
    shards = pkg.parallel.StreamShards(lambda: pool.pop(0), 4, 2, torch.device(DEV))
    whole = nets[2]
    warm = _frames(100 + 8, 4, v, 57)
    for t in range(0, 100, 4):
        cyc = [warm[t + f] for f in range(4)]
        shards.forward_cycle(cyc)
        whole.forward_cycle(cyc)
    x = _history(frames, 96)
    with pytest.raises(ValueError, match="not a multiple of the total stride"):
        shards.prime_streams(x[:2, :, :94].contiguous(), [2, 1])
    with pytest.raises(ValueError, match="outside a slab of 4"):
        shards.prime_streams(x[:2], [2, 4])
    shards.prime_streams(x[:2], [2, 1])
    whole.prime_streams(x[:2], [2, 1])
    assert shards.stream_ages().tolist() == whole.stream_ages().tolist() == [100, 96, 96, 100]
    for t in range(100, 108, 4):
        cyc = [warm[t + f] for f in range(4)]
        got, want = shards.forward_cycle(cyc), whole.forward_cycle(cyc)[-1]
        assert torch.equal(got, want), t


def test_online_ensemble_prime_streams_equals_priming_each_member():
    """joint + bone: the ensemble hands every member the same joint history; the fused predictions equal those of a second
    ensemble whose members were primed one by one."""
    A, frames, v = _stepped("stgcn", "ntu", "plain", 96, native_plan=True)
    (j1, j2), _ = _make("stgcn", "ntu", (3, 3), "plain", True, seed=7)
    (b1, b2), _ = _make("stgcn", "ntu", (3, 3), "bone", True, seed=8)
    ens, hand = pkg.fusion.OnlineEnsemble([j1, b1]), pkg.fusion.OnlineEnsemble([j2, b2])
    warm = _frames(100 + 8, 3, v, 58)
    for t in range(0, 100, 4):
        for e in (ens, hand):
            e.forward_cycle([warm[t + f] for f in range(4)])
    x = _history(frames, 96)
    with pytest.raises(ValueError, match="younger than"):
        ens.prime_streams(x[:1, :, :72].contiguous(), [1])
    ens.prime_streams(x[:1], [1])
    for net in hand.nets:
        net.prime_streams(x[:1], [1])
    assert ens.streams_ready().all() and j1.stream_ages().tolist() == b1.stream_ages().tolist() == [100, 96, 100]
    for t in range(100, 108, 4):
        cyc = [warm[t + f] for f in range(4)]
        got, want = ens.forward_cycle(cyc), hand.forward_cycle(cyc)
        assert len(got) == len(want) == 1 and torch.equal(got[0], want[0]), t
