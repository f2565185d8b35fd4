"""Moving live streams between continual slabs (export_streams / import_streams / resize_streams, csk_co_move_streams_f32).

The yardstick is the stream that NEVER MOVED: a twin slab with the same weights that simply keeps stepping.  A moved stream must
give layer-10 features and logits that are ``torch.equal`` to the twin's, on every emission after the move.  Bitwise is the
derived expectation: no kernel's summation order depends on the slab (stream count, ring depth, slot position), the record
holds every float a later launch reads, and the head sums its window oldest first."""
import contextlib
import ctypes
import io

import pytest
import torch

import _bootstrap
from tests.helpers import randomise_unit_

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native, mig = pkg.native, pkg.co_migrate
DEV = "cuda:0"
NAN = float("nan")


# ---- the kernel alone ------------------------------------------------------------------------------------------------
def _move(jobs, packed, record, streams, n_total, to_ring):
    idx = torch.tensor(streams, dtype=torch.int32, device=DEV)
    arr = (native.MoveJob * len(jobs))(*jobs)
    native.check(native.lib().csk_co_move_streams_f32(ctypes.byref(arr), len(jobs), native.ptr(packed), record, native.ptr(idx),
                                                      len(streams), n_total, int(to_ring), native.stream_of(idx)),
                 "csk_co_move_streams_f32")
    torch.cuda.synchronize()


def _pattern(shape, lead, base):
    """Distinct non-zero floats; ``lead`` floats in front put the ring's base on a 4-byte boundary only."""
    numel = shape[0] * shape[1] * shape[2]
    buf = (torch.arange(numel + lead, dtype=torch.float32) + base).to(DEV)
    return buf, buf[lead:].view(shape)


def _same_bits(a, b):
    return torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("mv", [50, 36, 25, 2, 1])
@pytest.mark.parametrize("rows", [3, 65])
def test_move_kernel_gathers_and_scatters_the_named_segments_only(rows, mv, lead):
    """Source ring [12][rows][P] of 5 streams -> records -> target ring [5][rows][P'] of 4 streams, plus a pooling ring each way,
    in one launch per direction; P = N * mv rounded up to 4.  Segment starts are 16-, 8- or 4-byte aligned depending on the
    stream, ``mv`` and ``lead`` (the rings' bases, the packed base and the second job's offset all move with it), so every load
    width and every head / tail length runs.  Records (with a NaN gap behind the jobs, NaN guard records around them and a
    record of an index outside the slab) and target rings equal the CPU-built expectation bit for bit."""
    n_src, n_dst, c = 5, 4, 7
    p_src, p_dst = (n_src * mv + 3) // 4 * 4, (n_dst * mv + 3) // 4 * 4
    window, pool_window = 4, 3
    size = window * rows * mv
    record = size + pool_window * c + 5                                         # 5 floats no job covers
    for streams_src, streams_dst, (new_src, new_dst, pool_src, pool_dst) in (([4, 1, 7], [0, 2, -1], (1, 4, 2, 0)),
                                                                            ([0, 2, 3], [3, 9, 1], (11, 2, 0, 1))):
        sbuf, src = _pattern((12, rows, p_src), lead, 1.0)
        spool_buf, spool = _pattern((pool_window, n_src, c), lead, 0.5)
        dbuf, dst = _pattern((5, rows, p_dst), 3 - lead, 100000.0)
        dpool_buf, dpool = _pattern((pool_window, n_dst, c), 0, 300000.0)
        k = len(streams_src)
        pbuf = torch.full((lead + (k + 2) * record,), NAN, device=DEV)
        packed = pbuf[lead + record: lead + (k + 1) * record].view(k, record)

        def jobs(ring, p, depth, n, newest, pool, pool_newest):
            return [native.MoveJob(ring.data_ptr(), p, 0, depth, rows, newest, window, mv, native.SCRUB_BLOCK_RING),
                    native.MoveJob(pool.data_ptr(), c, size, pool_window, n, pool_newest, pool_window, c, native.SCRUB_POOL_RING)]

        want = torch.full(pbuf.shape, NAN)
        wp = want[lead + record: lead + (k + 1) * record].view(k, record)
        s_cpu, sp_cpu = src.cpu(), spool.cpu()
        for j, n in enumerate(streams_src):
            if not 0 <= n < n_src:
                continue
            for i, slot in enumerate(mig.window_slots(new_src, 12, window)):
                wp[j, i * rows * mv:(i + 1) * rows * mv] = s_cpu[slot, :, n * mv:(n + 1) * mv].reshape(-1)
            for i, slot in enumerate(mig.window_slots(pool_src, pool_window, pool_window)):
                wp[j, size + i * c: size + (i + 1) * c] = sp_cpu[slot, n]
        _move(jobs(src, p_src, 12, n_src, new_src, spool, pool_src), packed, record, streams_src, n_src, to_ring=False)
        assert _same_bits(pbuf, want), (streams_src, "export")
        assert _same_bits(sbuf, _pattern((12, rows, p_src), lead, 1.0)[0]), "the export wrote to its source"

        packed.copy_(torch.arange(k * record, dtype=torch.float32).view(k, record) + 7000000.0)     # records with no NaN, all distinct
        rec = packed.cpu()
        wd, wdp = dbuf.cpu().clone(), dpool_buf.cpu().clone().view(pool_window, n_dst, c)
        wdv = wd[3 - lead:].view(5, rows, p_dst)
        for j, n in enumerate(streams_dst):
            if not 0 <= n < n_dst:
                continue
            for i, slot in enumerate(mig.window_slots(new_dst, 5, window)):
                wdv[slot, :, n * mv:(n + 1) * mv] = rec[j, i * rows * mv:(i + 1) * rows * mv].view(rows, mv)
            for i, slot in enumerate(mig.window_slots(pool_dst, pool_window, pool_window)):
                wdp[slot, n] = rec[j, size + i * c: size + (i + 1) * c]
        _move(jobs(dst, p_dst, 5, n_dst, new_dst, dpool, pool_dst), packed, record, streams_dst, n_dst, to_ring=True)
        assert _same_bits(dbuf, wd) and _same_bits(dpool, wdp), (streams_dst, "import")
        assert _same_bits(packed, rec), "the import wrote to the records"


# ---- models ----------------------------------------------------------------------------------------------------------
def _classes():
    return {"stgcn": pkg.CoStGcn, "agcn": pkg.CoAGcn, "str": pkg.CoSTr, "stgcnmod": pkg.CoStGcnMod}


def _make(model, graph, native_plan, sizes, seed=7, setup=None):
    """One model per entry of ``sizes`` with the same randomised weights on the device; ``setup(net)`` switches modes."""
    a = (pkg.ntu_graph() if graph == "ntu" else pkg.kinetics_graph()).A
    v = a.shape[-1]
    nets = [_classes()[model](a, (3, 300, v, 2), 60, pool_size=2, pool_padding=0).eval() for _ in sizes]
    randomise_unit_(nets[0], seed, attn_scale=1 / v if model == "agcn" else 1.0)
    for net in nets[1:]:
        net.load_state_dict(nets[0].state_dict())
    for net in nets:
        net.use_native_plan = native_plan
        if setup:
            setup(net)
    return [net.to(DEV) for net in nets], v


def _frames(t, n, v, seed):
    return torch.rand((t, n, 3, v, 2), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _steps(net, frames, t0, t1, r):
    for t in range(t0, t1, r):
        net._cycle([frames[t + f] for f in range(r)])


def _feat(net, slot, j, stream, mv):
    out = net.layers["layer10"]._state.out
    return out[(slot + j) % out.shape[0], :, stream * mv:(stream + 1) * mv]


def _same_streams(a, ra, rows_a, b, rb, rows_b, mv, where):
    """Results of one cycle: streams ``rows_a`` of model a against streams ``rows_b`` of model b, features and logits."""
    (slot_a, nf_a, log_a), (slot_b, nf_b, log_b) = ra, rb
    assert nf_a == nf_b and len(log_a) == len(log_b), where
    for sa, sb in zip(rows_a, rows_b):
        for j in range(nf_a):
            assert torch.equal(_feat(a, slot_a, j, sa, mv), _feat(b, slot_b, j, sb, mv)), (where, sa, sb, "features")
        for x, y in zip(log_a, log_b):
            assert torch.equal(x[sa], y[sb]), (where, sa, sb, "logits")
    return len(log_a)


T_A, T_B, T_MORE = 96, 100, 24         # A moves its streams at frame 96 into B, which stands at frame 100; 24 more frames


def _latency(net):
    net.set_latency_mode(8)


CASES = [("stgcn", "ntu", True, 1, None), ("stgcn", "ntu", True, 4, None), ("stgcn", "ntu", False, 1, None),
         ("stgcn", "ntu", False, 4, None), ("agcn", "kinetics", True, 4, None), ("str", "ntu", False, 4, None),
         ("stgcnmod", "ntu", True, 1, None), ("stgcn", "ntu", True, 4, _latency)]


@pytest.mark.parametrize("model,graph,native_plan,r,setup", CASES,
                         ids=[f"{m}-{g}-{'plan' if p else 'python'}-r{r}{'-latency' if s else ''}" for m, g, p, r, s in CASES])
def test_a_moved_stream_equals_the_stream_that_never_moved(model, graph, native_plan, r, setup):
    """Slab A (5 streams, default ring depths) at frame 96, slab B (3 streams, set_max_cycle(4): other depths) at frame 100:
    other slot positions in every ring.  Streams [4, 1] of A become streams [0, 2] of B.  For 24 more frames B's rows 0 and 2
    equal rows 4 and 1 of A's twin C (which never exported), B's row 1 equals B's twin (which never imported), and A itself
    goes on equal to C (the export is read-only).  ``latency``: set_latency_mode(8) everywhere -- the split-K scratch is not state."""
    (A, C, B, Bt), v = _make(model, graph, native_plan, (5, 5, 3, 3), setup=setup)
    mv = 2 * v
    for net in (B, Bt):
        net.set_max_cycle(4)
    fa, fb = _frames(T_A + T_MORE, 5, v, 21), _frames(T_B + T_MORE, 3, v, 22)
    for net in (A, C):
        _steps(net, fa, 0, T_A, r)
    for net in (B, Bt):
        _steps(net, fb, 0, T_B, r)
    assert [t.shape[0] for t in (A._xin0, B._xin0)] == [12, 8] and A._frames % A._xin0.shape[0] != B._frames % B._xin0.shape[0]
    before = A._position()
    state = A.export_streams([4, 1])
    assert A._position() == before and state.ages.tolist() == [T_A, T_A] and state.packed.shape == (2, A.record_floats())
    B.import_streams(state, [0, 2])
    assert B.stream_ages().tolist() == [T_A, T_B, T_A] and B.streams_ready().all() and B._counters() == Bt._counters()
    if model in ("stgcn", "stgcnmod"):
        assert (B.__dict__.get("_plan") is not None) == native_plan
    predictions = 0
    for t in range(0, T_MORE, r):
        cyc_a = [fa[T_A + t + f] for f in range(r)]
        cyc_bt = [fb[T_B + t + f] for f in range(r)]
        cyc_b = []
        for xa, xb in zip(cyc_a, cyc_bt):
            x = xb.clone()
            x[[0, 2]] = xa[[4, 1]]
            cyc_b.append(x)
        ra, rc, rb, rbt = A._cycle(cyc_a), C._cycle(cyc_a), B._cycle(cyc_b), Bt._cycle(cyc_bt)
        predictions += _same_streams(B, rb, [0, 2], C, rc, [4, 1], mv, (t, "moved"))
        _same_streams(B, rb, [1], Bt, rbt, [1], mv, (t, "the target's own stream"))
        _same_streams(A, ra, range(5), C, rc, range(5), mv, (t, "the source"))
    assert predictions >= T_MORE // A.stride - 1
    assert B.stream_ages().tolist() == [T_A + T_MORE, T_B + T_MORE, T_A + T_MORE]


# ---- one pair of ready slabs with every small state, shared by the tests that only look at the import itself ----------------
def _with_small_states(net):
    pkg.set_input_modality(net, "joint_motion")
    pkg.set_pre_normalization(net)


@pytest.fixture(scope="module")
def ready_pair():
    (A, B), v = _make("stgcn", "ntu", True, (5, 3), setup=_with_small_states)
    B.set_max_cycle(4)
    _steps(A, _frames(T_A, 5, v, 31), 0, T_A, 4)
    _steps(B, _frames(T_B, 3, v, 32), 0, T_B, 4)
    return A, B


@contextlib.contextmanager
def _restored(net):
    """Put the slab back as it was (tensors and stepping position): the pair is shared."""
    tensors = net._state_tensors()
    keep, position = [t.clone() for t in tensors], net._position()
    try:
        yield
    finally:
        for t, k in zip(tensors, keep):
            t.copy_(k)
        net._set_position(position)


def _job_tensors(net):
    by_ptr = {t.data_ptr(): t for t in net._state_tensors()}
    jobs, _ = net._move_jobs()
    return [(job, by_ptr[job.ring]) for job in jobs]


def test_an_import_touches_nothing_but_the_window_of_the_named_streams(ready_pair):
    """All 25 jobs (21 rings, previous frame + flag of the motion modality, rotations + flag of the pre-normalisation): after the
    import every state tensor of B equals its pre-import copy with the window slots of streams 0 and 2 replaced by A's window
    of streams 4 and 1 -- so the neighbours, the P padding, the slots outside the window, layer 10's output ring and the pooled
    buffer are unchanged.  The records sit between NaN guard records and a NaN record behind the two that are moved."""
    A, B = ready_pair
    with _restored(B):
        record = A.record_floats()
        guard = torch.full((6, record), NAN, device=DEV)
        packed = guard[2:5]                                                     # 3 records; the export fills 2
        idx = A._device_indices([4, 1])
        A._move(packed, idx, 2, to_ring=False)
        torch.cuda.synchronize()
        assert bool(torch.isnan(guard[:2]).all()) and bool(torch.isnan(guard[4:]).all())
        assert torch.equal(packed[:2], A.export_streams([4, 1]).packed) and not bool(torch.isnan(packed[:2]).any())
        tensors = B._state_tensors()
        want = {t.data_ptr(): t.clone() for t in tensors}
        pairs = list(zip(_job_tensors(A), _job_tensors(B)))
        assert len(pairs) == 25
        for (ja, ta), (jb, tb) in pairs:
            w = want[tb.data_ptr()]
            assert ja.window == jb.window and ja.seg == jb.seg
            if ja.depth > 1:
                assert (ja.depth, ja.newest) != (jb.depth, jb.newest) or ja.kind == native.SCRUB_POOL_RING
            for sa, sb in zip(mig.window_slots(ja.newest, ja.depth, ja.window), mig.window_slots(jb.newest, jb.depth, jb.window)):
                for src, dst in ((4, 0), (1, 2)):
                    if ja.kind == native.SCRUB_POOL_RING:
                        w[sb, dst] = ta[sa, src]
                    elif ta.dim() == 3:
                        w[sb, :, dst * ja.seg:(dst + 1) * ja.seg] = ta[sa, :, src * ja.seg:(src + 1) * ja.seg]
                    else:                                                       # a per-stream array: row = stream
                        w[dst] = ta[src]
        B.import_streams(pkg.StreamState(packed[:2], torch.tensor([T_A, T_A]), A.move_signature()), [0, 2])
        torch.cuda.synchronize()
        for t in tensors:
            assert _same_bits(t, want[t.data_ptr()]), tuple(t.shape)
        assert bool(torch.isnan(guard[:2]).all()) and bool(torch.isnan(guard[4:]).all())


def test_an_import_through_host_memory_gives_the_same_bits(ready_pair):
    A, B = ready_pair
    with _restored(B):
        state = A.export_streams([4, 1])
        B.import_streams(state, [0, 2])
        direct = [t.clone() for t in B._state_tensors()]
        ages = B.stream_ages().tolist()
    with _restored(B):
        buf = io.BytesIO()
        torch.save(state.cpu(), buf)
        buf.seek(0)
        back = torch.load(buf)
        assert back.packed.device.type == "cpu"
        with pytest.raises(RuntimeError, match="packed records must be"):
            B.import_streams(back, [0, 2])                                      # host records do not launch
        B.import_streams(back.to(DEV), [0, 2])
        assert all(_same_bits(t, d) for t, d in zip(B._state_tensors(), direct)) and B.stream_ages().tolist() == ages


# ---- the small per-stream states -----------------------------------------------------------------------------------------
def _offsets(net):
    out, offset = {}, 0
    for name, rows, seg, window in net._move_windows():
        out[name] = (offset, rows * seg * window)
        offset += rows * seg * window
    return out


@pytest.mark.parametrize("which", ["joint_motion", "pre_normalization"])
def test_the_small_states_travel_with_the_stream(which):
    """With a motion modality the previous raw frame and its flag, with the pre-normalisation the rotations latched from the
    stream's first frame and their flag are part of the record: the moved stream equals the unmoved twin.  A second target
    imports the same records with those fields zeroed (a move that left them behind): its moved rows then DIFFER from the twin
    in the logits, so the comparison above does depend on them."""
    setup = (lambda net: pkg.set_input_modality(net, "joint_motion")) if which == "joint_motion" else pkg.set_pre_normalization
    (A, C, B, Bad), v = _make("stgcn", "ntu", True, (5, 5, 3, 3), setup=setup)
    mv, r = 2 * v, 4
    for net in (B, Bad):
        net.set_max_cycle(4)
    fa, fb = _frames(T_A + T_MORE, 5, v, 41), _frames(T_B + T_MORE, 3, v, 42)
    for net in (A, C):
        _steps(net, fa, 0, T_A, r)
    for net in (B, Bad):
        _steps(net, fb, 0, T_B, r)
    state = A.export_streams([4, 1])
    B.import_streams(state, [0, 2])
    broken = pkg.StreamState(state.packed.clone(), state.ages, state.signature)
    offsets = _offsets(A)
    for name in (("mod_prev", "mod_flags") if which == "joint_motion" else ("pn_rot", "pn_flags")):
        o, size = offsets[name]
        assert bool((state.packed[:, o:o + size].view(torch.int32) != 0).any()), name
        broken.packed[:, o:o + size] = 0.0
    Bad.import_streams(broken, [0, 2])
    differed = 0
    for t in range(0, T_MORE, r):
        cyc_a = [fa[T_A + t + f] for f in range(r)]
        cyc_b = []
        for xa, xb in zip(cyc_a, [fb[T_B + t + f] for f in range(r)]):
            x = xb.clone()
            x[[0, 2]] = xa[[4, 1]]
            cyc_b.append(x)
        rc, rb, rbad = C._cycle(cyc_a), B._cycle(cyc_b), Bad._cycle(cyc_b)
        _same_streams(B, rb, [0, 2], C, rc, [4, 1], mv, (t, which))
        _same_streams(Bad, rbad, [1], B, rb, [1], mv, (t, "the stream that did not move"))
        differed += sum(not torch.equal(x[[0, 2]], y[[4, 1]]) for x, y in zip(rbad[2], rc[2]))
    assert differed >= 1, "zeroing the small states in the record changed no prediction: the test would not see them missing"


# ---- resize ----------------------------------------------------------------------------------------------------------------
def test_resize_keeps_the_named_streams_and_starts_the_others_fresh():
    """7 ready streams -> resize_streams(4, keep=[6, 0, 3]) at frame 96: new streams 0-2 continue as old 6, 0, 3 do in the twin
    that was not resized; new stream 3 is a fresh model from that frame on (features and logits from the fresh model's first
    emission), and ``streams_ready()`` turns true for it exactly when the fresh model first answers."""
    (S, T, F), v = _make("stgcn", "ntu", True, (7, 7, 1))
    mv, r, t_end = 2 * v, 4, T_A + 92
    fs, ff = _frames(t_end, 7, v, 51), _frames(t_end, 1, v, 52)
    for net in (S, T):
        _steps(net, fs, 0, T_A, r)
    counters = S._counters()
    S.resize_streams(4, keep=[6, 0, 3])
    assert S._n == 4 and S._counters() == counters and S.stream_ages().tolist() == [T_A, T_A, T_A, 0]
    assert S.__dict__.get("_plan") is not None and S._xin0.shape[2] == 200
    assert S.streams_ready().tolist() == [True, True, True, False] and S._cohorts[T_A][0] == [3]
    answered, compared = False, 0
    for t in range(T_A, t_end, r):
        cyc_t = [fs[t + f] for f in range(r)]
        cyc_f = [ff[t + f] for f in range(r)]
        cyc_s = [torch.cat([x[[6, 0, 3]], y], dim=0) for x, y in zip(cyc_t, cyc_f)]
        rs, rt, rf = S._cycle(cyc_s), T._cycle(cyc_t), F._cycle(cyc_f)
        _same_streams(S, rs, [0, 1, 2], T, rt, [6, 0, 3], mv, (t, "kept"))
        (slot_s, nf_s, log_s), (slot_f, nf_f, log_f) = rs, rf
        if nf_f:
            assert nf_s == nf_f
            for j in range(nf_f):
                compared += 1
                assert torch.equal(_feat(S, slot_s, j, 3, mv), _feat(F, slot_f, j, 0, mv)), (t, "fresh features")
        if log_f:
            assert len(log_s) == len(log_f)
            for x, y in zip(log_s, log_f):
                compared += 1
                assert torch.equal(x[3], y[0]), (t, "fresh logits")
        answered = answered or bool(log_f)
        assert S.streams_ready().tolist() == [True, True, True, answered], t
    assert answered and compared >= 5 and not S._warming()


# ---- StreamShards ------------------------------------------------------------------------------------------------------------
def test_a_stream_moves_between_the_shards_of_a_stream_shards():
    """2 shards x 3 streams: global stream 1 (shard 0) replaces global stream 4 (shard 1).  Row 4 then continues as row 1 of a
    twin set-up that moved nothing; the other rows equal the twin's.  The records come in the order of the indices."""
    nets, v = _make("stgcn", "ntu", True, (3, 3, 3, 3))
    pool = list(nets)
    moved = pkg.parallel.StreamShards(lambda: pool.pop(0), 6, 2, torch.device(DEV))
    twin = pkg.parallel.StreamShards(lambda: pool.pop(0), 6, 2, torch.device(DEV))
    frames, r = _frames(T_A + T_MORE, 6, v, 61), 4
    for t in range(0, T_A, r):
        for shards in (moved, twin):
            shards.forward_cycle([frames[t + f] for f in range(r)])
    state = moved.export_streams([4, 1])
    torch.cuda.synchronize()
    assert torch.equal(state.packed[0], moved.models[1].export_streams([1]).packed[0])
    assert torch.equal(state.packed[1], moved.models[0].export_streams([1]).packed[0]) and state.ages.tolist() == [T_A, T_A]
    with pytest.raises(ValueError, match="outside a slab of 6"):
        moved.export_streams([6])
    one = moved.export_streams([1])
    moved.import_streams(one, [4])
    predictions = 0
    for t in range(T_A, T_A + T_MORE, r):
        cyc = [frames[t + f] for f in range(r)]
        cyc_m = []
        for x in cyc:
            y = x.clone()
            y[4] = x[1]
            cyc_m.append(y)
        got, want = moved.forward_cycle(cyc_m), twin.forward_cycle(cyc)
        assert (got is None) == (want is None)
        if got is not None:
            predictions += 1
            assert torch.equal(got[4], want[1]) and torch.equal(got[[0, 1, 2, 3, 5]], want[[0, 1, 2, 3, 5]]), t
    assert predictions >= 5 and moved.stream_ages().tolist() == [T_A + T_MORE] * 6
