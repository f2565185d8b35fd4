"""Moving streams between slabs, the parts that need no GPU: the symbol and its signature, the argument checks of
csk_co_move_streams_f32 (made on the host side of the entry), the job arithmetic against a brute-force ring model, the record
sizes, every refusal of export_streams / import_streams / resize_streams (no launch), and the StreamState round trip."""
import ctypes as C
import io
import os
import random
import re

import pytest
import torch

import _bootstrap

pkg = _bootstrap.load()
native, mig = pkg.native, pkg.co_migrate
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = pkg.ntu_graph().A


def test_symbol_signature_and_abi():
    hdr = open(os.path.join(ROOT, "include", "cskel.h")).read()
    decl = re.search(r"int csk_co_move_streams_f32\(([^;]*)\);", hdr)
    assert decl, "csk_co_move_streams_f32 is not declared in include/cskel.h"
    params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
    kinds = [C.c_void_p if "*" in p else (C.c_int64 if p.startswith("int64_t") else C.c_int) for p in params]
    assert native.SIGNATURES["csk_co_move_streams_f32"] == kinds and len(kinds) == 9
    lib = C.CDLL(native.LIB_PATH)
    assert hasattr(lib, "csk_co_move_streams_f32")
    assert native.lib().csk_abi_version() == native.ABI_VERSION == 16
    assert int(re.search(r"#define CSK_CO_MOVE_MAX_JOBS (\d+)", hdr).group(1)) == native.MOVE_MAX_JOBS
    # the struct mirror: field order and sizes of csk_move_job
    body = re.search(r"typedef struct csk_move_job \{(.*?)\} csk_move_job;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for line in body.split(";") if line.strip() for n in line.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in native.MoveJob._fields_]
    assert C.sizeof(native.MoveJob) == 8 + 8 + 8 + 6 * 4


def _job(ring=0x1000, row_floats=252, offset=0, depth=12, rows=64, newest=3, window=4, seg=50, kind=native.SCRUB_BLOCK_RING):
    return native.MoveJob(ring, row_floats, offset, depth, rows, newest, window, seg, kind)


def _call(jobs, n_jobs=None, packed=0x2000, record=1 << 20, streams=0x3000, n_streams=2, n_total=5, to_ring=0):
    arr = (native.MoveJob * max(1, len(jobs)))(*jobs)
    return native.lib().csk_co_move_streams_f32(C.byref(arr) if jobs else None, len(jobs) if n_jobs is None else n_jobs,
                                                C.c_void_p(packed), record, C.c_void_p(streams), n_streams, n_total, to_ring, None)


@pytest.mark.parametrize("kwargs, needle", [
    (dict(jobs=[]), "null pointer"),
    (dict(jobs=[_job()], n_jobs=0), "jobs per launch"),
    (dict(jobs=[_job()], n_jobs=native.MOVE_MAX_JOBS + 1), "jobs per launch"),
    (dict(jobs=[_job()], n_streams=-1), "n_streams < 0"),
    (dict(jobs=[_job()], n_total=0), "n_total >= 1"),
    (dict(jobs=[_job()], record=0), "record of 0"),
    (dict(jobs=[_job()], to_ring=2), "to_ring"),
    (dict(jobs=[_job()], streams=0), "null pointer"),
    (dict(jobs=[_job()], packed=0), "null pointer"),
    (dict(jobs=[_job()], packed=0x2002), "4-byte aligned"),
    (dict(jobs=[_job(ring=0)]), "null pointer"),
    (dict(jobs=[_job(ring=0x1002)]), "4-byte aligned"),
    (dict(jobs=[_job(depth=0)]), "bad dims"),
    (dict(jobs=[_job(seg=0)]), "bad dims"),
    (dict(jobs=[_job(newest=12)]), "newest slot"),
    (dict(jobs=[_job(newest=-1)]), "newest slot"),
    (dict(jobs=[_job(window=13)]), "longer than the ring"),
    (dict(jobs=[_job(window=-1)]), "longer than the ring"),
    (dict(jobs=[_job(seg=51)]), "cannot fit a row"),
    (dict(jobs=[_job(kind=7)]), "unknown ring kind"),
    (dict(jobs=[_job(kind=native.SCRUB_POOL_RING, rows=4, row_floats=256, seg=256)]), "pooling ring"),
    (dict(jobs=[_job(offset=-1)]), "of a record of"),
    (dict(jobs=[_job()], record=4 * 64 * 50 - 1), "of a record of"),
    (dict(jobs=[_job(offset=1)], record=4 * 64 * 50), "of a record of"),
])
def test_move_entry_refuses_bad_arguments_without_a_gpu(kwargs, needle):
    lib = native.lib()
    assert _call(**kwargs) < 0
    assert needle in lib.csk_last_error().decode()


def test_move_entry_with_nothing_to_do_launches_nothing():
    assert _call([_job()], n_streams=0, streams=0, packed=0) == 0
    assert _call([_job(window=0), _job(window=0, kind=native.SCRUB_POOL_RING, rows=5, row_floats=256, seg=256)]) == 0


def _ring_model(depth, frames):
    """Brute force: feed frames 0 .. frames - 1 into a ring of ``depth`` slots; returns {frame number: slot} of what it holds."""
    slots = {}
    for s in range(frames):
        slots[s % depth] = s
    return {frame: slot for slot, frame in slots.items()}


def test_job_arithmetic_against_a_brute_force_ring():
    """A window exported at (source count, source depth) and imported at (target count, target depth): record entry i must be
    source frame count_s - window + i and must land in the slot where the target's kernels look for frame count_t - window + i
    (slot = frame % depth); no slot outside the window is addressed on either side."""
    rng = random.Random(19)
    for _ in range(2000):
        d_src, d_dst = rng.randint(5, 16), rng.randint(5, 16)
        window = rng.choice([0, 4, 8])
        if window > min(d_src, d_dst):
            continue
        s_src, s_dst = rng.randint(window, 400), rng.randint(window, 400)
        held_src, held_dst = _ring_model(d_src, s_src), _ring_model(d_dst, s_dst)
        (n_src, w_src), (n_dst, w_dst) = mig.ring_window(s_src, d_src, window), mig.ring_window(s_dst, d_dst, window)
        src, dst = mig.window_slots(n_src, d_src, w_src), mig.window_slots(n_dst, d_dst, w_dst)
        assert len(src) == len(dst) == window and len(set(src)) == len(set(dst)) == window
        for i in range(window):
            assert held_src[s_src - window + i] == src[i]                          # oldest first, the frames that are live
            assert (s_dst - window + i) % d_dst == dst[i] == held_dst[s_dst - window + i]
        assert all(0 <= s < d_src for s in src) and all(0 <= s < d_dst for s in dst)
    with pytest.raises(ValueError):
        mig.ring_window(20, 5, 6)


def _cpu_bound(cls=None, n=5, max_cycle=8, frames=0, **kw):
    net = (cls or pkg.CoStGcn)(A, pool_size=3, pool_padding=1, **kw).eval()
    net.use_native_plan = False
    net.set_max_cycle(max_cycle)
    net._bind(n, torch.device("cpu"))
    if frames:
        _set_position(net, frames)
    return net


def _set_position(net, frames):
    """The counters a slab has after ``frames`` frames (continual.emissions per block, the head behind them)."""
    r, ctr = frames, [frames]
    per_block = []
    for blk in net._blocks:
        _, e = pkg.continual.emissions(0, r, blk.delay, blk.stride)
        per_block += [r, e]
        r = e
    net._set_counters(ctr + [r] + per_block)


@pytest.mark.parametrize("cls", ["CoStGcn", "CoStGcnMod"])
def test_model_job_list_matches_the_ring_model(cls):
    """The whole job list of a bound slab, at two positions and two sets of ring depths: every job's window is the newest
    frames of the counter that owns the ring, the offsets tile the record without gap or overlap."""
    for max_cycle, frames in ((8, 96), (4, 100), (1, 164)):
        net = _cpu_bound(getattr(pkg, cls), max_cycle=max_cycle, frames=frames)
        jobs, record = net._move_jobs()
        assert record == net.record_floats() and len(jobs) == 21 <= native.MOVE_MAX_JOBS
        rings = [(net._xin0, net._frames)]
        for blk in net._blocks:
            rings += [(blk._state.y, blk._state.s), (blk._state.out, blk._state.e)]
        rings = rings[:-1] + [(net._pool_ring, net._feats)]
        offset = 0
        for job, (t, count) in zip(jobs, rings):
            assert job.ring == t.data_ptr() and job.depth == t.shape[0] and job.offset == offset
            held = _ring_model(job.depth, count)
            slots = mig.window_slots(job.newest, job.depth, job.window)
            live = [held.get(count - job.window + i, None) for i in range(job.window)]
            assert all(a is None or a == b for a, b in zip(live, slots))         # None: a frame the ring has not received yet
            assert [s for s in slots] == [(count - job.window + i) % job.depth for i in range(job.window)]
            rows = 1 if job.kind == native.SCRUB_POOL_RING else job.rows
            offset += job.window * rows * job.seg
        assert offset == record


def _expected_record(table, c, v, m, pool_size, extra=0):
    mv = v * m
    words = 4 * c * mv + sum(8 * co * mv for _, co, _, _ in table) + sum(4 * co * mv for _, co, _, _ in table[:-1])
    return words + pool_size * 256 + extra


def test_record_size_is_the_sum_of_the_windows():
    table, table_mod = pkg.models.layer_table(3, False), pkg.models.layer_table(3, True)
    K = pkg.kinetics_graph().A
    ntu = pkg.CoStGcn(A)
    assert ntu.record_floats() == _expected_record(table, 3, 25, 2, ntu.pool_size) == 813400
    mod = pkg.CoStGcnMod(A)
    assert mod.record_floats() == _expected_record(table_mod, 3, 25, 2, mod.pool_size)
    kin = pkg.CoStGcn(K, input_shape=(3, 300, 18, 2), num_classes=400)
    assert kin.record_floats() == _expected_record(table, 3, 18, 2, kin.pool_size)
    kin_mod = pkg.CoStGcnMod(K, input_shape=(3, 300, 18, 2), num_classes=400, pool_size=5, pool_padding=0)
    assert kin_mod.record_floats() == _expected_record(table_mod, 3, 18, 2, 5)
    pkg.set_input_modality(ntu, "joint_motion")
    assert ntu.record_floats() == _expected_record(table, 3, 25, 2, ntu.pool_size, extra=3 * 25 * 2 + 1)
    pkg.set_pre_normalization(ntu)
    assert ntu.record_floats() == _expected_record(table, 3, 25, 2, ntu.pool_size, extra=3 * 25 * 2 + 1 + 36 + 1)
    assert len(ntu._move_windows()) == 25 <= native.MOVE_MAX_JOBS
    # the windows follow the blocks: a shorter temporal kernel in one block shrinks its y window and its input's lag
    ntu.layers["layer3"].kernel_size = 5
    w = dict((name, window) for name, _, _, window in ntu._move_windows())
    assert (w["y2"], w["out1"], w["y3"], w["out2"]) == (4, 2, 8, 4)


class _NoLaunch:
    """Stands in for the library: any call is a failure of the test."""
    calls = 0

    def __getattr__(self, name):
        def entry(*a, **k):
            _NoLaunch.calls += 1
            raise AssertionError(f"{name} was called")
        return entry


def _state_of(net, n=2, ages=(200, 200)):
    return pkg.StreamState(torch.zeros((n, net.record_floats())), torch.tensor(list(ages[:n]), dtype=torch.int64), net.move_signature())


def test_every_refusal_is_made_on_the_host_without_a_launch(monkeypatch):
    monkeypatch.setattr(native, "lib", lambda: _NoLaunch())
    _NoLaunch.calls = 0
    fresh = pkg.CoStGcn(A, pool_size=3, pool_padding=1).eval()
    for call in (lambda: fresh.export_streams([1]), lambda: fresh.import_streams(_state_of(fresh, 1), [1]),
                 lambda: fresh.resize_streams(3, [1])):
        with pytest.raises(RuntimeError, match="no state slab is bound"):
            call()
    net = _cpu_bound(frames=200)
    state = _state_of(net)
    for bad, needle in ((torch.tensor([1]), "not a tensor"), (1, "sequence of ints"), ([1.0], "takes ints"), ([True], "takes ints"),
                        ([1, 1], "duplicate"), ([5], "outside a slab of 5"), ([-1], "outside a slab of 5")):
        with pytest.raises(ValueError, match=needle):
            net.export_streams(bad)
        with pytest.raises(ValueError, match=needle):
            net.import_streams(state, bad)
        with pytest.raises(ValueError, match=needle):
            net.resize_streams(4, bad)
    # frame count not a multiple of the total stride
    for frames in (201, 202, 203):
        net._frames = frames
        for call in (lambda: net.export_streams([1]), lambda: net.import_streams(state, [1, 2]), lambda: net.resize_streams(4, [1])):
            with pytest.raises(RuntimeError, match="multiple of 4"):
                call()
    net._frames = 200
    net._flushed = True
    for call in (lambda: net.export_streams([1]), lambda: net.import_streams(state, [1, 2]), lambda: net.resize_streams(4, [1])):
        with pytest.raises(RuntimeError, match="flushed"):
            call()
    net._flushed = False
    # a warming stream does not leave
    net._reset_at[2] = 160
    net._cohorts[160] = ([2], None)
    with pytest.raises(RuntimeError, match=r"streams \[2\] are still warming.*streams_ready\(\)"):
        net.export_streams([1, 2])
    net._forget_resets()
    # the target must be ready
    young = _cpu_bound(frames=80)
    assert young._ready_age() == 81
    with pytest.raises(RuntimeError, match="step it through its warm-up first"):
        young.import_streams(state, [0, 1])
    with pytest.raises(RuntimeError, match="still warming"):
        young.export_streams([0])
    # counts
    with pytest.raises(ValueError, match="1 indices for 2 records"):
        net.import_streams(state, [1])
    with pytest.raises(TypeError, match="StreamState"):
        net.import_streams(state.packed, [1, 2])
    with pytest.raises(ValueError, match="do not fit a slab of 1"):
        net.resize_streams(1, [0, 1])
    with pytest.raises(ValueError, match="positive int"):
        net.resize_streams(0, [])
    # a slab whose pooling window counts fewer entries than the stream brings (pool_padding > 0)
    ripe = _cpu_bound(frames=84)                                    # features: frames 76, 80 -> 2 of 3 window entries
    assert ripe._feats == 2
    with pytest.raises(RuntimeError, match="brings 3 pooling-window entries"):
        ripe.import_streams(state, [0, 1])
    assert _NoLaunch.calls == 0


def test_signature_mismatch_names_the_first_differing_field(monkeypatch):
    monkeypatch.setattr(native, "lib", lambda: _NoLaunch())
    _NoLaunch.calls = 0
    net = _cpu_bound(frames=200)
    state = _state_of(net)
    fields = [name for name, _ in net.move_signature()]
    assert fields == ["graph_convs", "layers", "input_cvm", "pool_size", "pool_padding", "input_modality", "pre_normalization",
                      "split_k", "step_precision"]

    def other(**kw):
        o = pkg.CoStGcn(A, **{**dict(pool_size=3, pool_padding=1), **kw}).eval()
        return o

    cases = {"pool_size": other(pool_size=4), "pool_padding": other(pool_padding=0),
             "input_modality": pkg.set_input_modality(other(), "joint_motion"),
             "pre_normalization": pkg.set_pre_normalization(other()),
             "layers": pkg.CoStGcnMod(A, pool_size=3, pool_padding=1).eval(),
             "graph_convs": pkg.CoAGcn(A, pool_size=3, pool_padding=1).eval(),
             "input_cvm": pkg.CoStGcn(pkg.kinetics_graph().A, input_shape=(3, 300, 18, 2), pool_size=3, pool_padding=1).eval()}
    lat = other()
    lat.set_latency_mode(8)
    cases["split_k"] = lat
    cases["step_precision"] = pkg.set_step_precision(other(), "bf16x3")
    assert set(cases) == set(fields)
    for field, model in cases.items():
        foreign = pkg.StreamState(state.packed, state.ages, model.move_signature())
        with pytest.raises(ValueError, match=f"differs in '{field}'"):
            net.import_streams(foreign, [0, 1])
    assert _NoLaunch.calls == 0


def test_stream_state_round_trip_through_torch_save():
    net = pkg.CoStGcn(A, pool_size=3, pool_padding=1).eval()
    packed = torch.randn((3, net.record_floats()))
    state = pkg.StreamState(packed, torch.tensor([100, 164, 96]), net.move_signature())
    buf = io.BytesIO()
    torch.save(state, buf)
    buf.seek(0)
    back = torch.load(buf)
    assert isinstance(back, pkg.StreamState) and len(back) == 3 and back.record_floats == net.record_floats()
    assert torch.equal(back.packed, packed) and back.ages.tolist() == [100, 164, 96]
    assert back.signature == state.signature and mig.first_difference(net.move_signature(), back.signature) is None
    assert back.cpu().packed.device.type == "cpu" and back.to("cpu").signature == state.signature


def test_import_bookkeeping_keeps_true_ages(monkeypatch):
    """``_adopt``: an imported stream older than the slab gets a negative ``_reset_at``; it leaves its warming cohort."""
    net = _cpu_bound(frames=200)
    monkeypatch.setattr(net, "_device_indices", lambda idx: None)
    net._reset_at[1] = net._reset_at[3] = 160
    net._cohorts[160] = ([1, 3], None)
    net._adopt([3, 0], [1000, 120])
    assert net.stream_ages().tolist() == [120, 40, 200, 1000, 200] and net._reset_at[3] == -800
    assert net._cohorts[160][0] == [1] and net.streams_ready().tolist() == [True, False, True, True, True]
