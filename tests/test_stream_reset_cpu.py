"""Per-stream reset, the parts that need no GPU: the argument checks of csk_co_scrub_streams_f32 (made on the host side of
the entry, before any launch), the D(L) table derived from the blocks, and everything ``reset_streams`` refuses before it
touches the device (a slab bound to CPU memory stands in for the device slab: the checks never reach a launch)."""
import ctypes as C

import pytest
import torch

import _bootstrap

pkg = _bootstrap.load()
native = pkg.native
A = pkg.ntu_graph().A


def _job(ring=0x1000, row_floats=252, depth=12, rows=64, slot0=0, n_slots=4, seg=50, kind=native.SCRUB_BLOCK_RING):
    return native.ScrubJob(ring, row_floats, depth, rows, slot0, n_slots, seg, kind)


def _call(jobs, n_jobs=None, streams=0x2000, n_streams=2, n_total=5):
    arr = (native.ScrubJob * max(1, len(jobs)))(*jobs)
    return native.lib().csk_co_scrub_streams_f32(C.byref(arr) if jobs else None, len(jobs) if n_jobs is None else n_jobs,
                                                 C.c_void_p(streams) if streams else None, n_streams, n_total, None)


@pytest.mark.parametrize("kwargs,needle", [
    (dict(jobs=[]), "null pointer"),
    (dict(jobs=[_job()], n_jobs=0), "jobs per launch"),
    (dict(jobs=[_job()], n_jobs=native.SCRUB_MAX_JOBS + 1), "jobs per launch"),
    (dict(jobs=[_job()], n_streams=-1), "n_streams < 0"),
    (dict(jobs=[_job()], n_total=0), "n_total"),
    (dict(jobs=[_job()], n_streams=6), "cannot fit a slab"),
    (dict(jobs=[_job()], streams=0), "null pointer"),
    (dict(jobs=[_job(ring=0)]), "null pointer"),
    (dict(jobs=[_job(ring=0x1002)]), "4-byte aligned"),
    (dict(jobs=[_job(depth=0)]), "bad dims"),
    (dict(jobs=[_job(rows=0)]), "bad dims"),
    (dict(jobs=[_job(seg=0)]), "bad dims"),
    (dict(jobs=[_job(slot0=12)]), "outside a ring"),
    (dict(jobs=[_job(slot0=-1)]), "outside a ring"),
    (dict(jobs=[_job(n_slots=13)]), "longer than the ring"),
    (dict(jobs=[_job(n_slots=-1)]), "longer than the ring"),
    (dict(jobs=[_job(seg=51)]), "cannot fit a row"),                       # 5 streams x 51 floats > P = 252
    (dict(jobs=[_job(), _job(row_floats=200)]), "cannot fit a row"),       # every job of the table is checked
    (dict(jobs=[_job(kind=native.SCRUB_POOL_RING, rows=4, row_floats=256, seg=256)]), "pooling ring"),
    (dict(jobs=[_job(kind=native.SCRUB_POOL_RING, rows=5, row_floats=256, seg=128)]), "pooling ring"),
    (dict(jobs=[_job(kind=7)]), "unknown ring kind"),
])
def test_scrub_entry_refuses_bad_arguments_without_a_gpu(kwargs, needle):
    lib = native.lib()
    assert _call(**kwargs) == -1
    assert needle in lib.csk_last_error().decode(), lib.csk_last_error().decode()


def test_scrub_entry_with_nothing_to_do_launches_nothing():
    """No stream listed, or only empty slot runs: accepted, returns 0 -- and on a machine without a GPU that can only be
    because no launch was attempted."""
    assert _call([_job()], n_streams=0, streams=0) == 0
    assert _call([_job(n_slots=0), _job(n_slots=0, kind=native.SCRUB_POOL_RING, rows=5, row_floats=256, seg=256)]) == 0


def test_cumulative_delays_come_from_the_blocks():
    net = pkg.CoStGcn(A, pool_size=3, pool_padding=1).eval()
    assert net._cum_delays() == [0, 4, 8, 12, 16, 20, 28, 36, 44, 60, 76]
    assert net._cum_delays()[10] == net.delay and all(d % net.stride == 0 for d in net._cum_delays())
    assert net._ready_age() == 76 + 4 * 1 + 1                      # the pooling window emits from its second entry on
    assert pkg.CoStGcn(A, pool_size=1, pool_padding=0)._ready_age() == 77
    assert pkg.CoStGcn(A)._ready_age() == 76 + 4 * (75 - 19 - 1) + 1
    net.layers["layer3"].delay = 8                                 # derived, not a table: a longer delay moves all behind it
    assert net._cum_delays()[3:] == [16, 20, 24, 32, 40, 48, 64, 80]


def _cpu_bound(n=5):
    net = pkg.CoStGcn(A, pool_size=3, pool_padding=1).eval()
    net.use_native_plan = False
    net._bind(n, torch.device("cpu"))
    return net


def test_reset_streams_refuses_on_the_host():
    net = pkg.CoStGcn(A, pool_size=3, pool_padding=1).eval()
    with pytest.raises(ValueError, match="not a tensor"):
        net.reset_streams(torch.tensor([1]))
    with pytest.raises(ValueError, match="sequence of ints"):
        net.reset_streams(1)
    with pytest.raises(ValueError, match="takes ints"):
        net.reset_streams([1.0])
    with pytest.raises(ValueError, match="takes ints"):
        net.reset_streams([True])
    with pytest.raises(RuntimeError, match="no state slab is bound"):
        net.reset_streams([1])
    with pytest.raises(RuntimeError, match="no state slab is bound"):
        net.stream_ages()
    net = _cpu_bound()
    with pytest.raises(ValueError, match="duplicate"):
        net.reset_streams([1, 3, 1])
    with pytest.raises(ValueError, match="outside a slab of 5"):
        net.reset_streams([5])
    with pytest.raises(ValueError, match="outside a slab of 5"):
        net.reset_streams([-1])
    for frames in (1, 2, 3, 82):
        net._frames = frames
        with pytest.raises(RuntimeError, match="multiple of 4"):
            net.reset_streams([1])
    net._frames = 80
    net._flushed = True
    with pytest.raises(RuntimeError, match="flushed"):
        net.reset_streams([1])
    net._flushed = False
    net.reset_streams([])                                           # nothing to do: no launch, no cohort
    assert not net._warming() and net.stream_ages().tolist() == [80] * 5
    net.set_max_cycle(4)                                            # the slab is dropped: unbound again
    with pytest.raises(RuntimeError, match="no state slab is bound"):
        net.reset_streams([1])


def test_ages_follow_the_frame_counter_and_clean_state_clears_them():
    net = _cpu_bound()
    assert net.stream_ages().tolist() == [0] * 5 and not net.streams_ready().any()
    net._frames = 80
    assert net.stream_ages().tolist() == [80] * 5 and not net.streams_ready().any()
    net._frames = 81                                                # a fresh model has answered at frame index 80
    assert net.streams_ready().all()
    net._reset_at[2] = 40                                           # what reset_streams([2]) at frame 40 records
    net._cohorts[40] = ([2], None)
    assert net.stream_ages().tolist() == [81, 81, 41, 81, 81] and net.streams_ready().tolist() == [True, True, False, True, True]
    for r in (1, 2, 3):                                             # frame 81 is phase 1 of the stride cycle
        net._check_cycle_while_warming(r)
    for r in (4, 8):
        with pytest.raises(ValueError, match="crosses a multiple of 4"):
            net._check_cycle_while_warming(r)
    net._frames = 84
    for r in (1, 2, 3, 4):
        net._check_cycle_while_warming(r)
    for r in (5, 8):
        with pytest.raises(ValueError, match="crosses a multiple of 4"):
            net._check_cycle_while_warming(r)
    net.clean_state()
    assert net.stream_ages().tolist() == [0] * 5 and not net._warming()
    net._check_cycle_while_warming(8)                               # nothing warms: any cycle
