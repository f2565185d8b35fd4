"""The one inventory of a slab's rings (co_rings.py), the parts that need no GPU: every driver that works on "the segments of
some streams in some slots of every ring" reads ``_rings()``, so a ring the inventory misses is a ring a reset leaves stale
and a record lacks.  A slab bound to CPU memory stands in for the device slab; the job lists are built and never launched."""
import pytest
import torch

import _bootstrap

pkg = _bootstrap.load()
native = pkg.native
A = pkg.ntu_graph().A
MODELS = ["CoStGcn", "CoStGcnMod", "CoAGcn", "CoSTr"]


def _cpu_bound(cls, stages_on, n=5):
    net = cls(A, pool_size=3, pool_padding=1).eval()
    if stages_on:
        pkg.set_input_modality(net, "joint_motion")
        pkg.set_pre_normalization(net)
    net.use_native_plan = False
    net._bind(n, torch.device("cpu"))
    return net


def _check_the_inventory_covers_the_slab(net):
    """The full-reset job list covers every state tensor but the head's output row and what a reset leaves on purpose; the
    move job list is the windowed entries of the inventory, in order, offsets tiling the record."""
    # ---- reset: every ring of the slab, whole depth, plus the stages' flags ----
    jobs = net._reset_jobs()
    assert all(job.slot0 == 0 and job.n_slots == job.depth for job in jobs)
    stage_kept = {t.data_ptr() for stage in net._record_stages for t in stage.tensors() if t is not stage.flags}
    assert len(stage_kept) == sum(len(stage.tensors()) - 1 for stage in net._record_stages if stage.flags is not None)
    want = {t.data_ptr() for t in net._state_tensors()} - {net._pooled.data_ptr()} - stage_kept
    got = [job.ring for job in jobs]
    assert len(set(got)) == len(got) and set(got) == want, (len(got), len(want))
    # ---- move: the entries with a window, record order, running offsets ----
    rings = net._rings()
    assert [r.name for r in rings] == ["xin0"] + [f"{kind}{i}" for i in range(10) for kind in ("y", "out")] + ["pool"]
    assert [r.name for r in rings if r.window is None] == ["out9"]
    windowed = [(r.tensor.data_ptr(), r.rows * r.seg * r.window, r.seg) for r in rings if r.window is not None]
    windowed += [(t.data_ptr(), rows * seg * window, seg) for stage in net._record_stages
                 for (_, rows, seg, window), t in zip(stage.windows(), stage.tensors())]
    moves, record = net._move_jobs()
    assert len(moves) == len(windowed) == len(net._move_windows())
    offset = 0
    for job, (ptr, floats, seg) in zip(moves, windowed):
        assert (job.ring, job.offset, job.seg) == (ptr, offset, seg)
        offset += floats
    assert offset == record == net.record_floats()


@pytest.mark.parametrize("stages_on", [False, True], ids=["stages_off", "motion_prenorm"])
@pytest.mark.parametrize("cls", MODELS)
def test_the_inventory_is_complete(cls, stages_on):
    net = _cpu_bound(getattr(pkg, cls), stages_on)
    assert len(net._reset_jobs()) == 22 + (2 if stages_on else 0) <= native.SCRUB_MAX_JOBS
    _check_the_inventory_covers_the_slab(net)


def test_a_ring_the_inventory_does_not_know_fails_the_check():
    class WithAStrayRing(pkg.CoStGcn):
        def _bind(self, n, device):
            super()._bind(n, device)
            self._stray = torch.zeros((4, 8, self._p))

        def _state_tensors(self):
            return super()._state_tensors() + [self._stray]

    with pytest.raises(AssertionError):
        _check_the_inventory_covers_the_slab(_cpu_bound(WithAStrayRing, False))


# _cum_delays() == [0, 4, 8, 12, 16, 20, 28, 36, 44, 60, 76]: a cohort of age a has y_i scrubbed while a < D(i), out_i while
# a < D(i + 1), the pooling window while a < D(10).  FIRST_DEAD[age] = (first i whose y ring is scrubbed, first i whose out ring is).
FIRST_DEAD = {0: (1, 0), 4: (2, 1), 20: (6, 5), 40: (8, 7), 72: (10, 9), 76: (10, 10)}
# what a 4-frame cycle adds to the counters {frames, features, (received, emitted) x 10}: strides 1 1 1 1 2 1 1 2 1 1
CYCLE = [4, 1] + [4, 4] * 4 + [4, 2] + [2, 2] * 2 + [2, 1] + [1, 1] * 2


def _expected_scrub(age, before):
    y_from, out_from = FIRST_DEAD[age]
    names = [f"{kind}{i}" for i in range(10) for kind, first in (("y", y_from), ("out", out_from)) if i >= first]
    names += ["pool"] if age < 76 else []
    index = {"pool": 1, **{f"y{i}": 2 + 2 * i for i in range(10)}, **{f"out{i}": 3 + 2 * i for i in range(10)}}
    return [(name, before[index[name]], CYCLE[index[name]]) for name in names]


@pytest.mark.parametrize("age", sorted(FIRST_DEAD))
def test_scrub_cycle_jobs_are_the_table_of_the_delays(age):
    net = _cpu_bound(pkg.CoStGcn, False)
    assert net._cum_delays() == [0, 4, 8, 12, 16, 20, 28, 36, 44, 60, 76]
    at = 160                                             # the cohort was reset at frame 160 of a slab that runs on
    before = [at + age, 37] + [c for i in range(10) for c in (1000 + 7 * i, 2000 + 11 * i)]
    after = [b + c for b, c in zip(before, CYCLE)]
    tensors = {r.name: r.tensor for r in net._rings()}
    (jobs,) = net._scrub_cycle_jobs([age], before, after)
    want = _expected_scrub(age, before)
    assert len(jobs) == len(want)
    for job, (name, first, count) in zip(jobs, want):
        t = tensors[name]
        assert job.ring == t.data_ptr() and job.depth == t.shape[0] and job.rows == t.shape[1] and job.row_floats == t.shape[2], name
        assert (job.slot0, job.n_slots) == (first % t.shape[0], count), name
        assert (job.kind, job.seg) == ((native.SCRUB_POOL_RING, 256) if name == "pool" else (native.SCRUB_BLOCK_RING, 50)), name
    # a counter that did not move launches nothing for its ring
    assert net._scrub_cycle_jobs([age], before, before) == [[]]
