"""The session fixture (stream_session_fixture.py) without a GPU: the schedules meet their coverage conditions, the ledger's
delays, ready ages, counters and ring depths are the models', every schedule compares every live stream often enough, and the
ledger's expectations catch seeded bookkeeping defects.  The defects are seeded in the real bookkeeping of slabs bound to CPU
memory whose launches are stubbed out (``_scrub``, ``_move``, the engines): the host side of every operation runs as it is."""
import builtins

import pytest
import torch

import _bootstrap
from tests import stream_session_fixture as fx

pkg = _bootstrap.load()
A = pkg.ntu_graph().A
CLASSES = {fx.PADDED: ["CoStGcn", "CoAGcn", "CoSTr"], fx.PADDED_POOL41: ["CoStGcn"], fx.UNPADDED: ["CoStGcnMod"]}
# tensors the GPU test compares per session (features and logits, per row and emission), derived by the ledger alone; the GPU
# test ends on the same figures (test_gpu_stream_session.py reads them from ``fx.comparisons``)
COMPARISONS = {"main": 547, "pool41": 306, "unpadded": 1978}


def test_the_sessions_meet_their_coverage_conditions():
    fx.assert_sessions_covered()


def test_a_session_without_a_required_event_is_not_covered(monkeypatch):
    """``assert_sessions_covered`` does notice: the main session without its imports into warming rows fails it."""
    schedule, geometry, primes = fx.SESSIONS["main"]
    cut = [e for e in schedule if e != ("move", "B", [1], "A", [3])]
    monkeypatch.setitem(fx.SESSIONS, "main", (cut, geometry, primes))
    with pytest.raises(AssertionError):
        fx.assert_sessions_covered()


def _bound(cls, geometry, slab="A"):
    n, max_cycle = fx.SLABS[slab]
    net = getattr(pkg, cls)(A, (3, 300, 25, 2), 60, pool_size=geometry.pool_size, pool_padding=geometry.pool_padding).eval()
    net.use_native_plan = False
    net.set_max_cycle(max_cycle)
    net._bind(n, torch.device("cpu"))
    return net


def _counters_after(net, frames):
    """The counters of a slab that was only stepped (continual.emissions per block, the head behind them)."""
    r, per_block = frames, []
    for blk in net._blocks:
        _, e = pkg.continual.emissions(0, r, blk.delay, blk.stride)
        per_block += [r, e]
        r = e
    return [frames, r] + per_block


@pytest.mark.parametrize("geometry,cls", [(g, c) for g, classes in CLASSES.items() for c in classes],
                         ids=[f"{c}-pool{g.pool_size}{g.pool_padding}" for g, classes in CLASSES.items() for c in classes])
def test_the_ledgers_geometry_is_the_models(geometry, cls):
    padded = [0, 4, 8, 12, 16, 20, 28, 36, 44, 60, 76]
    assert fx.PADDED.cum_delays() == padded and fx.UNPADDED.cum_delays() == list(range(0, 88, 8))
    for slab in fx.SLABS:
        net = _bound(cls, geometry, slab)
        assert geometry.cum_delays() == net._cum_delays() and geometry.ready_age() == net._ready_age()
        assert geometry.stride == net.stride
        assert [(name, level, counter, depth) for name, level, counter, depth in geometry.rings(net.max_cycle)] == \
               [(r.name, r.level, r.counter, r.tensor.shape[0]) for r in net._rings()]
        for frames in (0, 1, 75, 76, 77, 80, 81, 84, 85, 100, 163, 272):
            assert geometry.counters_at(frames) == _counters_after(net, frames), frames
            assert geometry.emissions_at(frames) == net._emissions_at(frames) == geometry.counters_at(frames)[1]


@pytest.mark.parametrize("name", sorted(fx.SESSIONS))
def test_every_live_stream_is_compared_and_most_logits_rows_mean_something(name):
    schedule, geometry, primes = fx.SESSIONS[name]
    per_stream, total, skipped = fx.comparisons(schedule, geometry, primes)
    assert total == COMPARISONS[name] == sum(per_stream.values())
    live = fx.live_streams(schedule, geometry, primes)
    assert live and all(per_stream.get(sid, 0) >= 3 for sid in live), sorted((per_stream.get(s, 0), str(s)) for s in live)[:3]
    assert skipped < 0.5, skipped
    assert sum(len(schedule) for schedule, _, _ in fx.SESSIONS.values()) < 600      # events, not frames: sessions stay short


# ---- the real bookkeeping on CPU-bound slabs, launches stubbed out ------------------------------------------------------------
class Mismatch(AssertionError):
    pass


class HostSession:
    """Plays a schedule on the host side of real models and compares ages, readiness, cohorts, counters and the rings each
    per-cycle scrub names with the ledger after every event."""

    def __init__(self, name, seed_defect=None):
        self.schedule, self.geometry, primes = fx.SESSIONS[name]
        self.ledger = fx.Ledger(self.geometry, primes)
        cls = CLASSES[self.geometry][0]
        self.nets = {slab: self._stubbed(_bound(cls, self.geometry, slab)) for slab in fx.SLABS}
        self.records = {}
        if seed_defect:
            for net in self.nets.values():
                seed_defect(net)

    @staticmethod
    def _stubbed(net):
        net.scrubbed = []
        net._device_indices = lambda idx: None
        net._move = lambda *a, **k: None
        net._scrub = lambda jobs, dev, count: jobs and net.scrubbed.append(sorted(job.ring for job in jobs))    # no jobs: no launch
        return net

    def _cycle(self, net, r):
        """``CoStGcn._cycle`` around its launches: the cycle-length checks, the counters, the scrub behind the cycle."""
        if not 1 <= r <= net.max_cycle:
            raise ValueError("cycle length")
        if net._cohorts:
            net._check_cycle_while_warming(r)
        before = net._counters()
        net.scrubbed.clear()                    # a reset scrubs too: only the scrub behind this cycle is compared
        net._set_counters(_counters_after(net, before[0] + r))
        if net._cohorts:
            net._scrub_cycle(before)

    def _do(self, event):
        kind, nets = event[0], self.nets
        if kind == "cycle":
            self._cycle(nets[event[1]], event[2])
        elif kind == "reset":
            nets[event[1]].reset_streams(event[2])
        elif kind == "take":
            self.records[event[3]] = nets[event[1]].export_streams(event[2])
        elif kind == "put":
            nets[event[2]].import_streams(self.records[event[1]], event[3])
        elif kind == "move":
            nets[event[3]].import_streams(nets[event[1]].export_streams(event[2]), event[4])
        elif kind == "prime":
            net, n, t = nets[event[1]], len(event[2]), event[3]
            if net.unpadded:
                net._check_prime(torch.zeros((n, 3, t, 25, 2)))
            net.import_streams(pkg.StreamState(torch.zeros((n, net.record_floats())), torch.full((n,), t, dtype=torch.int64),
                                               net.move_signature()), event[2])
        elif kind == "resize":
            nets[event[1]].resize_streams(event[2], event[3])

    def _compare(self, event, outcome):
        for slab, net in self.nets.items():
            got = (net.stream_ages().tolist(), net.streams_ready().tolist(), {at: sorted(m) for at, (m, _) in net._cohorts.items()},
                   net._counters(), net._n)
            want = (self.ledger.ages(slab), self.ledger.ready(slab), self.ledger.cohorts(slab), self.ledger.counters(slab),
                    self.ledger.slabs[slab].n)
            if got != want:
                raise Mismatch((event, slab, got, want))
        if isinstance(outcome, fx.Cycle):
            net = self.nets[outcome.slab]
            rings = {r.name: r for r in net._rings()}
            before, after = self.geometry.counters_at(net._frames - outcome.r), net._counters()
            wrote = {name for name, r in rings.items() if after[r.counter] > before[r.counter]}
            want = sorted(sorted(rings[name].tensor.data_ptr() for name in dead if name in wrote)
                          for _, dead in {(age, tuple(d)) for age, d in outcome.dead.values()})
            if sorted(jobs for jobs in net.scrubbed) != [w for w in want if w]:
                raise Mismatch((event, "scrubbed rings"))
            net.scrubbed.clear()

    def run(self):
        for event in self.schedule:
            outcome = self.ledger.apply(event)
            if event[0] == "refused":
                positions = {slab: net._position() for slab, net in self.nets.items()}
                try:
                    self._do(event[1])
                except getattr(builtins, event[2]):
                    pass
                else:
                    raise Mismatch((event, "was not refused"))
                if any(net._position() != positions[slab] for slab, net in self.nets.items()):
                    raise Mismatch((event, "left a trace"))
            else:
                self._do(event)
            self._compare(event, outcome)
        return self


@pytest.mark.parametrize("name", sorted(fx.SESSIONS))
def test_the_models_bookkeeping_follows_the_ledger(name):
    HostSession(name).run()


def _import_keeps_the_cohort(net):
    def adopt(idx, ages):
        for i, age in zip(idx, ages):
            net._reset_at[i] = net._frames - int(age)
    net._adopt = adopt


def _merge_drops_the_earlier_members(net):
    def reset_streams(indices):
        idx = net._check_reset(indices)
        net._leave_cohorts(idx)
        net._cohorts[net._frames] = (idx, None)
        for i in idx:
            net._reset_at[i] = net._frames
    net.reset_streams = reset_streams


def _resize_forgets_the_ages(net):
    real = net.resize_streams

    def resize_streams(n, keep):
        real(n, keep)
        net._reset_at = [net._frames if at < net._frames else at for at in net._reset_at]
        net._reset_at[:len(keep)] = [0] * len(keep)
    net.resize_streams = resize_streams


def _the_age_stays_behind(net):
    def adopt(idx, ages):
        net._leave_cohorts(idx)
    net._adopt = adopt


DEFECTS = [_import_keeps_the_cohort, _merge_drops_the_earlier_members, _resize_forgets_the_ages, _the_age_stays_behind]


@pytest.mark.parametrize("defect", DEFECTS, ids=[d.__name__.strip("_") for d in DEFECTS])
def test_a_seeded_bookkeeping_defect_is_caught(defect):
    """Each defect fails at least one schedule's expectations (and every schedule passes without it, above)."""
    caught = []
    for name in sorted(fx.SESSIONS):
        try:
            HostSession(name, defect).run()
        except Mismatch:
            caught.append(name)
    assert caught, defect.__name__
