"""The continual stream slab in service ("Slab in service"): sessions of interleaved reset, move, prime and resize.

The project holds bitwise, each on its own, stream-position, cycle-length and engine invariance, "a reset stream is a fresh
model", "a moved stream is the stream that never moved" and "a primed record does not depend on batch or chunking".  It follows
that a logical stream's layer-10 features and logits depend on its own frames and its age alone, whatever happened to it or
around it.  Here schedules of tests/stream_session_fixture.py are played on slabs A (5 streams) and B (3 streams,
set_max_cycle(4)); the fixture's ledger -- not the model -- says which row holds which logical stream at which age, and every
emission is compared ``torch.equal`` with a reference slab that holds one row per logical stream and is only ever stepped, in
4-frame cycles from the clean state (streams born by ``prime_streams``: a second reference slab, stepped to readiness on other
frames, primed once per stream, then only stepped).  After every event the host bookkeeping equals the ledger's, the counters
equal those of a twin that only stepped; after a cycle every warming row is exactly +0 in the slots the cycle wrote of every
ring that is not live yet at its age; a refused event raises the ledger's exception type and leaves every state byte and the
position as they were.  A peek (``forward_step(update_state=False)``) by its documented contract overwrites the slots the next
real step rewrites (and the head's output row): every other byte of the state and the position are unchanged.

``CoAGcn`` primes through ``prime_streams_as_steps``; its reference is primed the same way.  ``CoStGcnMod`` has no priming: its
schedule holds the refusal (NotImplementedError, no trace) in the place of prime events.

The number of tensors compared per session is derived on the CPU (test_stream_session_fixture_cpu.py: COMPARISONS) and
asserted at the end of every case."""
import builtins

import pytest
import torch

import _bootstrap
from tests import stream_session_fixture as fx
from tests.helpers import randomise_unit_

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
DEV = "cuda:0"
WARM = 96               # frames the primed streams' reference slab steps on other frames before it is primed


def _small_states(net):
    pkg.set_input_modality(net, "joint_motion")
    pkg.set_pre_normalization(net)


def _latency(net):
    net.set_latency_mode(8)


SETUPS = {None: None, "small": _small_states, "latency": _latency}
CLASSES = {"stgcn": "CoStGcn", "agcn": "CoAGcn", "str": "CoSTr", "stgcnmod": "CoStGcnMod"}
# (model, graph, native plan, session, setup)
CASES = [("stgcn", "ntu", True, "main", None), ("stgcn", "ntu", True, "pool41", None), ("stgcn", "ntu", True, "main", "small"),
         ("stgcn", "ntu", False, "main", None), ("stgcn", "ntu", True, "main", "latency"), ("str", "ntu", False, "main", None),
         ("agcn", "kinetics", True, "main", None), ("stgcnmod", "ntu", True, "unpadded", None)]


def _make(model, graph, geometry, native_plan, setup, sizes, weights=None, seed=7):
    """One model per entry of ``sizes``, all with the same weights: ``weights`` (a state dict), else randomised here."""
    a = (pkg.ntu_graph() if graph == "ntu" else pkg.kinetics_graph()).A
    v = a.shape[-1]
    nets = [getattr(pkg, CLASSES[model])(a, (3, 300, v, 2), 60, pool_size=geometry.pool_size,
                                         pool_padding=geometry.pool_padding).eval() for _ in sizes]
    if weights is None:
        randomise_unit_(nets[0], seed, attn_scale=1 / v if model == "agcn" else 1.0)
    else:
        nets[0].load_state_dict(weights)
    for net in nets[1:]:
        net.load_state_dict(nets[0].state_dict())
    for net in nets:
        net.use_native_plan = native_plan
        if SETUPS[setup]:
            SETUPS[setup](net)
    return [net.to(DEV) for net in nets], v


def _sequences(t, n, v, seed):
    """(t, n, 3, v, 2): the frames of ``n`` logical streams, each its own."""
    return torch.rand((t, max(n, 1), 3, v, 2), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _history(seq, j, t):
    return seq[:t, j].permute(1, 0, 2, 3).unsqueeze(0).contiguous()            # (1, C, T, V, M)


def _prime(net, model):
    return net.prime_streams_as_steps if model == "agcn" else net.prime_streams


class Reference:
    """What every logical stream emits, by (stream id, emission index): layer-10 features (256, M * V) and logits (60,), on the
    CPU.  Built once per (model, graph, geometry, setup); read-only afterwards."""

    def __init__(self, model, graph, geometry, setup, session):
        schedule, _, primes = fx.SESSIONS[session]
        fresh, primed, oldest = fx.born(schedule, geometry, primes)
        plan = model != "str"                                                    # the engines agree bit for bit: one reference
        (ref, pref), v = _make(model, graph, geometry, plan, setup, (fresh, max(primed, 1)))
        self.v, self.mv, self.geometry, t_end = v, 2 * v, geometry, (oldest + 7) // 4 * 4
        self.fresh, self.primed = _sequences(t_end, fresh, v, 100), _sequences(t_end + 24, primed, v, 200)
        self.features, self.logits = {}, {}
        self.weights = {k: w.detach().cpu().clone() for k, w in ref.state_dict().items()}     # the sessions run on these
        ages = [0] * fresh
        for t in range(0, t_end, 4):
            self._record(ref, ref._cycle([self.fresh[t + f] for f in range(4)]), list(range(fresh)), ages)
            ages = [a + 4 for a in ages]
        if primed:
            other = _sequences(WARM, primed, v, 300)
            for t in range(0, WARM, 4):
                pref._cycle([other[t + f] for f in range(4)])
            ages = [fx.PRIME_T[j % 2] for j in range(primed)]
            for j, t in enumerate(ages):
                _prime(pref, model)(_history(self.primed, j, t), [j])
            for s in range(0, t_end - min(ages), 4):                             # the youngest reaches the greatest age too
                frames = [torch.stack([self.primed[a + f, j] for j, a in enumerate(ages)]) for f in range(4)]
                self._record(pref, pref._cycle(frames), [("p", j) for j in range(primed)], ages)
                ages = [a + 4 for a in ages]
            assert not pref._cohorts and pref.stream_ages().tolist() == ages

    def _record(self, net, result, ids, ages):
        """The emissions of one 4-frame cycle of a reference slab whose row i holds stream ids[i] at ages[i]."""
        slot, n_feat, logits = result
        g, out, start = self.geometry, net.layers["layer10"]._state.out, net._frames - 4
        d10 = g.cum_delays()[-1]
        emits = [fi for fi in range(start, start + 4) if fi >= d10 and (fi - d10) % g.stride == 0]
        assert len(emits) == n_feat
        feats = [out[(slot + j) % out.shape[0]].cpu() for j in range(n_feat)]
        logits = [x.cpu() for x in logits]
        for i, (sid, age) in enumerate(zip(ids, ages)):
            for j, fi in enumerate(emits):
                si = age + fi - start                                            # the stream's own index of the emitting frame
                if si < d10:
                    continue
                e, k = (si - d10) // g.stride, j - (n_feat - len(logits))         # the logits returned belong to the last emissions
                self.features[sid, e] = feats[j][:, i * self.mv:(i + 1) * self.mv]
                if k >= 0 and e >= g.first_logit():
                    self.logits[sid, e] = logits[k][i]

    def frame(self, sid, age):
        return self.primed[age, sid[1]] if isinstance(sid, tuple) else self.fresh[age, sid]


@pytest.fixture(scope="module")
def references():
    cache = {}

    def get(model, graph, geometry, setup, session):
        key = (model, graph, geometry, setup, session)
        if key not in cache:
            cache[key] = Reference(*key)
        return cache[key]
    return get


def _bytes(net):
    return [t.clone() for t in net._state_tensors()]


def _same(a, b):
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


class Session:
    def __init__(self, model, graph, native_plan, session, setup, ref):
        self.schedule, self.g, primes = fx.SESSIONS[session]
        self.model, self.ref, self.mv = model, ref, ref.mv
        self.ledger = fx.Ledger(self.g, primes)
        sizes = [n for n, _ in fx.SLABS.values()]
        nets, self.v = _make(model, graph, self.g, native_plan, setup, sizes + [1] * len(sizes), ref.weights)
        self.nets, self.twins = dict(zip(fx.SLABS, nets)), dict(zip(fx.SLABS, nets[len(sizes):]))
        for name, (_, max_cycle) in fx.SLABS.items():
            self.nets[name].set_max_cycle(max_cycle)
            self.twins[name].set_max_cycle(max_cycle)
        self.twin_frame = torch.rand((1, 3, self.v, 2), generator=torch.Generator().manual_seed(5)).to(DEV)
        self.records, self.compared, self.zero_checks, self.no_trace_checks = {}, 0, 0, 0
        for name, net in self.nets.items():                                      # bind: one peek at the first frame
            net._ensure_bound(self._frames(name, 1)[0])
            self.twins[name]._ensure_bound(self.twin_frame)

    def _frames(self, name, r):
        rows = self.ledger.slabs[name].rows
        return [torch.stack([self.ref.frame(sid, age + f) for sid, age in rows]) for f in range(r)]

    # ---- the events ----------------------------------------------------------------------------------------------------
    def _do(self, event, frames=None):
        kind, nets = event[0], self.nets
        if kind == "cycle":
            frames = frames or self._frames(event[1], event[2])
            result = nets[event[1]]._cycle(frames)
            self.twins[event[1]]._cycle([self.twin_frame] * event[2])
            return result
        if kind == "peek":
            return nets[event[1]].forward_step(self._frames(event[1], 1)[0], update_state=False)
        if kind == "reset":
            return nets[event[1]].reset_streams(event[2])
        if kind == "take":
            self.records[event[3]] = nets[event[1]].export_streams(event[2])
        elif kind == "put":
            nets[event[2]].import_streams(self.records[event[1]], event[3])
        elif kind == "move":
            nets[event[3]].import_streams(nets[event[1]].export_streams(event[2]), event[4])
        elif kind == "prime":
            n = len(event[2])                                                    # the ledger has already named the new streams
            streams = [0] * n if self._refusing else range(self.ledger.primed - n, self.ledger.primed)
            x = torch.cat([_history(self.ref.primed, j, event[3]) for j in streams])
            _prime(nets[event[1]], self.model)(x, event[2])
        elif kind == "resize":
            nets[event[1]].resize_streams(event[2], event[3])

    _refusing = False

    def _refused(self, event):
        before = {name: (_bytes(net), net._position()) for name, net in self.nets.items()}
        self._refusing = True
        try:
            with pytest.raises(getattr(builtins, event[2])):
                self._do(event[1])
        finally:
            self._refusing = False
        torch.cuda.synchronize()
        for name, net in self.nets.items():
            tensors, position = before[name]
            assert net._position() == position, (event, name, "position")
            assert all(_same(a, b) for a, b in zip(net._state_tensors(), tensors)), (event, name, "state bytes")
        self.no_trace_checks += 1

    def _peek(self, event):
        """Every byte but the slots the next one-frame step rewrites and the head's output row; the position."""
        name = event[1]
        net = self.nets[name]
        before, position, rings = _bytes(net), net._position(), net._rings()
        c0, c1 = self.g.counters_at(net._frames), self.g.counters_at(net._frames + 1)
        self._do(event)
        torch.cuda.synchronize()
        assert net._position() == position, (event, "position")
        after = net._state_tensors()
        for i, (a, b) in enumerate(zip(after, before)):
            if i < len(rings):
                depth, ring = a.shape[0], rings[i]
                written = {c % depth for c in range(c0[ring.counter], c1[ring.counter])}
                keep = [s for s in range(depth) if s not in written]
                assert _same(a[keep], b[keep]), (event, ring.name)
            elif a is not net._pooled:
                assert _same(a, b), (event, "stage state", i)
        self.no_trace_checks += 1

    # ---- what holds after every event --------------------------------------------------------------------------------------
    def _bookkeeping(self, event):
        for name, net in self.nets.items():
            where = (event, name)
            assert net._n == self.ledger.slabs[name].n, where
            assert net.stream_ages().tolist() == self.ledger.ages(name), where
            assert net.streams_ready().tolist() == self.ledger.ready(name), where
            assert {at: sorted(m) for at, (m, _) in net._cohorts.items()} == self.ledger.cohorts(name), where
            for at, (members, dev) in net._cohorts.items():
                assert dev.cpu().tolist() == members, (where, "the device copy of a cohort's indices")
            assert net._counters()[:3] == self.twins[name]._counters()[:3], where
            assert net._counters() == self.twins[name]._counters() == self.ledger.counters(name), where

    def _emissions(self, event, cycle, result):
        net = self.nets[cycle.slab]
        slot, n_feat, logits = result
        assert (n_feat, len(logits)) == (cycle.n_feat, cycle.n_logits), event
        out = net.layers["layer10"]._state.out
        feats = [out[(slot + j) % out.shape[0]].cpu() for j in range(n_feat)]
        logits = [x.cpu() for x in logits]
        for row, j, sid, e in cycle.features:
            assert torch.equal(feats[j][:, row * self.mv:(row + 1) * self.mv], self.ref.features[sid, e]), (event, row, sid, e, "features")
            self.compared += 1
        for row, k, sid, e in cycle.logits:
            assert torch.equal(logits[k][row], self.ref.logits[sid, e]), (event, row, sid, e, "logits")
            self.compared += 1

    def _warming_rows_are_zero(self, event, cycle):
        """The claim of the scrub: in the slots this cycle wrote, a warming row is +0 in every ring not live yet at its age."""
        net = self.nets[cycle.slab]
        before, after = self.g.counters_at(net._frames - cycle.r), net._counters()
        rings = {ring.name: ring for ring in net._rings()}
        checked = []
        for row, (age, names) in cycle.dead.items():
            for name in names:
                ring = rings[name]
                depth = ring.tensor.shape[0]
                slots = sorted({c % depth for c in range(before[ring.counter], after[ring.counter])})
                if not slots:
                    continue
                part = ring.tensor[slots][:, row] if ring.kind == pkg.native.SCRUB_POOL_RING else \
                    ring.tensor[slots][:, :, row * ring.seg:(row + 1) * ring.seg]
                checked.append(((row, age, name, slots), torch.count_nonzero(part.contiguous().view(torch.int32))))
        if checked:
            counts = torch.stack([c for _, c in checked]).cpu().tolist()
            bad = [what for (what, _), c in zip(checked, counts) if c]
            assert not bad, (event, "not +0 (row, age, ring, slots)", bad[:4])
            self.zero_checks += len(checked)

    def run(self):
        for event in self.schedule:
            if event[0] == "refused":
                outcome = self.ledger.apply(event)
                self._refused(event)
            elif event[0] == "peek":
                outcome = self.ledger.apply(event)
                self._peek(event)
            else:
                frames = self._frames(event[1], event[2]) if event[0] == "cycle" else None      # at the ages before the cycle
                outcome = self.ledger.apply(event)
                result = self._do(event, frames)
                if isinstance(outcome, fx.Cycle):
                    self._emissions(event, outcome, result)
                    self._warming_rows_are_zero(event, outcome)
            self._bookkeeping(event)
        return self


@pytest.mark.parametrize("model,graph,native_plan,session,setup", CASES,
                         ids=[f"{m}-{g}-{'plan' if p else 'python'}-{s}{'-' + u if u else ''}" for m, g, p, s, u in CASES])
def test_a_stream_depends_on_its_own_frames_and_age_alone(model, graph, native_plan, session, setup, references):
    schedule, geometry, primes = fx.SESSIONS[session]
    ref = references(model, graph, geometry, setup, session)
    run = Session(model, graph, native_plan, session, setup, ref).run()
    _, total, _ = fx.comparisons(schedule, geometry, primes)
    print(f"session {session}: {run.compared} tensors compared (derived on the host: {total}), {run.zero_checks} ring segments "
          f"checked for +0, {run.no_trace_checks} events checked for no trace")
    assert run.compared == total == sum(run.ledger.compared.values())
    assert run.zero_checks > 0 and run.no_trace_checks > 0
