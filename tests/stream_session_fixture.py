"""Sessions of a continual stream slab in service ("Slab in service"): a schedule language, a ledger and the fixed
schedules.  Host only, pure Python: nothing here imports the package or needs a GPU.

A session is a list of events over the slabs "A" (5 streams, default ring depths) and "B" (3 streams, set_max_cycle(4): other
depths in every ring, other slot positions at the same frame count); each slab has its own frame count.  Events are tuples:

    ("cycle", slab, r)                            forward_cycle of r frames
    ("peek", slab)                                forward_step(update_state=False)
    ("reset", slab, rows)                         reset_streams
    ("move", src, src_rows, dst, dst_rows)        export_streams, then import_streams
    ("take", slab, rows, tag) / ("put", tag, slab, rows)    the two halves of a move, any number of events apart
    ("prime", slab, rows, T)                      prime_streams of the streams' first T frames
    ("resize", slab, n, keep)                     resize_streams
    ("refused", event, exception name)            the event must raise and leave no trace

The ``Ledger`` maps every (slab, row) to (logical stream id, age) and advances with each event by the documented rules alone:
D(L) from the block delays and strides, ready age = D(10) + stride * max(0, pool_size - pool_padding - 1) + 1, a fresh or reset
row takes a new logical id at age 0, an import or a prime takes the record's id and age, a resize keeps (id, age) of the kept
rows and starts fresh ids behind them.  It, not the model, decides which row is compared with which reference emission, which
rows are exactly zero in which rings, which events are refused and what stream_ages() / streams_ready() / the cohorts are."""
from collections import namedtuple

SLABS = {"A": (5, 8), "B": (3, 4)}          # name -> (streams, max_cycle)
PRIME_T = (96, 76)                          # primed logical stream j has a history of PRIME_T[j % 2] frames


class Geometry(namedtuple("Geometry", "block_delay strides pool_size pool_padding")):
    """What the ledger knows of a model: the per-block delay and strides of its ten-block table and the pooling window."""

    @property
    def stride(self):
        s = 1
        for x in self.strides:
            s *= x
        return s

    def cum_delays(self):
        """[D(0) .. D(10)]: D(L) = D(L-1) + delay * (stride in front of block L)."""
        d, cum, out = 0, 1, [0]
        for s in self.strides:
            d += self.block_delay * cum
            cum *= s
            out.append(d)
        return out

    def ready_age(self):
        return self.cum_delays()[-1] + self.stride * max(0, self.pool_size - self.pool_padding - 1) + 1

    def emissions_at(self, age):
        """Layer-10 emissions of a stream (or slab) that has received ``age`` frames."""
        return max(0, -(-(age - self.cum_delays()[-1]) // self.stride))

    def first_logit(self):
        """Index of the first emission with which the pooling window answers."""
        return max(0, self.pool_size - self.pool_padding - 1)

    def counters_at(self, frames):
        """{frames, features, (received, emitted) per block} of a slab that was only stepped: block i emits at its steps
        s >= delay with (s - delay) % stride == 0."""
        r, per_block = frames, []
        for s in self.strides:
            e = 0 if r <= self.block_delay else (r - 1 - self.block_delay) // s + 1
            per_block += [r, e]
            r = e
        return [frames, r] + per_block

    def rings(self, max_cycle):
        """[(name, producer level, counter index, depth)] in slab order: depths from the frames one launch can bring."""
        recv, emits, cum = [], [], 1
        for s in self.strides:
            recv.append(max(1, max_cycle // cum))
            cum *= s
            emits.append(max(1, max_cycle // cum))
        out = [("xin0", 0, 0, 4 + max_cycle)]
        for i in range(10):
            out.append((f"y{i}", i, 2 + 2 * i, 8 + recv[i]))
            out.append((f"out{i}", i + 1, 3 + 2 * i, 4 + recv[i + 1] if i < 9 else max(4, emits[i])))
        return out + [("pool", 10, 1, self.pool_size)]

    def dead_rings(self, age):
        """Names of the rings that a fresh model of this age has not written yet: the level that feeds them is not live."""
        d = self.cum_delays()
        return [name for name, level, _, _ in self.rings(8) if age < d[level]]


PADDED = Geometry(4, (1, 1, 1, 1, 2, 1, 1, 2, 1, 1), 2, 0)
PADDED_POOL41 = PADDED._replace(pool_size=4, pool_padding=1)
UNPADDED = Geometry(8, (1,) * 10, 2, 0)


class Refused(Exception):
    """The ledger's verdict on an event: the exception type the model must raise, and which documented rule it is."""

    def __init__(self, exc, rule):
        super().__init__(f"{exc}: {rule}")
        self.exc, self.rule = exc, rule


class _Slab:
    def __init__(self, n, max_cycle):
        self.n, self.max_cycle, self.frames = n, max_cycle, 0
        self.rows = []              # [logical id, age] per row
        self.cohorts = {}           # reset frame -> rows, while they warm
        self.last_op = {}           # row -> (op, frame, detail): what last changed the row without stepping it


Cycle = namedtuple("Cycle", "slab r features logits dead n_feat n_logits")
# features: [(row, j, stream id, emission)] -- emission j of the cycle in that row is that stream's emission of that index;
# logits: [(row, k, stream id, emission)] -- row of the k-th returned logits; dead: {row: (age, ring names that must be +0
# in the slots the cycle wrote)}; n_feat / n_logits: what the slab itself emits and returns in the cycle.


class Ledger:
    def __init__(self, geometry, primes=True):
        self.g, self.primes = geometry, primes
        self.slabs = {name: _Slab(n, mc) for name, (n, mc) in SLABS.items()}
        self.fresh = self.primed = 0
        self.records = {}           # tag -> (source slab, its frame, [(id, age)], [source rows])
        self.seen = set()           # coverage flags
        self.compared = {}          # stream id -> tensors compared so far
        self.logit_rows = [0, 0]    # returned logits rows: compared, all
        self.moves = {}             # stream id -> imports of an exported record
        self.two_cohorts = {name: [] for name in SLABS}     # cycle lengths stepped while two cohorts of different ages warm
        self.marks = {name: [] for name in SLABS}           # frame count at every non-cycle event that was not refused
        for slab in self.slabs.values():
            slab.rows = [[self._new_id(), 0] for _ in range(slab.n)]

    def _new_id(self):
        self.fresh += 1
        return self.fresh - 1

    # ---- what the model must report ------------------------------------------------------------------------------
    def ages(self, name):
        return [age for _, age in self.slabs[name].rows]

    def ready(self, name):
        return [age >= self.g.ready_age() for age in self.ages(name)]

    def cohorts(self, name):
        return {at: sorted(rows) for at, rows in self.slabs[name].cohorts.items()}

    def counters(self, name):
        return self.g.counters_at(self.slabs[name].frames)

    # ---- which events are refused ----------------------------------------------------------------------------------
    def _on_grid(self, slab, what):
        if slab.frames % self.g.stride:
            raise Refused("RuntimeError", f"{what}-off-grid")

    def _check_export(self, slab, rows):
        self._on_grid(slab, "export")
        if any(slab.rows[i][1] < self.g.ready_age() for i in rows):
            primed = any(isinstance(slab.rows[i][0], tuple) for i in rows)
            raise Refused("RuntimeError", "export-primed-not-ready" if primed else "export-warming")

    def _check_import(self, slab, ages):
        self._on_grid(slab, "import")
        if slab.frames < self.g.ready_age():
            raise Refused("RuntimeError", "import-young-slab")
        have = min(self.g.emissions_at(slab.frames), self.g.pool_size)
        if max(min(self.g.pool_size, self.g.emissions_at(a)) for a in ages) > have:
            raise Refused("RuntimeError", "import-pool-window")

    def check(self, event):
        """Raises ``Refused`` where the documented rules refuse the event; otherwise returns."""
        kind, slabs = event[0], self.slabs
        if kind == "cycle":
            slab, r = slabs[event[1]], event[2]
            if r > slab.max_cycle:
                raise Refused("ValueError", "cycle-longer-than-max-cycle")
            if slab.cohorts and slab.frames % self.g.stride + r > self.g.stride:
                raise Refused("ValueError", "cycle8-warming" if r == 8 else "cycle-crosses")
        elif kind == "reset":
            self._on_grid(slabs[event[1]], "reset")
        elif kind == "take":
            self._check_export(slabs[event[1]], event[2])
        elif kind == "put":
            self._check_import(slabs[event[2]], [age for _, age in self.records[event[1]][2]])
        elif kind == "move":
            self._check_export(slabs[event[1]], event[2])
            self._check_import(slabs[event[3]], [slabs[event[1]].rows[i][1] for i in event[2]])
        elif kind == "prime":
            if not self.primes:
                raise Refused("NotImplementedError", "prime-not-built")
            if event[3] % self.g.stride or event[3] < self.g.cum_delays()[-1]:
                raise Refused("ValueError", "prime-history")
            self._check_import(slabs[event[1]], [event[3]])
        elif kind == "resize":
            self._on_grid(slabs[event[1]], "resize")

    # ---- the events ----------------------------------------------------------------------------------------------------
    def apply(self, event):
        """Advance by one event.  Returns a ``Cycle`` for a cycle, the new logical ids for reset / prime / resize, the
        ``Refused`` for a refused event, else None."""
        kind = event[0]
        if kind == "refused":
            try:
                self.check(event[1])
            except Refused as refused:
                assert refused.exc == event[2], (event, refused.exc)
                self.seen.add("refused:" + refused.rule)
                return refused
            raise AssertionError(f"the ledger does not refuse {event[1]}")
        self.check(event)
        if kind not in ("cycle", "peek", "take"):
            name = event[3] if kind == "move" else event[2] if kind == "put" else event[1]
            self.marks[name].append(self.slabs[name].frames)
        return getattr(self, "_" + kind)(*event[1:])

    def _peek(self, name):
        return None

    def _leave(self, slab, rows, by_import):
        for at, members in list(slab.cohorts.items()):
            left = [i for i in members if i not in rows]
            if len(left) != len(members):
                slab.cohorts[at] = left
                if not left:
                    del slab.cohorts[at]
                    if by_import:
                        self.seen.add("cohort:emptied-by-import")

    def _pair(self, slab, row, op):
        """Record the ordered pair (last operation on the row, this one) when at most 8 frames lie between them."""
        last = slab.last_op.get(row)
        if last and slab.frames - last[1] <= 8:
            self.seen.add(f"pair:{last[0]}>{op}")
        return last

    def _reset(self, name, rows):
        slab, at, ids = self.slabs[name], self.slabs[name].frames, []
        for i in rows:
            last = self._pair(slab, i, "reset")
            older = [a for a, members in slab.cohorts.items() if i in members and a != at]
            if older and last and last[0] == "reset" and at - last[1] <= 8 and set(slab.cohorts[older[0]]) - set(rows):
                self.seen.add("pair:reset>reset:cohort-survives")
        self._leave(slab, rows, False)
        if at in slab.cohorts:
            self.seen.add("cohort:two-resets-one-frame")
        slab.cohorts[at] = slab.cohorts.get(at, []) + list(rows)
        for i in rows:
            slab.rows[i] = [self._new_id(), 0]
            slab.last_op[i] = ("reset", at, None)
            ids.append(slab.rows[i][0])
        return ids

    def _take(self, name, rows, tag):
        slab = self.slabs[name]
        self.records[tag] = (name, slab.frames, [tuple(slab.rows[i]) for i in rows], list(rows))

    def _put(self, tag, name, rows, op="import"):
        slab = self.slabs[name]
        src, src_frames, streams, src_rows = self.records[tag]
        for i, (sid, age), j in zip(rows, streams, src_rows):
            warming = any(i in members for members in slab.cohorts.values())
            self._pair(slab, i, op)
            slab.rows[i] = [sid, age]
            slab.last_op[i] = (op, slab.frames, age > slab.frames)
            if op == "import":
                self.moves[sid] = self.moves.get(sid, 0) + 1
                self.seen.add(f"move:{src}>{name}")
                if src == name and slab.frames >= src_frames + 8 and i != j:
                    self.seen.add("move:same-slab-later")
                if self.moves[sid] >= 2:
                    self.seen.add("move:twice")
                if warming:
                    self.seen.add("import:into-warming")
            elif warming:
                self.seen.add("prime:into-warming")
        self._leave(slab, rows, True)

    def _move(self, src, src_rows, dst, dst_rows):
        self._take(src, src_rows, "_move")
        self._put("_move", dst, dst_rows)

    def _prime(self, name, rows, t):
        assert all(PRIME_T[(self.primed + k) % 2] == t for k in range(len(rows))), "primed stream j has PRIME_T[j % 2] frames"
        ids = [("p", self.primed + k) for k in range(len(rows))]
        self.primed += len(rows)
        self.records["_prime"] = (None, None, [(sid, t) for sid in ids], [None] * len(rows))
        self._put("_prime", name, rows, op="prime")
        self.seen.add(f"prime:T{t}-{'ready' if t >= self.g.ready_age() else 'not-ready'}")
        return ids

    def _resize(self, name, n, keep):
        slab, at = self.slabs[name], self.slabs[name].frames
        kinds = set()
        for i in keep:
            last = self._pair(slab, i, "resize")
            if any(i in members for members in slab.cohorts.values()):
                kinds.add("warming")
            if last and at - last[1] <= 8:
                kinds.add({"import": "imported-negative" if last[2] else "imported", "prime": "primed"}.get(last[0], last[0]))
        if {"warming", "imported-negative", "primed"} <= kinds and list(keep) != sorted(keep):
            self.seen.add("resize:warming+imported-negative+primed+permuted")
        new_of = {old: j for j, old in enumerate(keep)}
        slab.cohorts = {a: [new_of[i] for i in members if i in new_of] for a, members in slab.cohorts.items()}
        slab.cohorts = {a: members for a, members in slab.cohorts.items() if members}
        fresh = list(range(len(keep), n))
        if fresh:
            slab.cohorts[at] = slab.cohorts.get(at, []) + fresh
        slab.rows = [slab.rows[i] for i in keep] + [[self._new_id(), 0] for _ in fresh]
        slab.last_op = {new_of[i]: op for i, op in slab.last_op.items() if i in new_of}
        slab.last_op.update({j: ("reset", at, None) for j in fresh})
        slab.n = n
        return [slab.rows[j][0] for j in fresh]

    def _cycle(self, name, r):
        slab, g = self.slabs[name], self.g
        f, d10 = slab.frames, g.cum_delays()[-1]
        emits = [fi for fi in range(f, f + r) if fi >= d10 and (fi - d10) % g.stride == 0]
        answered = [j for j in range(len(emits)) if g.emissions_at(f) + j >= g.first_logit()]
        features, logits = [], []
        for row, (sid, age) in enumerate(slab.rows):
            for j, fi in enumerate(emits):
                si = age + fi - f                       # the stream's own frame index of the slab's emitting frame
                if si < d10:
                    continue
                assert (si - d10) % g.stride == 0, "a stream off the stride phase of its slab"
                features.append((row, j, sid, (si - d10) // g.stride))
                if j in answered and (si - d10) // g.stride >= g.first_logit():
                    logits.append((row, answered.index(j), sid, (si - d10) // g.stride))
        dead = {}
        for at, members in slab.cohorts.items():
            for row in members:
                assert slab.rows[row][1] == f - at and at % g.stride == 0
                dead[row] = (f - at, g.dead_rings(f - at))
        if len(slab.cohorts) >= 2:
            self.two_cohorts[name].append(r)
            seq = self.two_cohorts[name]
            if sum(seq) >= 40 and {1, 2, 4} <= set(seq) and seq != sorted(seq) and seq != sorted(seq, reverse=True):
                self.seen.add("cohort:two-ages-40-frames-mixed-1-2-4")
        if r == 8 and name == "A":
            self.seen.add("cycle8:after-cohorts" if "_reset_seen" in self.seen and not slab.cohorts else "cycle8:before-reset")
        if slab.cohorts:
            self.seen.add("_reset_seen")
        for row in slab.rows:
            row[1] += r
        slab.frames += r
        slab.cohorts = {at: m for at, m in slab.cohorts.items() if slab.frames - at < g.ready_age()}
        for _, _, sid, _ in features + logits:
            self.compared[sid] = self.compared.get(sid, 0) + 1
        self.logit_rows[0] += len(logits)
        self.logit_rows[1] += len(answered) * slab.n
        return Cycle(name, r, features, logits, dead, len(emits), len(answered))


def play(schedule, geometry, primes=True):
    """The ledger after the whole schedule, and what every event returned."""
    ledger = Ledger(geometry, primes)
    return ledger, [ledger.apply(event) for event in schedule]


def comparisons(schedule, geometry, primes=True):
    """(tensors compared per logical stream, in total, share of the returned logits rows that are skipped)."""
    ledger, _ = play(schedule, geometry, primes)
    return dict(ledger.compared), sum(ledger.compared.values()), 1 - ledger.logit_rows[0] / max(1, ledger.logit_rows[1])


def live_streams(schedule, geometry, primes=True):
    """Logical streams that ever reach the age at which layer 10 emits for them."""
    ledger, live = Ledger(geometry, primes), set()
    for event in schedule:
        ledger.apply(event)
        live |= {sid for slab in ledger.slabs.values() for sid, age in slab.rows if age > geometry.cum_delays()[-1]}
    return live


def born(schedule, geometry, primes=True):
    """(fresh logical streams, primed logical streams, greatest age any stream reaches) of a schedule."""
    ledger, oldest = Ledger(geometry, primes), 0
    for event in schedule:
        ledger.apply(event)
        oldest = max([oldest] + [age for slab in ledger.slabs.values() for _, age in slab.rows])
    return ledger.fresh, ledger.primed, oldest


# ---- the schedules --------------------------------------------------------------------------------------------------------
def _c(slab, *rs):
    return [("cycle", slab, r) for r in rs]


def _main_session():
    """Slabs A and B of the padded ten-block table (stride 4, D(10) = 76, ready at 81).  Frame counts in the comments."""
    s = _c("A", *[8] * 11) + _c("B", *[4] * 25)                                                # A 88, B 100: both ready
    s += [("peek", "A"), ("reset", "A", [1]), ("reset", "A", [3]), ("peek", "A")]              # two calls, one cohort {1, 3}
    s += [("refused", ("take", "A", [1], "x"), "RuntimeError"), ("refused", ("cycle", "A", 8), "ValueError")]
    s += _c("A", 4, 1, 1, 2)                                                                   # A 96
    s += [("take", "A", [4], "late")]                                                          # stream 4 of A, as of frame 96
    s += [("reset", "A", [3]), ("reset", "A", [0])]                # 3 leaves the cohort of 88, which keeps 1; cohort {3, 0} of 96
    s += _c("A", 2, 2, 1, 1, 1)                                                                # A 103: off the stride grid
    s += [("refused", ("cycle", "A", 2), "ValueError"), ("refused", ("reset", "A", [0]), "RuntimeError"),
          ("refused", ("take", "A", [2], "x"), "RuntimeError"), ("refused", ("move", "B", [0], "A", [2]), "RuntimeError")]
    s += _c("A", 1)                                                                            # A 104
    s += [("peek", "A"), ("move", "B", [1], "A", [3]), ("peek", "A")]                          # B -> A into a warming row
    s += [("put", "late", "A", [2])]                               # the record of frame 96 into another row of A at frame 104
    s += _c("A", 1, 2, 1, 4)                                                                   # A 112
    s += [("reset", "A", [3])]                                                                 # reset of an imported row
    s += _c("A", 4, 4)                                                                         # A 120
    s += [("prime", "A", [3], 96)]                                 # prime into a warming row: the cohort of 112 disappears
    s += _c("A", 2, 2, 4)                                                                      # A 128
    s += [("reset", "A", [3])]                                                                 # reset of a primed row
    s += _c("A", 4, 1, 1, 1, 1)                                                                # A 136
    s += [("prime", "A", [3], 76), ("refused", ("take", "A", [3], "x"), "RuntimeError")]       # live in every block, not ready
    s += _c("A", 4)
    s += [("refused", ("take", "A", [3], "x"), "RuntimeError")]                                # age 80
    s += _c("A", 4)                                                                            # A 144
    # slab B: a cohort of 100, a cohort of 104 and a prime; then the streams of A arrive
    s += [("reset", "B", [2])] + _c("B", 1, 2, 1)                                              # B 104
    s += [("reset", "B", [0]), ("prime", "B", [1], 96)] + _c("B", 4)                           # B 108
    s += [("move", "A", [2], "B", [2])]                            # A -> B, the second move of that stream, older than B: negative
    s += [("peek", "B"), ("resize", "B", 5, [2, 0, 1]), ("peek", "B")]                         # imported, warming, primed; 2 fresh
    s += [("move", "A", [3], "B", [4])]                                                        # the primed stream of age 84
    s += _c("B", 4) + [("reset", "B", [2])]                                                    # B 112: reset of a kept primed row
    s += _c("B", *[1, 2, 1, 4, 4, 2, 2] * 4) + [("reset", "B", [0])]                           # B 176: three cohorts warm, a fourth
    s += _c("B", *[1, 2, 1, 4, 4, 2, 2] * 5) + _c("B", *[4] * 4)                               # B 272: every cohort has left
    # slab A again
    s += _c("A", 2, 1, 1, 4)                                                                   # A 152
    s += [("resize", "A", 4, [4, 1, 0])]                           # an old stream, the cohorts of 88 and 96, one fresh row
    s += _c("A", 4, 1, 1, 2, 2, 2, 4) + [("reset", "A", [0])]                                  # A 168
    s += _c("A", *[4, 1, 1, 2, 2, 2, 4] * 5) + _c("A", 4)                                      # A 252: the cohort of 168 has left
    s += _c("A", 4, 8, 8)                                                                      # A 272
    return s


def _pool_session():
    """pool_size = 4, pool_padding = 1 (ready at 85): a slab that is ready counts three pooling entries at frame 88, a stream
    of age 96 brings four -- refused; one cycle later the same import succeeds."""
    s = _c("A", *[8] * 11) + _c("B", *[4] * 24)                                                # A 88, B 96
    s += [("refused", ("move", "B", [0], "A", [1]), "RuntimeError")]
    s += _c("A", 4)                                                                            # A 92
    s += [("peek", "A"), ("move", "B", [0], "A", [1]), ("peek", "A"), ("reset", "A", [2])]
    s += _c("A", 4, 2, 2, 1, 1, 1, 1)                                                          # A 104
    s += [("prime", "A", [3], 96), ("reset", "A", [4])]
    s += _c("A", *[4, 1, 2, 1] * 11) + _c("A", 4, 4, 4) + _c("A", *[8] * 2)                    # A 192 .. 220
    s += _c("B", *[4] * 2)
    return s


def _unpadded_session():
    """The '*' table: stride 1, D(10) = 80, ready at 82; while a cohort warms only one-frame cycles are aligned."""
    s = _c("A", *[8] * 11) + _c("B", *[4] * 23)                                                # A 88, B 92
    s += [("peek", "A"), ("reset", "A", [1]), ("reset", "A", [3]), ("peek", "A")]
    s += [("refused", ("cycle", "A", 2), "ValueError"), ("refused", ("take", "A", [1], "x"), "RuntimeError"),
          ("refused", ("prime", "A", [2], 96), "NotImplementedError")]
    s += _c("A", *[1] * 5)                                                                     # A 93
    s += [("reset", "A", [3]), ("move", "B", [1], "A", [1])]                                   # the cohort of 88 is emptied
    s += _c("A", *[1] * 3) + [("take", "A", [4], "late")] + _c("A", *[1] * 8)                  # A 104
    s += [("put", "late", "A", [2]), ("move", "A", [1], "B", [0]), ("resize", "A", 4, [3, 2, 0])]
    s += _c("A", *[1] * 82) + _c("A", *[4, 8, 2] * 7)                                          # A 186 .. 284
    s += _c("B", *[4, 2, 1, 1] * 12)                                                           # B 188
    return s


SESSIONS = {"main": (_main_session(), PADDED, True), "pool41": (_pool_session(), PADDED_POOL41, True),
            "unpadded": (_unpadded_session(), UNPADDED, False)}

REQUIRED = {
    "pair:reset>import", "pair:reset>prime", "pair:import>reset", "pair:prime>reset", "pair:reset>reset:cohort-survives",
    "import:into-warming", "prime:into-warming", "resize:warming+imported-negative+primed+permuted",
    "cohort:two-resets-one-frame", "cohort:two-ages-40-frames-mixed-1-2-4", "cohort:emptied-by-import",
    "cycle8:before-reset", "cycle8:after-cohorts",
    "move:A>B", "move:B>A", "move:same-slab-later", "move:twice",
    "prime:T96-ready", "prime:T76-not-ready", "refused:export-primed-not-ready",
    "refused:export-warming", "refused:cycle-crosses", "refused:cycle8-warming", "refused:reset-off-grid",
    "refused:export-off-grid", "refused:import-off-grid", "refused:import-pool-window",
    "peek:before-reset", "peek:after-reset", "peek:before-import", "peek:after-import", "peek:before-resize", "peek:after-resize",
}


def _peek_flags(schedule):
    def kind(event, slab):
        if event[0] in ("move", "put"):
            return "import" if (event[3] if event[0] == "move" else event[2]) == slab else None
        return event[0] if event[0] in ("reset", "resize") and event[1] == slab else None
    seen = set()
    for i, event in enumerate(schedule):
        if event[0] == "peek":
            if i and kind(schedule[i - 1], event[1]):
                seen.add("peek:after-" + kind(schedule[i - 1], event[1]))
            if i + 1 < len(schedule) and kind(schedule[i + 1], event[1]):
                seen.add("peek:before-" + kind(schedule[i + 1], event[1]))
    return seen


def session_facts(name):
    """(coverage flags of the session, per slab: wraps of the slowest ring between the first and the last non-cycle event,
    frames stepped after the last one)."""
    schedule, geometry, primes = SESSIONS[name]
    ledger, _ = play(schedule, geometry, primes)
    facts = {}
    for slab, marks in ledger.marks.items():
        if not marks:
            continue
        first, last = geometry.counters_at(marks[0]), geometry.counters_at(marks[-1])
        wraps = min((last[counter] - first[counter]) // depth for _, _, counter, depth in geometry.rings(SLABS[slab][1]))
        facts[slab] = (wraps, ledger.slabs[slab].frames - marks[-1])
    return {flag for flag in ledger.seen if not flag.startswith("_")} | _peek_flags(schedule), facts


def assert_sessions_covered():
    """Every coverage condition of DESIGN.md "Slab in service" is met by the schedules together; the wrap and the tail by each
    slab of each schedule that has a non-cycle event."""
    seen = set()
    for name, (schedule, geometry, _) in SESSIONS.items():
        flags, facts = session_facts(name)
        seen |= flags
        for slab, (wraps, tail) in facts.items():
            assert tail >= geometry.ready_age() + 4 * geometry.pool_size, (name, slab, "tail", tail)
            if name == "main":
                assert wraps >= 2, (name, slab, "every ring wraps twice between the first and the last operation", wraps)
    missing = REQUIRED - seen
    assert not missing, sorted(missing)
