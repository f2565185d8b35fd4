"""Moving live streams between ``CoStGcn`` slabs: ``export_streams`` gathers what a stream's future
launches can still read into a packed, position-independent record, ``import_streams`` scatters such records into the ring
positions of another slab (other stream count, other ring depths, other frame count), ``resize_streams`` re-binds a slab for
another stream count and carries the kept streams over.  One launch of csk_co_move_streams_f32 each way (csrc/stream_move.hip).

What a future launch can read of a ring is its "window" in the slab's one ring inventory (co_rings.py).  A frame s lives in slot s % depth of its
ring, so the window of a ring that has received ``count`` frames is the slots of frames count - window .. count - 1: the
export reads them at the source's (count, depth), the import writes them at the target's.  The summation order of no kernel
depends on the slab (``_pick_ksplit``, ``_use_split_step``), so the stream's results continue bit for bit."""
import ctypes

import torch

from . import native
from .co_rings import array_ring, move_job, ring_window, window_slots  # noqa: F401  (the window arithmetic is read from here too)


class StreamState:
    """The state of some streams outside any slab: ``packed`` (n, record_floats) float32, one record per stream (layout:
    DESIGN.md 3d); ``ages`` (n,) int64 CPU, frames each stream has received since its start; ``signature``, what the record
    means, as nested tuples of names, ints and strings.  Plain data only: ``torch.save`` / ``torch.load`` keep it whole."""

    def __init__(self, packed, ages, signature):
        self.packed, self.ages, self.signature = packed, ages, signature

    def __len__(self):
        return self.packed.shape[0]

    record_floats = property(lambda self: self.packed.shape[1])

    def to(self, device):
        return StreamState(self.packed.to(device), self.ages, self.signature)

    def cpu(self):
        return self.to("cpu")


torch.serialization.add_safe_globals([StreamState])     # torch.load(weights_only=True) rebuilds it: tensors, tuples, ints, strings


def _index_list(what, indices):
    """The stream indices ``what`` was handed as a list of ints; anything else is refused."""
    if isinstance(indices, torch.Tensor) or not isinstance(indices, (list, tuple, range)):
        raise ValueError(f"{what} takes a sequence of ints (a list, tuple or range), not a tensor: the indices are "
                         "host-side bookkeeping and reading a device tensor would cost a sync")
    idx = list(indices)
    if any(isinstance(i, bool) or not isinstance(i, int) for i in idx):
        raise ValueError(f"{what} takes ints, got {[type(i).__name__ for i in idx]}")
    return idx


def _distinct_in_range(idx, n):
    if len(set(idx)) != len(idx):
        raise ValueError(f"duplicate stream indices in {idx}")
    if n is not None and any(not 0 <= i < n for i in idx):
        raise ValueError(f"stream indices {idx} outside a slab of {n} streams")


def _check_indices(what, indices, n):
    """THE rule for stream indices: a list, tuple or range of distinct ints inside the slab (``n`` None: no slab yet).
    ``reset_streams`` makes the two halves around its own refusals (``StreamReset._check_reset``)."""
    idx = _index_list(what, indices)
    _distinct_in_range(idx, n)
    return idx


def first_difference(mine, theirs):
    """Name of the first signature field that differs, or None."""
    a, b = dict(mine), dict(theirs)
    for name, value in mine:
        if name not in b or b[name] != value:
            return name
    for name, _ in theirs:
        if name not in a:
            return name
    return None


class StreamMove:
    """Base class of ``CoStGcn``; it has no state of its own: ages and cohorts are ``StreamReset``'s, the counters the model's."""

    # ---- what a record holds ---------------------------------------------------------------------
    def move_signature(self):
        """What a record of this model means: every setting that decides its layout or the arithmetic that continues on
        it.  Weights are not part of it (the caller owns them)."""
        c, _, v, m = self.input_shape
        blks = self._blocks
        return (("graph_convs", tuple(type(b.gcn).__name__ for b in blks)),
                ("layers", tuple((b.in_channels, b.out_channels, b.stride, b.kernel_size, b.delay, b.kind) for b in blks)),
                ("input_cvm", (c, v, m)),
                ("pool_size", self.pool_size), ("pool_padding", self.pool_padding),
                *(entry for stage in self._record_stages for entry in stage.signature()),
                ("split_k", tuple((b._pick_ksplit(0), b._pick_gcn_ksplit(0)) for b in blks)),
                ("step_precision", tuple("bf16x3" if b._use_split_step() else "f32" for b in blks)))

    def _move_windows(self):
        """[(name, rows, seg, window)] in record order, from the blocks alone (no slab needed): the rings of the inventory
        that have a window (co_rings.py: ``_rings``), then the small per-stream states of the input pre-passes as arrays of
        32-bit words with a window of one (input_stage.py)."""
        return ([(ring.name, ring.rows, ring.seg, ring.window) for ring in self._record_rings()]
                + [entry for stage in self._record_stages for entry in stage.windows()])

    def record_floats(self):
        """32-bit words of one stream's record: the sum of the windows."""
        return sum(rows * seg * window for _, rows, seg, window in self._move_windows())

    def _move_jobs(self):
        """The job list of this slab at its present position: the windows above, each with its tensor, the slot of its
        newest frame (from the counter that owns the ring; a per-stream array is one slot that holds its one frame) and its
        offset in the record."""
        counters = self._counters()
        entries = [(ring, counters[ring.counter]) for ring in self._record_rings()]
        entries += [(array_ring(entry, tensor), 1) for stage in self._record_stages
                    for entry, (_, tensor) in zip(stage.windows(), stage.state())]
        jobs, offset = [], 0
        for ring, count in entries:
            jobs.append(move_job(ring, count, offset))
            offset += ring.rows * ring.seg * ring.window
        return jobs, offset

    def _move(self, packed, dev_idx, count, to_ring):
        jobs, record = self._move_jobs()
        if len(jobs) > native.MOVE_MAX_JOBS:
            raise RuntimeError(f"{len(jobs)} rings in one move launch (limit {native.MOVE_MAX_JOBS})")
        if packed.dim() != 2 or packed.shape[0] < count or packed.shape[1] != record or packed.dtype != torch.float32 or not packed.is_contiguous() or packed.device != self._xin0.device:
            raise RuntimeError(f"packed records must be contiguous float32 (n, {record}) on {self._xin0.device}, got "
                               f"{tuple(packed.shape)} {packed.dtype} on {packed.device}")
        arr = (native.MoveJob * len(jobs))(*jobs)
        rc = native.lib().csk_co_move_streams_f32(ctypes.byref(arr), len(jobs), native.ptr(packed), record, native.ptr(dev_idx), count,
                                                  self._n, int(to_ring), native.stream_of(self._xin0))
        native.check(rc, "csk_co_move_streams_f32")

    # ---- checks (host only, before anything launches) ---------------------------------------------
    def _check_position(self, what):
        self._require_bound(what)
        if self._flushed:
            raise RuntimeError(f"{what}: the state was flushed by forward_steps(pad_end=True); call clean_state() instead")
        if self._frames % self.stride:
            raise RuntimeError(f"{what}: streams can move when the frame count is a multiple of {self.stride} (it is {self._frames}): "
                               "the stride phase of the strided blocks must match on both sides")

    def _check_export(self, indices):
        idx = _check_indices("export_streams", indices, self._n)
        self._check_position("export_streams")
        ready = self._ready_age()
        young = [i for i in idx if self._frames - self._reset_at[i] < ready]
        if young:
            raise RuntimeError(f"export_streams: streams {young} are still warming up (age < {ready} frames): their state is not "
                               "complete yet; streams_ready() says which streams can move")
        return idx

    def _emissions_at(self, age):
        """Layer-10 emissions a stream of this age has produced."""
        return max(0, -(-(age - self._cum_delays()[10]) // self.stride))

    def _check_import(self, state, indices):
        idx = _check_indices("import_streams", indices, self._n)
        if not isinstance(state, StreamState):
            raise TypeError(f"import_streams takes a StreamState (export_streams), got {type(state).__name__}")
        self._check_position("import_streams")
        field = first_difference(self.move_signature(), state.signature)
        if field is not None:
            raise ValueError(f"import_streams: the streams were exported from a model that differs in {field!r}: "
                             f"{dict(state.signature).get(field)!r} there, {dict(self.move_signature()).get(field)!r} here")
        if len(idx) != len(state):
            raise ValueError(f"import_streams: {len(idx)} indices for {len(state)} records")
        if self._frames < self._ready_age():
            raise RuntimeError(f"import_streams: this slab has received {self._frames} frames; every block and the pooling window "
                               f"must be live (at least {self._ready_age()} frames): step it through its warm-up first (warm_up)")
        have = min(self._feats, self.pool_size)
        need = max([min(self.pool_size, self._emissions_at(int(a))) for a in state.ages.tolist()] + [0])
        if need > have:
            raise RuntimeError(f"import_streams: a stream brings {need} pooling-window entries, this slab's window counts {have} so "
                               "far (pool_padding > 0 and a young slab): step the slab until its window is that full")
        return idx

    # ---- public ----------------------------------------------------------------------------------
    def _export(self, idx):
        packed = torch.empty((len(idx), self.record_floats()), device=self._xin0.device, dtype=torch.float32)
        if idx:
            self._move(packed, self._device_indices(idx), len(idx), to_ring=False)
        ages = torch.tensor([self._frames - self._reset_at[i] for i in idx], dtype=torch.int64)
        return StreamState(packed, ages, self.move_signature())

    def export_streams(self, indices):
        """``StreamState`` of the streams ``indices`` (sequence of distinct ints in [0, N)): one packed record per stream, in
        that order, their ages and the signature of this model.  Read-only for the slab: no ring, counter or cohort changes.
        Allowed when the frame count is a multiple of the total stride, the slab is bound and not flushed, and every named
        stream is ready (``streams_ready()``).  One launch on the current stream, no host sync."""
        return self._export(self._check_export(indices))

    def import_streams(self, state, indices):
        """Write record j of ``state`` into stream ``indices[j]`` of this slab, at this slab's ring positions; from the next
        frame the stream continues bit for bit as it would have where it came from.  Its age travels with it
        (``stream_ages()``), it leaves any warming cohort it was in here; every other stream and every counter stay as they
        were.  The slab must be bound, not flushed, at a frame count that is a multiple of the total stride and READY: it has
        received at least ``_ready_age()`` frames, so that every block and the pooling window are live -- a fresh slab is
        stepped through its warm-up first (``warm_up``, or any frames).  The signatures must match (``ValueError`` names the
        first field that differs).  One launch on the current stream, no host sync beyond the pinned index copy."""
        idx = self._check_import(state, indices)
        if not idx:
            return
        self._move(state.packed, self._device_indices(idx), len(idx), to_ring=True)
        self._adopt(idx, state.ages.tolist())

    def _adopt(self, idx, ages):
        """Bookkeeping of an import: the streams ``idx`` now hold streams of these ages (``_reset_at`` may go negative) and
        warm no longer."""
        self._leave_cohorts(idx)
        for i, age in zip(idx, ages):
            self._reset_at[i] = self._frames - int(age)

    def resize_streams(self, n, keep):
        """Re-bind the slab for ``n`` streams AT ITS PRESENT POSITION (the counters stay, so its readiness carries over): new
        stream j continues old stream ``keep[j]`` -- ready or still warming, with its age and cohort -- and the new streams
        behind ``len(keep)`` start at the current frame as freshly reset streams (``reset_streams``' bookkeeping on a zeroed
        slab).  Allowed under ``reset_streams``' frame-count condition.  The kept streams go through a packed copy: during
        the call the old slab, the records and the new slab exist side by side.  The native plan is rebuilt for the new rings."""
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"resize_streams: n must be a positive int, got {n!r}")
        self._require_bound("resize_streams")
        keep = _check_indices("resize_streams", keep, self._n)
        if len(keep) > n:
            raise ValueError(f"resize_streams: {len(keep)} streams to keep do not fit a slab of {n}")
        self._check_position("resize_streams")
        state = self._export(keep)
        counters, device = self._counters(), self._xin0.device
        new_of = {old: j for j, old in enumerate(keep)}
        reset_at = [self._reset_at[old] for old in keep] + [self._frames] * (n - len(keep))
        cohorts = {at: [new_of[i] for i in members if i in new_of] for at, (members, _) in self._cohorts.items()}
        self._bind(n, device)                           # zeroed rings, a plan on the new pointers
        self._set_counters(counters)
        if keep:
            self._move(state.packed, self._device_indices(list(range(len(keep)))), len(keep), to_ring=True)
        fresh = list(range(len(keep), n))
        if fresh:
            cohorts[self._frames] = cohorts.get(self._frames, []) + fresh
        self._reset_at = reset_at
        self._cohorts = {at: (members, self._device_indices(members)) for at, members in cohorts.items() if members}
