"""Per-stream reset of a ``CoStGcn`` slab: one stream starts over while the others run on ("Per-stream reset").  Zeroing the stream's
slice of every ring is not enough: in a running slab every launch emits for every stream, so a block whose window is
still filling pushes ReLU(bias + partial window) into the rings below it, where a fresh model pushes nothing.  With
D(L) = cumulative delay through block L in input frames, block L of a stream of age a (frames since its reset) is
live -- would run in a fresh model -- once a >= D(L-1), and emits once a >= D(L).  Every D(L) is a multiple of the
total stride, so a stream reset at a multiple of it and stepped in cycles that do not cross one has every block
wholly live or wholly not in each cycle: after the cycle's launches, what the not-yet-live blocks wrote for the
stream is zeroed again (csk_co_scrub_streams_f32) and its state is a fresh model's.  The step kernels do not change."""
import ctypes

import torch

from . import native
from .co_migrate import _distinct_in_range, _index_list
from .co_rings import scrub_job


class StreamReset:
    """Base class of ``CoStGcn``; its state is ``_reset_at`` and ``_cohorts`` (``_forget_resets``), part of the stepping position."""

    _scrub_warming = True   # private test switch: False leaves the per-cycle scrub out (the naive zero-only reset)

    def _forget_resets(self):
        """Ages count from the clean state: no stream was reset, nothing warms."""
        self._reset_at = [0] * (self._n or 0)     # input frame count at which each stream last started over
        self._cohorts = {}                        # reset frame -> (stream indices, device int32 copy), while they warm

    def _cum_delays(self):
        """[D(0) .. D(10)]: D(L) = D(L-1) + delay_L * (cumulative stride in front of block L), from the blocks."""
        d, cum, out = 0, 1, [0]
        for blk in self._blocks:
            d += blk.delay * cum
            cum *= blk.stride
            out.append(d)
        return out

    def _ready_age(self):
        """Frames after which a fresh model has returned its first logits: layer 10 emits at frame indices D(10) + j * stride
        and the pooling window emits from its (pool_size - pool_padding)-th entry on."""
        return self._cum_delays()[10] + self.stride * max(0, self.pool_size - self.pool_padding - 1) + 1

    def _require_bound(self, what):
        if self._n is None:
            raise RuntimeError(f"{what}: no state slab is bound yet (step once, or after set_max_cycle / set_latency_mode step again)")

    def stream_ages(self):
        """(N,) int64 CPU tensor: frames each stream has received since its reset (``reset_streams``), since
        ``clean_state()`` / the binding of the slab for streams never reset.  Host-side state, no GPU work."""
        self._require_bound("stream_ages")
        return torch.tensor([self._frames - r for r in self._reset_at], dtype=torch.int64)

    def streams_ready(self):
        """(N,) bool CPU tensor: True where a fresh model fed the stream's frames since its reset would already have returned
        logits.  ``forward_step`` / ``forward_cycle`` return logits for all N streams; this mask says which rows mean
        something."""
        return self.stream_ages() >= self._ready_age()

    def _warming(self):
        return bool(self._cohorts)

    def _check_reset(self, indices):
        """Everything ``reset_streams`` refuses, checked on the host before anything is launched; returns the index list."""
        idx = _index_list("reset_streams", indices)                # the two halves of ``_check_indices``, the slab's state between
        self._require_bound("reset_streams")
        if self._flushed:
            raise RuntimeError("the state was flushed by forward_steps(pad_end=True); call clean_state() instead")
        _distinct_in_range(idx, self._n)
        if self._frames % self.stride:
            raise RuntimeError(f"streams can be reset when the frame count is a multiple of {self.stride} (it is {self._frames}): "
                               "the stride phase of the strided blocks must match a fresh model's")
        return idx

    def _device_indices(self, idx):
        host = torch.tensor(idx, dtype=torch.int32).pin_memory()
        return host.to(self._xin0.device, non_blocking=True)       # stream-ordered copy from pinned memory: no host sync

    def _scrub(self, jobs, dev_idx, count):
        if not jobs:
            return
        if len(jobs) > native.SCRUB_MAX_JOBS:
            raise RuntimeError(f"{len(jobs)} rings in one scrub launch (limit {native.SCRUB_MAX_JOBS})")
        arr = (native.ScrubJob * len(jobs))(*jobs)
        rc = native.lib().csk_co_scrub_streams_f32(ctypes.byref(arr), len(jobs), native.ptr(dev_idx), count, self._n,
                                                   native.stream_of(self._xin0))
        native.check(rc, "csk_co_scrub_streams_f32")

    def _reset_jobs(self):
        """The job list of a full reset: every slot of every ring of the inventory (``_rings``), then what the input pre-passes
        with state clear (the streams' next frame is a first frame).  Built, not launched."""
        jobs = [scrub_job(ring, 0, ring.tensor.shape[0]) for ring in self._rings()]
        return jobs + [job for stage in self._record_stages for job in stage.reset_jobs()]

    def _scrub_cycle_jobs(self, ages, before, after):
        """Per cohort age in ``ages``, the job list of the scrub behind a cycle that moved the counters from ``before`` to
        ``after``: of the rings the cycle wrote (one job each, the slots it wrote), those that are not live yet for a stream of
        that age -- age < D(L) of the level L that feeds the ring."""
        d = self._cum_delays()
        wrote = [(d[ring.level], scrub_job(ring, before[ring.counter], after[ring.counter] - before[ring.counter]))
                 for ring in self._rings() if after[ring.counter] > before[ring.counter]]
        return [[job for live, job in wrote if age < live] for age in ages]

    def _leave_cohorts(self, idx):
        """The streams ``idx`` stop warming with whatever cohort they were in (reset again, or replaced by an imported stream)."""
        gone = set(idx)
        for at, (members, _) in list(self._cohorts.items()):
            left = [i for i in members if i not in gone]
            if len(left) != len(members):
                if left:
                    self._cohorts[at] = (left, self._device_indices(left))
                else:
                    del self._cohorts[at]

    def reset_streams(self, indices):
        """Start the streams ``indices`` (sequence of distinct ints in [0, N)) over while the others run on: from the next
        frame their features and predictions are bit for bit those of a fresh model fed their frames alone, available
        ``streams_ready()`` says when.  Allowed when the frame count is a multiple of the total stride (4); while a reset
        stream warms up, cycles must not cross a multiple of it (1-, 2-, 4-frame cycles aligned to it; ``_cycle``).  One
        launch on the current stream (every slot of every ring and of the pooling window, for these streams), no host sync."""
        idx = self._check_reset(indices)
        if not idx:
            return
        dev = self._device_indices(idx)
        self._scrub(self._reset_jobs(), dev, len(idx))
        self._leave_cohorts(idx)                                   # a stream reset again leaves its earlier cohort
        at = self._frames
        if at in self._cohorts:                                    # a second call at the same frame: one cohort
            idx = self._cohorts[at][0] + idx
            dev = self._device_indices(idx)
        self._cohorts[at] = (idx, dev)
        for i in idx:
            self._reset_at[i] = at

    def _check_cycle_while_warming(self, r):
        if self._cohorts and self._frames % self.stride + r > self.stride:
            raise ValueError(f"a cycle of {r} frames at frame {self._frames} crosses a multiple of {self.stride} while reset streams "
                             f"are warming up (streams_ready()): step in cycles of 1, 2 or {self.stride} frames aligned to it")

    def _scrub_cycle(self, before):
        """After the launches of a cycle that moved the counters from ``before`` to their present value: per cohort, zero what
        the blocks that are not live yet for it wrote -- block L's y slots while age < D(L-1), its output slots while
        age < D(L), the pooling-window slots while age < D(10) -- one launch per cohort; cohorts that are ready leave."""
        after, ready, cohorts = self._counters(), self._ready_age(), list(self._cohorts.items())
        jobs = self._scrub_cycle_jobs([before[0] - at for at, _ in cohorts], before, after)
        for (at, (idx, dev)), cohort_jobs in zip(cohorts, jobs):
            if self._scrub_warming:
                self._scrub(cohort_jobs, dev, len(idx))    # nothing left to scrub (age >= D(10)): no launch
            if after[0] - at >= ready:
                del self._cohorts[at]
