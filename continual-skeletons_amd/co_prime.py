"""Priming streams of a ``CoStGcn`` slab from buffered history: ``prime_state`` computes the packed
record of 3d (``StreamState``, co_migrate.py) for streams that have received the T frames of a history tensor -- with ONE clip
pass over the history instead of T steps -- and ``prime_streams`` imports it through ``import_streams``.  The clip kernels
compute, for the same frames, the activations the steps compute (the project's clip-versus-steps parity); the record says
which of them are state; csk_co_prime_pack_f32 (csrc/stream_prime.hip) reads them off the clip tensors in one launch.

Which clip frames: with D(L) the cumulative delays of 3a and S(L) the cumulative stride through block L (S(0) = 1), a fresh
stream of age T has pushed e(L) = max(0, ceil((T - D(L)) / S(L))) frames out of block L (e(0) = T: the input), so the ring fed
by block L -- the post-GCN ring of block L + 1 and the output ring of block L behind it -- has received e(L) frames and the
pooling window e(10) entries.  Frame j of a ring is frame j of the clip tensor of the same name, a window of w takes frames
e - w .. e - 1, and an index below 0 is the zero state of a fresh model (``prime_table``).  No frame the clip's right padding
has touched is taken: DESIGN.md 3e has the induction."""
import ctypes

import torch

from . import co_rings, native
from .blocks import SpatioTemporalBlock
from .co_migrate import StreamState


class StreamPrime:
    """Base class of ``CoStGcn``; it has no state of its own."""

    # Bytes of clip intermediates one launch group may hold: the streams of a call are primed in chunks that stay below it
    # (at least one stream per chunk).  ``prime_stream_bytes`` is what one stream needs.
    prime_budget_bytes = 1 << 30

    # ---- which clip frames are state (host only) ---------------------------------------------------
    def _cum_strides(self):
        """[S(0) .. S(10)]: S(L) = the product of the strides of blocks 1 .. L."""
        out = [1]
        for blk in self._blocks:
            out.append(out[-1] * blk.stride)
        return out

    def prime_counts(self, t):
        """[e(0) .. e(10)]: frames a fresh stream of age ``t`` has pushed out of block L (e(0) = t, the input frames)."""
        d, s = self._cum_delays(), self._cum_strides()
        return [max(0, -(-(t - d[i]) // s[i])) for i in range(len(d))]

    def prime_clip_frames(self, t):
        """[T_0 .. T_10]: frames of the clip tensors for a history of ``t`` frames (T_0 = t; block L maps T to
        (T + 2 * padding - k) // stride + 1)."""
        out = [t]
        for blk in self._blocks:
            out.append((out[-1] + 2 * blk.padding - blk.kernel_size) // blk.stride + 1)
        return out

    def prime_table(self, t):
        """[(name, source, count, first, window)] in record order (``_move_windows``) for the rings and the pooling window of
        a fresh stream of age ``t``: the ring ``name`` has received ``count`` = e(L) frames, L the level that feeds it, frame j
        of it is frame j of the clip tensor ``source`` -- xin0: the input-norm output, y<i> / out<i>: post-GCN tensor /
        output of block i (0-based) -- and its window is the frames ``first`` .. ``first + window - 1`` (``first`` = count -
        window < 0: that many leading zero frames).  Host only; from the inventory (co_rings.py: ``_rings``), that is from
        ``delay``, ``stride`` and ``kernel_size`` of the blocks.  The small per-stream states are not frames: not listed."""
        e = self.prime_counts(t)
        return [(ring.name, ring.source, e[ring.level], e[ring.level] - ring.window, ring.window) for ring in self._record_rings()]

    def prime_stream_bytes(self, t):
        """Bytes of clip intermediates ONE stream of ``t`` history frames holds while it is primed: the derived input, the
        input-norm output and the post-GCN tensor and the output of every block (all of them are read by the one pack
        launch).  84.8 MB for the NTU model at t = 300."""
        c, _, v, m = self.input_shape
        frames = self.prime_clip_frames(t)
        words = 2 * c * t * v * m
        for i, blk in enumerate(self._blocks):
            words += blk.out_channels * (frames[i] + frames[i + 1]) * v * m
        return 4 * words

    # ---- checks (host only, before anything launches) ------------------------------------------------
    def _check_prime(self, x_hist, framewise=False):
        """Everything ``prime_state`` refuses; returns T.  ``framewise``: the caller's clip pass forms the attention of an
        adaptive graph conv per frame (``CoAGcn.prime_state_as_steps``, agcn.py), so that refusal is not made; every other
        check is the same."""
        self._require_eval()
        if self.unpadded:
            raise NotImplementedError(f"prime_state is not built for the unpadded '*' models ({type(self).__name__}): their valid clip "
                                      "form shifts every frame index; that table is a follow-up -- reset_streams and step the history")
        if not framewise and any(any(k.__name__ == "AdaptiveGraphConvolution" for k in type(b.gcn).__mro__) for b in self._blocks):
            raise NotImplementedError(f"prime_state cannot serve {type(self).__name__}: the clip form of the adaptive graph conv forms one "
                                      "adjacency over all T frames, the steps one per frame (clip != step by design); reset_streams "
                                      "and step the history")
        if any(b.precision != "f32" or getattr(b.gcn, "precision", "f32") != "f32" for b in self._blocks):
            raise NotImplementedError("prime_state takes the exact-fp32 clip kernels: the clip precision of this model is 'bf16x3' "
                                      "(set_precision(model, 'f32'))")
        if not isinstance(x_hist, torch.Tensor) or x_hist.dim() != 5:
            raise RuntimeError(f"prime_state takes an (n, C, T, V, M) history tensor, got "
                               f"{tuple(x_hist.shape) if isinstance(x_hist, torch.Tensor) else type(x_hist).__name__}")
        t = self._fed().check_history(x_hist)           # channel-first, or the layout of the intake that is on
        if t % self.stride:
            raise ValueError(f"prime_state: a history of {t} frames is not a multiple of the total stride {self.stride}: the stride "
                             "phase of the strided blocks must match the slab's (drop the oldest frames)")
        d10 = self._cum_delays()[-1]
        if t < d10:
            raise ValueError(f"prime_state: a history of {t} frames is younger than the {d10} frames after which every block of a "
                             "fresh model is live; such a stream needs its warm-up: reset_streams and step the history")
        native.require_device_f32(x_hist, "history tensor")
        return t

    def _check_prime_streams(self, x_hist, indices, framewise=False):
        """The host checks of both halves of ``prime_streams``: ``prime_state``'s, then ``import_streams``' on a record-less
        stand-in with the lengths, ages and signature the real state will have."""
        t = self._check_prime(x_hist, framewise)
        ages = torch.full((x_hist.shape[0],), t, dtype=torch.int64)
        return self._check_import(StreamState(torch.empty((x_hist.shape[0], 0)), ages, self.move_signature()), indices)

    # ---- the clip pass -----------------------------------------------------------------------------------
    def _prime_chunk(self, x, packed, parts=SpatioTemporalBlock.forward_parts):
        """Records of the streams ``x`` (n, C, T, V, M) into ``packed`` (n, record_floats): the clip pass with every block's
        post-GCN tensor and output kept, then one pack launch.  With an intake on, ``x`` is the history in its layout and
        the channel-first clip takes its place first; the blocks run on the frames the steps would have derived from it
        (``_prepare_clip_as_stepped``), and every pre-pass with state gives its part of the record (``prime``).  ``parts(blk, h)`` yields ``(y, out)`` of a block: its
        two clip stages, or a caller's form of them whose tensors are the steps' (agcn.py: the frame-wise graph conv)."""
        x = self._intake_clip(x)
        n, c, t, v, m = x.shape
        entered, d = self._prepare_clip_as_stepped(x)
        clip = {co_rings.XIN0: self.input_norm(d)}      # the clip tensors under the names the rings' ``source`` asks for
        names = iter(co_rings.block_ring_names(len(self._blocks)))

        def keep_parts(blk, h):
            y_name, out_name = next(names)
            clip[y_name], clip[out_name] = parts(blk, h)
            return clip[out_name]
        self._through_blocks(clip[co_rings.XIN0], keep_parts)
        small = {}
        for stage in reversed(entered):                 # record order (``_record_stages``)
            small.update(stage.prime(entered[stage], t))
        e, jobs, offset = self.prime_counts(t), [], 0
        for ring in self._record_rings():               # a pooling entry is one row of seg channels, pooled by the launch
            src = clip[ring.source]
            kind, rows = (native.PRIME_POOL, ring.seg) if ring.kind == native.SCRUB_POOL_RING else (native.PRIME_RING, ring.rows)
            jobs.append(native.PrimeJob(src.data_ptr(), offset, kind, rows, src.shape[2], e[ring.level] - ring.window, ring.window, 0))
            offset += ring.rows * ring.seg * ring.window
        for stage in self._record_stages:
            for name, rows, seg, window in stage.windows():
                jobs.append(native.PrimeJob(small[name].data_ptr(), offset, native.PRIME_WORDS, seg, 1, 0, window, 0))
                offset += rows * seg * window
        if len(jobs) > native.MOVE_MAX_JOBS:
            raise RuntimeError(f"{len(jobs)} jobs in one pack launch (limit {native.MOVE_MAX_JOBS})")
        arr = (native.PrimeJob * len(jobs))(*jobs)
        rc = native.lib().csk_co_prime_pack_f32(ctypes.byref(arr), len(jobs), native.ptr(packed), offset, n, m, v, native.stream_of(x))
        native.check(rc, "csk_co_prime_pack_f32")

    # ---- public ------------------------------------------------------------------------------------------
    def prime_state(self, x_hist):
        """``StreamState`` of ``n`` streams that have received the frames of ``x_hist`` (n, C, T, V, M), device fp32: one
        record per stream, ages T, this model's ``move_signature()`` -- what ``export_streams`` would return for fresh streams
        stepped through the history, within the clip-versus-steps tolerance of the activations (the small states bit for
        bit), computed by one clip pass and one pack launch per chunk of streams.  T must be a multiple of the total stride
        and at least D(10), the age from which every block of a fresh model is live (76 for the ten-block table).  Needs no
        bound slab and neither reads nor writes the continual state.  Memory: ``prime_stream_bytes(T)`` of intermediates per
        stream (84.8 MB for NTU at T = 300: 12 streams per chunk); the streams are primed in chunks that stay below ``prime_budget_bytes``
        (1 GiB; at least one stream per chunk).  Not built for the '*' models and the 'bf16x3' clip precision; ``CoAGcn`` is
        refused under this name (its clip form is not its steps') and served by ``CoAGcn.prime_state_as_steps``."""
        return self._prime_records(x_hist, self._check_prime(x_hist))

    def _prime_records(self, x_hist, t, parts=SpatioTemporalBlock.forward_parts):
        """``prime_state`` behind its checks: the chunks of streams under ``prime_budget_bytes``, each through ``_prime_chunk``."""
        n = x_hist.shape[0]
        packed = torch.empty((n, self.record_floats()), device=x_hist.device, dtype=torch.float32)
        chunk = max(1, int(self.prime_budget_bytes // self.prime_stream_bytes(t)))
        for lo in range(0, n, chunk):
            self._prime_chunk(x_hist[lo:lo + chunk], packed[lo:lo + chunk], parts)
        return StreamState(packed, torch.full((n,), t, dtype=torch.int64), self.move_signature())

    def prime_streams(self, x_hist, indices):
        """``import_streams(prime_state(x_hist), indices)``: stream ``indices[j]`` of this slab continues as a fresh stream that
        has received the frames of ``x_hist[j]``.  Every host check of both halves runs before the first launch."""
        self._check_prime_streams(x_hist, indices)
        self.import_streams(self.prime_state(x_hist), indices)
