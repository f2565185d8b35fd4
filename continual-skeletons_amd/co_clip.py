"""A stored clip at the steps' arithmetic for every continual model: ``forward_clip_as_steps`` returns the
predictions ``clean_state(); forward_steps(x, pad_end)`` returns -- what the reference's ``evaluate_*_onestream`` scripts report,
which is not the clip logit -- by ONE clip pass and ONE head call.  The clip kernels compute, frame for frame, the activations
the steps compute (the project's clip-versus-steps parity, the ground ``prime_state`` stands on), so only the head differs: the
steps' pooling window starts as zeros, takes one entry per layer-10 frame and releases a prediction per entry from
``pool_size - pool_padding`` entries on.  ``clip_as_steps_map`` says which entries those are; csk_co_head_clip_f32
(csrc/head.hip) forms all of them in one call.  ``CoAGcn`` overrides the three methods (agcn.py): its clip pass must form the
attention per frame."""
import torch

from . import native


class ClipAsSteps:
    """Base class of ``CoStGcn``; it has no state of its own."""

    def clip_as_steps_map(self, t, pad_end=False):
        """Host only.  ``(frames, entries)`` for a fresh model stepped through ``t`` frames: layer 10 has emitted ``frames``
        feature frames -- frame j of the clip pass -- (``prime_counts(t)[-1]``; with ``pad_end`` every block is flushed with its
        ``padding`` zero frames and all ``prime_clip_frames(t)[-1]`` frames of the clip come out -- for the unpadded '*' models
        a block's padding is 0, the flush pushes nothing and the two counts are the same), the pooling window has taken them
        in order, followed with ``pad_end`` by ``pool_padding`` zero entries; entry j (0-based) releases a prediction when
        j + 1 >= pool_size - pool_padding, the mean over pool_size of entries max(0, j + 1 - pool_size) .. j (entries >=
        ``frames`` and the ones before the first are zeros).  ``entries`` lists (first, last) of every prediction, inclusive,
        in order."""
        flush = pad_end and t > 0
        frames = max(0, self.prime_clip_frames(t)[-1]) if flush else self.prime_counts(t)[-1]
        total = frames + (self.pool_padding if flush else 0)
        first = max(0, self.pool_size - self.pool_padding - 1)
        return frames, [(max(0, j + 1 - self.pool_size), j) for j in range(first, total)]

    def _check_clip_as_steps(self):
        self._require_eval()
        if any(b.precision != "f32" or getattr(b.gcn, "precision", "f32") != "f32" for b in self._blocks):
            raise NotImplementedError("forward_clip_as_steps takes the exact-fp32 clip kernels: the clip precision of this model is "
                                      "'bf16x3' (set_precision(model, 'f32'))")

    def features_clip_as_steps(self, x):
        """(N, C, T, V, M) -> (N*M, 256, T', V): the layer-10 feature frames of the model's own clip pass over the frames the
        steps would have derived -- the input pre-passes as the steps apply them (a motion modality: the backward
        difference; ``_prepare_clip_as_stepped``).  Frame j is what the steps emit as their j-th layer-10 frame, as long
        as they emit it (``clip_as_steps_map``); the frames behind it are the ones the end padding releases.  The unpadded
        '*' models need T >= 81, as their clip forward does.  Reads and writes no continual state."""
        self._check_clip_as_steps()
        x = self._intake_clip(x)
        if self.unpadded and (x.dim() != 5 or x.shape[2] < self.receptive_field):
            raise ValueError(f"{type(self).__name__}'s clip forward needs T >= {self.receptive_field} frames, got {tuple(x.shape)}")
        native.require_device_f32(x, f"{type(self).__name__} input")
        return self._clip_stack(self._prepare_clip_as_stepped(x)[1])

    def forward_clip_as_steps(self, x, pad_end=False):
        """(N, C, T, V, M) -> (N, classes, n_predictions): what ``clean_state(); forward_steps(x, pad_end)`` returns (within the
        clip-versus-steps tolerance), by one clip pass (``features_clip_as_steps``) and one csk_co_head_clip_f32 call on its
        feature frames in the steps' alignment (``clip_as_steps_map``): per-frame spatial pool, the zero-initialised pooling
        window re-summed per prediction, oldest entry first, and the FC -- the step kernels' summation orders.  A history
        too short to predict gives an empty (N, classes, 0) tensor, as the steps do.  Neither reads nor writes the continual
        state; needs no bound slab.  The 'bf16x3' clip precision raises."""
        self._check_clip_as_steps()
        n, t = x.shape[0], x.shape[self.time_axis]
        _, _, v, m = self.input_shape
        frames, entries = self.clip_as_steps_map(t, pad_end)
        if not entries:
            return torch.empty((n, self.num_classes, 0), device=x.device)
        if frames:
            h = self.features_clip_as_steps(x)
            if h.shape[2] < frames:
                raise RuntimeError(f"the clip pass gave {h.shape[2]} feature frames, the steps emit {frames}")
        else:                                           # predictions from the window's end padding alone: no frame is read
            native.require_device_f32(x, f"{type(self).__name__} input")
            h = torch.zeros((n * m, 256, 1, v), device=x.device, dtype=torch.float32)
        return self._head_clip(h, frames, entries[0][1], len(entries), n)

    def _head_clip(self, h, frames, first_entry, n_pred, n):
        """The continual head on the clip tensor ``h`` (n * M, 256, T', V) whose first ``frames`` frames are the entries of the
        pooling window: predictions closing on entries ``first_entry`` .. ``first_entry + n_pred - 1`` -> (n, classes,
        n_pred).  One call (profiles/r24_clip_as_steps.md)."""
        _, _, v, m = self.input_shape
        dev = h.device
        entries = torch.empty((frames, n, 256), device=dev, dtype=torch.float32) if frames else None
        pooled = torch.empty((n_pred, n, 256), device=dev, dtype=torch.float32)
        logits = torch.empty((n_pred, n, self.num_classes), device=dev, dtype=torch.float32)
        rc = native.lib().csk_co_head_clip_f32(native.ptr(h), h.shape[2], frames, native.ptr(entries), self.pool_size, first_entry, n_pred,
                                               native.ptr(self.fc.weight.detach()), native.ptr(self.fc.bias.detach()), native.ptr(pooled),
                                               native.ptr(logits), n, m, 256, v, self.num_classes, native.stream_of(h))
        native.check(rc, "csk_co_head_clip_f32")
        return logits.permute(1, 2, 0).contiguous()
