"""Pre-normalisation of raw skeleton frames on the device (csrc/prenorm.hip).

Published NTU RGB+D checkpoints were trained on pre-normalised joint files: the reference runs
``datasets/data_preparation/preprocess.py:14-93`` over the whole dataset (``ntu60_prep.py:179`` / ``ntu120_prep.py:219``).
It centres every frame on the main body's joint 1 and rotates the clip so that the ``zaxis`` bone of the first frame lies
on z and the ``xaxis`` line on x.  A live stream has no preprocessed file, so here it is a pre-pass in front of the unchanged
model, and in front of the modality pre-pass (modality.py): the reference derives bone and motion from the normalised file.

The centring is per frame, so it is causal; the two rotation matrices are latched from a stream's first frame.  That is
per-stream state -- ``rot`` (N, 18) fp64 and ``has_rot`` (N,) int32 -- and it follows the rules of the rest of the continual
state (``ContinualPreNorm``).  The arithmetic is stated in include/cskel.h and DESIGN.md section 3c; the reference's padding
of null frames looks ahead and is not reproduced, in either form (whole clips: the pre-pass of ntu_intake.py, in front of this one).
"""
import ctypes

import torch

from . import native, parallel

ZAXIS, XAXIS = (0, 1), (8, 4)       # the reference's defaults: hip -> spine on z, right -> left shoulder on x (NTU RGB+D)


def _check_joints(num_joints, zaxis, xaxis):
    """The four joint indices as ints; ValueError for anything that is not a pair of indices in [0, V)."""
    out = []
    for name, pair in (("zaxis", zaxis), ("xaxis", xaxis)):
        try:
            pair = tuple(pair)
        except TypeError:
            pair = ()
        if len(pair) != 2 or any(isinstance(j, bool) or not isinstance(j, int) for j in pair):
            raise ValueError(f"{name} must be a pair of joint indices, got {pair!r}")
        if any(not 0 <= j < num_joints for j in pair):
            raise ValueError(f"{name} = {pair} outside [0, {num_joints}): the skeleton has {num_joints} joints")
        out += list(pair)
    if num_joints < 2:
        raise ValueError(f"pre-normalisation centres on joint 1: a skeleton of {num_joints} joint has none")
    return tuple(out)


def pre_normalize_clip(x: torch.Tensor, zaxis=ZAXIS, xaxis=XAXIS) -> torch.Tensor:
    """(N, 3, T, V, M) raw joints -> a new tensor, the pre-normalised clip (matrices from frame 0 of every sample)."""
    native.require_device_f32(x, "joint clip")
    if x.dim() != 5 or x.shape[1] != 3:
        raise RuntimeError(f"expected an (N, 3, T, V, M) clip, got {tuple(x.shape)}")
    n, _, t, v, m = x.shape
    joints = _check_joints(v, zaxis, xaxis)
    out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    rc = native.lib().csk_prenorm_f32(native.ptr(x), native.ptr(out), n, t, v, m, *joints, native.stream_of(x))
    native.check(rc, "csk_prenorm_f32")
    return out


def _check_model_shape(model, zaxis, xaxis):
    c, _, v, _ = model.input_shape
    if c != 3:
        raise ValueError(f"pre-normalisation rotates 3-D coordinates: the model takes C = {c} input channels")
    return _check_joints(v, zaxis, xaxis)


class PreNorm:
    """Base class of the clip models (``StGcn`` and its siblings): the switch and the clip pre-pass."""

    pre_normalization = False
    _pn_joints = ZAXIS + XAXIS

    def _set_pre_normalization(self, enabled, joints):
        self.pre_normalization = bool(enabled)
        self._pn_joints = joints

    def _prenorm_clip(self, x):
        if not self.pre_normalization:
            return x
        native.require_device_f32(x, "model input")
        return pre_normalize_clip(x, self._pn_joints[:2], self._pn_joints[2:])


class ContinualPreNorm(PreNorm):
    """Base class of ``CoStGcn``: the step pre-pass and its state.  ``_pn_scratch`` [max_cycle](N, 3, V, M) takes the
    normalised frames of a cycle (scratch); ``_pn_rot`` (N, 18) fp64, a stream's Rz then Rx, and ``_pn_flags`` (N,) int32,
    "this stream has latched its rotations", are continual state:
      * allocated when the slab is bound (``_bind``), only when the switch is on;
      * ``clean_state`` clears the flags; ``reset_streams`` clears the flags of the reset streams in its own launch;
      * the single-step peek ``forward_step(update_state=False)`` runs the pre-pass with ``update = 0`` (nothing is written);
      * the snapshot of ``forward_steps(update_state=False)`` holds them (``_state_tensors``)."""

    _pn_scratch = _pn_rot = _pn_flags = None

    def _set_pre_normalization(self, enabled, joints):
        if bool(enabled) == self.pre_normalization and joints == self._pn_joints:
            return
        if self._n is not None and self._frames != 0:
            raise RuntimeError(f"the model has stepped {self._frames} frames with pre-normalisation "
                               f"{'on' if self.pre_normalization else 'off'}: its rings hold features of that input; call "
                               "clean_state() before changing the pre-normalisation")
        super()._set_pre_normalization(enabled, joints)
        if self._n is not None:
            self._bind_prenorm(self._n, self._xin0.device)

    def _bind_prenorm(self, n, device):
        _, _, v, m = self.input_shape
        self._pn_scratch = self._pn_rot = self._pn_flags = None
        if self.pre_normalization:
            self._pn_scratch = torch.empty((self.max_cycle, n, 3, v, m), device=device, dtype=torch.float32)
            self._pn_rot = torch.zeros((n, 18), device=device, dtype=torch.float64)
            self._pn_flags = torch.zeros((n,), device=device, dtype=torch.int32)

    def _clean_prenorm(self):
        if self._pn_flags is not None:
            self._pn_rot.zero_()
            self._pn_flags.zero_()

    def _prenorm_tensors(self):
        return [] if self._pn_flags is None else [self._pn_rot, self._pn_flags]

    def _prenorm_state_bytes(self):
        return sum(t.numel() * t.element_size() for t in self._prenorm_tensors())

    def _prenorm_reset_jobs(self):
        """Scrub job (co_reset.py) that clears the flags of the streams being reset: the flag array as a ring of one slot and
        one row in which every stream owns one 4-byte element (the all-zero pattern is int32 0).  The matrices stay: a clear
        flag makes the next frame a first frame, which overwrites them."""
        if self._pn_flags is None:
            return []
        n = self._pn_flags.shape[0]
        return [native.ScrubJob(self._pn_flags.data_ptr(), n, 1, 1, 0, 1, 1, native.SCRUB_BLOCK_RING)]

    def _prenorm_frames(self, frames, update=True):
        """The cycle's raw joint frames -> the normalised frames (the list itself when the switch is off).  ``update=False``:
        the latched rotations and the flags stay as they are."""
        if not self.pre_normalization:
            return frames
        r = len(frames)
        n, _, v, m = frames[0].shape
        out = [self._pn_scratch[i] for i in range(r)]
        srcs = (ctypes.c_void_p * r)(*[x_t.data_ptr() for x_t in frames])
        dsts = (ctypes.c_void_p * r)(*[o.data_ptr() for o in out])
        rc = native.lib().csk_prenorm_frames_f32(srcs, dsts, r, native.ptr(self._pn_rot), native.ptr(self._pn_flags), int(update),
                                                 n, v, m, *self._pn_joints, native.stream_of(frames[0]))
        native.check(rc, "csk_prenorm_frames_f32")
        return out


def set_pre_normalization(model, enabled: bool = True, zaxis=ZAXIS, xaxis=XAXIS):
    """Make ``model`` pre-normalise the raw joint frames it is fed (default off: no launch, no buffer).  For ``StGcn`` /
    ``AGcn`` / ``STr``, ``CoStGcn`` / ``CoAGcn`` / ``CoSTr`` and a ``StreamShards`` (every shard model).  ``zaxis`` /
    ``xaxis``: the joint pairs whose first-frame bones are turned onto z and x (the reference's NTU defaults).  The
    pre-pass runs in front of the modality pre-pass (``set_input_modality``), as the reference derives bone and motion from
    the normalised joints.  ``ValueError`` for a model that does not take C = 3 channels or a joint index outside [0, V);
    a continual model that has stepped (frame counter not 0) raises ``RuntimeError``: ``clean_state()`` first.
    Returns ``model``."""
    if isinstance(model, parallel.StreamShards):
        checked = []
        for shard in model.models:      # all validated before any is switched: the shards step in lock step
            if not isinstance(shard, PreNorm):
                raise TypeError(f"{type(shard).__name__} has no pre-normalisation")
            joints = _check_model_shape(shard, zaxis, xaxis)
            changes = bool(enabled) != shard.pre_normalization or joints != shard._pn_joints
            if isinstance(shard, ContinualPreNorm) and changes and shard._n is not None and shard._frames:
                raise RuntimeError("a shard has stepped: call clean_state() on every shard model before changing the pre-normalisation")
            checked.append(joints)
        for shard, joints in zip(model.models, checked):
            shard._set_pre_normalization(enabled, joints)
        return model
    if not isinstance(model, PreNorm):
        raise TypeError(f"{type(model).__name__} has no pre-normalisation (StGcn, CoStGcn, their siblings, or a StreamShards)")
    model._set_pre_normalization(enabled, _check_model_shape(model, zaxis, xaxis))
    return model
