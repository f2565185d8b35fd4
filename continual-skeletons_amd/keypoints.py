"""Kinetics keypoint intake on the device (csrc/keypoints.hip): a pose estimator's people in, the model's input out.

The published Kinetics-skeleton checkpoints were trained on files the reference writes offline with
``datasets/data_preparation/kinetics400_prep.py:100-138`` (``Feeder_kinetics.__getitem__``): up to five OpenPose skeletons per
frame, x and y centred and y flipped, the coordinates of undetected joints (score 0) zeroed, and in every frame on its own the
people ordered by the sum of their joint scores and the best two kept.  A live stream has no such file, so here it is a
pre-pass in front of the unchanged model -- in front of the pre-normalisation (prenorm.py) and the modality (modality.py)
pre-passes: a model with the switch on takes keypoint tensors ``(N, T, P, V, 3)`` (frames: ``(N, P, V, 3)``), ``[..., p, v, :]
= (x, y, score)``, in the place of channel-first ones.

The operation is per frame, so it is causal and has NO state: nothing to clean, reset, move, resize or prime; the continual
model only owns a scratch ``[max_cycle](N, 3, V, M)`` for the selected frames of a cycle.  The arithmetic, the tie and the NaN
rule are stated in include/cskel.h and DESIGN.md section 3f; tracking people across frames (``datasets/tools.py:openpose_match``,
which the reference's pipeline does not call) and reading the estimator's JSON are not reproduced.
"""
import ctypes

import torch

from . import native, parallel

PEOPLE_IN = 5                       # the reference's num_person_in; num_person_out is the model's M
MAX_PEOPLE, MAX_JOINTS = 8, 64      # limits of the entries (include/cskel.h)


def _check_limits(people_in, joints, people_out):
    if isinstance(people_in, bool) or not isinstance(people_in, int) or not people_out <= people_in <= MAX_PEOPLE:
        raise ValueError(f"people_in must be an integer in [{people_out}, {MAX_PEOPLE}] (the people kept .. the entries' limit), "
                         f"got {people_in!r}")
    if not 1 <= joints <= MAX_JOINTS or people_out < 1:
        raise ValueError(f"the keypoint intake takes 1..{MAX_JOINTS} joints and keeps at least one person, got V = {joints}, "
                         f"M = {people_out}")


def select_people_clip(k: torch.Tensor, people_out: int = 2) -> torch.Tensor:
    """(N, T, P, V, 3) keypoints -> a new (N, 3, T, V, people_out) tensor: per frame the ``people_out`` best-scored people,
    centred, y flipped, undetected joints zeroed (csk_select_people_f32)."""
    native.require_device_f32(k, "keypoint clip")
    if k.dim() != 5 or k.shape[4] != 3:
        raise RuntimeError(f"expected an (N, T, P, V, 3) keypoint clip, got {tuple(k.shape)}")
    n, t, p, v, _ = k.shape
    if isinstance(people_out, bool) or not isinstance(people_out, int):
        raise ValueError(f"people_out must be an integer, got {people_out!r}")
    _check_limits(p, v, people_out)
    out = torch.empty((n, 3, t, v, people_out), device=k.device, dtype=torch.float32)
    rc = native.lib().csk_select_people_f32(native.ptr(k), native.ptr(out), n, t, p, v, people_out, native.stream_of(k))
    native.check(rc, "csk_select_people_f32")
    return out


def _check_model_shape(model, people_in):
    c, _, v, m = model.input_shape
    if c != 3:
        raise ValueError(f"the keypoint intake writes (x, y, score): the model takes C = {c} input channels")
    _check_limits(people_in, v, m)
    return people_in


def _check_other_intake(model, enabled):
    if enabled and getattr(model, "ntu_intake", False):        # ntu_intake.py: the clip models' other intake
        raise ValueError("the NTU intake is on: a model runs one intake, switch it off first "
                         "(ntu_intake.set_ntu_intake(model, enabled=False))")


class KeypointIntake:
    """Base class of the clip models (``StGcn`` and its siblings): the switch and the clip pre-pass."""

    keypoint_intake = False
    _kp_people = PEOPLE_IN

    def _set_keypoint_intake(self, enabled, people_in):
        self.keypoint_intake = bool(enabled)
        self._kp_people = people_in

    def _keypoint_shape(self, n, t=None):
        """The input shape with the switch on: (n, P, V, 3) frames, (n, t, P, V, 3) clips."""
        return (n,) + (() if t is None else (t,)) + (self._kp_people, self.input_shape[2], 3)

    def _intake_clip(self, k):
        """The keypoint clip -> the channel-first clip the model runs on (the tensor itself when the switch is off)."""
        if not self.keypoint_intake:
            return k
        native.require_device_f32(k, "model input")
        if k.dim() != 5 or tuple(k.shape) != self._keypoint_shape(k.shape[0], k.shape[1]):
            raise RuntimeError(f"keypoint intake: expected an (N, T, {self._kp_people}, {self.input_shape[2]}, 3) keypoint clip, "
                               f"got {tuple(k.shape)}")
        return select_people_clip(k, self.input_shape[3])


class ContinualKeypointIntake(KeypointIntake):
    """Base class of ``CoStGcn``: the step pre-pass.  ``_kp_scratch`` [max_cycle](N, 3, V, M) takes the selected frames of a
    cycle; it is scratch, allocated when the slab is bound (``_bind``) and only when the switch is on.  There is no state:
    a peek (``update_state=False``) runs the same launch."""

    _kp_scratch = None
    time_axis = property(lambda self: 1 if self.keypoint_intake else 2, doc="the frame axis of the clips the model is fed")

    def _set_keypoint_intake(self, enabled, people_in):
        if bool(enabled) == self.keypoint_intake and people_in == self._kp_people:
            return
        if self._n is not None and self._frames != 0:
            raise RuntimeError(f"the model has stepped {self._frames} frames with the keypoint intake "
                               f"{'on' if self.keypoint_intake else 'off'}: its rings hold features of that input; call "
                               "clean_state() before changing the keypoint intake")
        super()._set_keypoint_intake(enabled, people_in)
        if self._n is not None:
            self._bind_intake(self._n, self._xin0.device)

    def _bind_intake(self, n, device):
        _, _, v, m = self.input_shape
        self._kp_scratch = None
        if self.keypoint_intake:
            self._kp_scratch = torch.empty((self.max_cycle, n, 3, v, m), device=device, dtype=torch.float32)

    def _check_keypoint_frames(self, frames):
        """Host checks of a cycle's keypoint frames; returns the stream count."""
        x0 = frames[0]
        for x_t in frames:
            native.require_device_f32(x_t, "CoStGcn keypoint frame")
            if x_t.shape != x0.shape or x_t.device != x0.device:
                raise RuntimeError("all frames of a cycle must have the same shape and device")
        if x0.dim() != 4 or tuple(x0.shape) != self._keypoint_shape(x0.shape[0]):
            raise RuntimeError(f"keypoint intake: frame shape {tuple(x0.shape)} does not match (N, {self._kp_people}, "
                               f"{self.input_shape[2]}, 3)")
        return x0.shape[0]

    def _intake_frames(self, frames):
        """The cycle's keypoint frames -> the selected channel-first frames (the list itself when the switch is off)."""
        if not self.keypoint_intake:
            return frames
        r = len(frames)
        n, p, v, _ = frames[0].shape
        out = [self._kp_scratch[i] for i in range(r)]
        srcs = (ctypes.c_void_p * r)(*[x_t.data_ptr() for x_t in frames])
        dsts = (ctypes.c_void_p * r)(*[o.data_ptr() for o in out])
        rc = native.lib().csk_select_people_frames_f32(srcs, dsts, r, n, p, v, self.input_shape[3], native.stream_of(frames[0]))
        native.check(rc, "csk_select_people_frames_f32")
        return out


def set_keypoint_intake(model, people_in: int = PEOPLE_IN, enabled: bool = True):
    """Make ``model`` take keypoint tensors -- ``(N, T, P, V, 3)`` clips and histories, ``(N, P, V, 3)`` frames, ``P =
    people_in``, ``[..., p, v, :] = (x, y, score)`` -- and select, centre and zero them on the device first, as the reference's
    Kinetics feeder does offline (default off: no launch, no buffer).  For ``StGcn`` / ``AGcn`` / ``STr``, ``CoStGcn`` /
    ``CoAGcn`` / ``CoSTr``, their ``*Mod`` forms and a ``StreamShards`` (every shard model).  The number of people kept is the
    model's ``input_shape[3]``.  The intake runs in front of the pre-normalisation and the modality pre-passes.
    ``ValueError`` for a model that does not take C = 3 channels, ``people_in`` outside [M, 8] or a clip model whose NTU intake
    (ntu_intake.py) is on; a continual model that has stepped (frame counter not 0) raises ``RuntimeError``: ``clean_state()``
    first.  Returns ``model``."""
    if isinstance(model, parallel.StreamShards):
        for shard in model.models:      # all validated before any is switched: the shards step in lock step
            if not isinstance(shard, KeypointIntake):
                raise TypeError(f"{type(shard).__name__} has no keypoint intake")
            _check_model_shape(shard, people_in)
            changes = bool(enabled) != shard.keypoint_intake or people_in != shard._kp_people
            if isinstance(shard, ContinualKeypointIntake) and changes and shard._n is not None and shard._frames:
                raise RuntimeError("a shard has stepped: call clean_state() on every shard model before changing the keypoint intake")
        for shard in model.models:
            shard._set_keypoint_intake(enabled, people_in)
        return model
    if not isinstance(model, KeypointIntake):
        raise TypeError(f"{type(model).__name__} has no keypoint intake (StGcn, CoStGcn, their siblings, or a StreamShards)")
    _check_other_intake(model, enabled)
    model._set_keypoint_intake(enabled, _check_model_shape(model, people_in))
    return model
