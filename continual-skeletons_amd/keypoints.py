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
import torch

from . import native
from .input_stage import InputStage, check_one_intake, switch_stage

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


class KeypointIntake(InputStage):
    """The keypoint intake of one model (input_stage.py): the switch, ``people`` (P), the clip pre-pass and the step pre-pass.
    ``scratch`` [max_cycle](N, 3, V, M) takes the selected frames of a cycle, allocated when the slab is bound and only when
    the switch is on.  There is no state: ``update`` is ignored and a peek (``update_state=False``) runs the same launch.
    With the switch on, the stage also says what the model is fed: the frame, clip and history shapes and their error texts."""

    name, what, intake, time_axis = "keypoints", "keypoint intake", True, 1
    off_call = "keypoints.set_keypoint_intake(model, enabled=False)"
    def __init__(self, shape):
        super().__init__(shape)
        self.on, self.people = False, PEOPLE_IN

    @property
    def enabled(self):
        return self.on

    @property
    def settings(self):
        return self.on, self.people

    def set(self, settings):
        self.on, self.people = settings

    def fed_shape(self, n, t=None):
        """The input shape with the switch on: (n, P, V, 3) frames, (n, t, P, V, 3) clips."""
        return (n,) + (() if t is None else (t,)) + (self.people, self.shape[2], 3)

    def clip(self, k):
        """The keypoint clip -> the channel-first clip the model runs on (the tensor itself when the switch is off)."""
        if not self.on:
            return k
        native.require_device_f32(k, "model input")
        if k.dim() != 5 or tuple(k.shape) != self.fed_shape(k.shape[0], k.shape[1]):
            raise RuntimeError(f"keypoint intake: expected an (N, T, {self.people}, {self.shape[2]}, 3) keypoint clip, "
                               f"got {tuple(k.shape)}")
        return select_people_clip(k, self.shape[3])

    def bind(self, n, device, max_cycle):
        _, _, v, m = self.shape
        self.scratch = torch.empty((max_cycle, n, 3, v, m), device=device, dtype=torch.float32) if self.on else None

    def check_frames(self, frames):
        x0 = frames[0]
        for x_t in frames:
            native.require_device_f32(x_t, "CoStGcn keypoint frame")
            if x_t.shape != x0.shape or x_t.device != x0.device:
                raise RuntimeError("all frames of a cycle must have the same shape and device")
        if x0.dim() != 4 or tuple(x0.shape) != self.fed_shape(x0.shape[0]):
            raise RuntimeError(f"keypoint intake: frame shape {tuple(x0.shape)} does not match (N, {self.people}, "
                               f"{self.shape[2]}, 3)")
        return x0.shape[0]

    def check_history(self, x_hist):
        t = x_hist.shape[1]
        if tuple(x_hist.shape) != self.fed_shape(x_hist.shape[0], t):
            raise RuntimeError(f"keypoint history shape {tuple(x_hist.shape)} does not match (n, T, {self.people}, "
                               f"{self.shape[2]}, 3)")
        return t

    def random_frame(self, n, device):
        return torch.rand(self.fed_shape(n), device=device)

    def frames(self, frames, update=True):
        """The cycle's keypoint frames -> the selected channel-first frames (the list itself when the switch is off)."""
        if not self.on:
            return frames
        n, p, v, _ = frames[0].shape
        out, srcs, dsts = self._into_scratch(frames)
        rc = native.lib().csk_select_people_frames_f32(srcs, dsts, len(frames), n, p, v, self.shape[3], native.stream_of(frames[0]))
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
    def check(m, stage):
        check_one_intake(m, stage, enabled)
        return bool(enabled), _check_model_shape(m, people_in)
    return switch_stage(model, "keypoints", KeypointIntake.what, check)
