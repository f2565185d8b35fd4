"""Pre-normalisation of raw skeleton frames on the device (csrc/prenorm.hip).

Published NTU RGB+D checkpoints were trained on pre-normalised joint files: the reference runs
``datasets/data_preparation/preprocess.py:14-93`` over the whole dataset (``ntu60_prep.py:179`` / ``ntu120_prep.py:219``).
It centres every frame on the main body's joint 1 and rotates the clip so that the ``zaxis`` bone of the first frame lies
on z and the ``xaxis`` line on x.  A live stream has no preprocessed file, so here it is a pre-pass in front of the unchanged
model, and in front of the modality pre-pass (modality.py): the reference derives bone and motion from the normalised file.

The centring is per frame, so it is causal; the two rotation matrices are latched from a stream's first frame.  That is
per-stream state -- ``rot`` (N, 18) fp64 and ``has_rot`` (N,) int32 -- and it follows the rules of the rest of the continual
state (``PreNorm``).  The arithmetic is stated in include/cskel.h and DESIGN.md section 3c; the reference's padding
of null frames looks ahead and is not reproduced, in either form (whole clips: the pre-pass of ntu_intake.py, in front of this one).
"""
import torch

from . import native
from .input_stage import InputStage, frame_pointers, switch_stage

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


class PreNorm(InputStage):
    """The pre-normalisation of one model (input_stage.py): the switch, the four joints, the clip pre-pass and the step
    pre-pass with its state.  ``scratch`` [max_cycle](N, 3, V, M) takes the normalised frames of a cycle; ``rot`` (N, 18)
    fp64, a stream's Rz then Rx, and ``flags`` (N,) int32, "this stream has latched its rotations", are continual state:
      * allocated when the slab is bound, only when the switch is on;
      * ``clean_state`` clears them; ``reset_streams`` clears the flags of the reset streams in its own launch (the matrices
        stay: a clear flag makes the next frame a first frame, which overwrites them);
      * the single-step peek ``forward_step(update_state=False)`` runs the pre-pass with ``update = 0`` (nothing is written);
      * the snapshot of ``forward_steps(update_state=False)`` holds them."""

    name, what = "prenorm", "pre-normalisation"
    def __init__(self, shape):
        super().__init__(shape)
        self.on, self.joints = False, ZAXIS + XAXIS
        self.rot = None

    @property
    def enabled(self):
        return self.on

    @property
    def settings(self):
        return self.on, self.joints

    def set(self, settings):
        self.on, self.joints = settings

    def stepped_with(self):
        return f"with pre-normalisation {'on' if self.on else 'off'}"

    def clip(self, x):
        if not self.on:
            return x
        native.require_device_f32(x, "model input")
        return pre_normalize_clip(x, self.joints[:2], self.joints[2:])

    def bind(self, n, device, max_cycle):
        _, _, v, m = self.shape
        self.scratch = self.rot = self.flags = None
        if self.on:
            self.scratch = torch.empty((max_cycle, n, 3, v, m), device=device, dtype=torch.float32)
            self.rot = torch.zeros((n, 18), device=device, dtype=torch.float64)
            self.flags = torch.zeros((n,), device=device, dtype=torch.int32)

    def state(self):
        return [] if self.flags is None else [("pn_rot", self.rot), ("pn_flags", self.flags)]

    def windows(self):
        return [("pn_rot", 1, 36, 1), ("pn_flags", 1, 1, 1)] if self.on else []       # (18,) fp64 = 36 words

    def signature(self):
        return [("pre_normalization", (int(self.on),) + tuple(self.joints))]

    def _latch(self, srcs, dsts, r, rot, flags, update, like):
        n, _, v, m = like.shape
        rc = native.lib().csk_prenorm_frames_f32(srcs, dsts, r, native.ptr(rot), native.ptr(flags), int(update), n, v, m,
                                                 *self.joints, native.stream_of(like))
        native.check(rc, "csk_prenorm_frames_f32")

    def prime(self, x_in, t):
        """The rotations a stream latches from its first frame, by the step entry itself (the bits of the steps)."""
        if not self.on:
            return {}
        first, dev = x_in[:, :, 0].contiguous(), x_in.device
        rot = torch.zeros((first.shape[0], 18), device=dev, dtype=torch.float64)
        flags, sink = torch.zeros((first.shape[0],), device=dev, dtype=torch.int32), torch.empty(first.shape, device=dev)
        self._latch(*frame_pointers([first], [sink]), 1, rot, flags, True, first)
        return {"pn_rot": rot, "pn_flags": flags}

    def frames(self, frames, update=True):
        """The cycle's raw joint frames -> the normalised frames (the list itself when the switch is off).  ``update=False``:
        the latched rotations and the flags stay as they are."""
        if not self.on:
            return frames
        out, srcs, dsts = self._into_scratch(frames)
        self._latch(srcs, dsts, len(frames), self.rot, self.flags, update, frames[0])
        return out


def set_pre_normalization(model, enabled: bool = True, zaxis=ZAXIS, xaxis=XAXIS):
    """Make ``model`` pre-normalise the raw joint frames it is fed (default off: no launch, no buffer).  For ``StGcn`` /
    ``AGcn`` / ``STr``, ``CoStGcn`` / ``CoAGcn`` / ``CoSTr`` and a ``StreamShards`` (every shard model).  ``zaxis`` /
    ``xaxis``: the joint pairs whose first-frame bones are turned onto z and x (the reference's NTU defaults).  The
    pre-pass runs in front of the modality pre-pass (``set_input_modality``), as the reference derives bone and motion from
    the normalised joints.  ``ValueError`` for a model that does not take C = 3 channels or a joint index outside [0, V);
    a continual model that has stepped (frame counter not 0) raises ``RuntimeError``: ``clean_state()`` first.
    Returns ``model``."""
    return switch_stage(model, "prenorm", PreNorm.what, lambda m, stage: (bool(enabled), _check_model_shape(m, zaxis, xaxis)))
