"""NTU RGB+D body intake for whole clips on the device (csrc/ntu_intake.hip): a recorded Kinect clip in, the model's input out.

The published NTU checkpoints were trained on files the reference writes in three steps: ``read_xyz`` keeps the two of the
sensor's (up to four) bodies with the largest motion energy (``datasets/data_preparation/ntu60_prep.py:101-128``), ``gendata``
places them into ``max_frame`` = 300 frames (``:169-177``), and ``pre_normalization`` (``preprocess.py:14-93``) first pads the null
frames -- a body that appears late is moved to the front, a clip shorter than 300 frames is filled by repeating itself -- and
then centres and rotates.  The last part is prenorm.py; this module is everything in front of it, as a pre-pass in front of the
unchanged clip model: a model with the switch on takes body tensors ``(N, T, P, V, 3)``, ``[..., p, v, :] = (x, y, z)``, with
``T`` at most the model's frame count, in the place of channel-first clips.  ``set_ntu_intake`` + ``set_pre_normalization``
together are the reference's pipeline from ``read_xyz`` on.

Both steps look ahead -- the energy is a whole-clip statistic, the padding repeats frames that come later -- so they exist for
whole clips only: a continual model or a ``StreamShards`` refuses the switch.  A history for ``prime_streams`` is a whole
clip, though: prepare it with ``select_bodies_clip``.  The keypoint intake (keypoints.py) is the Kinetics counterpart; a model
runs one of the two.  The definition, the tie rule and the NaN note are in include/cskel.h and DESIGN.md section 3g.

Out of scope: reading ``.skeleton`` text files (the caller parses them into the body tensor), and a causal, running-energy
selection for live streams.
"""
import torch

from . import native, parallel
from .input_stage import InputStage, check_one_intake, switch_stage

BODIES_IN = 4                                   # the reference's max_body_kinect; max_body_true is the model's M
MAX_BODIES, MAX_JOINTS, MAX_FRAMES = 8, 64, 1024    # limits of the entry (include/cskel.h; CSK_NTU_MAX_FRAMES)


def _is_int(value):
    return isinstance(value, int) and not isinstance(value, bool)


def _check_limits(bodies_in, joints, bodies_out):
    if not _is_int(bodies_in) or not bodies_out <= bodies_in <= MAX_BODIES:
        raise ValueError(f"bodies_in must be an integer in [{bodies_out}, {MAX_BODIES}] (the bodies kept .. the entry's limit), "
                         f"got {bodies_in!r}")
    if not 1 <= joints <= MAX_JOINTS or bodies_out < 1:
        raise ValueError(f"the NTU intake takes 1..{MAX_JOINTS} joints and keeps at least one body, got V = {joints}, "
                         f"M = {bodies_out}")


def select_bodies_clip(bodies: torch.Tensor, frames_out: int = None, bodies_out: int = 2) -> torch.Tensor:
    """(N, T, P, V, 3) bodies -> a new (N, 3, frames_out, V, bodies_out) tensor: the ``bodies_out`` bodies with the largest motion
    energy, late bodies moved to the front, the clip repeated up to ``frames_out`` frames (``None``: T) -- csk_ntu_intake_f32."""
    native.require_device_f32(bodies, "body clip")
    if bodies.dim() != 5 or bodies.shape[4] != 3:
        raise RuntimeError(f"expected an (N, T, P, V, 3) body clip, got {tuple(bodies.shape)}")
    n, t, p, v, _ = bodies.shape
    frames_out = t if frames_out is None else frames_out
    if not _is_int(bodies_out) or not _is_int(frames_out):
        raise ValueError(f"bodies_out and frames_out must be integers, got {bodies_out!r}, {frames_out!r}")
    _check_limits(p, v, bodies_out)
    if not t <= frames_out <= MAX_FRAMES:
        raise ValueError(f"frames_out must lie in [T, {MAX_FRAMES}] = [{t}, {MAX_FRAMES}], got {frames_out}")
    out = torch.empty((n, 3, frames_out, v, bodies_out), device=bodies.device, dtype=torch.float32)
    rc = native.lib().csk_ntu_intake_f32(native.ptr(bodies), native.ptr(out), n, t, p, v, bodies_out, frames_out,
                                         native.stream_of(bodies))
    native.check(rc, "csk_ntu_intake_f32")
    return out


def _check_model_shape(model, bodies_in):
    c, t, v, m = model.input_shape
    if c != 3:
        raise ValueError(f"the NTU intake writes (x, y, z): the model takes C = {c} input channels")
    _check_limits(bodies_in, v, m)
    if t > MAX_FRAMES:
        raise ValueError(f"the NTU intake fills at most {MAX_FRAMES} frames: the model takes T = {t}")
    return bodies_in


class NtuIntake(InputStage):
    """The NTU intake of one clip model (input_stage.py), in front of the keypoint intake: the switch, ``bodies`` (P) and the
    clip pre-pass.  It has no step form: the continual models' chains do not hold it."""

    name, what, intake, time_axis = "ntu", "NTU intake", True, 1
    off_call = "ntu_intake.set_ntu_intake(model, enabled=False)"
    def __init__(self, shape):
        super().__init__(shape)
        self.on, self.bodies = False, BODIES_IN

    @property
    def enabled(self):
        return self.on

    @property
    def settings(self):
        return self.on, self.bodies

    def set(self, settings):
        self.on, self.bodies = settings

    def clip(self, x):
        """The body clip -> the channel-first clip of ``input_shape[1]`` frames the model runs on."""
        if not self.on:
            return x
        native.require_device_f32(x, "model input")
        _, t, v, m = self.shape
        if x.dim() != 5 or tuple(x.shape[2:]) != (self.bodies, v, 3) or not 1 <= x.shape[1] <= t:
            raise RuntimeError(f"NTU intake: expected an (N, T <= {t}, {self.bodies}, {v}, 3) body clip, got {tuple(x.shape)}")
        return select_bodies_clip(x, t, m)


def set_ntu_intake(model, enabled: bool = True, bodies_in: int = BODIES_IN):
    """Make the clip model ``model`` take recorded NTU body clips -- ``(N, T, P, V, 3)``, ``P = bodies_in``, ``[..., p, v, :] =
    (x, y, z)``, ``T <= input_shape[1]`` -- and select, compact and repeat them on the device first, as the reference's
    ``read_xyz``, ``gendata`` and the padding step of ``pre_normalization`` do offline (default off: no launch, no buffer).
    For ``StGcn`` / ``AGcn`` / ``STr`` and their ``*Mod`` forms.  The clip is filled to ``input_shape[1]`` frames, the bodies kept
    are the model's ``input_shape[3]``.  The intake runs in front of the pre-normalisation and the modality pre-passes.
    ``ValueError`` for a model that does not take C = 3 channels, ``bodies_in`` outside [M, 8], or a model whose keypoint intake
    is on (one intake per model); ``TypeError`` for a continual model or a ``StreamShards``.  Returns ``model``."""
    from .continual import CoStGcn
    if isinstance(model, (CoStGcn, parallel.StreamShards)):
        raise TypeError(f"{type(model).__name__} steps frame by frame, and the NTU intake looks ahead: the energy that picks the "
                        "bodies is a whole-clip statistic and the padding repeats frames that come later.  It runs on whole clips "
                        "only; to start streams from recorded frames, prepare the history with ntu_intake.select_bodies_clip and "
                        "hand it to prime_streams")

    def check(m, stage):
        _check_model_shape(m, bodies_in)
        check_one_intake(m, stage, enabled)
        return bool(enabled), bodies_in
    return switch_stage(model, "ntu", NtuIntake.what, check, family="StGcn, AGcn, STr or their '*' forms")
