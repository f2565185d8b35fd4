"""Bone and motion input modalities, derived from the joint tensor on the device (csrc/modality.hip).

The reference derives them offline, over whole datasets on disk, with two numpy scripts:
``datasets/data_preparation/bone_data_prep.py:158-163`` (``b[v] = x[v] - x[parent(v)]``) and ``motion_data_prep.py:28-30``
(``m[t] = x[t+1] - x[t]``, ``m[T-1] = 0``); the bone-motion stream is the motion of the stored bone file.  A live stream has
no preprocessed file, so here the derivation is a pre-pass in front of the unchanged model: one launch into a scratch
tensor, then the input-norm kernel and everything behind it run on the derived frames exactly as they run on joints.

Clip forwards keep the reference's forward difference.  The continual path is causal and cannot see frame ``t + 1``: its
step form is the backward difference ``m'[s] = x[s] - x[s-1]`` with ``m' = 0`` on a stream's first frame, i.e.
``m'[s] = m[s-1]`` -- a motion model's continual predictions are those of the forward-difference stream one frame later
(DESIGN.md).  That needs state: the previous raw frame and a per-stream "has a previous frame" flag, which follow the
rules of the rest of the continual state (``InputModality``).
"""
import ctypes

import numpy as np
import torch

from . import graph, native
from .input_stage import InputStage, switch_stage

MODALITIES = ("joint", "bone", "joint_motion", "bone_motion")
MODE = {name: code for code, name in enumerate(MODALITIES)}       # CSK_MODALITY_* (include/cskel.h)
MOTION = ("joint_motion", "bone_motion")                           # the modes with a previous-frame state when stepping
BONE = ("bone", "bone_motion")                                     # the modes that need a parent table


def bone_parents(num_joints: int) -> np.ndarray:
    """(V,) int32 parent table of the skeleton with ``num_joints`` joints (graph.Graph.bone_parents): 25 = NTU RGB+D,
    18 = Kinetics / OpenPose."""
    makers = {25: graph.ntu_graph, 18: graph.kinetics_graph}
    if num_joints not in makers:
        raise ValueError(f"no bone parent table for a skeleton of {num_joints} joints (known: {sorted(makers)})")
    return makers[num_joints]().bone_parents


def _check_modality(modality):
    if modality not in MODALITIES:
        raise ValueError(f"input modality must be one of {MODALITIES}, got {modality!r}")


def _parents_arg(modality, num_joints, parents=None):
    """Host int32 array of the parent table as the entries take it, or None where the mode reads no parents."""
    if modality not in BONE:
        return None
    table = bone_parents(num_joints) if parents is None else np.asarray(parents, dtype=np.int32)
    if table.shape != (num_joints,):
        raise ValueError(f"parent table of shape {table.shape} for {num_joints} joints")
    return (ctypes.c_int32 * num_joints)(*[int(p) for p in table])


def derive_clip(x: torch.Tensor, modality: str, parents=None) -> torch.Tensor:
    """(N, C, T, V, M) joints -> the same clip in ``modality`` (clip form: forward difference, last frame 0).  ``parents``:
    (V,) 0-based parent joints, by default the skeleton's table.  "joint" returns ``x`` itself: no launch, no allocation."""
    _check_modality(modality)
    if modality == "joint":
        return x
    native.require_device_f32(x, "joint clip")
    if x.dim() != 5:
        raise RuntimeError(f"expected an (N, C, T, V, M) clip, got {tuple(x.shape)}")
    n, c, t, v, m = x.shape
    out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    rc = native.lib().csk_derive_modality_f32(native.ptr(x), native.ptr(out), MODE[modality], _parents_arg(modality, v, parents),
                                              n, c, t, v, m, native.stream_of(x))
    native.check(rc, "csk_derive_modality_f32")
    return out


class InputModality(InputStage):
    """The modality of one model (input_stage.py): ``mode``, the clip pre-pass and the step pre-pass with its state.
    ``scratch`` [max_cycle](N, C, V, M) takes the derived frames of a cycle (any non-joint mode); ``prev`` (N, C, V, M), the
    last raw frame, and ``flags`` (N,) int32, "this stream has a previous frame", are continual state of the two motion modes:
      * allocated when the slab is bound, only for the modes that need them;
      * ``clean_state`` clears them; ``reset_streams`` clears the flags of the reset streams in its own launch;
      * the single-step peek ``forward_step(update_state=False)`` runs the pre-pass with ``update = 0`` (nothing is written);
      * the snapshot of ``forward_steps(update_state=False)`` holds them."""

    name, what = "modality", "input modality"
    def __init__(self, shape):
        super().__init__(shape)
        self.mode, self.parents = "joint", None     # ``parents``: the host table of a bone mode, as the entries take it
        self.prev = None

    @property
    def enabled(self):
        return self.mode != "joint"

    @property
    def settings(self):
        return self.mode

    def set(self, mode):
        self.parents = _parents_arg(mode, self.shape[2])        # raises for an unknown skeleton
        self.mode = mode

    def stepped_with(self):
        return f"in modality {self.mode!r}"

    def clip(self, x):
        if self.mode == "joint":
            return x
        native.require_device_f32(x, "model input")
        return derive_clip(x, self.mode, self.parents)

    def clip_as_stepped(self, x):
        """A motion mode steps on the BACKWARD difference: frame 0 is zero and frame s is the forward difference of the clip
        form at s - 1 -- the same subtraction, shifted by one frame."""
        d = self.clip(x)
        if self.mode in MOTION:
            shifted = torch.empty_like(d)
            shifted[:, :, 0] = 0.0
            shifted[:, :, 1:] = d[:, :, :-1]
            d = shifted
        return d

    def bind(self, n, device, max_cycle):
        c, _, v, m = self.shape
        self.scratch = self.prev = self.flags = None
        if self.mode != "joint":
            self.scratch = torch.empty((max_cycle, n, c, v, m), device=device, dtype=torch.float32)
        if self.mode in MOTION:
            self.prev = torch.zeros((n, c, v, m), device=device, dtype=torch.float32)
            self.flags = torch.zeros((n,), device=device, dtype=torch.int32)

    def state(self):
        return [] if self.prev is None else [("mod_prev", self.prev), ("mod_flags", self.flags)]

    def windows(self):
        c, _, v, m = self.shape
        return [("mod_prev", 1, c * v * m, 1), ("mod_flags", 1, 1, 1)] if self.mode in MOTION else []

    def signature(self):
        return [("input_modality", self.mode)]

    def prime(self, x_in, t):
        """The last frame that entered the stage; every stream has a previous frame."""
        if self.mode not in MOTION:
            return {}
        return {"mod_prev": x_in[:, :, t - 1].contiguous(),
                "mod_flags": torch.ones((x_in.shape[0],), device=x_in.device, dtype=torch.int32)}

    def frames(self, frames, update=True):
        """The cycle's joint frames -> the frames the model steps on (the list itself for "joint").  ``update=False``: the
        previous-frame buffer and the flags stay as they are."""
        if self.mode == "joint":
            return frames
        n, c, v, m = frames[0].shape
        out, srcs, dsts = self._into_scratch(frames)
        rc = native.lib().csk_derive_modality_frames_f32(srcs, dsts, len(frames), MODE[self.mode], self.parents,
                                                         native.ptr(self.prev), native.ptr(self.flags), int(update),
                                                         n, c, v, m, native.stream_of(frames[0]))
        native.check(rc, "csk_derive_modality_frames_f32")
        return out


def set_input_modality(model, modality: str = "joint"):
    """Select what ``model`` derives from the joint frames it is fed: "joint" (default: the input itself, no launch, no
    buffer), "bone", "joint_motion" or "bone_motion".  For ``StGcn`` / ``AGcn`` / ``STr``, ``CoStGcn`` / ``CoAGcn`` /
    ``CoSTr`` and a ``StreamShards`` (every shard model).  The bone modes need the skeleton's parent table
    (``Graph.bone_parents``: 25 or 18 joints); a model with another joint count raises here.  A continual model that has
    stepped (frame counter not 0) raises ``RuntimeError``: ``clean_state()`` first.  Returns ``model``."""
    _check_modality(modality)

    return switch_stage(model, "modality", InputModality.what, lambda m, stage: modality,
                        then=lambda m, mode: _parents_arg(mode, m.input_shape[2]))      # a bone mode: raises for an unknown skeleton
