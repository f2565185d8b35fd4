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
rules of the rest of the continual state (``ContinualModality``).
"""
import ctypes

import numpy as np
import torch

from . import graph, native, parallel

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


class InputModality:
    """Base class of the clip models (``StGcn`` and its siblings): the mode and the clip pre-pass."""

    input_modality = "joint"

    def _set_input_modality(self, modality):
        self.__dict__["_mod_parents"] = _parents_arg(modality, self.input_shape[2])     # raises for an unknown skeleton
        self.input_modality = modality

    def _derive_clip(self, x):
        if self.input_modality == "joint":
            return x
        native.require_device_f32(x, "model input")
        return derive_clip(x, self.input_modality, self.__dict__["_mod_parents"])


class ContinualModality(InputModality):
    """Base class of ``CoStGcn``: the step pre-pass and its state.  ``_mod_scratch`` [max_cycle](N, C, V, M) takes the derived
    frames of a cycle (scratch, any non-joint mode); ``_mod_prev`` (N, C, V, M), the last raw frame, and ``_mod_flags`` (N,)
    int32, "this stream has a previous frame", are continual state of the two motion modes:
      * allocated when the slab is bound (``_bind``), only for the modes that need them;
      * ``clean_state`` clears them; ``reset_streams`` clears the flags of the reset streams in its own launch;
      * the single-step peek ``forward_step(update_state=False)`` runs the pre-pass with ``update = 0`` (nothing is written);
      * the snapshot of ``forward_steps(update_state=False)`` holds them (``_state_tensors``)."""

    _mod_scratch = _mod_prev = _mod_flags = None

    def _set_input_modality(self, modality):
        if modality == self.input_modality:
            return
        if self._n is not None and self._frames != 0:
            raise RuntimeError(f"the model has stepped {self._frames} frames in modality {self.input_modality!r}: its rings hold "
                               "features of that input; call clean_state() before changing the input modality")
        super()._set_input_modality(modality)
        if self._n is not None:
            self._bind_modality(self._n, self._xin0.device)

    def _bind_modality(self, n, device):
        c, _, v, m = self.input_shape
        mode = self.input_modality
        self._mod_scratch = self._mod_prev = self._mod_flags = None
        if mode != "joint":
            self._mod_scratch = torch.empty((self.max_cycle, n, c, v, m), device=device, dtype=torch.float32)
        if mode in MOTION:
            self._mod_prev = torch.zeros((n, c, v, m), device=device, dtype=torch.float32)
            self._mod_flags = torch.zeros((n,), device=device, dtype=torch.int32)

    def _clean_modality(self):
        if self._mod_prev is not None:
            self._mod_prev.zero_()
            self._mod_flags.zero_()

    def _modality_tensors(self):
        return [] if self._mod_prev is None else [self._mod_prev, self._mod_flags]

    def _modality_reset_jobs(self):
        """Scrub job (co_reset.py) that clears the flags of the streams being reset: the flag array as a ring of one slot and
        one row in which every stream owns one 4-byte element (the all-zero pattern is int32 0)."""
        if self._mod_flags is None:
            return []
        n = self._mod_flags.shape[0]
        return [native.ScrubJob(self._mod_flags.data_ptr(), n, 1, 1, 0, 1, 1, native.SCRUB_BLOCK_RING)]

    def _derive_frames(self, frames, update=True):
        """The cycle's joint frames -> the frames the model steps on (the list itself for "joint").  ``update=False``: the
        previous-frame buffer and the flags stay as they are."""
        mode = self.input_modality
        if mode == "joint":
            return frames
        r = len(frames)
        n, c, v, m = frames[0].shape
        out = [self._mod_scratch[i] for i in range(r)]
        srcs = (ctypes.c_void_p * r)(*[x_t.data_ptr() for x_t in frames])
        dsts = (ctypes.c_void_p * r)(*[o.data_ptr() for o in out])
        rc = native.lib().csk_derive_modality_frames_f32(srcs, dsts, r, MODE[mode], self.__dict__["_mod_parents"],
                                                         native.ptr(self._mod_prev), native.ptr(self._mod_flags), int(update),
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
    if isinstance(model, parallel.StreamShards):
        for shard in model.models:      # all validated before any is switched: the shards step in lock step
            if not isinstance(shard, InputModality):
                raise TypeError(f"{type(shard).__name__} has no input modality")
            if isinstance(shard, ContinualModality) and modality != shard.input_modality and shard._n is not None and shard._frames:
                raise RuntimeError("a shard has stepped: call clean_state() on every shard model before changing the input modality")
            _parents_arg(modality, shard.input_shape[2])
        for shard in model.models:
            shard._set_input_modality(modality)
        return model
    if not isinstance(model, InputModality):
        raise TypeError(f"{type(model).__name__} has no input modality (StGcn, CoStGcn, their siblings, or a StreamShards)")
    model._set_input_modality(modality)
    return model
