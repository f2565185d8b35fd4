"""The input pre-passes of a model as an ordered chain of stages with one protocol.

A pre-pass runs in front of the unchanged model: the NTU body intake (ntu_intake.py) and the keypoint intake (keypoints.py)
change the layout of what the model is fed, the pre-normalisation (prenorm.py) and the input modality (modality.py) run on
channel-first input behind them.  Each is an ``InputStage`` in its own module; a model (``InputChain``: ``StGcn``, ``CoStGcn``
and their siblings) holds one object per entry of its ``STAGES`` tuple, in that order, and its drivers loop over them -- bind,
clean, bytes, snapshot, reset, move, prime -- and name none.  A stage that is off is the identity: ``clip`` and ``frames``
return the object they were handed, ``bind`` allocates nothing, every list is empty.

This module also has what the stages' setters share: the pointer marshalling of a cycle's frames, the "has stepped" guard
with the re-bind behind it, the validate-every-shard-then-switch loop, and the rule that a model runs one intake.
"""
import ctypes

import torch

from . import native, parallel


def frame_pointers(frames, out):
    """(srcs, dsts): the data pointers of ``frames`` and of as many leading entries of ``out`` as ``void*`` arrays, the way
    the ``*_frames_f32`` entries take a cycle."""
    array = ctypes.c_void_p * len(frames)
    return array(*[x_t.data_ptr() for x_t in frames]), array(*[o.data_ptr() for o in out])


class InputStage:
    """One pre-pass of one model.  The defaults are those of a stage that is off and of the channel-first layout; ``shape``
    is the model's ``input_shape`` (C, T, V, M)."""

    name = None         # the key of ``InputChain.stage``
    what = None         # as the error texts call it: "input modality", "keypoint intake", ...
    intake = False      # True: changes the layout, runs in front of the shape check; False: runs on channel-first input
    off_call = None     # an intake: how to switch it off, for the one-intake rule
    time_axis = 2       # the frame axis of the clips the model is fed while this stage decides the layout

    def __init__(self, shape):
        self.shape = tuple(shape)
        self.scratch = None     # [max_cycle] frames of a cycle behind this stage, once bound and on
        self.flags = None       # (N,) int32: the per-stream element a reset clears, once bound and on

    @property
    def enabled(self):
        return False

    @property
    def settings(self):
        """What the setter compares and ``set`` takes."""
        return ()

    def set(self, settings):
        raise NotImplementedError

    def stepped_with(self):
        """The stage's half sentence of the "has stepped" message: the setting the stepped frames went through."""
        return f"with the {self.what} {'on' if self.enabled else 'off'}"

    # ---- the two forms ----------------------------------------------------------------------------
    def clip(self, x):
        return x

    def clip_as_stepped(self, x):
        """The clip form aligned to what ``frames`` gives for the same frames, one by one (priming, clip-as-steps)."""
        return self.clip(x)

    def frames(self, frames, update=True):
        """A cycle's frames -> the frames behind this stage, in ``scratch``.  ``update=False`` (a peek) writes no state."""
        return frames

    def _into_scratch(self, frames):
        """(out, srcs, dsts) of a cycle: the scratch frames that take the results and both pointer arrays."""
        out = [self.scratch[i] for i in range(len(frames))]
        return (out,) + frame_pointers(frames, out)

    # ---- continual state ----------------------------------------------------------------------------
    def bind(self, n, device, max_cycle):
        """Allocate scratch and state for a slab of ``n`` streams; nothing when off."""
        self.scratch = None

    def state(self):
        """Ordered (record name, tensor) pairs of the per-stream state of a bound slab."""
        return []

    def tensors(self):
        return [tensor for _, tensor in self.state()]

    def clean(self):
        for tensor in self.tensors():
            tensor.zero_()

    def reset_jobs(self):
        """Scrub job (co_reset.py) that clears the flags of the streams being reset: the flag array as a ring of one slot and
        one row in which every stream owns one 4-byte element (the all-zero pattern is int32 0).  The rest of the state stays:
        a clear flag makes the next frame a first frame, which overwrites it."""
        flags = self.flags
        if flags is None:
            return []
        return [native.ScrubJob(flags.data_ptr(), flags.shape[0], 1, 1, 0, 1, 1, native.SCRUB_BLOCK_RING)]

    # ---- records (co_migrate.py, co_prime.py): from the settings alone, no slab needed ------------------
    def windows(self):
        """[(name, rows, seg, window)] of ``state()``, as arrays of 32-bit words with a window of one."""
        return []

    def signature(self):
        """This stage's entries of ``move_signature``."""
        return []

    def prime(self, x_in, t):
        """{record name: tensor} for streams that have stepped the ``t`` frames of ``x_in``, the clip that entered this stage."""
        return {}

    # ---- the layout the model is fed: the channel-first one unless an intake that is on says otherwise ----
    def check_frames(self, frames):
        """Host checks of a cycle's frames; returns the stream count."""
        x0 = frames[0]
        for x_t in frames:
            native.require_device_f32(x_t, "CoStGcn frame")
            if x_t.shape != x0.shape or x_t.device != x0.device:
                raise RuntimeError("all frames of a cycle must have the same shape and device")
        n, c, v, m = x0.shape
        if (c, v, m) != (self.shape[0], self.shape[2], self.shape[3]):
            raise RuntimeError(f"frame shape {tuple(x0.shape)} does not match input_shape {self.shape}")
        return n

    def check_history(self, x_hist):
        """Host check of a 5-d history tensor for ``prime_state``; returns its frame count."""
        n, c, t, v, m = x_hist.shape
        if (c, v, m) != (self.shape[0], self.shape[2], self.shape[3]):
            raise RuntimeError(f"history shape {tuple(x_hist.shape)} does not match input_shape {self.shape}")
        return t

    def random_frame(self, n, device):
        c, _, v, m = self.shape
        return torch.randn((n, c, v, m), device=device)


def _of_stage(name, attribute, default, doc):
    def get(self):
        stage = self._stage_of.get(name)
        return default if stage is None else getattr(stage, attribute)
    return property(get, doc=doc)


class InputChain:
    """Base class of the models: the stage objects and the calls the drivers make on them.  ``STAGES`` is THE order: first
    the intakes, then the stages on channel-first input, each group in the order it runs."""

    STAGES = ()

    def _init_stages(self):
        self.stages = tuple(cls(self.input_shape) for cls in self.STAGES)
        self._stage_of = {stage.name: stage for stage in self.stages}
        self._plain = InputStage(self.input_shape)
        # the order in which the stages' state stands in records, snapshots and job lists: the modality's in front of the
        # pre-normalisation's, as the first exported records had it (co_migrate.py: every StreamState ever saved)
        self._record_stages = self.stages[::-1]

    def stage(self, name):
        return self._stage_of[name]

    input_modality = _of_stage("modality", "mode", "joint", "what the model derives from the joint frames it is fed (modality.py)")
    pre_normalization = _of_stage("prenorm", "enabled", False, "raw joint frames are pre-normalised first (prenorm.py)")
    keypoint_intake = _of_stage("keypoints", "enabled", False, "the model is fed keypoint tensors (keypoints.py)")
    ntu_intake = _of_stage("ntu", "enabled", False, "the model is fed NTU body clips (ntu_intake.py)")
    time_axis = property(lambda self: self._fed().time_axis, doc="the frame axis of the clips the model is fed")

    def _fed(self):
        """The stage that decides the layout of the model's input: the intake that is on, else the channel-first default."""
        for stage in self.stages:
            if stage.intake and stage.enabled:
                return stage
        return self._plain

    def _intake_clip(self, x):
        """What the model is fed -> the channel-first clip (all intakes off: ``x`` itself)."""
        for stage in self.stages:
            if stage.intake:
                x = stage.clip(x)
        return x

    def _prepare_clip(self, x):
        """The channel-first clip -> the clip the blocks run on (all off: ``x`` itself)."""
        for stage in self.stages:
            if not stage.intake:
                x = stage.clip(x)
        return x

    def _prepare_clip_as_stepped(self, x):
        """The same, aligned to the frames the steps derive (priming, clip-as-steps) -> ({stage: the clip that entered it},
        the clip the blocks run on)."""
        entered = {}
        for stage in self.stages:
            if not stage.intake:
                entered[stage] = x
                x = stage.clip_as_stepped(x)
        return entered, x

    # ---- behind the pre-passes: the head of every clip pass (a model: ``_Folded`` with scale / shift, ``layers``) ----
    def input_norm(self, x):
        """(N, C, T, V, M) -> (N*M, C, T, V): permute + data_bn (models/st_gcn/st_gcn.py:49-57) of the clip the blocks run on."""
        native.require_device_f32(x, f"{type(self).__name__} input")
        n, c, t, v, m = x.shape
        ops = self._packed_ops(x.device)
        if ops["scale"].numel() != m * v * c:
            raise RuntimeError(f"input (C,V,M)=({c},{v},{m}) does not match data_bn with {ops['scale'].numel()} channels")
        h = torch.empty((n * m, c, t, v), device=x.device, dtype=torch.float32)
        rc = native.lib().csk_input_norm_f32(native.ptr(x), native.ptr(ops["scale"]), native.ptr(ops["shift"]),
                                             native.ptr(h), n, c, t, v, m, c * t * v, t * v, native.stream_of(x))
        native.check(rc, "csk_input_norm_f32")
        return h

    def _through_blocks(self, h, block):
        """``h`` through the blocks in stack order; ``block(blk, h)`` is one block's output and the next one's input.  The
        caller names the per-block call: ``__call__``, the clip ``forward`` of a continual block, a form that keeps parts."""
        for blk in self.layers.values():
            h = block(blk, h)
        return h

    def _stage_frames(self, frames, update=True):
        """A cycle's frames through the whole chain (all off: the list itself)."""
        for stage in self.stages:
            frames = stage.frames(frames, update)
        return frames

    def _slab(self):
        """(streams, device, max_cycle, frames stepped) of the bound continual slab; None for a clip model or no slab."""
        return None


def switch_stage(model, name, what, check, family="StGcn, CoStGcn, their siblings, or a StreamShards", then=None):
    """The setters' common half.  ``model``: a model or a ``StreamShards`` (every shard model).  ``check(m, stage)`` validates
    the request against one model and returns the settings for ``stage.set``.  Every model is validated before any is
    switched (the shards step in lock step); a continual model that has stepped refuses a change; a bound slab is re-bound
    for the new settings.  ``then(m, settings)``: a check that runs behind the "has stepped" refusal.  ``family``: the models that have the stage, for the ``TypeError``.  Returns ``model``."""
    sharded = isinstance(model, parallel.StreamShards)
    plan = []
    for m in model.models if sharded else [model]:
        if not isinstance(m, InputChain) or name not in m._stage_of:
            raise TypeError(f"{type(m).__name__} has no {what}" + ("" if sharded else f" ({family})"))
        stage = m.stage(name)
        settings = check(m, stage)
        if settings == stage.settings:
            continue
        slab = m._slab()
        if slab is not None and slab[3] != 0:
            if sharded:
                raise RuntimeError(f"a shard has stepped: call clean_state() on every shard model before changing the {what}")
            raise RuntimeError(f"the model has stepped {slab[3]} frames {stage.stepped_with()}: its rings hold features of that "
                               f"input; call clean_state() before changing the {what}")
        if then is not None:
            then(m, settings)
        plan.append((stage, settings, slab))
    for stage, settings, slab in plan:
        stage.set(settings)
        if slab is not None:
            stage.bind(*slab[:3])
    return model


def check_one_intake(model, stage, enabled):
    """A model runs one intake: switching ``stage`` on while another intake of the chain is on raises."""
    for other in model.stages:
        if enabled and other.intake and other is not stage and other.enabled:
            raise ValueError(f"the {other.what} is on: a model runs one intake, switch it off first ({other.off_call})")
