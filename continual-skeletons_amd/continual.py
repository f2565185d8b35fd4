"""Continual (frame-by-frame) block library and the CoST-GCN step driver.

Counterpart of the reference's ``CoGraphConvolution`` / ``CoTemporalConvolution`` /
``CoSpatioTemporalBlock`` (models/base.py:273-276, 307-334, 390-446), ``CoModelBase`` (base.py:19-227)
and ``CoStGcn`` (models/cost_gcn/cost_gcn.py).  In the reference the step arithmetic lives in the
third-party ``continual-inference`` package (per-module Python-side buffers, one small ATen op per
module per frame); here every block owns a slice of a persistent HBM state slab and a step is two
kernel launches (csk_gcn_stage_f32 on the new frame, csk_tcn_step_f32 over the ring).

Protocol (anchored on the reference's tests, see oracle/stgcn_oracle.py:CoBlockOracle):
  * ``forward_step(x_t)`` -> output frame or ``None``; nothing is emitted during the first
    ``delay = k-1-padding`` steps, and with temporal stride S only every S-th step emits;
  * the emission of step s equals the clip block's output at t = (s - delay) / S;
  * ``forward_steps(x, pad_end)``: all frames, optionally flushed with ``padding`` zero post-GCN frames;
  * ``clean_state()`` zeroes the window (zero state == the clip conv's left zero padding).
State layout (channel-major, see include/cskel.h): per block a y ring [8 + max_in][C_out][P] and an output ring
[4 + max_in of the next block][C_out][P] (max_in = frames one launch can receive = 8 / cumulative stride); the output
ring of block l is the input/residual history of block l+1, so the residual FIFO (``co.Delay``) costs no copy.  ``engine_advance`` consumes up to 8 frames per call (4 = one
stride cycle of the 10-block stack) with one GCN launch and one multi-emission TCN launch per block,
which is what fills the GPU at ~1000 streams; per-frame stepping is the same code with r = 1.
"""
import contextlib
import ctypes
import math
from collections import OrderedDict
from typing import Optional

import torch
import torch.nn as nn

from . import blocks, fold, native
from .blocks import GraphConvolution, SpatioTemporalBlock, TemporalConvolution, _Folded, init_weights, is_plain_graph_conv, unity, zero
from .co_clip import ClipAsSteps
from .co_plan import NativePlan
from .co_migrate import StreamMove
from .co_prime import StreamPrime
from .co_rings import SlabRings
from .co_reset import StreamReset
from .input_stage import InputChain
from .keypoints import KeypointIntake
from .modality import InputModality
from .prenorm import PreNorm
from .models import MOD_TEMPORAL_PADDING, layer_table, per_layer

MAX_CYCLE = native.CO_MAX_CYCLE
RES_MODE = {"none": 0, "identity": 1, "conv": 2}    # block residual as the step kernels and csk_co_layer.res_kind take it


def y_slots(max_in: int) -> int:
    """Depth of a post-GCN ring: the k-1 = 8 window frames of co.Conv2d + the frames one launch can receive
    (include/cskel.h: CSK_CO_Y_SLOTS)."""
    return 8 + max_in


def in_slots(max_in: int) -> int:
    """Depth of an input / output history ring: residual lag (k-1)/2 = 4 (co.Delay) + the frames one launch of the
    CONSUMING block can receive (include/cskel.h: CSK_CO_IN_SLOTS)."""
    return 4 + max_in


def _round4(n: int) -> int:
    return (n + 3) // 4 * 4


def emissions(s0: int, r: int, delay: int, stride: int):
    """Of the steps ``s0 .. s0 + r - 1``, those that emit are the s >= delay with (s - delay) % stride == 0: returns
    (first of them, how many), or (None, 0) if there is none."""
    first = max(s0, delay)
    first += (delay - first) % stride
    if first >= s0 + r:
        return None, 0
    return first, (s0 + r - 1 - first) // stride + 1


def ring_runs(s0: int, r: int, *depths: int):
    """Yield ``(s, run)``: the frames ``s0 .. s0 + r - 1`` cut into runs that wrap in none of the rings of these depths (frame s
    lives in slot s % depth), so that one launch can take a run with a constant slot stride."""
    s, end = s0, s0 + r
    while s < end:
        run = min([end - s] + [d - s % d for d in depths])
        yield s, run
        s += run


def frame_to_slot(x_t, slot):
    """Store an (N, C, V) frame into a channel-major ring slot [C][P] (positions n * V + v; the padding up to P stays)."""
    n, c, v = x_t.shape
    slot[:, : n * v] = x_t.permute(1, 0, 2).reshape(c, n * v)


def slot_to_frame(slot, n: int, v: int):
    """The (N, C, V) frame held by a channel-major ring slot [C][P], as a contiguous tensor."""
    return slot[:, : n * v].reshape(slot.shape[0], n, v).permute(1, 0, 2).contiguous()


@contextlib.contextmanager
def _snapshot(tensors, get_position, set_position):
    """``forward_steps(update_state=False)``: several frames overwrite live window slots, so the steps run on the real state
    and a copy of ``tensors`` and of the stepping position is put back afterwards, whatever the steps raise."""
    keep, position = [t.clone() for t in tensors], get_position()
    try:
        yield
    finally:
        for t, k in zip(tensors, keep):
            t.copy_(k)
        set_position(position)


def CoGraphConvolution(in_channels, out_channels, A, bn_momentum=0.1):
    """models/base.py:273-276 -- the per-frame graph conv is stateless, so it is the same module."""
    return GraphConvolution(in_channels, out_channels, A, bn_momentum)


class CoTemporalConvolution(TemporalConvolution):
    """models/base.py:307-334: (k,1) conv + BN with a (k-1)-frame window.  ``padding="equal"`` -> (k-1)/2.
    Note the reference's argument order (kernel_size, padding, stride) differs from TemporalConvolution's."""

    def __init__(self, in_channels, out_channels, kernel_size=9, padding=0, stride=1):
        if padding == "equal":
            padding = int((kernel_size - 1) / 2)
        super().__init__(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding)
        self.receptive_field = kernel_size
        self.delay = kernel_size - 1 - padding
        self._ring = None
        self._s = 0

    # -- continual interface on (N, C, V) frames -------------------------------------------------
    def clean_state(self):
        self._ring, self._s = None, 0

    def _state(self, n, v, device):
        p = _round4(n * v)
        c = self.t_conv.in_channels
        if self._ring is None or self._ring.shape != (self.kernel_size, c, p) or self._ring.device != device:
            self._ring = torch.zeros((self.kernel_size, c, p), device=device, dtype=torch.float32)
            self._s = 0
        return p

    def _emit(self, n, v, p):
        ops = self._packed_ops(self._ring.device)
        out = torch.empty((ops["c_out"], p), device=self._ring.device, dtype=torch.float32)
        rc = native.lib().csk_tcn_step_f32(
            native.ptr(self._ring), self.kernel_size, self._s % self.kernel_size, 0, 1, native.ptr(ops["w"]),
            None, 0, 0, 0, None, native.ptr(ops["bias"]), native.ptr(out), 1, 0,
            ops["c_in"], ops["c_out"], p, self.kernel_size, 0, 0, 0, 1, None, native.stream_of(out))
        native.check(rc, "csk_tcn_step_f32")
        return slot_to_frame(out, n, v)

    def forward_step(self, x_t, update_state=True):
        """One frame.  ``update_state=False`` computes the step without advancing: the frame lands in the ring slot
        of the frame that has just left the window, so putting the counter back is all there is to undo."""
        self._require_eval()
        native.require_device_f32(x_t, "CoTemporalConvolution frame")
        n, c, v = x_t.shape
        p = self._state(n, v, x_t.device)
        frame_to_slot(x_t, self._ring[self._s % self.kernel_size])
        out = self._emit(n, v, p) if emissions(self._s, 1, self.delay, self.stride)[1] else None
        if update_state:
            self._s += 1
        return out

    def forward_steps(self, x, pad_end=False, update_state=True):
        n, c, t, v = x.shape
        if not update_state:
            self._state(n, v, x.device)
            with _snapshot([self._ring], lambda: self._s, lambda s: setattr(self, "_s", s)):
                return self.forward_steps(x, pad_end, True)
        outs = [o for o in (self.forward_step(x[:, :, i].contiguous()) for i in range(t)) if o is not None]
        if pad_end:
            p = self._state(n, v, x.device)
            for _ in range(self.padding):
                self._ring[self._s % self.kernel_size].zero_()
                if emissions(self._s, 1, self.delay, self.stride)[1]:
                    outs.append(self._emit(n, v, p))
                self._s += 1
        return torch.stack(outs, dim=2)


def _counter(i, doc):
    """Attribute that IS element ``i`` of the owner's ctypes counter array ``_ctr`` (no copy to keep in step)."""
    return property(lambda self: self._ctr[i], lambda self, value: self._ctr.__setitem__(i, value), doc=doc)


class _BlockState:
    """Slice of the state slab owned by one block: y ring, output ring, (optionally own) input ring, counters.
    ``counters``: the block's (received, emitted) pair inside its model's counter buffer (CoStGcn._bind); a stand-alone
    block makes its own."""

    def __init__(self, c_in, c_out, k, p, device, xin=None, ksplit=1, max_emit=MAX_CYCLE, scratch=None, max_in=MAX_CYCLE,
                 out_slots=None, gcn_ksplit=1, counters=None):
        self.p = p
        self.ksplit = ksplit
        self.gcn_ksplit = gcn_ksplit      # split-K of the graph conv (latency mode); shares the partial-sum buffer
        # split-K scratch of the TCN step: raw partial sums of the emissions ONE launch can produce (max_emit: MAX_CYCLE
        # for a stand-alone block, MAX_CYCLE / cumulative stride inside a stack).  Launches are stream-ordered, so a
        # stack shares one scratch buffer (``scratch``, sized by its largest user) instead of one per block.
        self.max_emit = max_emit
        self.owns_partial = (ksplit > 1 or gcn_ksplit > 1) and scratch is None
        slabs = max(max_emit * ksplit if ksplit > 1 else 0, max_in * gcn_ksplit if gcn_ksplit > 1 else 0)   # [c_out][p] each
        need = slabs * c_out * p
        if slabs == 0:
            self.partial = None
        elif scratch is not None:
            if scratch.numel() < need:
                raise ValueError(f"shared split-K scratch holds {scratch.numel()} floats, block needs {need}")
            self.partial = scratch[:need].view(slabs, c_out, p)
        else:
            self.partial = torch.empty((slabs, c_out, p), device=device, dtype=torch.float32)
        # ring depths from what ONE launch can receive / emit (y_slots / in_slots above); a stand-alone block keeps an
        # output ring deep enough for max_emit emissions (and the 4 a fused cycle writes)
        self.max_in = max_in
        self.y = torch.zeros((y_slots(max_in), c_out, p), device=device, dtype=torch.float32)
        self.out = torch.zeros((out_slots or max(4, max_emit), c_out, p), device=device, dtype=torch.float32)
        self.owns_xin = xin is None
        self.xin = torch.zeros((in_slots(max_in), c_in, p), device=device, dtype=torch.float32) if xin is None else xin
        if self.xin.shape[0] < in_slots(max_in):
            raise ValueError(f"input ring of {self.xin.shape[0]} slots is too shallow for launches of {max_in} frames")
        self._ctr = (ctypes.c_int64 * 2)() if counters is None else counters

    s = _counter(0, "frames received")
    e = _counter(1, "frames emitted")

    def zero_(self):
        self.y.zero_()
        self.out.zero_()
        if self.owns_xin:
            self.xin.zero_()
        self.s = self.e = 0


class CoSpatioTemporalBlock(SpatioTemporalBlock):
    """models/base.py:390-446.  Same call signature as the reference's factory function; ``forward`` is the
    clip computation (== SpatioTemporalBlock with ``temporal_padding=padding``), ``forward_step`` /
    ``forward_steps`` run on the persistent state.

    state_dict layout = the reference's container layout (tests/test_cost_gcn.py:97-98,145,193-198):
    no residual -> ``gcn.* / tcn.*``; identity -> ``0.1.gcn.* / 0.1.tcn.*``; conv residual ->
    ``0.0.residual.*`` + ``0.1.gcn.* / 0.1.tcn.*``.  The plain SpatioTemporalBlock layout also loads.
    """

    def __init__(self, in_channels, out_channels, A, stride=1, residual=True, window_size=1, padding=0,
                 CoGraphConv=CoGraphConvolution, CoTempConv=None):
        if padding == "equal":
            padding = 4
        window_size = int(window_size)  # unused by the reference as well (base.py:401)

        def graph_conv(ci, co, a):
            return CoGraphConv(ci, co, a, bn_momentum=0.1)

        def temp_conv(ci, co, kernel_size=9, stride=1, padding=0):
            if CoTempConv is None:
                return TemporalConvolution(ci, co, kernel_size=kernel_size, stride=stride, padding=padding)
            return CoTempConv(ci, co, kernel_size=kernel_size, padding=padding, stride=stride)

        super().__init__(in_channels, out_channels, A, stride=stride, residual=residual, temporal_kernel_size=9,
                         temporal_padding=padding, GraphConv=graph_conv, TempConv=temp_conv)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size = 9
        self.padding = padding
        self.receptive_field = self.kernel_size
        self.delay = self.kernel_size - 1 - padding
        self.kind = "none" if self.residual is zero else ("identity" if self.residual is unity else "conv")
        self._prefix_map = {"none": {}, "identity": {"gcn.": "0.1.gcn.", "tcn.": "0.1.tcn."},
                            "conv": {"gcn.": "0.1.gcn.", "tcn.": "0.1.tcn.", "residual.": "0.0.residual."}}[self.kind]
        self._state: Optional[_BlockState] = None
        self._register_state_dict_hook(CoSpatioTemporalBlock._to_co_keys)
        self._register_load_state_dict_pre_hook(self._from_co_keys)
        if not self._native_tail:
            raise NotImplementedError("continual blocks need the native TemporalConvolution (the ring-buffer step kernel)")
        # self.gcn may be any per-frame graph-conv module (models/base.py:273-276 applies it frame by frame): native
        # ones bring a ``stage`` method on the channel-major state layout, foreign ones go through _foreign_gcn_stage

    # ---- state_dict key layout -------------------------------------------------------------------
    @staticmethod
    def _to_co_keys(module, state_dict, prefix, local_metadata):
        for plain, co in module._prefix_map.items():
            for k in [k for k in state_dict if k.startswith(prefix + plain)]:
                state_dict[prefix + co + k[len(prefix + plain):]] = state_dict.pop(k)
        return state_dict

    def _from_co_keys(self, state_dict, prefix, *args):
        for plain, co in self._prefix_map.items():
            for k in [k for k in state_dict if k.startswith(prefix + co)]:
                state_dict[prefix + plain + k[len(prefix + co):]] = state_dict.pop(k)

    def _fold(self):                      # fold from the PLAIN layout whatever state_dict() emits
        sd = {}
        for k, v in nn.Module.state_dict(self).items():
            for plain, co in self._prefix_map.items():
                if k.startswith(co):
                    k = plain + k[len(co):]
                    break
            sd[k] = v
        split = self.precision == "bf16x3" or self.step_precision == "bf16x3"
        return fold.fold_block_tail(sd, "", has_conv_residual=self.kind == "conv", split=split, stride=self.stride)

    # ---- persistent state --------------------------------------------------------------------------
    def bind_state(self, p: int, device, xin: Optional[torch.Tensor] = None, max_emit: int = MAX_CYCLE,
                   scratch: Optional[torch.Tensor] = None, max_in: int = MAX_CYCLE, out_slots: Optional[int] = None,
                   counters=None) -> _BlockState:
        """(Re)allocate this block's slab slice for P positions; ``xin`` = upstream block's output ring; ``max_in`` /
        ``max_emit`` = frames one launch of this block can receive / emit; ``out_slots`` = depth of the output ring (what
        the consuming block needs as its input history); ``scratch`` = split-K scratch shared with the other blocks;
        ``counters`` = this block's pair of the model's counter buffer."""
        self._state = _BlockState(self.in_channels, self.out_channels, self.kernel_size, p, device, xin,
                                  ksplit=self._pick_ksplit(p), max_emit=max_emit, scratch=scratch, max_in=max_in,
                                  out_slots=out_slots, gcn_ksplit=self._pick_gcn_ksplit(p), counters=counters)
        return self._state

    def scratch_floats(self, p: int, max_emit: int = MAX_CYCLE, max_in: int = MAX_CYCLE) -> int:
        """Split-K scratch this block needs for launches of up to ``max_in`` received frames / ``max_emit`` emissions
        (0 without split-K)."""
        ks, gks = self._pick_ksplit(p), self._pick_gcn_ksplit(p)
        return max(max_emit * ks if ks > 1 else 0, max_in * gks if gks > 1 else 0) * self.out_channels * p

    split_k = 0     # 0: no split-K; n > 1: latency mode -- up to n channel ranges per tile when a launch is too small

    THROUGHPUT_SPLIT_K = 1   # split-K of the 256-channel blocks in the default mode (see _pick_ksplit)

    def _pick_ksplit(self, p: int) -> int:
        """Split-K factor of this block's TCN step (csk_tcn_step_f32 ``ksplit``) -- a function of (C_out, split_k) ONLY: a
        stream's results never depend on how many streams share the slab (``p`` is not used).
        * Default mode: no split.  (Rounds 2-5 cut the 2304-deep K loop of the C_out >= 256 blocks into 3 channel ranges to
          pack 800 tiles of 128 x 128 onto 512 resident slots; the slot-balanced tiles of csrc/step16.hip make every launch
          of the 1024-stream cycle exactly 512 equal workgroups, without partial sums and a reduction launch.)
        * Latency mode (``split_k`` > 1, meant for a handful of streams): up to 4 * split_k ranges (<= 32), at least one
          8-channel chunk each -- a 9-tap chunk is 3.8 us of MFMAs for one workgroup, and with a handful of tiles the other
          250 CUs are idle anyway.  (Until round 4 the factor was also capped by 256 // tiles, i.e. by the slab size: one
          stream got 32 ranges at C = 256 and sixteen streams 18 -- different summation orders for the same stream.)"""
        base = self.THROUGHPUT_SPLIT_K if self.out_channels >= 256 else 1
        if self.split_k <= 1:
            return base
        return max(base, min(4 * self.split_k, 32, -(-self.out_channels // 8)))

    def _pick_gcn_ksplit(self, p: int) -> int:
        """Split-K factor of this block's graph conv (csk_gcn_stage_splitk_f32), latency mode only: with a handful of
        streams one workgroup per tile walks all 3 * C_in / 8 K-chunks alone (52 us at C_in = 256 -- 60 % of a frame's
        latency at one stream, profiles/r04_latency_1stream.md).  A function of (C_in, split_k) only (``p`` is not used)."""
        if self.split_k <= 1 or type(self.gcn) is not GraphConvolution or self.in_channels < 16:
            return 1
        return max(1, min(4 * self.split_k, 32, -(-self.in_channels // 8)))

    def clean_state(self):
        if self._state is not None:
            self._state.zero_()

    def engine_advance(self, r: int, n_frames: int, V: int, flush: bool = False):
        """Consume ``r`` (<= MAX_CYCLE) frames already stored in ``xin[(s .. s+r-1) % HIST]`` (channel-major).  Returns
        ``(first_out_slot, n_emit)`` for the emissions of these frames, or None.  ``flush`` pushes zero
        post-GCN frames instead (end padding)."""
        st, k = self._state, self.kernel_size
        HIST, YRING, OUT = st.xin.shape[0], st.y.shape[0], st.out.shape[0]      # ring depths of this block's slab slice
        if self.precision != "f32" and self.step_precision == "f32":
            raise NotImplementedError(
                "precision 'bf16x3' covers the clip kernels only: in step mode every ring slot feeds ONE tap per emission, so "
                "the split kernel would stage twice the bytes per MFMA of the clip form and is bound by staging, not by the "
                "matrix pipe (priced in DESIGN.md); step with the default precision")
        if not 1 <= r <= st.max_in:
            raise ValueError(f"engine_advance handles 1..{st.max_in} frames per call of this block, got {r}")
        s0, p = st.s, st.p
        if not flush and self._fusable(r, s0, V):
            return self._fused_advance(n_frames, V)
        split = dict(ksplit=st.gcn_ksplit, partial=st.partial) if st.gcn_ksplit > 1 else {}     # latency mode
        for s, run in ring_runs(s0, r, YRING) if flush else ring_runs(s0, r, HIST, YRING):
            if flush:
                st.y[s % YRING: s % YRING + run].zero_()
            elif hasattr(self.gcn, "stage"):     # per-frame graph conv, one launch per non-wrapping slot run
                self.gcn.stage(st.xin[s % HIST], st.y[s % YRING], n_seg=run, frames=n_frames,
                               x_strides=(self.in_channels * p, p), y_strides=(self.out_channels * p, p), **split)
            else:
                self._foreign_gcn_stage(st, s, run, n_frames, V)
        first, n_emit = emissions(s0, r, self.delay, self.stride)
        st.s += r
        if not n_emit:
            return None
        ops = self._packed_ops(st.y.device)
        lag = (k - 1) // 2              # emission s pairs with input frame s - 4 (co.Delay / residual_shrink)
        mode, slot0 = RES_MODE[self.kind], st.e % OUT
        if self._use_split_step():      # csk_tcn_step_bf16x3: the same rings and slot arithmetic, the split weight images (no split-K)
            launcher, w, w_res, splitk = "tcn_step_split_launch", ops["w_split"], ops["w_res_split"], ()
        else:
            launcher, w, w_res, splitk = "tcn_step_launch", ops["w"], ops["w_res"], (st.ksplit, native.ptr(st.partial))
        # one launch; with split-K at most max_emit emissions per launch (the scratch holds that many partial sums) --
        # only the end-padding flush of a stack exceeds it (per-output summation order does not depend on the grouping)
        group = n_emit if (st.partial is None or st.ksplit <= 1) else min(n_emit, st.max_emit)     # only a split temporal conv is bound by the scratch
        for e0 in range(0, n_emit, group):
            ne, f0 = min(group, n_emit - e0), first + e0 * self.stride
            getattr(blocks, launcher)(      # looked up per call: tools and tests time / count launches by replacing the attribute
                native.ptr(st.y), YRING, f0 % YRING, self.stride, ne, native.ptr(w),
                native.ptr(st.xin) if mode else None, HIST, (f0 - lag) % HIST, self.stride,
                native.ptr(w_res), native.ptr(ops["bias"]), native.ptr(st.out), OUT, (slot0 + e0) % OUT,
                self.out_channels, self.out_channels, p, k, mode, self.in_channels if mode else 0, 1, *splitk,
                native.stream_of(st.y))
        st.e += n_emit
        return slot0, n_emit

    fuse_step = True    # one launch per block and stride cycle where csk_co_block_step_f32 applies (bit-identical)

    step_precision = "f32"      # or "bf16x3" (opt-in, set_step_precision): arithmetic of the temporal STEP kernel
    SPLIT_STEP_MIN_CHANNELS = 128   # narrowest layer csk_tcn_step_bf16x3 takes (layers 5-10 of the ten-block table)

    def _use_split_step(self) -> bool:
        """csk_tcn_step_bf16x3 takes this block's emitting steps: the mode is on, the block is one of the 128- / 256-channel
        layers (64-channel blocks keep the fused one-launch exact stack) with stride 1 or 2 and runs without split-K (latency
        mode keeps its exact kernels).  A function of the LAYER only -- never of the slab, the cycle length or the ring
        position -- so a stream's results do not depend on how many streams share the slab."""
        return (self.step_precision == "bf16x3" and self.kernel_size == 9 and self.out_channels >= self.SPLIT_STEP_MIN_CHANNELS
                and self.stride in (1, 2) and self._pick_ksplit(0) == 1 and self._pick_gcn_ksplit(0) == 1)

    def _fusable(self, r: int, s0: int, V: int) -> bool:
        """csk_co_block_step_f32 (include/cskel.h): 64-row blocks, stride 1, a whole 4-frame cycle of emitting steps,
        native sparse graph conv, block residual none / identity, no split-K."""
        if self._use_split_step():
            return False
        if not (self.fuse_step and r == 4 and self.stride == 1 and self.out_channels <= 64 and s0 >= self.delay
                and self.kind in ("none", "identity") and is_plain_graph_conv(self.gcn) and self._state.ksplit == 1
                and self._state.gcn_ksplit == 1):
            return False
        g = self.gcn._packed_ops(self._state.y.device)
        cnt = g["ell_cnt_host"]
        return int(cnt[0]) <= 1 and int(cnt[1]) <= 1 and int(cnt[2]) <= 4 and ((64 + V - 2) // V + 1) * V <= 128

    def _layer_struct(self, device):
        """(csk_co_layer of this block, objects to keep alive): the packed graph-conv and temporal-conv operands and the bound
        state as the native side takes them -- the plan as an array of these (co_plan.py), csk_co_block_step_f32 field by
        field (``_fused_advance``).  ``keep`` = [graph-conv operands, temporal-conv operands]."""
        g, t, st = self.gcn._packed_ops(device), self._packed_ops(device), self._state
        L = native.CoLayer()
        L.c_in, L.c_out, L.stride, L.res_kind = self.in_channels, self.out_channels, self.stride, RES_MODE[self.kind]
        L.gcn_res_mode, L.ell_w = g["res_mode"], g["ell_w"]
        L.ell_cnt[:] = [int(c) for c in g["ell_cnt_host"][:3]]
        L.gcn_w, L.gcn_bias, L.ell_src = g["w"].data_ptr(), g["bias"].data_ptr(), g["ell_src"].data_ptr()
        L.ell_val = g["ell_val"].data_ptr() if g["ell_val"] is not None else None
        L.tcn_w, L.tcn_bias = t["w"].data_ptr(), t["bias"].data_ptr()
        L.tcn_w_res = t["w_res"].data_ptr() if t["w_res"] is not None else None
        L.y_ring, L.out_ring = st.y.data_ptr(), st.out.data_ptr()
        L.y_slots, L.out_slots, L.tcn_ksplit = st.y.shape[0], st.out.shape[0], st.ksplit
        L.partial_emits = st.max_emit if (st.partial is not None and st.ksplit > 1) else 0
        L.gcn_ksplit, L.gcn_partial_frames = st.gcn_ksplit, (st.max_in if st.gcn_ksplit > 1 else 0)
        L.tcn_partial = st.partial.data_ptr() if st.partial is not None else None
        return L, [g, t]

    def _fused_advance(self, n_skel: int, V: int):
        st, P = self._state, ctypes.c_void_p
        L, (g, _) = self._layer_struct(st.y.device)
        HIST, s0, slot0 = st.xin.shape[0], st.s, st.e % L.out_slots
        rc = native.lib().csk_co_block_step_f32(
            native.ptr(st.xin), HIST, s0 % HIST, L.c_in, P(L.gcn_w), P(L.gcn_bias), P(L.ell_src), P(L.ell_val),
            native.ptr(g["ell_cnt_host"]), L.ell_w, L.gcn_res_mode,       # the entry reads the counts through a host pointer
            P(L.y_ring), L.y_slots, s0 % L.y_slots, P(L.tcn_w), P(L.tcn_bias),
            L.res_kind, (s0 - (self.kernel_size - 1) // 2) % HIST, P(L.out_ring), L.out_slots, slot0,
            L.c_out, n_skel, V, st.p, native.stream_of(st.y))
        native.check(rc, "csk_co_block_step_f32")
        st.s, st.e = st.s + 4, st.e + 4
        return slot0, 4

    def _foreign_gcn_stage(self, st, s: int, run: int, n_frames: int, V: int):
        """Graph-conv modules without a native ``stage`` (e.g. the S-TR spatial attention a sibling model passes as
        ``CoGraphConv``, models/base.py:390-400): applied per frame as ``module(x_t.unsqueeze(2)).squeeze(2)``
        (base.py:273-276) on (NM, C, 1, V) tensors converted from / to the channel-major ring slots."""
        HIST, YRING = st.xin.shape[0], st.y.shape[0]
        for j in range(run):
            xs, ys = st.xin[(s + j) % HIST], st.y[(s + j) % YRING]
            y_t = self.gcn(slot_to_frame(xs, n_frames, V).unsqueeze(2))
            if tuple(y_t.shape) != (n_frames, self.out_channels, 1, V) or y_t.dtype != torch.float32 or y_t.device != xs.device:
                raise RuntimeError(f"graph-conv module returned {tuple(y_t.shape)} {y_t.dtype} on {y_t.device}, expected "
                                   f"{(n_frames, self.out_channels, 1, V)} float32 on {xs.device}")
            frame_to_slot(y_t.squeeze(2), ys)

    def engine_step(self, n_frames: int, V: int, flush: bool = False) -> Optional[int]:
        """One frame; returns the output-ring slot of this step's emission or None."""
        res = self.engine_advance(1, n_frames, V, flush)
        return None if res is None else res[0]

    # ---- continual interface on (N, C, V) frames (module boundary: converts layouts) ------------
    def _ensure_state(self, n, v, device):
        p = _round4(n * v)
        if self._state is None or self._state.p != p or self._state.y.device != device or not self._state.owns_xin:
            self.bind_state(p, device)
        return self._state

    def forward_step(self, x_t, update_state=True):
        self._require_eval()
        native.require_device_f32(x_t, "CoSpatioTemporalBlock frame")
        n, c, v = x_t.shape
        if c != self.in_channels:
            raise RuntimeError(f"expected (N, {self.in_channels}, V) frame, got {tuple(x_t.shape)}")
        st = self._ensure_state(n, v, x_t.device)
        keep = (st.s, st.e)
        frame_to_slot(x_t, st.xin[st.s % st.xin.shape[0]])
        slot = self.engine_step(n, v)
        if not update_state:       # one step only touches ring slots that are older than every window: counters suffice
            st.s, st.e = keep
        return None if slot is None else slot_to_frame(st.out[slot], n, v)

    def forward_steps(self, x, pad_end=False, update_state=True):
        n, c, t, v = x.shape
        if not update_state:
            st = self._ensure_state(n, v, x.device)
            with _snapshot([st.y, st.out, st.xin], lambda: list(st._ctr), lambda ctr: st._ctr.__setitem__(slice(None), ctr)):
                return self.forward_steps(x, pad_end, True)
        outs = [o for o in (self.forward_step(x[:, :, i].contiguous()) for i in range(t)) if o is not None]
        if pad_end:
            st = self._state
            for _ in range(self.padding):
                slot = self.engine_step(n, v, flush=True)
                if slot is not None:
                    outs.append(slot_to_frame(st.out[slot], n, v))
        return torch.stack(outs, dim=2)


STEP_PRECISIONS = ("f32", "bf16x3")


def set_step_precision(module: nn.Module, precision: str = "f32") -> nn.Module:
    """Select the arithmetic of the continual temporal STEP of every ``CoSpatioTemporalBlock`` below ``module``.

    "f32" (default): the exact-fp32 step kernels.  "bf16x3" (opt-in): the blocks ``_use_split_step`` covers (128 and 256
    channels, no split-K) launch ``csk_tcn_step_bf16x3`` -- fp32 operands as three bf16 pieces, six piece products per fp32
    product on the bf16 matrix pipe, fp32 accumulation, the identity residual exact fp32 (csrc/step_split.hip); every other
    block keeps its exact kernel.  fp32-GRADE, never reported as fp32.  Independent of ``set_precision`` (the clip kernels):
    with the step precision "bf16x3" stepping is allowed whatever the clip precision is.  A ``CoStGcn`` in the mode runs on
    the Python engine (no native plan).  Built for plain graph convs: a model whose blocks carry another graph-conv module
    (CoAGcn, CoSTr) is refused.  Everything is validated before anything is switched; bound continual state is dropped, as
    on a shape change.  Call it on the model (or on a block that is stepped on its own), not on a single block inside a
    ``CoStGcn``: the model owns the slab and the plan of its blocks and would not see the switch."""
    if precision not in STEP_PRECISIONS:
        raise ValueError(f"step precision must be one of {STEP_PRECISIONS}, got {precision!r}")
    blocks_ = [m for m in module.modules() if isinstance(m, CoSpatioTemporalBlock)]
    if not blocks_:
        raise ValueError("no CoSpatioTemporalBlock below this module: nothing to set")
    if precision != "f32" and any(type(m.gcn) is not GraphConvolution for m in blocks_):
        raise NotImplementedError("step precision 'bf16x3' is built for blocks with the plain GraphConvolution (CoStGcn); "
                                  "the model is unchanged")
    models = [m for m in module.modules() if isinstance(m, CoStGcn)]
    if precision != "f32" and any(m.unpadded for m in models):
        raise NotImplementedError("step precision 'bf16x3' is not built for the unpadded '*' models (CoStGcnMod); the model is unchanged")
    owned = {id(b) for m in models for b in m.layers.values()}
    for m in models:                # as set_max_cycle: the native plan goes now, the slab is re-bound (zeroed) on the next step
        m._destroy_plan()
        m._n = None
    for m in blocks_:
        m.step_precision = precision
        m.refold()
        if id(m) not in owned:      # a block stepped on its own: its state is bound again on its next step
            m._state = None
    return module


def co_geometry(c_in=3, unpadded=False):
    """receptive_field / padding / stride of the ten-block stack (read from co.Sequential at base.py:86-97), from the layer
    table: (153, 76, 4) for the padded table, (81, 0, 1) for the "*" table (``unpadded``: stride 1, temporal padding 0)."""
    r, p, s = 1, 0, 1
    block_padding = MOD_TEMPORAL_PADDING if unpadded else 4
    for (_, _, st, _) in layer_table(c_in, unpadded):
        r += 8 * s
        p += block_padding * s
        s *= st
    return r, p, s


class CoStGcn(NativePlan, SlabRings, StreamReset, StreamMove, StreamPrime, ClipAsSteps, InputChain, _Folded):
    """CoST-GCN: models/cost_gcn/cost_gcn.py:21-41 + CoModelBase (models/base.py:68-227) without the Ride shell.

    ``forward_step(x_t: (N, C, V, M))`` -> logits (N, classes) on the steps where the whole stack (10 blocks,
    total stride 4) and the temporal average pool emit, else None.  ``forward_steps(x: (N, C, T, V, M))``
    -> (N, classes, n_predictions).  ``forward(x)`` = clip mode of CoModelBase.forward (base.py:166-181).
    state_dict keys equal the reference's (``layers.layerK.0.1.gcn...``); a regular StGcn state_dict loads too
    (what ``map_state_dict`` does in the reference, base.py:200-224).  This class binds the state slab and steps on it; the
    native plan (co_plan.py: NativePlan), the one inventory of the slab's rings (co_rings.py: SlabRings), the per-stream reset (co_reset.py: StreamReset), moving streams between slabs
    (co_migrate.py: StreamMove), priming streams from buffered history with one clip pass (co_prime.py: StreamPrime), a stored clip at the
    steps' arithmetic (co_clip.py: ClipAsSteps -- ``forward_clip_as_steps``) are base classes.  The input pre-passes are the
    stage objects of ``STAGES`` (input_stage.py: InputChain), all off by default and run in that order in front of every cycle:
    the keypoint intake (keypoints.py; with it the model is fed ``(N, P, V, 3)`` keypoint frames / ``(N, T, P, V, 3)`` clips in the
    place of the channel-first ones named here), the pre-normalisation of raw joint frames (prenorm.py) and the input modality
    (modality.py: bone / motion frames derived from the joint frames).
    """

    # False: drive every launch from Python (same kernels, same results).  Read on every cycle: both engines step on the one
    # counter buffer, so they may alternate; the plan itself is built when the slab is bound with the attribute set
    use_native_plan = True
    unpadded = False        # CoStGcnMod: the "*" layer table (stride 1, block padding 0 -> delay 8 per block)
    STAGES = (KeypointIntake, PreNorm, InputModality)   # the input pre-passes, in order (the NTU intake has no step form)

    def __init__(self, graph_A, input_shape=(3, 300, 25, 2), num_classes=60, pool_size=-1, pool_padding=-1,
                 CoGraphConv=CoGraphConvolution):
        super().__init__()
        (c_in, t, v, m) = input_shape
        self.input_shape, self.num_classes = tuple(input_shape), num_classes
        self._init_stages()
        self.data_bn = nn.BatchNorm1d(m * c_in * v)
        convs = [CoGraphConvolution if f is None else f for f in per_layer(CoGraphConv)]   # one factory, or ten (None: default)
        self.layers = nn.ModuleDict(OrderedDict(
            (f"layer{i + 1}", CoSpatioTemporalBlock(ci, co, graph_A, stride=s, residual=r,
                                                    padding=MOD_TEMPORAL_PADDING if self.unpadded else "equal", CoGraphConv=convs[i]))
            for i, (ci, co, s, r) in enumerate(layer_table(c_in, self.unpadded))))
        self.fc = nn.Linear(256, num_classes)
        init_weights(self.data_bn, bs=1)
        init_weights(self.fc, bs=num_classes)
        self.receptive_field, self.padding, self.stride = co_geometry(c_in, self.unpadded)
        self.delay = self.padding
        if pool_size == -1:                                                   # base.py:86-90
            pool_size = math.ceil((t - self.receptive_field + 2 * self.padding + 1) / self.stride)
        if pool_padding == -1:                                                # base.py:92-96
            pool_padding = pool_size - math.ceil((t - self.receptive_field + self.padding + 1) / self.stride)
        self.pool_size, self.pool_padding = pool_size, max(0, pool_padding)
        self._n = None
        self._flushed = False
        self._forget_resets()

    # ---- weights ---------------------------------------------------------------------------------
    def map_state_dict(self, state_dict, strict=True):
        """Regular-layout keys -> this module's (reference Co) layout (models/base.py:200-224).  A state dict
        that already holds every key of this module is returned unchanged, as in the reference."""
        own = nn.Module.state_dict(self).keys()
        if not (own - state_dict.keys()):
            return state_dict

        def short(k):
            return k.replace("0.1.", "").replace("0.0.residual", "residual")
        short2long = {short(k): k for k in own}
        return OrderedDict((short2long[k], v) for k, v in state_dict.items() if strict or k in short2long)

    def map_loaded_weights(self, file, loaded_state_dict):
        """Hook called by the checkpoint loader (models/base.py:226-227; weights.load_pretrained here)."""
        return self.map_state_dict(loaded_state_dict)

    def _fold(self):
        s, t = fold.fold_data_bn({k: v for k, v in nn.Module.state_dict(self).items() if k.startswith("data_bn.")})
        return dict(scale=s, shift=t)

    def _watched(self):
        return [self.data_bn]

    # ---- state slab --------------------------------------------------------------------------------
    _blocks = property(lambda self: list(self.layers.values()), doc="the ten blocks in stack order")

    def _bind(self, n, device):
        c_in, _, v, m = self.input_shape
        p = _round4(n * m * v)
        mc = self.max_cycle
        xin = torch.zeros((in_slots(mc), c_in, p), device=device, dtype=torch.float32)
        self._xin0, self._p, self._n = xin, p, n
        # frames one launch of block i can receive / emit: max_cycle input frames / cumulative temporal stride.  They size
        # the rings (y: 8 + max_in, output = next block's input history: 4 + its max_in) and the split-K scratch, which is
        # ONE buffer sized by its largest user (launches of a model are stream-ordered)
        blks, recv, emits, cum = self._blocks, [], [], 1
        for blk in blks:
            recv.append(max(1, mc // cum))
            cum *= blk.stride
            emits.append(max(1, mc // cum))
        need = max(blk.scratch_floats(p, emits[i], recv[i]) for i, blk in enumerate(blks))
        if need * 4 > self.LATENCY_SCRATCH_CAP_BYTES:
            raise RuntimeError(
                f"set_latency_mode({self.layers.layer1.split_k}) on a slab of {n} streams needs a {need * 4 / 1e9:.2f} GB split-K "
                f"scratch (cap {self.LATENCY_SCRATCH_CAP_BYTES / 1e9:.1f} GB): the latency mode splits every K loop into up to 32 "
                "channel ranges whatever the slab size -- it is meant for a handful of streams; use the default mode "
                "(set_latency_mode(0)) for slabs that fill the GPU")
        self._scratch = torch.empty((need,), device=device, dtype=torch.float32) if need else None
        # THE stepping position, in the layout csk_co_plan_cycle takes (include/cskel.h): {frames, features, then (received,
        # emitted) per block}.  _frames / _feats and every block's s / e are views of it; nothing else holds a counter
        self._ctr = (ctypes.c_int64 * 22)()
        for i, blk in enumerate(blks):
            out_slots = in_slots(recv[i + 1]) if i < 9 else max(4, emits[i])
            xin = blk.bind_state(p, device, xin, max_emit=emits[i], scratch=self._scratch, max_in=recv[i], out_slots=out_slots,
                                 counters=(ctypes.c_int64 * 2).from_buffer(self._ctr, 16 * (i + 1))).out
        self._pool_ring = torch.zeros((self.pool_size, n, 256), device=device, dtype=torch.float32)
        self._pooled = torch.empty((n, 256), device=device, dtype=torch.float32)
        self._bound_rings = self._describe_rings(True)
        self._flushed = False
        self._forget_resets()
        for stage in self._record_stages:
            stage.bind(n, device, mc)
        self._build_plan(device)

    def _slab(self):
        return None if self._n is None else (self._n, self._xin0.device, self.max_cycle, self._frames)

    _frames = _counter(0, "input frames received")
    _feats = _counter(1, "layer-10 emissions the head has taken")

    max_cycle = MAX_CYCLE   # frames ONE forward_cycle may carry: sizes the state rings (set_max_cycle)

    def set_max_cycle(self, frames: int = MAX_CYCLE):
        """Largest launch cycle (1..8 frames) the state slab is sized for.  A block's rings hold the 8-frame window of its
        temporal conv / the 4-frame residual lag PLUS the frames one launch brings (``max_cycle`` / cumulative stride), so the
        default of 8 pays for cycles the 4-frames-per-launch mode never issues: 5.75 GB at 1024 NTU streams against 4.65 GB with
        ``set_max_cycle(4)`` (SURVEY 8a's per-frame minimum: 3.25 GB).  Results do not depend on it (a frame lives in slot
        s % depth, the kernels take the depths as arguments).  Takes effect from a clean state (the slab is re-bound)."""
        if not isinstance(frames, int) or not 1 <= frames <= MAX_CYCLE:
            raise ValueError(f"max_cycle must be an integer in [1, {MAX_CYCLE}]")
        self.max_cycle = frames
        self._n = None

    LATENCY_SCRATCH_CAP_BYTES = 1 << 30   # split-K scratch above which binding a slab in latency mode is refused

    def set_latency_mode(self, split_k: int = 8):
        """Few-stream operation (one camera, a handful of streams): the TCN step of a block then holds one workgroup
        per tile that walks all 9*C/8 K-chunks alone (123 us at C = 256).  With ``split_k`` > 1 such launches cut the
        channel axis into up to ``split_k`` ranges computed by separate workgroups and summed in a fixed order
        (csk_tcn_step_f32 ``ksplit``); launches that fill the GPU anyway are left alone.  Results differ from the
        default by fp32 summation order only.  Takes effect from a clean state (the slab is re-bound).  (Replaying a
        frame's launches from hipGraphs was built and measured slower than eager launches on ROCm 7.2 -- 0.41 vs 0.36 ms per
        frame-step -- and removed: profiles/HISTORY.md.)  The split factor does not shrink with the slab (a stream's bits must
        not depend on its neighbours), so the scratch grows with it: binding a slab whose scratch would exceed
        LATENCY_SCRATCH_CAP_BYTES (1 GiB: about 300 NTU streams at split_k = 8) raises instead of silently running slower than the default mode."""
        for blk in self._blocks:
            blk.split_k = int(split_k)
        self._n = None

    def state_bytes(self):
        """Persistent continual state (input ring, per-block rings, pooling window; the state of the input pre-passes: previous
        frame and flags of a motion modality, latched rotations and flags of the pre-normalisation)."""
        return (4 * sum(ring.tensor.numel() for ring in self._rings())
                + sum(t.numel() * t.element_size() for t in self._stage_tensors()))

    def scratch_bytes(self):
        """Transient scratch, not state: the split-K partial sums (shared by the blocks that split their K loop) and, for
        adaptive graph convs, the per-skeleton-frame adjacencies of a launch (shared by all blocks); for every input pre-pass
        that is on, the frames of a cycle behind it."""
        buffers = [self._scratch, self.__dict__.get("_agcn_adj")] + [stage.scratch for stage in self.stages]
        return 4 * sum(t.numel() for t in buffers if t is not None)

    def clean_state(self):
        if self._n is not None:
            for ring in self._rings():
                ring.tensor.zero_()
            for stage in self._record_stages:
                stage.clean()
            self._set_counters([0] * 22)
            self._flushed = False
            self._forget_resets()

    # ---- stepping ------------------------------------------------------------------------------------
    def _cycle(self, frames, peek=False):
        """Advance by 1..MAX_CYCLE frames (list of (N, C, V, M) tensors): data_bn, ten blocks, head.
        Returns (slot, n_feat, logits): layer 10's emissions of this cycle (first output-ring slot, count;
        (None, 0) if none) and the list of predictions.  While reset streams warm up (``reset_streams``) the cycle must not
        cross a multiple of the total stride, and what the not-yet-live blocks wrote for them is zeroed after its launches;
        ``peek``: the caller puts the counters back (one step, update_state=False) -- the next real step rewrites and scrubs
        the same slots, so a peek does neither.  The engines step on ``_stage_frames(frames)``: the frames themselves with
        every input pre-pass off, else what the chain makes of them (a peek runs it with ``update=False``: the stages' state
        stays).  The frames are checked in the layout the model is fed (``_fed``): channel-first against ``input_shape``, or
        that of the intake that is on."""
        self._require_eval()
        frames = list(frames)
        if not 1 <= len(frames) <= self.max_cycle:
            raise ValueError(f"a cycle holds 1..{self.max_cycle} frames (set_max_cycle), got {len(frames)}")
        x0 = frames[0]
        n = self._fed().check_frames(frames)
        if self._n != n or self._xin0.device != x0.device:           # clean_state_on_shape_change (base.py:161-164)
            self._bind(n, x0.device)
        if any(b.precision != "f32" and b.step_precision == "f32" for b in self.layers.values()):
            raise NotImplementedError("precision 'bf16x3' covers the clip kernels only (DESIGN.md section 4): step with the default "
                                      "precision -- set_precision(model, 'f32')")
        if self._flushed:
            raise RuntimeError("the state was flushed by forward_steps(pad_end=True): the end padding has consumed ring slots "
                               "and advanced the blocks past the input frame count; call clean_state() before stepping on")
        engine = self._plan_cycle if self.use_native_plan and self.__dict__.get("_plan") else self._python_cycle
        if not self._cohorts or peek:              # nothing warms: the cycle is the one that runs without any reset
            return engine(self._stage_frames(frames, update=not peek))
        self._check_cycle_while_warming(len(frames))
        before = self._counters()
        res = engine(self._stage_frames(frames))
        self._scrub_cycle(before)
        return res

    # ---- update_state=False (base.py:183-190 hand the flag through to co.Sequential) -------------------
    def _counters(self):
        return list(self._ctr)

    def _set_counters(self, snap):
        self._ctr[:] = snap

    def _position(self):
        """The stepping position beyond the tensors: counters, the flushed mark and the streams' ages (co_reset.py)."""
        return self._counters(), self._flushed, list(self._reset_at), dict(self._cohorts)

    def _set_position(self, position):
        self._ctr[:], self._flushed, self._reset_at, self._cohorts = position

    def _state_tensors(self):
        return [ring.tensor for ring in self._rings()] + [self._pooled] + self._stage_tensors()

    def _stage_tensors(self):
        """The per-stream state of the input pre-passes, in record order."""
        return [t for stage in self._record_stages for t in stage.tensors()]

    def _ensure_bound(self, x_t):
        native.require_device_f32(x_t, "CoStGcn frame")
        if self._n != x_t.shape[0] or self._xin0.device != x_t.device:
            self._bind(x_t.shape[0], x_t.device)

    def _python_cycle(self, frames):
        """Same protocol driven from Python (any graph-conv module with a ``stage`` method)."""
        n, c, v, m = frames[0].shape
        ops = self._packed_ops(frames[0].device)
        # reshape1 + data_bn + reshape2 (base.py:73-82) of the cycle's frames straight into the channel-major input ring
        depth = self._xin0.shape[0]
        srcs = (ctypes.c_void_p * len(frames))(*[x_t.data_ptr() for x_t in frames])
        dsts = (ctypes.c_void_p * len(frames))(*[self._xin0[(self._frames + f) % depth].data_ptr() for f in range(len(frames))])
        rc = native.lib().csk_input_norm_frames_f32(srcs, dsts, len(frames), native.ptr(ops["scale"]), native.ptr(ops["shift"]),
                                                    n, c, v, m, self._p, native.stream_of(frames[0]))
        native.check(rc, "csk_input_norm_frames_f32")
        self._frames += len(frames)
        r = len(frames)
        for blk in self._blocks:
            res = blk.engine_advance(r, n * m, v)
            if res is None:
                return None, 0, []
            r = res[1]
        return res[0], res[1], self._emit_heads(res[0], res[1], n)

    def _emit_heads(self, slot0, n_emit, n):
        """Head steps of ``n_emit`` layer-10 emissions from output-ring slot ``slot0`` on (None: zero features) -> the logits released."""
        depth = self.layers["layer10"]._state.out.shape[0]
        outs = (self._head_step(None if slot0 is None else (slot0 + j) % depth, n) for j in range(n_emit))
        return [o for o in outs if o is not None]

    def _head_step(self, slot, n):
        """spatial_pool -> co.AvgPool1d window -> co.Linear (base.py:84-101)."""
        _, _, v, m = self.input_shape
        st10 = self.layers["layer10"]._state
        head = self._feats % self.pool_size
        self._feats += 1
        emit = self._feats >= self.pool_size - self.pool_padding
        count = min(self._feats, self.pool_size)
        logits = torch.empty((n, self.num_classes), device=st10.out.device, dtype=torch.float32) if emit else None
        # slot None: end padding of the pooling window (a zero feature enters it)
        native.check(native.lib().csk_co_head_step_f32(
            native.ptr(st10.out[slot]) if slot is not None else None, native.ptr(self._pool_ring), native.ptr(self._pooled),
            native.ptr(self.fc.weight.detach()), native.ptr(self.fc.bias.detach()), native.ptr(logits), n, 256, m * v, self._p,
            self.pool_size, head, count, int(emit), self.num_classes, native.stream_of(st10.out)), "csk_co_head_step_f32")
        return logits

    def features_step(self, x_t):
        """(N, C, V, M) frame -> slot of layer 10's output ring holding this step's emission, or None
        (the head advances as well, exactly as in ``forward_step``)."""
        return self._cycle([x_t])[0]

    def forward_step(self, x_t, update_state=True):
        """CoModelBase.forward_step (base.py:183-185): logits (N, classes) on predicting steps, else None.
        ``update_state=False`` computes the step without advancing: a single step only overwrites ring slots whose
        content has left every window (and the oldest entry of the pooling window, which the next real step replaces
        as well), so restoring the counters restores the state."""
        if update_state:
            outs = self._cycle([x_t])[2]
        else:
            self._ensure_bound(x_t)
            with _snapshot((), self._counters, self._set_counters):
                outs = self._cycle([x_t], peek=True)[2]
        return outs[-1] if outs else None

    def forward_cycle(self, frames):
        """Up to MAX_CYCLE (8) consecutive frames in one go (list of (N, C, V, M) tensors): same results as calling
        ``forward_step`` on each, with len(frames)x fewer and larger launches (4 = one stride cycle of the stack).  Returns the list of logits emitted."""
        return self._cycle(frames)[2]

    def forward_steps(self, x, pad_end=False, update_state=True):
        """(N, C, T, V, M) -> (N, classes, n_predictions) (empty last dim if nothing was emitted).  ``pad_end`` is handed
        through to every module as in the reference (base.py:187-190): each block's temporal conv is flushed with its
        ``padding`` zero frames, first block first, so that the stack emits what the clip stack computes for the same
        frames, and the temporal average pool is flushed with ``pool_padding`` zero features."""
        axis = self.time_axis           # 2; 1 for the (N, T, P, V, 3) clips of the keypoint intake
        if not update_state:
            self._ensure_bound(x.select(axis, 0).contiguous())
            with _snapshot(self._state_tensors(), self._position, self._set_position):
                return self.forward_steps(x, pad_end, True)
        if pad_end and self._cohorts:
            raise RuntimeError("forward_steps(pad_end=True) while reset streams are warming up (streams_ready()): the end padding "
                               "flushes every block for every stream, live for the stream or not")
        outs = []
        for t in range(x.shape[axis]):
            o = self.forward_step(x.select(axis, t).contiguous())
            if o is not None:
                outs.append(o)
        if pad_end and x.shape[axis] > 0:
            outs += self._flush()
            self._flushed = True                   # stepping on needs clean_state() (see _flush)
        if not outs:
            return torch.empty((x.shape[0], self.num_classes, 0), device=x.device)
        return torch.stack(outs, dim=2)

    def _flush(self):
        """End padding of the whole model (``pad_end=True``): returns the predictions it releases.  Runs on the Python
        engine.  The flush ends the sequence: it zeroes y-ring slots and advances the per-block counters by their padding
        while the input frame count stays, so the rings no longer line up with ``frames % depth`` -- the model is marked
        flushed and the next step raises until ``clean_state()`` (continual-inference's own end padding does not save state
        either; a caller that wants to go on uses ``update_state=False``, which runs the flush on a snapshot)."""
        n = self._n
        _, _, v, m = self.input_shape
        outs, blks = [], self._blocks
        for i, blk in enumerate(blks):
            left = blk.padding
            while left:                                # at most max_in frames per launch (ring depths); order is unchanged
                r = min(left, blk._state.max_in)
                left -= r
                res = blk.engine_advance(r, n * m, v, flush=True)
                for below in blks[i + 1:]:             # what block i released travels down the rest of the stack
                    if res is None:
                        break
                    res = below.engine_advance(res[1], n * m, v)
                if res is not None:
                    outs += self._emit_heads(res[0], res[1], n)
        return outs + self._emit_heads(None, self.pool_padding, n)     # co.AvgPool1d end padding: zero features enter the window

    def forward(self, x, forward_mode="clip"):
        """CoModelBase.forward (base.py:166-181).  'clip': whole-clip computation with the continual head
        (zero-padded temporal average pool, first window); 'frame': stepping with a fresh state."""
        self._require_eval()
        if forward_mode == "frame":
            self.clean_state()
            ret = self.forward_steps(x)
            return ret[:, :, 0]
        x = self._intake_clip(x)        # the intake that is on (input_stage.py); none: x itself
        n, c, t, v, m = x.shape
        h = self._clip_features(x)                                        # (N*M, 256, T', V)
        tp = h.shape[2]
        # spatial_pool per frame, then AvgPool1d(pool_size, stride 1, padding) output index 0:
        # frames [0, pool_size - pool_padding) summed, divided by pool_size (zeros included)
        take = min(tp, self.pool_size - self.pool_padding)
        feat = torch.empty((n, 256), device=x.device, dtype=torch.float32)
        hs = h[:, :, :take].contiguous()
        rc = native.lib().csk_pool_scaled_f32(native.ptr(hs), native.ptr(feat), n, m, 256, take * v,
                                              take / self.pool_size, native.stream_of(x))
        native.check(rc, "csk_pool_scaled_f32")
        return self._fc(feat)

    def _fc(self, feat):
        """co.Linear on pooled features, (..., 256) -> (..., classes): the last launch of every clip-side continual head."""
        logits = torch.empty(feat.shape[:-1] + (self.num_classes,), device=feat.device, dtype=torch.float32)
        rc = native.lib().csk_fc_f32(native.ptr(feat), native.ptr(self.fc.weight.detach()), native.ptr(self.fc.bias.detach()),
                                     native.ptr(logits), feat.numel() // 256, 256, self.num_classes, native.stream_of(feat))
        native.check(rc, "csk_fc_f32")
        return logits

    def _clip_features(self, x):
        native.require_device_f32(x, "CoStGcn input")
        return self._clip_stack(self._prepare_clip(x))      # the pre-passes on channel-first input, clip form; all off: x itself

    def _clip_stack(self, x):
        """Input norm and the ten clip blocks on the derived frames ``x`` (N, C, T, V, M) -> (N*M, 256, T', V)."""
        # SpatioTemporalBlock.forward by name: the clip computation, whatever a continual block's own ``forward`` is
        return self._through_blocks(self.input_norm(x), SpatioTemporalBlock.forward)

    def warm_up(self, n, device, frames=None):
        """Feed ``receptive_field - padding - 1`` random frames (models/base.py:144-159) so that the next
        frame produces layer-10 output."""
        self.clean_state()
        frames = self.receptive_field - self.padding - 1 if frames is None else frames
        for _ in range(frames):
            self.forward_step(self._fed().random_frame(n, device))


class CoStGcnMod(CoStGcn):
    """CoST-GCN*: models/cost_gcn_mod/cost_gcn_mod.py:29-40 -- ten continual blocks with ``padding=0`` and stride 1 (``window_size`` is
    accepted by the block and unused, as in the reference).  Geometry from the table (``co_geometry(c, unpadded=True)``): receptive
    field 81, padding 0, stride 1, delay 0; the defaults of base.py:86-97 then give pool_size = T - 80 and pool_padding = 0.  Every
    block waits k - 1 = 8 frames (delay 8 against CoStGcn's 4), so the first layer-10 feature comes with frame 80 and every
    frame after it yields one: emission s is StGcnMod's clip feature frame s - 80.  state_dict keys are the reference's; a StGcnMod
    state dict loads through ``map_state_dict``.  Steps on the native plan (per-layer delay: csk_co_plan_set_delays) and on the
    Python engine; stream reset, input modality and pre-normalisation are CoStGcn's (generic in delay and stride).  The latency
    mode and the "bf16x3" precisions are not built for it: they raise."""

    unpadded = True

    def __init__(self, graph_A, input_shape=(3, 300, 25, 2), num_classes=60, pool_size=-1, pool_padding=-1,
                 CoGraphConv=CoGraphConvolution):
        super().__init__(graph_A, input_shape, num_classes, pool_size, pool_padding, CoGraphConv=CoGraphConv)

    def set_latency_mode(self, split_k: int = 8):
        raise NotImplementedError("the latency mode is not built for the unpadded '*' models; the model is unchanged")

    def _clip_features(self, x):
        if any(b.precision != "f32" for b in self._blocks):
            raise NotImplementedError("precision 'bf16x3' is not built for the unpadded '*' models: set_precision(model, 'f32')")
        if x.dim() != 5 or x.shape[2] < self.receptive_field:
            raise ValueError(f"{type(self).__name__}'s clip forward needs T >= {self.receptive_field} frames, got {tuple(x.shape)}")
        return super()._clip_features(x)
