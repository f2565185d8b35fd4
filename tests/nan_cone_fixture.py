"""NaN containment: where ONE NaN inside an operand has to show in the output, and where it must not.  Test infrastructure,
CPU only: tests/test_nan_cone_fixture_cpu.py proves the masks on the host, tests/test_gpu_nan_containment.py holds every kernel
family to them.

For a case -- an operation, a shape and a poisoned element x[n0, c0, t0, v0] -- the fixture gives two boolean masks over the
output, both from the plain fp64 reference of the operation (oracle/stgcn_oracle.py), never from the code under test:

``must``  the structural dependency cone.  The reference runs on a one-hot input at the poisoned element with every weight 1,
          every bias and running mean 0 and every BN scale 1 (running_var = 1 - eps), so no two terms can cancel; every term is
          then >= 0 and the reference's ReLU is the identity on that run (it is "taken away" by the operands, not by editing the
          reference).  The sparse graph conv uses the case's OWN adjacency pattern, whose zeros the ELL kernels skip; the adaptive
          graph conv an all-ones adjacency.  ``must = out > 0``.
``may``   the same cone with an all-ones adjacency: the reference's dense matmul gives 0 x NaN = NaN for every joint of the frame.

A kernel may neither swallow (isnan(got) must contain ``must``) nor leak (isnan(got) must lie in ``may``); every mask is False
in all other sequences.

The attention of the CLIP form of the adaptive graph conv is a product of two embeddings of the same input, summed over all
frames of the sequence: a one-hot probe cannot see it (the other factor is zero), NaN does (NaN x 0).  ``_attention_taint``
restates that rule -- a product is tainted where either factor is -- and the CPU test holds the result to the really poisoned
reference.

The two Winograd transforms of csrc/tcn_wino.hip are restated here in fp64 (``wino_s1`` / ``wino_s2``; checked against the
direct conv on the CPU) together with the frames a poisoned input frame reaches through them (``wino_frames``).  FINDING: the
F(2,3) stride-1 form keeps the direct cone (Y0 uses d0..d2, Y1 d1..d3); the stride-2 polyphase form does NOT: its 2-tap groups
(even taps 6, 8 and odd taps 1, 3 / 5, 7) are F(2,3) with a ZERO third tap, so Y0 = g0 d0 + g1 d1 + 0 d2 in exact arithmetic but
b0 = d0 - d2, b1 = d1 + d2, b2 = d2 - d1 all carry d2: input frames 2 t + 5 and 2 t + 6 reach the even output frame t, which the
direct window 2 t - 4 .. 2 t + 4 does not hold.  The extra outputs are in the SAME sequence, one output frame earlier than the
direct cone starts.  ``may`` is NOT widened for it: ``BlockCase.may_wino_s2`` is a separate, named mask that only the launches
which the route model says run tcn_stage_wino_s2_kernel are held to, and ``extra_wino_s2`` is the difference, asserted on the
CPU to be exactly those frames."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch
import torch.nn.functional as F

import _bootstrap
from oracle import stgcn_oracle as o
from tests.helpers import randomise_unit_

pkg = _bootstrap.load()

T = 20                      # frames of every clip case: a 16-frame tile and a ragged one
BN_ONE = 1.0 - o.BN_EPS     # running_var that makes the BN scale exactly 1 / sqrt(1) = 1


def graph_A(v):
    return (o.ntu_graph() if v == 25 else o.kinetics_graph()).astype(np.float32)


# ---- poison positions ------------------------------------------------------------------------------------------------------
# (sequence, channel, frame, joint) with -1 = the last one and "mid" sequence 1 (neither first nor last at 3 and 4 sequences).
# Between them: first and last frame, both sides of the 16-frame seam, joints 0 and V - 1, channel 0 and the last, sequence 1.
POSITIONS = (
    (1, 0, 0, 0), (0, -1, 15, -1), (-1, 0, 16, 7), (1, -1, 19, -1), (-1, -1, 15, 0), (0, 0, 16, 12),
)


def _resolve(pos, n, c, t, v):
    return tuple(p % d for p, d in zip(pos, (n, c, t, v)))


# ---- clip blocks -----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class BlockCase:
    ci: int
    co: int
    stride: int
    res: str               # none | identity | conv
    V: int
    N: int
    pad: int               # -1: the padded block; 0: the unpadded "*" block
    poison: Tuple[int, int, int, int]

    @property
    def id(self):
        star = "*" if self.pad == 0 else ""
        return f"{self.ci}-{self.co}{star}-s{self.stride}-{self.res}-V{self.V}-N{self.N}-p{'.'.join(map(str, self.poison))}"

    @property
    def geometry(self):
        return (self.ci, self.co, self.stride, self.res, self.V, self.N, self.pad)

    @property
    def t_out(self):
        t = T if self.pad < 0 else T - 8
        return (t - 1) // self.stride + 1

    @property
    def out_shape(self):
        return (self.N, self.co, self.t_out, self.V)


LAYER_ROWS = ((3, 64, 1, "none"), (64, 64, 1, "identity"), (64, 128, 2, "conv"), (128, 128, 1, "identity"), (128, 256, 2, "conv"),
              (256, 256, 1, "identity"))
# the unpadded "*" rows (stride 1 throughout): the identity rows run csk_tcn_stage_wino_valid_f32, the conv rows
# csk_tcn_stage_wino_valid_res_f32 with wino_valid_res set
MOD_ROWS = ((64, 64, 1, "identity"), (64, 128, 1, "conv"), (128, 128, 1, "identity"), (128, 256, 1, "conv"), (256, 256, 1, "identity"))


def _block_cases(rows, pad, first, shapes=((25, 3), (18, 4))):
    out, k = [], first
    for ci, co, stride, res in rows:
        for V, N in shapes:
            for j in range(3):
                out.append(BlockCase(ci, co, stride, res, V, N, pad, _resolve(POSITIONS[(k + j) % len(POSITIONS)], N, ci, T, V)))
            k += 1
    return out


BLOCK_CASES = _block_cases(LAYER_ROWS, -1, 0)
MOD_CASES = _block_cases(MOD_ROWS, 0, 1)
# 6 sequences: gcn16_kernel picks F = 4 / 2 / 1 by the sequence count (multiple of 4 / of 2 / odd); run with the 16-wide families forced
SIX_CASES = _block_cases(((64, 64, 1, "identity"), (64, 128, 2, "conv")), -1, 2, ((25, 6), (18, 6)))


def make_block(geometry, seed=5):
    """the module of a geometry with randomised O(1) weights (host, eval) -- the GPU test moves it to the device, the CPU test
    hands its state dict to the fp64 reference"""
    ci, co, stride, res, V, N, pad = geometry
    blk = pkg.SpatioTemporalBlock(ci, co, graph_A(V), stride, res != "none", temporal_padding=pad).eval()
    randomise_unit_(blk, seed + ci + co)
    return blk


def _sd64(module):
    return {k: v.detach().double().clone() for k, v in module.state_dict().items()}


def probe_sd(sd, adjacency):
    """the state dict of the probe: weights 1, biases and running means 0, BN scale 1, graph_attn 1 (plain graph conv: a
    multiplicative mask) or 0 (adaptive: added to A), A = ``adjacency`` ("own": the non-zeros of the case's A; "ones")"""
    adaptive = any(".a_conv." in k or k.startswith("a_conv.") for k in sd)
    out = {}
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            out[k] = v
        elif k.endswith(".A") or k == "A":
            out[k] = torch.ones_like(v) if adjacency == "ones" else (v != 0).double()
        elif k.endswith("graph_attn"):
            out[k] = torch.zeros_like(v) if adaptive else torch.ones_like(v)
        elif k.endswith("running_var"):
            out[k] = torch.full_like(v, BN_ONE)
        elif k.endswith("running_mean") or k.endswith("bias"):
            out[k] = torch.zeros_like(v)
        else:
            out[k] = torch.ones_like(v)              # conv weights, BN weights
    return out


def one_hot(shape, idx):
    x = torch.zeros(shape, dtype=torch.float64)
    x[idx] = 1.0
    return x


@functools.lru_cache(maxsize=None)
def _block_sd(geometry):
    return _sd64(make_block(geometry))


def block_reference(case, x, sd=None):
    """o.st_block in fp64 on x (N, ci, T, V)"""
    sd = _block_sd(case.geometry) if sd is None else sd
    with torch.no_grad():
        return o.st_block(x.double(), sd, "", case.stride, case.res != "none", case.pad)


@functools.lru_cache(maxsize=None)
def block_masks(case):
    """(must, may) of a clip block case"""
    x = one_hot((case.N, case.ci, T, case.V), case.poison)
    sd = _block_sd(case.geometry)
    must = block_reference(case, x, probe_sd(sd, "own")) > 0
    may = block_reference(case, x, probe_sd(sd, "ones")) > 0
    return must, may


def block_input(case, clean=False):
    """the case's input (fp32, host): seeded by the geometry, so the three poison positions of a geometry share the clean run"""
    g = torch.Generator().manual_seed(17 + case.ci + 3 * case.V)
    x = torch.rand((case.N, case.ci, T, case.V), generator=g)
    if not clean:
        x[case.poison] = float("nan")
    return x


# ---- the Winograd transforms of csrc/tcn_wino.hip, restated --------------------------------------------------------------
WINO_BT = ((1, 0, -1, 0), (0, 1, 1, 0), (0, -1, 1, 0), (0, 1, 0, -1))       # b = BT d
WINO_AT = ((1, 1, 1, 0), (0, 1, -1, -1))                                      # (Y0, Y1) = AT m
WINO_G = ((1, 0, 0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0, 0, 1))           # u = G g
# stride 1: three 3-tap groups; sample i of pair j of group g is frame 2 j - pad + 3 g + i
# stride 2 (polyphase): (first tap, taps, frame of sample 0 relative to 4 j - 4, frames per sample); taps of a group are 2 apart
S2_GROUPS = ((0, 3, 0, 2), (6, 2, 6, 2), (1, 2, 1, 2), (5, 2, 5, 2))


def _groups(stride, pad):
    """per group: (tap indices (None: the zero third tap), frame of sample i of pair j = a j + b + c i, samples read)"""
    if stride == 1:
        return [((3 * g, 3 * g + 1, 3 * g + 2), (2, 3 * g - pad, 1), 4) for g in range(3)]
    out = []
    for first, ntaps, f0, per in S2_GROUPS:
        taps = tuple(first + 2 * i if i < ntaps else None for i in range(3))
        out.append((taps, (4, f0 - 4, per), 4 if ntaps == 3 else 3))       # a 2-tap group has no product m3: d3 is never read
    return out


def wino(y, w, stride, pad=4):
    """the Winograd form in fp64: y (C, T, V), w (Co, C, 9) -> (Co, T_out, V)"""
    c, t, v = y.shape
    t_out = (t + 2 * pad - 9) // stride + 1
    npair = (t_out + 1) // 2
    lo, hi = 16, 16 + t
    yp = np.zeros((c, t + 40, v))
    yp[:, lo:hi] = y
    out = np.zeros((w.shape[0], 2 * npair, v))
    for taps, (a, b, cc), nread in _groups(stride, pad):
        g = np.stack([w[:, :, r] if r is not None else np.zeros_like(w[:, :, 0]) for r in taps], 0)          # (3, Co, C)
        u = np.einsum("pr,roc->poc", np.array(WINO_G), g)
        d = [yp[:, lo + b + cc * i: lo + b + cc * i + a * npair: a] if i < nread else None for i in range(4)]
        for p in range(nread if nread == 3 else 4):
            bp = sum(WINO_BT[p][i] * d[i] for i in range(4) if WINO_BT[p][i] and d[i] is not None)
            m = np.einsum("oc,cjv->ojv", u[p], bp)
            for e in (0, 1):
                if WINO_AT[e][p]:
                    out[:, e::2] += WINO_AT[e][p] * m
    return out[:, :t_out]


def direct(y, w, stride, pad=4):
    with torch.no_grad():
        return F.conv2d(torch.from_numpy(y)[None], torch.from_numpy(w)[..., None], stride=(stride, 1), padding=(pad, 0))[0].numpy()


def wino_frames(t0, t_in, stride, pad=4):
    """output frames that input frame t0 reaches THROUGH THE TRANSFORMS: sample i enters product p where BT[p][i] != 0 and the
    group has that product, product p enters frame e of the pair where AT[e][p] != 0 -- whatever the weights are"""
    t_out = (t_in + 2 * pad - 9) // stride + 1
    hit = set()
    for j in range((t_out + 1) // 2):
        for taps, (a, b, cc), nread in _groups(stride, pad):
            for i in range(nread):
                if a * j + b + cc * i != t0:
                    continue
                for p in range(nread if nread == 3 else 4):
                    for e in (0, 1):
                        if WINO_BT[p][i] and WINO_AT[e][p] and 2 * j + e < t_out:
                            hit.add(2 * j + e)
    return sorted(hit)


def direct_frames(t0, t_in, stride, pad=4):
    t_out = (t_in + 2 * pad - 9) // stride + 1
    return [t for t in range(t_out) if 0 <= t0 - (stride * t - pad) < 9]


def may_wino_s2(case):
    """``may`` of a stride-2 block whose temporal conv runs tcn_stage_wino_s2_kernel: the direct cone plus the frames of
    ``wino_frames`` at the joints the graph conv may reach (the module docstring's finding)"""
    assert case.stride == 2 and case.pad < 0
    must, may = block_masks(case)
    n0, _, t0, _ = case.poison
    joints = may[n0].any(0).any(0)                                  # (V,) joints of the frame the dense graph conv reaches
    out = may.clone()
    for t in wino_frames(t0, T, 2):
        out[n0, :, t, :] |= joints[None, :]
    return out


# ---- adaptive graph conv ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class AgcnCase:
    ci: int
    co: int
    V: int
    N: int
    form: str              # clip: attention over the whole sequence | frame: per frame (the steps' arithmetic)
    poison: Tuple[int, int, int, int]
    frames: int = T        # the step form: skeletons of a channel-major ring slot (the "frames" of a launch of ``stage``)

    @property
    def id(self):
        return f"agcn-{self.form}-{self.ci}-{self.co}-V{self.V}-N{self.N}-p{'.'.join(map(str, self.poison))}"

    @property
    def geometry(self):
        return (self.ci, self.co, self.V, self.N)

    @property
    def out_shape(self):
        return (self.N, self.co, self.frames, self.V)


def _agcn_cases():
    out, k = [], 2
    for form in ("clip", "frame"):
        for ci, co in ((3, 64), (64, 64), (64, 128), (128, 256)):
            for V, N in ((18, 4), (25, 3)):
                for j in range(3):
                    out.append(AgcnCase(ci, co, V, N, form, _resolve(POSITIONS[(k + j) % len(POSITIONS)], N, ci, T, V)))
                k += 1
    return out


AGCN_CASES = _agcn_cases()
# ``AdaptiveGraphConvolution.stage`` as the continual engine calls it: N ring slots of 7 skeletons each (a ragged tile that holds
# several streams); the reference sees a slot as a sequence and a skeleton as a frame.  Poison: (slot, channel, skeleton, joint).
AGCN_STEP_CASES = tuple(AgcnCase(ci, co, V, 2, "frame", _resolve(pos, 2, ci, 7, V), frames=7)
                        for (ci, co, V), pos in zip(((3, 64, 18), (64, 64, 25), (64, 128, 18), (128, 256, 25)),
                                                    ((1, -1, 3, -1), (0, 0, 6, 0), (1, 0, 0, 7), (-1, -1, 3, 12))))


def make_agcn(geometry, seed=9):
    ci, co, V, N = geometry
    g = pkg.AdaptiveGraphConvolution(ci, co, graph_A(V)).eval()
    randomise_unit_(g, seed + ci, attn_scale=1.0 / V)
    return g


@functools.lru_cache(maxsize=None)
def _agcn_sd(geometry):
    return _sd64(make_agcn(geometry))


def agcn_reference(case, x, sd=None):
    """o.adaptive_graph_conv in fp64; form "frame": every frame as a sample of its own with T = 1 (what a step computes)"""
    sd = _agcn_sd(case.geometry) if sd is None else sd
    x = x.double()
    n, c, t, v = x.shape
    with torch.no_grad():
        if case.form == "clip":
            return o.adaptive_graph_conv(x, sd, "")
        xf = x.permute(0, 2, 1, 3).reshape(n * t, c, 1, v)
        return o.adaptive_graph_conv(xf, sd, "").view(n, t, -1, v).permute(0, 2, 1, 3).contiguous()


def _attention_taint(case):
    """(N, V, V) bool: entries of the softmaxed attention of the clip form that the poisoned element reaches.  logits[v, w] =
    sum_k a1[v, k] a2[k, w] with a1, a2 1 x 1 convs of x: a product is tainted where either factor is, so row v0 (a1) and column
    v0 (a2) of the poisoned sequence; the softmax over dim -2 normalises every column by all of its entries, and row v0 puts a
    tainted entry into every column -- the whole matrix of that sequence."""
    n0, _, _, v0 = case.poison
    logits = torch.zeros((case.N, case.V, case.V), dtype=torch.bool)
    logits[n0, v0, :] = True
    logits[n0, :, v0] = True
    return logits.any(1, keepdim=True).expand(-1, case.V, -1).clone()     # a column with a tainted entry is tainted whole


@functools.lru_cache(maxsize=None)
def agcn_masks(case):
    x = one_hot((case.N, case.ci, case.frames, case.V), case.poison)
    sd = probe_sd(_agcn_sd(case.geometry), "ones")
    linear = agcn_reference(case, x, sd) > 0                              # x enters x @ attn: its frame, every joint
    if case.form == "clip":
        cols = _attention_taint(case).any(1)                              # (N, V): columns w of a tainted attention
        linear = linear | cols[:, None, None, :].expand(case.out_shape)   # xa[n, :, t, w] for EVERY frame t
    return linear, linear.clone()                                         # dense: must == may


def agcn_input(case, clean=False):
    g = torch.Generator().manual_seed(23 + case.ci + 3 * case.V)
    x = torch.rand((case.N, case.ci, case.frames, case.V), generator=g)
    if not clean:
        x[case.poison] = float("nan")
    return x


# ---- head --------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class HeadCase:
    N: int
    M: int
    V: int
    t: int
    classes: int
    poison: Tuple[int, int, int, int]       # (sequence n * M + m, channel, frame, joint) of the features

    @property
    def id(self):
        return f"head-N{self.N}-M{self.M}-V{self.V}-t{self.t}-k{self.classes}-p{'.'.join(map(str, self.poison))}"


HEAD_C = 256
HEAD_CASES = (HeadCase(3, 1, 25, 5, 60, (1, 0, 0, 0)), HeadCase(2, 2, 18, 5, 400, (1, 255, 4, 17)),
              HeadCase(3, 2, 25, 3, 60, (2, 128, 1, 24)), HeadCase(4, 1, 18, 20, 7, (2, 255, 16, 0)))


def head_operands(case):
    g = torch.Generator().manual_seed(case.classes + case.V)
    h = torch.rand((case.N * case.M, HEAD_C, case.t, case.V), generator=g)
    w = torch.randn((case.classes, HEAD_C), generator=g) / 16.0
    b = torch.rand((case.classes,), generator=g) - 0.5
    return h, w, b


def head_reference(case, h, w, b):
    with torch.no_grad():
        return o.stgcn_head(h.double(), {"fc.weight": w.double(), "fc.bias": b.double()}, case.N, case.M)


def head_masks(case):
    h = one_hot((case.N * case.M, HEAD_C, case.t, case.V), case.poison)
    must = head_reference(case, h, torch.ones((case.classes, HEAD_C)), torch.zeros(case.classes)) > 0
    return must, must.clone()


# the continual head (csk_co_head_step_f32 step by step, csk_co_head_clip_f32 over the whole clip): spatial mean of a feature
# frame -> zero-initialised pooling window with a fixed divisor -> FC, a prediction from the (window - padding)-th frame on
@dataclass(frozen=True)
class CoHeadCase:
    N: int
    M: int
    V: int
    steps: int             # layer-10 feature frames fed
    window: int            # pool_size
    padding: int           # pool_padding
    classes: int
    poison: Tuple[int, int, int, int]       # (sequence n * M + m, channel, feature frame, joint)

    @property
    def id(self):
        return f"cohead-N{self.N}-M{self.M}-V{self.V}-s{self.steps}-w{self.window}.{self.padding}-k{self.classes}-p{'.'.join(map(str, self.poison))}"

    @property
    def first_entry(self):
        return max(0, self.window - self.padding - 1)


# the NaN in the first frame (a partly filled window), in the middle (it slides out: the head recovers) and in the last frame;
# N = 5, M = 2 as the model cases; a window of 1 (no memory) and windows longer than the frames that follow
CO_HEAD_CASES = (CoHeadCase(5, 2, 25, 9, 3, 1, 60, (5, 0, 0, 0)), CoHeadCase(5, 2, 18, 9, 4, 0, 400, (4, 255, 4, 17)),
                 CoHeadCase(3, 1, 25, 7, 1, 0, 60, (1, 128, 3, 24)), CoHeadCase(3, 2, 18, 8, 5, 2, 7, (2, 255, 7, 0)))


class _HeadOracle(o.CoStGcnOracle):
    """the head of CoStGcnOracle alone (its own pooling window and FC, untouched): ``forward_step`` is fed the layer-10 feature
    frame itself, laid out as a model input (N, C, V, M)"""

    def __init__(self, w, b, pool_size, pool_padding):
        self.sd, self.blocks = {"fc.weight": w, "fc.bias": b}, []
        self.pool_size, self.pool_padding = pool_size, pool_padding
        self.clean_state()

    def features_step(self, x_t):
        n, c, v, m = x_t.shape
        return x_t.permute(0, 3, 1, 2).reshape(n * m, c, v)


def co_head_operands(case):
    """(features (steps, N * M, C, V), fc weight, fc bias), fp32 host"""
    g = torch.Generator().manual_seed(case.classes + case.V + case.window)
    h = torch.rand((case.steps, case.N * case.M, HEAD_C, case.V), generator=g)
    w = torch.randn((case.classes, HEAD_C), generator=g) / 16.0
    b = torch.rand((case.classes,), generator=g) - 0.5
    return h, w, b


def co_head_poisoned(case, h):
    s, c, t, v = case.poison
    h = h.clone()
    h[t, s, c, v] = float("nan")
    return h


def co_head_reference(case, h, w, b):
    """(n_pred, N, classes) fp64: CoStGcnOracle's head stepped through the feature frames"""
    orc = _HeadOracle(w.double(), b.double(), case.window, case.padding)
    out = []
    with torch.no_grad():
        for t in range(case.steps):
            x_t = h[t].double().view(case.N, case.M, HEAD_C, case.V).permute(0, 2, 3, 1)
            y = orc.forward_step(x_t)
            if y is not None:
                out.append(y)
    return torch.stack(out, 0)


def co_head_masks(case):
    h = torch.zeros((case.steps, case.N * case.M, HEAD_C, case.V), dtype=torch.float64)
    s, c, t, v = case.poison
    h[t, s, c, v] = 1.0
    must = co_head_reference(case, h, torch.ones((case.classes, HEAD_C)), torch.zeros(case.classes)) > 0
    return must, must.clone()


# ---- the continual model -------------------------------------------------------------------------------------------------------
CO_STREAMS, CO_POISONED, CO_M = 5, 2, 2
CO_POOL = (3, 1)            # pool_size, pool_padding: small, so that the head's window forgets within three emissions
CO_POISON_FRAME = 6         # the step whose frame holds the NaN: inside the first 8-frame cycle, off a stride-4 boundary
CO_FRAMES = 176             # receptive field 153 from frame 6 on, + the pooling window, rounded up to whole 8-frame cycles


def co_frames(v, clean=False, poison=(1, 3, 1)):
    """(CO_FRAMES, CO_STREAMS, 3, V, M) frames (fp32, host); the NaN at stream CO_POISONED, step CO_POISON_FRAME, ``poison`` =
    (channel, joint, person)"""
    g = torch.Generator().manual_seed(31 + v)
    x = torch.rand((CO_FRAMES, CO_STREAMS, 3, v, CO_M), generator=g)
    if not clean:
        c, j, m = poison
        x[CO_POISON_FRAME, CO_POISONED, c, j, m] = float("nan")
    return x


def co_oracle_nan(sd, frames, gcn=o.graph_conv):
    """isnan of the fp64 oracle's logits, step by step, for ONE stream's frames (T, 3, V, M): a list with None where the oracle
    emits nothing, else a (classes,) bool tensor.  CoStGcnOracle, same frames; streams do not interact in the reference (eval-mode
    BN), so the poisoned stream alone decides."""
    sd = {k: v.double() for k, v in sd.items()}
    orc = o.CoStGcnOracle(sd, 3, *CO_POOL)
    for b in orc.blocks:
        b.gcn = gcn
    out = []
    with torch.no_grad():
        for t in range(frames.shape[0]):
            y = orc.forward_step(frames[t][None].double())
            out.append(None if y is None else torch.isnan(y[0]))
    return out


# ---- ties in the fused ranking ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class TieCase:
    n: int
    classes: int
    streams: int
    method: str
    steps: int             # 0: 2-D predictions

    @property
    def id(self):
        return f"n{self.n}-k{self.classes}-s{self.streams}-{self.method}-{'3d' if self.steps else '2d'}"


TIE_CASES = tuple(TieCase(n, k, s, m, st) for (n, k) in ((37, 60), (130, 400)) for s in (1, 2, 3, 4) for m in ("add", "maximum")
                  for st in (0, 3))


def tie_operands(case):
    """integer-valued logits in [-2, 2] and targets: classes tie all the time; the first samples' targets are class 0 and the
    last class"""
    rng = np.random.default_rng(case.n + case.classes + 7 * case.streams + case.steps)
    shape = (case.n, case.classes, case.steps) if case.steps else (case.n, case.classes)
    preds = [rng.integers(-2, 3, shape).astype(np.float32) for _ in range(case.streams)]
    targets = rng.integers(0, case.classes, case.n)
    targets[0], targets[1], targets[2], targets[3] = 0, case.classes - 1, 0, case.classes - 1
    return preds, targets


def tie_reference(case, preds, targets):
    """(fused, rank, top-1/3/5) of the definition"""
    fused = o.fuse_preds(preds, np.add if case.method == "add" else np.maximum)
    rank = (fused > fused[np.arange(case.n), targets][:, None]).sum(1)
    return fused, rank, o.topk_accuracies_np(fused, targets)


def tie_fraction(fused, targets):
    """fraction of samples in which another class scores exactly the target's score"""
    tv = fused[np.arange(len(targets)), targets][:, None]
    return float((((fused == tv).sum(1) - 1) > 0).mean())
