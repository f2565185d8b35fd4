"""Step cases for csk_tcn_step_bf16x3 (csrc/step_split.hip), derived from the clip fixtures of tests/split_fixture.py.

A ``tcn`` ``Case`` of T frames becomes a ring whose slots are the fixture's y frames, channel-major; the emissions are the
clip outputs t with a full window, 4 <= s t <= T - 5 for stride s (no zero padding takes part): emission j is clip output
t_lo + j, its newest window frame is s (t_lo + j) + 4, its residual frame s (t_lo + j).  T = s (n_emit - 1) + 9 gives exactly
n_emit such outputs.  Reference, tolerance and admissibility are the clip case's own (``split_fixture.analyse``: the fp64
product, tol = D / 2 with D the smallest shift a lost second-order product causes), cut to those outputs.

Every derived case has ONE product pair -- one hot (tap slot, 16-channel chunk) of the temporal conv (residual none or
identity, which adds no product), or one hot chunk of the 1 x 1 residual conv on its own -- so "a piece product lost in one hot
pair" is "that piece product lost", the loss D is defined by.  (With two equal pairs a product lost in one of them moves an
output by D / 2 = the tolerance: the rule cannot tell it from rounding.)

``MIXED`` are the cases in which a hot temporal pair and a hot chunk of the 1 x 1 residual conv (64 residual channels: two
32-channel stages of phase 2) meet in ONE accumulator.  They are two-pair cases, so what they pin at D / 2 is what the clip
fixture's two-pair cases pin: a second-order product lost in BOTH phases, or a phase lost, dropped or added twice -- not a
product lost in one of the two pairs, which the one-pair cases above catch for either phase on its own.

``WIDE`` are launches large enough for the cost model to pick the wide tiles (25 column blocks for an odd emission count, 13
for an even one): a P = 100 case repeated ``reps`` times along the position axis.  Positions are independent, so every
repetition has the small case's fp64 reference, and its bits must be those of the small launch, which a narrow tile computes.
"""
from dataclasses import dataclass

import torch

from tests import split_fixture as sf

CO = 128


@dataclass(frozen=True)
class StepCase:
    case: sf.Case
    n_emit: int
    wrap: bool                  # the 9-frame window of the first emission wraps the end of the ring (and the output ring wraps)

    @property
    def id(self):
        return f"{self.case.id}-e{self.n_emit}{'-wrap' if self.wrap else ''}"

    @property
    def t_lo(self):
        return -(-4 // self.case.stride)

    @property
    def P(self):
        return (self.case.N * self.case.V + 3) // 4 * 4


def _case(ci, stride, res, V, N, n_emit, pick):
    T = stride * (n_emit - 1) + 9
    nch = sf.n_chunks(ci)
    if res == "conv":           # the residual conv alone: input of 24 channels (two chunks, the second one padded)
        c_res = 24
        return sf.Case("tcn", ci, CO, V, T, N, stride, res="conv", res_hot=(pick % sf.n_chunks(c_res),), c_res=c_res)
    hot = ((pick % 9, (pick // 9) % nch),)
    return sf.Case("tcn", ci, CO, V, T, N, stride, hot=hot, res=res, c_res=CO if res == "ident" else 0)


def build_cases():
    cs, pick = [], 0
    # the matrix: C_in {16, 24 (padded chunk), 64} x stride {1, 2} x residual {none, identity, conv} x V {25, 18} x n_emit {1, 4}
    # (the identity residual exists for stride 1 only); N: P = 100 (V = 25) / 72 (V = 18) = one partial tile for every n_emit;
    # every other case N = 17 / 25: P = 428 / 452 = several tiles with a partial last one
    for ci in (16, 24, 64):
        for stride in (1, 2):
            for res in ("none", "ident", "conv"):
                if res == "ident" and stride != 1:
                    continue
                for V in (25, 18):
                    for n_emit in (1, 4):
                        big = pick % 2 == 1
                        N = (17 if V == 25 else 25) if big else 4
                        cs.append(StepCase(_case(ci, stride, res, V, N, n_emit, 5 * pick + 2), n_emit, wrap=pick % 3 != 0))
                        pick += 1
    # one-hot sweep: every (tap slot, chunk) of every C_in and stride, alternating n_emit and wrap
    for ci in (16, 24, 64):
        for stride in (1, 2):
            for c in range(sf.n_chunks(ci)):
                for s in range(9):
                    n_emit = 4 if (s + c) % 2 else 1
                    case = sf.Case("tcn", ci, CO, 25, stride * (n_emit - 1) + 9, 4, stride, hot=((s, c),))
                    sc = StepCase(case, n_emit, wrap=s % 2 == 0)
                    if sc.id not in {c.id for c in cs}:                  # (the matrix may hold it already)
                        cs.append(sc)
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids), "duplicate case"
    return cs


CASES = build_cases()


def build_mixed():
    cs = []
    for ci, stride, n_emit, hot, rhot, wrap in ((64, 1, 1, (3, 1), 0, False), (64, 1, 4, (8, 3), 3, True), (24, 2, 1, (5, 1), 2, True),
                                                (64, 2, 4, (0, 2), 1, False), (16, 2, 4, (6, 0), 3, True), (24, 1, 4, (4, 0), 2, False)):
        case = sf.Case("tcn", ci, CO, 25, stride * (n_emit - 1) + 9, 4, stride, hot=(hot,), res="conv", res_hot=(rhot,), c_res=64)
        cs.append(StepCase(case, n_emit, wrap))
    return cs


MIXED = build_mixed()


@dataclass(frozen=True)
class WideCase:
    sc: StepCase                # P = 100
    reps: int                   # the launch has 100 reps positions
    blocks: int                 # column blocks of the tile the launch must pick (csk_tcn_step_bf16x3_tile)

    @property
    def id(self):
        return f"{self.sc.id}-x{self.reps}-nb{self.blocks}"

    @property
    def P(self):
        return self.sc.P * self.reps


def build_wide():
    """every wide instantiation (25 blocks x 1 emission at either stride, 13 x 2 at stride 1 and at stride 2), each with a
    partial last tile: 40100 = 100 x 400 + 100, 12500 = 31 x 400 + 100, 10000 = 48 x 208 + 16"""
    w = []
    for ci, stride, res, n_emit, reps, blocks, pick in ((16, 1, "none", 1, 401, 25, 7), (64, 1, "ident", 3, 125, 25, 30), (24, 2, "conv", 3, 125, 25, 1),
                                                        (64, 2, "none", 3, 125, 25, 22), (64, 1, "ident", 4, 100, 13, 17), (24, 1, "conv", 4, 100, 13, 0),
                                                        (16, 2, "none", 4, 100, 13, 5), (64, 2, "conv", 4, 100, 13, 1), (64, 2, "none", 4, 100, 13, 33)):
        w.append(WideCase(StepCase(_case(ci, stride, res, 25, 4, n_emit, pick), n_emit, wrap=pick % 2 == 1), reps, blocks))
    return w


WIDE = build_wide()


def analyse(sc, fx):
    """the clip case's analysis cut to the emissions of the step case (same D, tol and bound)"""
    an = sf.analyse(fx)
    lo, hi = sc.t_lo, sc.t_lo + sc.n_emit
    assert sc.case.stride * lo >= 4 and sc.case.stride * (hi - 1) <= sc.case.T - 5 and hi <= an["want"].shape[2]
    out = dict(an)
    for k in ("want", "six", "nz", "with_terms"):
        out[k] = an[k][:, :, lo:hi]
    out["drops"] = {k: v[:, :, lo:hi] for k, v in an["drops"].items()}
    return out


def pair_products(sc, fx):
    """-> {(weight piece, activation piece): fp64 product of the case's one hot pair, cut to the emissions} for the six products"""
    case = sc.case
    assert len(case.hot) + len(case.res_hot) == 1 and not case.dense
    g = fx.groups[0] if case.hot else fx.groups[1]
    lo, hi = sc.t_lo, sc.t_lo + sc.n_emit
    return {pq: sf.conv64(g.wp[pq[0]], g.xp[pq[1]], g.stride, g.pad)[:, :, lo:hi] for pq in sf.SIX}


def channel_major(x, P):
    """(N, C, T, V) -> [T][C][P] frames, position n V + v; positions past N V are NaN (they reach padding outputs only)"""
    n, c, t, v = x.shape
    out = torch.full((t, c, P), float("nan"), dtype=torch.float32)
    out[:, :, : n * v] = x.permute(2, 1, 0, 3).reshape(t, c, n * v)
    return out


def ring_of(frames, slots, rot):
    """frames [T][C][P] -> ring [slots][C][P] with frame f in slot (f + rot) % slots; slots that hold no frame are NaN"""
    t = frames.shape[0]
    ring = torch.full((slots,) + tuple(frames.shape[1:]), float("nan"), dtype=torch.float32)
    for f in range(t):
        ring[(f + rot) % slots] = frames[f]
    return ring


def launch_geometry(sc):
    """ring depths and slot arguments of the launch: frame f of the y ring in slot (f + rot) % slots"""
    case, s = sc.case, sc.case.stride
    slots = case.T + 2
    first = s * sc.t_lo - 4                                     # oldest window frame of emission 0
    rot = (slots - 3 - first) % slots if sc.wrap else 1         # wrap: window slots slots - 3 .. slots - 1, 0 .. 5
    head = (s * sc.t_lo + 4 + rot) % slots
    xs = case.T + 1
    xrot = (xs - 1 - s * sc.t_lo) % xs if sc.wrap else 0        # wrap: the first residual frame in the last slot
    out_slots = sc.n_emit + 1
    return dict(slots=slots, rot=rot, head=head, x_slots=xs, x_rot=xrot, x_slot0=(s * sc.t_lo + xrot) % xs,
                out_slots=out_slots, out_slot0=out_slots - 1 if sc.wrap else 0)
