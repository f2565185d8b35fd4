"""Cases, operands, references and the launchers' kernel selection for tests/test_gpu_tcn_wino.py and
tests/test_tcn_wino_fixture_cpu.py: the Winograd F(2, 3) clip temporal convs of csrc/tcn_wino.hip behind csk_tcn_stage_wino_f32
("id"), csk_tcn_stage_wino_ext_f32 ("ext"), csk_tcn_stage_wino_valid_f32 ("valid") and csk_tcn_stage_wino_valid_res_f32
("valid_res").

select() restates, from tcn_stage_wino_launch with its table of forms (WINO_FORMS) and wino_pick_mw, what a
launch gets: whether the gate takes it, the template instantiation, the grid, and per column tile the pair range and the staging
form.  Nothing is read from csrc.  reachable() sweeps select() over the launchers' domain.

Four tiers of operands.  exact: small integers -- the weight transform has entries 0, +-1/2, 1, so the image is in halves, the
input transform is exact, and every product and partial sum is a multiple of 1/2 below 2^23 (partial_sum_bound): a launch must
equal the fp64 conv BIT FOR BIT, ReLU off so that both signs are compared.  route_*: unique integer ids under one-hot weights,
every output names the input element it came from.  round / cancel: random fp32 operands against the fp64 definition under the
derived bound gamma(n) S (error_bound).  NaN: nan_mask() is what the algorithm -- not the definition's window -- lets one NaN reach.

model() is the Winograd computation written out step by step on the host (work-item decode, tiles, staged span with zero fill,
channel tail, groups, transforms, phantom frame, residual phases) and takes one seeded defect at a time."""
import functools
from typing import NamedTuple, Tuple

import torch
import torch.nn.functional as F

import _bootstrap

fold = _bootstrap.load().fold          # host-side weight images and the group tables; no device code

N_SEG = 3
ACT = 3            # activations and block inputs: integers in [-ACT, ACT]
W_MAX = 4          # conv weights: integers in [-W_MAX, W_MAX], odd ones included (half-integer image entries)
W_RES = 3          # residual conv weights
BIAS = 8
RES_MODE = {"none": 0, "identity": 1, "conv": 2}
CPAD, MROWS, KC = 16, 64, 8
WMT, WNT = 64, 128                     # rows / pair columns of the wide workgroup tile
ENTRY_KW = {"id": "w_wino", "ext": "w_wino_ext", "valid": "w_wino_valid", "valid_res": "w_wino_valid_res"}

# F(2, 3), points 0, 1, -1, inf: input transform (rows: points, columns: the four samples d0 .. d3) and output transform (rows:
# the pair's two frames, columns: the four accumulator sets); the weight transform is fold.WINO_G
WINO_BT = ((1, 0, -1, 0), (0, 1, 1, 0), (0, -1, 1, 0), (0, 1, 0, -1))
WINO_AT = ((1, 1, 1, 0), (0, 1, -1, -1))


def _ceil_to(a, b):
    return (a + b - 1) // b * b


# ------------------------------------------------------------------------------------------------------------------------------
# the launchers' selection, restated
# ------------------------------------------------------------------------------------------------------------------------------
class Tile(NamedTuple):
    ja: int            # first and last output pair of the column tile
    jb: int
    interior: bool     # staged span inside the sequence: 16-byte staging; otherwise element-wise with zero fill
    front: bool        # the span starts in front of the sequence
    back: bool         # the span (rounded up to whole 16-byte vectors) ends behind it
    cols: int          # live pair columns


class Sel(NamedTuple):
    reject: str = ""                   # why the gate answers -2 ("" = the Winograd kernel runs)
    kernel: str = ""                   # "tcn_stage_wino_kernel" | "tcn_stage_wino_s2_kernel"
    vt: int = 0
    res: bool = False                  # identity residual in the epilogue (RES)
    mw: int = 0
    valid: bool = False
    resconv: bool = False              # conv-residual phase (RESCONV / CONV of the stride-2 kernel)
    stride: int = 1
    t_out: int = 0
    qp: int = 0                        # pair columns per sequence
    qtiles: int = 0
    mtiles: int = 0
    grid: int = 0
    tiles: Tuple[Tile, ...] = ()
    partial_last: bool = False         # the last column tile has clamped lanes
    phantom: bool = False              # odd output length: the last pair's second frame is computed and not stored
    chunks: int = 0                    # 8-channel chunks of the main loop
    res_chunks: int = 0                # ... of the residual phase

    @property
    def key(self):
        """the template instantiation"""
        if self.kernel == "tcn_stage_wino_s2_kernel":
            return (self.kernel, self.vt, self.resconv, self.mw)
        return (self.kernel, self.vt, self.res, self.mw, self.valid, self.resconv)

    @property
    def nt(self):
        return WNT // self.mw

    @property
    def mt(self):
        return WMT * self.mw


def pick_mw(qp, c_out, stride):
    """wino_pick_mw without the diagnostic override"""
    if c_out % (2 * WMT):
        return 1
    if stride == 2:
        return 2
    return 2 if 16 * _ceil_to(qp, WNT // 2) <= 15 * _ceil_to(qp, WNT) else 1


def gate(entry, c, c_out, c_res, t_in, V, k, stride, pad, res_mode, res_off, t_res, n_seg=N_SEG, has_x=True, has_wres=True):
    """every -2 condition of the three launchers, as a reason ("" = taken)"""
    none, ident, conv = (res_mode == m for m in (0, 1, 2))
    if entry == "ext" and stride not in (1, 2):
        return "ext: stride is neither 1 nor 2"
    s2 = entry == "ext" and stride == 2
    want = (2 if s2 else 1, 0 if entry in ("valid", "valid_res") else 4)
    if k != 9 or (stride, pad) != want:
        return f"k, stride, pad are not 9, {want[0]}, {want[1]}"
    if entry in ("valid", "valid_res") and t_in < 9:
        return "valid: fewer than 9 input frames"
    if entry == "id":
        if not ident or res_off != 0 or not has_x or c_res != c_out or t_res != t_in:
            return "id: not the identity residual over the same frames"
    elif entry == "ext" and not s2:
        if not none:
            return "ext stride 1: a residual"
    elif s2:
        if res_off != 0:
            return "ext stride 2: residual offset"
        if not conv and not none:
            return "ext stride 2: identity residual"
        if conv and (not has_x or not has_wres or c_res < 1 or t_res != t_in):
            return "ext stride 2: conv residual operands"
    elif entry == "valid":
        if not ident and not none:
            return "valid: conv residual"
        if ident and (res_off != 4 or not has_x or c_res != c_out or t_res != t_in):
            return "valid: not the centred identity residual"
    elif entry == "valid_res":
        if not conv:
            return "valid_res: not a conv residual"
        if res_off != 4 or not has_x or not has_wres or c_res < CPAD or c_res % CPAD or t_res != t_in:
            return "valid_res: residual not centred or c_res not whole 16-channel chunks"
    else:
        raise KeyError(entry)
    if V not in (25, 18) or c_out % WMT or c < 1 or n_seg < 1 or t_in < 1:
        return "V is neither 25 nor 18, or c_out is no multiple of 64"
    if t_in * V >= 1 << 26:
        return "32-bit lane offsets"
    return ""


def select(entry, c, c_out, c_res, t_in, V, k=9, stride=1, pad=4, res_mode=0, res_off=0, t_res=None, n_seg=N_SEG, **kw):
    t_res = t_in if t_res is None else t_res
    why = gate(entry, c, c_out, c_res, t_in, V, k, stride, pad, res_mode, res_off, t_res, n_seg, **kw)
    if why:
        return Sel(reject=why)
    valid, s2 = entry in ("valid", "valid_res"), stride == 2
    t_out = t_in - 8 if valid else (t_in - 1) // 2 + 1 if s2 else t_in
    qp = (t_out + 1) // 2 * V
    mw = pick_mw(qp, c_out, stride)
    nt = WNT // mw
    qtiles, mtiles = (qp + nt - 1) // nt, c_out // (WMT * mw)
    if qtiles * mtiles * n_seg >= 1 << 31:
        return Sel(reject="grid")
    tv, tiles = t_in * V, []
    for q0 in range(0, qp, nt):
        qend = min(q0 + nt, qp)
        ja, jb = q0 // V, (qend - 1) // V
        if s2:
            fa, span = 4 * ja - 4, (4 * (jb - ja) + 11) * V
        else:
            fa, span = (2 * ja if valid else 2 * ja - 4), (2 * (jb - ja) + 10) * V
        back = fa * V + 4 * ((span + 3) // 4) > tv
        tiles.append(Tile(ja, jb, fa >= 0 and not back, fa < 0, back, qend - q0))
    conv = res_mode == 2
    return Sel("", "tcn_stage_wino_s2_kernel" if s2 else "tcn_stage_wino_kernel", V, res_mode == 1, mw, valid, conv, stride, t_out,
               qp, qtiles, mtiles, qtiles * mtiles * n_seg, tuple(tiles), qp % nt != 0, t_out % 2 == 1, _ceil_to(c, CPAD) // KC,
               ((c_res + KC - 1) // KC if conv else 0))


@functools.lru_cache(maxsize=None)
def reachable():
    """every instantiation select() answers over the launchers' domain: the four entries, joints the gate takes and not, row
    counts with one, two and three 64-row tiles and a ragged one, every residual form, lengths either side of the tall / wide choice"""
    keys = set()
    for entry in ENTRY_KW:
        for V in (18, 20, 25):
            for c_out in (40, 64, 128, 192):
                for stride in (1, 2, 3):
                    for pad, res_off in ((4, 0), (0, 4), (0, 0)):
                        for res_mode, c_res in ((0, 0), (1, c_out), (2, 16), (2, 24)):
                            for t_in in range(1, 48):
                                s = select(entry, 12, c_out, c_res, t_in, V, 9, stride, pad, res_mode, res_off)
                                if not s.reject:
                                    keys.add(s.key)
    return frozenset(keys)


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    group: str
    seed: int
    entry: str         # "id" | "ext" | "valid" | "valid_res"
    c: int
    co: int
    t: int
    v: int
    stride: int = 1
    res: str = "none"
    c_res: int = 0
    relu: int = 0
    n: int = N_SEG
    tier: str = "exact"    # "exact" | "route_tap" | "route_res" | "round" | "cancel"
    tap: int = 0

    @property
    def pad(self):
        return 0 if self.entry in ("valid", "valid_res") else 4

    @property
    def res_off(self):
        return 4 if self.pad == 0 and self.res != "none" else 0

    @property
    def t_out(self):
        return (self.t + 2 * self.pad - 9) // self.stride + 1

    @property
    def name(self):
        s = f"{self.group}#{self.seed} {self.entry} c{self.c} co{self.co} T{self.t} V{self.v} s{self.stride} {self.res}"
        s += f"{self.c_res}" if self.res == "conv" else ""
        s += " relu" if self.relu else ""
        s += f" n{self.n}" if self.n != N_SEG else ""
        s += f" {self.tier}" + (f"{self.tap}" if self.tier == "route_tap" else "") if self.tier != "exact" else ""
        return s


def sel_of(case):
    return select(case.entry, case.c, case.co, case.c_res, case.t, case.v, 9, case.stride, case.pad, RES_MODE[case.res],
                  case.res_off, n_seg=case.n)


def kernel_of(case):
    """the three kernels of the tables: "s1" padded stride 1, "valid", "s2" """
    return "s2" if case.stride == 2 else "valid" if case.pad == 0 else "s1"


GROUPS = {}


def _add(group, entry, c, co, t, v, **kw):
    if kw.get("res") == "identity":
        kw["c_res"] = co
    table = GROUPS.setdefault(group, [])
    table.append(Case(group, len(table), entry, c, co, t, v, **kw))


# frames per (kernel, MW, V): lengths whose tiles are front border / interior / back border with a partial last tile, in both
# parities of the output length (test_tcn_wino_fixture_cpu.py shows that they are; found by sweeping select())
S1_T = {(1, 25): (26, 27), (1, 18): (34, 35), (2, 25): (21, 22), (2, 18): (20, 29)}
S1_WIDE128_T = {25: (9, 26, 35), 18: (13, 22)}                # c_out = 128 where the wide shape is picked: two row tiles
VALID_T = {(1, 25): (20, 21), (1, 18): (25, 26), (2, 25): (19, 20), (2, 18): (23, 24)}
S2_T = {(1, 25): (48, 49), (1, 18): (64, 65), (2, 25): (28, 29), (2, 18): (36, 37)}
CS = (3, 12, 16, 20, 64)
CRES_S2 = (3, 8, 24, 64)
CRES_V = (16, 48)


def _build():
    for v in (25, 18):
        # ---- padded stride 1: identity residual ("id") and none ("ext")
        for mw, cos in ((1, (64, 192)), (2, (128,))):
            g = f"s1-V{v}-mw{mw}"
            i = 0
            for co in cos:
                for t in S1_T[mw, v] + (1, 2, 3):
                    _add(g, "id", CS[i % 5], co, t, v, res="identity")
                    _add(g, "ext", CS[(i + 2) % 5], co, t, v)
                    i += 1
            _add(g, "id", 20, cos[0], S1_T[mw, v][0], v, res="identity", relu=1)
            _add(g, "ext", 12, cos[0], S1_T[mw, v][1], v, relu=1)
        g = f"s1-V{v}-mw1"
        for t in S1_WIDE128_T[v]:
            _add(g, "id", 12, 128, t, v, res="identity")
            _add(g, "ext", 20, 128, t, v)
        if v == 25:
            _add(g, "id", 256, 64, 5, v, res="identity")
            _add(g, "ext", 256, 128, 4, v)               # one tile of the wide shape, two row tiles
        # ---- valid: none / identity ("valid"), conv ("valid_res")
        for mw, cos in ((1, (64, 192)), (2, (128,))):
            g = f"valid-V{v}-mw{mw}"
            i = 0
            for co in cos:
                for t in VALID_T[mw, v] + (9, 10, 11):
                    _add(g, "valid", CS[i % 5], co, t, v)
                    _add(g, "valid", CS[(i + 1) % 5], co, t, v, res="identity")
                    _add(g, "valid_res", CS[(i + 3) % 5], co, t, v, res="conv", c_res=CRES_V[i % 2])
                    i += 1
            _add(g, "valid", 12, cos[0], VALID_T[mw, v][1], v, res="identity", relu=1)
            _add(g, "valid_res", 20, cos[0], VALID_T[mw, v][0], v, res="conv", c_res=16, relu=1)
        t = {25: 23, 18: 29}[v]                          # c_out = 128 where the wide shape is picked: two row tiles
        _add(f"valid-V{v}-mw1", "valid", 12, 128, t, v, res="identity")
        _add(f"valid-V{v}-mw1", "valid_res", 20, 128, t, v, res="conv", c_res=16)
        if v == 25:
            _add(f"valid-V{v}-mw2", "valid_res", 256, 128, 12, v, res="conv", c_res=48)
        # ---- stride 2: conv residual or none ("ext")
        for mw, cos in ((1, (64, 192)), (2, (128,))):
            g = f"s2-V{v}-mw{mw}"
            i = 0
            for co in cos:
                for t in S2_T[mw, v] + (1, 2, 3, 5):
                    _add(g, "ext", CS[i % 5], co, t, v, stride=2)
                    _add(g, "ext", CS[(i + 1) % 5], co, t, v, stride=2, res="conv", c_res=CRES_S2[i % 4])
                    i += 1
            _add(g, "ext", 12, cos[0], S2_T[mw, v][0], v, stride=2, res="conv", c_res=24, relu=1)
        if v == 25:
            _add(f"s2-V{v}-mw2", "ext", 256, 128, 7, v, stride=2, res="conv", c_res=64)
            _add(f"s2-V{v}-mw2", "ext", 12, 256, 28, v, stride=2, res="conv", c_res=8)      # two tall row tiles
    # ---- routing: every tap of each kernel, then each residual form alone (conv weights zero)
    for r in range(9):
        _add("route-s1", ("id", "ext")[r % 2], 12, 64, 29, 25, res=("identity", "none")[r % 2], tier="route_tap", tap=r)
        _add("route-valid", "valid", 12, 128, 26, 18, tier="route_tap", tap=r)
        _add("route-s2", "ext", 12, 128, 35, 25, stride=2, tier="route_tap", tap=r)
    _add("route-s1", "id", 12, 64, 29, 25, res="identity", tier="route_res")
    _add("route-valid", "valid", 12, 128, 26, 18, res="identity", tier="route_res")
    _add("route-valid", "valid_res", 12, 128, 26, 18, res="conv", c_res=48, tier="route_res")
    _add("route-valid", "valid_res", 12, 64, 31, 25, res="conv", c_res=16, tier="route_res")
    _add("route-s2", "ext", 12, 128, 35, 25, stride=2, res="conv", c_res=24, tier="route_res")
    _add("route-s2", "ext", 12, 64, 43, 18, stride=2, res="conv", c_res=3, tier="route_res")
    # ---- rounding: random fp32 operands, each kernel at 64 and 256 channels; one frame 2^10 times its neighbours
    for c in (64, 256):
        _add("round", "id", c, 64, 29, 25, res="identity", tier="round")
        _add("round", "valid_res", c, 128, 19, 18, res="conv", c_res=16, tier="round")
        _add("round", "ext", c, 128, 35, 25, stride=2, res="conv", c_res=24, tier="round")
    _add("round", "ext", 64, 64, 29, 25, tier="cancel")
    _add("round", "valid", 64, 128, 26, 18, res="identity", tier="cancel")
    _add("round", "ext", 64, 128, 35, 25, stride=2, tier="cancel")


_build()
ALL_CASES = [c for table in GROUPS.values() for c in table]
EXACT_GROUPS = [g for g in GROUPS if g[0] in "sv"]
ROUTE_GROUPS = [g for g in GROUPS if g.startswith("route")]
CANCEL_FRAME, CANCEL_SCALE = 13, 1024.0

# launches the gate must refuse (the entry then runs the direct kernels): (case, reason it is refused for)
REJECTED = (
    Case("gate", 0, "id", 12, 64, 11, 20, res="identity", c_res=64),            # V = 20
    Case("gate", 1, "id", 12, 70, 11, 25, res="identity", c_res=70),            # c_out no multiple of 64
    Case("gate", 2, "id", 12, 64, 11, 25),                                      # no residual at the identity entry
    Case("gate", 3, "id", 12, 64, 21, 25, stride=2, res="conv", c_res=16),      # stride 2 at the identity entry
    Case("gate", 4, "ext", 12, 64, 11, 25, res="identity", c_res=64),           # a residual at stride 1 of the ext entry
    Case("gate", 5, "valid", 12, 64, 11, 25, res="conv", c_res=16),             # conv residual at the valid entry
    Case("gate", 6, "valid_res", 12, 64, 11, 25, res="conv", c_res=24),         # c_res not whole 16-channel chunks
    Case("gate", 7, "valid_res", 12, 64, 11, 25, res="conv", c_res=8),
)

# one NaN in y under ReLU: (case, indices of the NaN in y: a front tile, an interior tile, the last frame of a sequence)
NAN_CASES = (
    (Case("nan-s1", 0, "id", 12, 64, 29, 25, res="identity", c_res=64, relu=1), ((1, 5, 1, 7), (0, 3, 13, 24), (1, 7, 28, 0))),
    (Case("nan-valid", 0, "valid_res", 12, 128, 26, 18, res="conv", c_res=16, relu=1), ((2, 5, 2, 7), (0, 3, 12, 17), (1, 7, 25, 0))),
    (Case("nan-s2", 0, "ext", 12, 128, 35, 25, stride=2, res="conv", c_res=8, relu=1), ((1, 5, 2, 7), (0, 3, 17, 24), (2, 7, 34, 3))),
)


# ------------------------------------------------------------------------------------------------------------------------------
# operands and references (host)
# ------------------------------------------------------------------------------------------------------------------------------
def _ints(gen, shape, bound):
    return (torch.randint(0, 2 * bound + 1, shape, generator=gen) - bound).float()


def _ids(shape, first=1):
    n = 1
    for d in shape:
        n *= d
    assert first + n < 1 << 22
    return torch.arange(first, first + n, dtype=torch.float32).view(shape)


@functools.lru_cache(maxsize=None)
def operands(case):
    """y (n, c, t, v), w (co, c, 9, 1), bias (co,), and for a residual x (n, c_res, t, v) (+ wres (co, c_res, 1, 1)); never modified"""
    n, c, co, t, v = case.n, case.c, case.co, case.t, case.v
    assert case.res == "none" or case.c_res > 0 and (case.res == "conv" or case.c_res == co)
    d = {}
    g = torch.Generator().manual_seed(991 * (sum(map(ord, case.group)) % 1013) + case.seed)
    if case.tier == "exact":
        d["y"] = _ints(g, (n, c, t, v), ACT)
        d["w"] = _ints(g, (co, c, 9, 1), W_MAX)
        d["bias"] = _ints(g, (co,), BIAS)
        if case.res != "none":
            d["x"] = _ints(g, (n, case.c_res, t, v), ACT)
        if case.res == "conv":
            d["wres"] = _ints(g, (co, case.c_res, 1, 1), W_RES)
        return d
    if case.tier in ("round", "cancel"):
        d["y"] = torch.randn((n, c, t, v), generator=g)
        if case.tier == "cancel":
            d["y"][:, :, CANCEL_FRAME] *= CANCEL_SCALE
        d["w"] = torch.randn((co, c, 9, 1), generator=g) / (9 * c) ** 0.5
        d["bias"] = torch.randn((co,), generator=g)
        if case.res != "none":
            d["x"] = torch.randn((n, case.c_res, t, v), generator=g)
        if case.res == "conv":
            d["wres"] = torch.randn((co, case.c_res, 1, 1), generator=g) / case.c_res ** 0.5
        return d
    d["y"] = _ids((n, c, t, v))
    d["w"] = torch.zeros((co, c, 9, 1))
    d["bias"] = torch.zeros(co)
    rows = torch.arange(co)
    if case.tier == "route_tap":
        d["w"][rows, rows % c, case.tap, 0] = 1.0
    if case.res != "none":
        d["x"] = _ids((n, case.c_res, t, v), first=1 + (1 << 20))
    if case.res == "conv":
        d["wres"] = torch.zeros((co, case.c_res, 1, 1))
        d["wres"][rows, rows % case.c_res, 0, 0] = 1.0
    return d


def partial_sum_bound(case):
    """Largest magnitude an accumulator, or a sum of the output transform, of an exact case can reach in the TRANSFORMED problem:
    image entries |U| <= 3 W_MAX / 2 (halves), transformed activations |B| <= 2 ACT, three (stride 2: four) groups per channel,
    the residual phase (valid: |wres| |x|, stride 2: |wres| |x0 - x1|), three accumulator sets per output frame, bias, identity."""
    groups = 4 if case.stride == 2 else 3
    acc = groups * case.c * (3 * W_MAX / 2) * (2 * ACT)
    if case.res == "conv":
        acc += case.c_res * W_RES * (2 * ACT if case.stride == 2 else ACT)
    return 3 * acc + BIAS + ACT


def images(case, d=None):
    """the transformed weight image the launch is given (fp32), and the direct residual image"""
    d = d or operands(case)
    ones = torch.ones(case.co, dtype=torch.float64)
    u = (fold.pack_conv_weight_wino_s2 if case.stride == 2 else fold.pack_conv_weight_wino)(d["w"], ones)
    return u, (fold.pack_conv_weight(d["wres"], ones)[0] if "wres" in d else None)


@functools.lru_cache(maxsize=None)
def reference(case):
    """the definition: fp64 conv plus residual and bias (exact tier: cast to fp32; rounding tiers: left in fp64)"""
    d = operands(case)
    s = case.stride
    out = F.conv2d(d["y"].double(), d["w"].double(), d["bias"].double(), stride=(s, 1), padding=(case.pad, 0))
    if case.res != "none":
        x = d["x"].double()[:, :, case.res_off::s][:, :, : case.t_out]
        out = out + (x if case.res == "identity" else F.conv2d(x, d["wres"].double()))
    out = torch.relu(out) if case.relu else out
    return out if case.tier in ("round", "cancel") else out.float()


def routing_expected(case):
    """what a routing case must give, read off the ids: y[n, o % c, stride t' + tap - pad, v] (0 in the padding), or the block
    input at frame stride t' + res_off: x[n, o, ...] (identity) / x[n, o % c_res, ...] (one-hot conv); both for a tap case with
    the identity residual"""
    d = operands(case)
    rows = torch.arange(case.co)
    frames = torch.arange(case.t_out) * case.stride
    out = torch.zeros((case.n, case.co, case.t_out, case.v), dtype=torch.float64)
    if case.tier == "route_tap":
        f = frames + case.tap - case.pad
        inside = (f >= 0) & (f < case.t)
        out += d["y"].double()[:, rows % case.c][:, :, f.clamp(0, case.t - 1)] * inside.view(1, 1, -1, 1)
    if case.res != "none":
        out += d["x"].double()[:, rows % case.c_res][:, :, frames + case.res_off]
    return out.float().contiguous()


def groups_of(case):
    """(first image row, products, raw frame of sample i of pair j as (per pair, first, per sample)) per group, from fold's tables"""
    points, taps = len(fold.WINO_G), len(fold.WINO_G[0])
    if case.stride == 2:
        out, row = [], 0
        for first, ntaps in fold.WINO_S2_GROUPS:
            out.append((row, ntaps + 1, (4, first - 4, 2)))
            row += ntaps + 1
        return out
    return [(points * g, points, (2, taps * g - case.pad, 1)) for g in range(9 // taps)]


def nan_mask(case, idx):
    """The outputs that a NaN at y[idx] reaches THROUGH THE ALGORITHM: sample f of a group enters accumulator set i where the
    input transform has a non-zero coefficient and the group has that product, and set i enters frame e of the pair where the
    output transform has one -- whatever the weights are (NaN x 0 = NaN).  Its segment and joint, every output channel."""
    n0, _, f0, v0 = idx
    mask = torch.zeros((case.n, case.co, case.t_out, case.v), dtype=torch.bool)
    for j in range((case.t_out + 1) // 2):
        for _, np_, (per_pair, first, per_sample) in groups_of(case):
            for f in range(4 if np_ == 4 else 3):                    # a 2-tap group reads d0 .. d2 only
                if per_pair * j + first + per_sample * f != f0:
                    continue
                for i in range(np_):
                    for e in (0, 1):
                        if WINO_BT[i][f] and WINO_AT[e][i] and 2 * j + e < case.t_out:
                            mask[n0, :, 2 * j + e, v0] = True
    return mask


def window_mask(case, idx):
    """the definition's window, for comparison with nan_mask"""
    n0, _, f0, v0 = idx
    mask = torch.zeros((case.n, case.co, case.t_out, case.v), dtype=torch.bool)
    for tt in range(case.t_out):
        if 0 <= f0 - (case.stride * tt - case.pad) < 9:
            mask[n0, :, tt, v0] = True
    return mask


# ------------------------------------------------------------------------------------------------------------------------------
# the Winograd computation step by step, with one seeded defect at a time
# ------------------------------------------------------------------------------------------------------------------------------
DEFECTS = ("m3_sign", "group_offset", "front_clamp", "back_reads_on", "phantom_stored", "clamped_lane_stored", "channel_tail",
           "valid_res_frame", "s2_inf_product", "s2_res_d1", "seg_stride_cpad", "decode_swapped")


def applies(defect, case, sel=None):
    """the cases that exist to catch the defect"""
    sel = sel or sel_of(case)
    conv_w = case.tier in ("exact", "route_tap")                     # the conv weights are not all zero
    k = kernel_of(case)
    if defect == "m3_sign":                                          # the point-inf row of a group: taps 2, 5, 8 (stride 2: tap 4)
        return case.tier == "exact" and case.t_out >= 2 or case.tier == "route_tap" and case.tap in ((4,) if k == "s2" else (2, 5, 8))
    if defect == "group_offset":
        return conv_w
    if defect == "front_clamp":                                      # needs a non-zero weight on a tap that reads in front
        return case.tier == "exact" and k != "valid" or case.tier == "route_tap" and k != "valid" and case.tap < 4
    if defect == "back_reads_on":
        if k == "valid":                                             # only the phantom frame's samples lie behind the row
            return False
        return case.tier == "exact" or case.tier == "route_tap" and case.tap > 4
    if defect == "phantom_stored":
        return sel.phantom and case.tier in ("exact", "route_tap", "route_res") and case.co * case.n > 1
    if defect == "clamped_lane_stored":
        return sel.partial_last and case.tier in ("exact", "route_res")
    if defect == "channel_tail":
        return case.tier == "exact" and case.c % CPAD != 0
    if defect == "valid_res_frame":
        return k == "valid" and case.res != "none"
    if defect == "s2_inf_product":
        return k == "s2" and case.tier == "exact"
    if defect == "s2_res_d1":
        return k == "s2" and case.res == "conv" and case.t_out >= 2
    if defect == "seg_stride_cpad":
        return case.c % CPAD != 0 and case.n > 1 and conv_w
    if defect == "decode_swapped":
        return sel.mtiles != sel.qtiles
    raise KeyError(defect)


def _gather(flat, base, pp, lo, hi, defect_front=False, defect_back=False):
    """flat[base + pp] for the positions lo <= pp < hi of a channel row, zero outside (the conv's zero padding); defects: clamp in
    front, read on behind"""
    inside = (pp >= lo) & (pp < hi)
    idx = pp.clamp(lo, hi - 1)
    if defect_front:
        inside = inside | (pp < lo)
    if defect_back:
        idx = torch.where(pp >= hi, pp, idx)
        inside = inside | (pp >= hi)
    idx = base + idx
    ok = inside & (idx >= 0) & (idx < flat.numel())
    return torch.where(ok, flat[idx.clamp(0, flat.numel() - 1)], torch.zeros((), dtype=flat.dtype))


def model(case, defect=None, dtype=torch.float64, y=None, absolute=False):
    """The launch as the kernel runs it, in `dtype` (fp64: cast to fp32 at the end; fp32: an emulation of the device arithmetic),
    from the fp32 weight image.  y: another activation tensor (reduced-precision operands).  absolute: every product, transform
    coefficient, bias and residual by magnitude -- the S of error_bound.  Outputs no work item stores stay NaN."""
    sel = sel_of(case)
    assert not sel.reject
    d = operands(case)
    n, c, co, t, v, s2, valid = case.n, case.c, case.co, case.t, case.v, case.stride == 2, case.pad == 0
    tv, t_out, cpad = t * v, case.t_out, _ceil_to(c, CPAD)
    u_img, wres_img = images(case, d)
    U = u_img.to(dtype)[:, :, :co]                                   # [rows][cpad][co]
    yflat = (d["y"] if y is None else y).to(dtype).reshape(-1)
    if absolute:
        U = U.abs()
    if defect == "channel_tail" and c < cpad:                        # padding rows repeat the last channel, in both operands
        U = U.clone()
        U[:, c:] = U[:, c - 1: c]
    bias = d["bias"].to(dtype)
    x = d["x"].to(dtype) if "x" in d else None
    wres = wres_img.to(dtype)[:, :co] if wres_img is not None else None          # [cres_pad][co]
    if absolute:
        bias = bias.abs()
        x = x.abs() if x is not None and case.res == "identity" else x
        wres = wres.abs() if wres is not None else None
    groups = groups_of(case)
    per_pair = 4 if s2 else 2
    nt, mt = sel.nt, sel.mt
    out = torch.full((n * co * t_out * v,), float("nan"), dtype=dtype)
    late = []                                                        # stores of a defect, made behind all others
    tile_cache = {}

    def tile(seg, qt):
        """(o0, o1) of all rows for the NT lanes of column tile qt, and the lanes' (jc, vc, live)"""
        q0 = qt * nt
        qend = min(q0 + nt, sel.qp)
        ja, jb = q0 // v, (qend - 1) // v
        lanes = torch.arange(q0, q0 + nt)
        qc = lanes.clamp(max=qend - 1)
        jc, vc = qc // v, qc % v
        off = per_pair * (jc - ja) * v + vc
        fa = 4 * ja - 4 if s2 else 2 * ja if valid else 2 * ja - 4
        span = ((4 * (jb - ja) + 11) if s2 else (2 * (jb - ja) + 10)) * v
        pp = fa * v + torch.arange(span)
        seg_c = cpad if defect == "seg_stride_cpad" else c
        rows_c = torch.arange(cpad).clamp(max=c - 1) if defect == "channel_tail" else torch.arange(cpad)
        staged = torch.zeros((cpad, span), dtype=dtype)
        for ch in range(cpad):
            if ch < c or defect == "channel_tail":
                base = (seg * seg_c + int(rows_c[ch])) * tv
                staged[ch] = _gather(yflat, base, pp, 0, tv, defect == "front_clamp", defect == "back_reads_on")
        M = [torch.zeros((co, nt), dtype=dtype) for _ in range(4)]
        for gi, (row0, np_, (_, first, per_sample)) in enumerate(groups):
            f0 = first - (fa - per_pair * ja)                        # frame of sample 0 relative to the staged span, at pair ja
            if defect == "group_offset" and not s2:
                f0 = 3 * gi + 1
            if defect == "group_offset" and s2:
                f0 += 1
            inf = defect == "s2_inf_product" and np_ == 3
            dd = []
            for f in range(4):
                if f == 3 and np_ == 3 and not inf:                  # a 2-tap group: d3 is not read
                    dd.append(torch.zeros_like(dd[0]))
                    continue
                pos = off + (f0 + per_sample * f) * v                # (a defect may step behind the staged span: zero there)
                dd.append(torch.where(pos < span, staged[:, pos.clamp(max=span - 1)], torch.zeros((), dtype=dtype)))
            b = [sum(cf * dd[f] for f, cf in enumerate(WINO_BT[i]) if cf) for i in range(4)]
            if absolute:
                b = [bi.abs() for bi in b]
            for i in range(np_ + (1 if inf else 0)):
                urow = U[row0 + i] if row0 + i < U.shape[0] else torch.zeros_like(U[0])
                M[i] = M[i] + urow.t() @ b[i]
        if case.res == "conv":
            cres = case.c_res
            xflat = x.reshape(-1)
            if s2:
                rspan = (4 * (jb - ja) + 3) * v
                pr = 4 * ja * v + torch.arange(rspan)
                d1_at = 1 if defect == "s2_res_d1" else 2
            else:
                fr = 2 * ja if defect == "valid_res_frame" else 2 * ja + 4
                rspan = (2 * (jb - ja) + 2) * v
                pr = fr * v + torch.arange(rspan)
                d1_at = 1
            rst = torch.stack([_gather(xflat, (seg * cres + ch) * tv, pr, 0, tv) for ch in range(cres)])
            d0, d1 = rst[:, off], rst[:, off + d1_at * v]
            w = wres[:cres].t()
            if s2:
                M[0] = M[0] + w @ ((d0 - d1).abs() if absolute else d0 - d1)
                M[1] = M[1] + w @ (d1.abs() if absolute else d1)
            else:
                M[0] = M[0] + w @ (d0.abs() if absolute else d0)
                M[3] = M[3] + w @ (d1.abs() if absolute else -d1)
        if absolute:
            o0, o1 = M[0] + M[1] + M[2], M[1] + M[2] + M[3]
        else:
            o0, o1 = M[0] + M[1] + M[2], M[1] - M[2] + (M[3] if defect == "m3_sign" else -M[3])
        o0, o1 = o0 + bias[:, None], o1 + bias[:, None]
        if case.res == "identity":
            roff = 0 if defect == "valid_res_frame" else case.res_off
            odd_ok = 2 * jc + 1 < t_out
            xs = x[seg]                                              # (co, t, v)
            o0 = o0 + xs[:, 2 * jc + roff, vc]
            o1 = o1 + xs[:, torch.where(odd_ok, 2 * jc + 1, 2 * jc) + roff, vc]
        if case.relu and not absolute:
            o0, o1 = torch.relu(o0), torch.relu(o1)
        return o0, o1, lanes, jc, vc, lanes < qend

    rows_all = torch.arange(co)
    for wid in range(sel.grid):
        if defect == "decode_swapped":
            m0, qt = (wid % sel.qtiles) * mt, (wid // sel.qtiles) % sel.mtiles
        else:
            m0, qt = (wid % sel.mtiles) * mt, (wid // sel.mtiles) % sel.qtiles
        seg = wid // (sel.mtiles * sel.qtiles)
        if m0 >= co or qt >= sel.qtiles:                             # (a swapped decode: a work item outside the problem)
            continue
        if (seg, qt) not in tile_cache:
            tile_cache[seg, qt] = tile(seg, qt)
        o0, o1, lanes, jc, vc, live = tile_cache[seg, qt]
        rows = rows_all[m0: m0 + mt]
        rowbase = ((seg * co + rows) * t_out * v)[:, None]
        a0 = rowbase + (2 * jc * v + vc)[None, :]
        odd_ok = (2 * jc + 1 < t_out)
        out[a0[:, live]] = o0[m0: m0 + mt][:, live]
        keep = live & odd_ok
        out[(a0 + v)[:, keep]] = o1[m0: m0 + mt][:, keep]
        if defect == "phantom_stored":
            ph = live & ~odd_ok
            late.append(((a0 + v)[:, ph], o1[m0: m0 + mt][:, ph]))
        if defect == "clamped_lane_stored":
            ju, vu = lanes // v, lanes % v
            au = rowbase + (2 * ju * v + vu)[None, :]
            late.append((au[:, ~live], o0[m0: m0 + mt][:, ~live]))
            late.append(((au + v)[:, ~live], o1[m0: m0 + mt][:, ~live]))
    for addr, val in late:
        ok = addr < out.numel()
        out[addr[ok]] = val[ok]
    out = out.view(n, co, t_out, v)
    return out if dtype != torch.float64 or absolute else out.float()


# ------------------------------------------------------------------------------------------------------------------------------
# the derived forward-error bound of the rounding tiers
# ------------------------------------------------------------------------------------------------------------------------------
U32 = 2.0 ** -24


def roundings(case):
    """n of gamma(n): the products of one accumulator element (three or four groups per channel, plus the residual channels), one
    rounding of the weight image, one of the input transform, and six for the output transform, bias and residual"""
    return (4 if case.stride == 2 else 3) * case.c + (case.c_res if case.res == "conv" else 0) + 1 + 1 + 6


@functools.lru_cache(maxsize=None)
def error_bound(case):
    """gamma(n) S per output element: S = the fp64 sum of |U| |B| over the accumulator sets that enter the output, + |bias| +
    |residual| (model(absolute=True))"""
    nu = roundings(case) * U32
    return nu / (1 - nu) * model(case, absolute=True)


def truncated(y, bits):
    """y with its significand cut to `bits` explicit bits (7: bf16 by truncation)"""
    mask = -(1 << (23 - bits))
    return (y.contiguous().view(torch.int32) & mask).view(torch.float32)
