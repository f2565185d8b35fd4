"""Cases, operands, references and the launcher's kernel selection for tests/test_gpu_tcn_direct.py and
tests/test_tcn_direct_fixture_cpu.py: the direct clip temporal conv behind csk_tcn_stage_f32 / csk_tcn_stage_splitk_f32
(tcn_stage_kernel and tcn_reduce_kernel of csrc/tcn.hip, tcn_stage16_kernel of csrc/tcn16.hip).

select() restates, from tcn_stage_impl and csk_launch_tcn_stage16, which kernel instantiation a launch gets; nothing is read from
csrc.  The case tables follow that selection: the CPU test proves that their union reaches every instantiation the launcher can
pick (REACHABLE, found by sweeping select() over the launcher's whole domain), the narrowed tiles, the split-K fall-back, full and
ragged row tiles and interior and border staging tiles of both families.

Two tiers of operands.  exact: small integers, so that every product and every partial sum is exact in fp32 in any order
(partial_sum_bound) and a launch must equal the fp64 conv BIT FOR BIT, ReLU off so that both signs are compared.  route_*: every
activation (block input) element carries its own integer id and the weights are one-hot, so every output element names the one
input element it came from -- integers in [-3, 3] repeat, ids do not.

model() is the same operation written out step by step on the host (explicit padding, channel ranges, tiles) and takes one seeded
defect at a time: the CPU test shows that each defect changes the result on every case that exists to catch it."""
import functools
from typing import NamedTuple

import torch
import torch.nn.functional as F

N_SEG = 3
ACT = 3            # activations and block inputs: integers in [-ACT, ACT]
W_MAX = 4          # conv weights: integers in [-W_MAX, W_MAX]
W_RES = 3          # residual conv weights: integers in [-W_RES, W_RES]
BIAS = 8           # bias: integers in [-BIAS, BIAS]

RES_MODE = {"none": 0, "identity": 1, "conv": 2}
CPAD, MROWS, KC = 16, 64, 8          # channel padding of the packed weights, row padding, channels per K chunk
LDS_MAX = 160 * 1024

S1_T = (1, 2, 9, 10, 11, 21, 45)                     # frames, stride 1
S2_T = (1, 2, 3, 5, 19, 21, 41, 90)                  # frames, stride 2
S1_T16 = S1_T + (37,)                                # 16x16x4 family: 37 and 45 frames are three tiles with an interior one
S2_T16 = S2_T + (71,)                                # ... 71 and 90 frames at stride 2; odd T: a row ends inside a quad
CRES = (3, 8, 16, 24, 40, 64)
CRES16 = (8, 16, 24, 40, 64)                         # the 16x16x4 kernel takes whole 8-channel chunks


def _ceil_to(a, b):
    return (a + b - 1) // b * b


def partial_sum_bound(c, c_res):
    """largest magnitude of any partial sum of a launch: 9 c products, c_res residual products, bias, identity residual"""
    return 9 * c * W_MAX * ACT + c_res * W_RES * ACT + BIAS + ACT


# ------------------------------------------------------------------------------------------------------------------------------
# the launcher's selection, restated
# ------------------------------------------------------------------------------------------------------------------------------
class Sel(NamedTuple):
    family: str        # "32": tcn_stage_kernel (32x32x2 tiles), "16": tcn_stage16_kernel (16x16x4 tiles)
    mt: int            # rows of a workgroup tile
    nj: int            # 64-position sweeps of the activation staging (template argument); 0 for the 16 family
    k9: bool           # the straight-line 9-tap form
    vt: int            # joints as a compile-time constant, 0 = run time
    split: bool
    res_g: int         # 8-channel groups per chunk of the conv-residual phase; 0 for the 16 family
    nt: int            # output positions per tile
    ksplit: int        # channel ranges that are launched
    ldb: int           # staged positions per channel row
    cper: int          # channels per range
    stride: int

    @property
    def key(self):
        """the template instantiation"""
        if self.family == "16":
            return ("tcn_stage16_kernel", self.vt, self.stride)
        return ("tcn_stage_kernel", self.mt, self.nj, self.k9, self.split, self.vt)


def _narrow(nt, nj_max, v, k, stride):
    while True:
        max_dt = (nt + v - 2) // v
        ldb = _ceil_to((stride * max_dt + k) * v, 4)
        if (ldb + 63) // 64 <= nj_max or nt == 1:
            return nt, ldb
        nt = nt - 16 if nt > 16 else nt // 2 if nt > 1 else 1


def _takes16(c, c_out, c_res, t_in, t_out, t_res, v, k, stride, pad, res_mode, res_off, ranges, mode):
    if mode == 1:
        return False
    if mode != 2 and v != 18 and c > (128 if stride == 2 else 64):
        return False
    if k != 9 or ranges != 1 or v not in (25, 18) or stride not in (1, 2):
        return False
    if (pad * v) & 3 or c % 8 or c < 8:
        return False
    if res_mode == 2 and (c_res % 8 or c_res < 8 or (res_off * v) & 3):
        return False
    if res_mode == 1 and stride != 1:
        return False
    if max(c * t_in, c_out * t_out, c_res * t_res) * v * 4 >= 1 << 31:
        return False
    return t_in * v >= 8 and (res_mode == 0 or t_res * v >= 8)


def select(c, c_out, c_res, t_in, V, k, stride, pad, res_mode, res_off, ksplit, tcn16_mode=0, t_res=None, n_seg=N_SEG):
    """The kernel a launch csk_tcn_stage_f32 (ksplit 1) / csk_tcn_stage_splitk_f32 gets.  tcn16_mode: CSK_TCN16 under CSK_DIAG=1
    (0: not set, 1: never the 16x16x4 family, 2: wherever it is built for)."""
    assert 1 <= k <= 9 and stride >= 1 and 0 <= pad < k and 2 <= V <= 64 and t_in + 2 * pad >= k and 1 <= ksplit <= 64
    assert ksplit == 1 or k == 9
    t_out = (t_in + 2 * pad - k) // stride + 1
    c_res = c_res if c_res > 0 else 1
    t_res = (t_in if t_res is None else t_res) if res_mode else 1
    cpad, mpad, cres_pad = _ceil_to(c, CPAD), _ceil_to(c_out, MROWS), _ceil_to(c_res, CPAD)
    cper = _ceil_to((cpad + ksplit - 1) // ksplit, KC)
    ranges = (c + cper - 1) // cper if ksplit > 1 else 1
    if ranges == 1 and _takes16(c, c_out, c_res, t_in, t_out, t_res, V, k, stride, pad, res_mode, res_off, ranges, tcn16_mode):
        return Sel("16", 64, 0, True, V, False, 0, 16 * V, 1, _ceil_to((15 * stride + 9) * V, 4), cpad, stride)
    big = mpad % 128 == 0
    nt64, ldb64 = _narrow(256, 14, V, k, stride)
    nt128, ldb128 = _narrow(128, 9, V, k, stride) if big else (0, 0)
    if big and nt128 < 128 and nt64 * 128 > nt128 * 256:
        big = False
    mt, nj_max = (128, 9) if big else (64, 14)
    nt, ldb = (nt128, ldb128) if big else (nt64, ldb64)
    nj = (ldb + 63) // 64
    if nj > nj_max:
        raise ValueError(f"activation tile of {ldb} positions exceeds the staged maximum")
    lds = (k * KC * mt + KC * ldb) * 4
    vt_ok = True
    if res_mode == 2:
        ldb2 = _ceil_to((stride * ((nt + V - 2) // V) + 1) * V, 4)
        assert ldb2 <= ldb
        lds2 = lambda g: (g * KC * mt + g * KC * ldb2) * 4
        vt_ok = cres_pad % (4 * KC) == 0 and 2 * lds2(4) <= LDS_MAX
        lds = max(lds, lds2(4 if vt_ok and k == 9 and V in (25, 18) else 2))
    if lds > LDS_MAX:
        raise ValueError(f"LDS tile {lds} B exceeds 160 KiB")
    inst = 6 if nj <= 6 else 9 if nj <= 9 else 14
    k9 = k == 9 and inst != 14
    vt = V if k == 9 and V in (25, 18) and vt_ok and nj <= 9 else 0
    if ranges > 1 and (nj > 9 or n_seg > 65535):
        ranges, cper = 1, cpad
    split = ranges > 1
    if split:
        vt = 0
    return Sel("32", mt, inst, k9, vt, split, 4 if vt else 2, nt, ranges, ldb, cper, stride)


@functools.lru_cache(maxsize=None)
def reachable():
    """every instantiation select() can answer over the launcher's domain: V 2 .. 64, k 1 .. 9 with each pad, stride 1 .. 4, both
    tile heights, residual forms with both paddings of c_res, channel counts either side of the 16x16x4 gate, split or not, and
    the three family modes"""
    keys = set()
    for V in range(2, 65):
        for k in range(1, 10):
            for stride in (1, 2, 3, 4):
                for pad in {0, k // 2, k - 1}:
                    t_in = max(k, 4)
                    for c_out in (64, 128):
                        for res_mode, c_res in ((0, 0), (1, c_out), (2, 8), (2, 32)):
                            for c in (12, 64, 256) if k == 9 else (12,):
                                for ksplit in (1, 4) if k == 9 else (1,):
                                    for mode in (0, 1, 2) if k == 9 and V in (25, 18) else (0,):
                                        try:
                                            keys.add(select(c, c_out, c_res, t_in, V, k, stride, pad, res_mode, 0, ksplit, mode).key)
                                        except ValueError:
                                            pass
    return frozenset(keys)


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    group: str
    seed: int
    c: int
    co: int
    t: int
    v: int
    k: int = 9
    stride: int = 1
    pad: int = 4
    res: str = "none"
    c_res: int = 0
    res_off: int = 0
    relu: int = 0
    ksplit: int = 1
    mode: int = 0          # the CSK_TCN16 mode the case needs (0: the default path)
    n: int = N_SEG
    tier: str = "exact"    # "exact" | "route_tap" | "route_conv" | "route_ident"
    tap: int = 0           # route_tap: the tap that carries the one-hot weight

    @property
    def t_out(self):
        return (self.t + 2 * self.pad - self.k) // self.stride + 1

    @property
    def name(self):
        s = f"{self.group}#{self.seed} c{self.c} co{self.co} T{self.t} V{self.v} k{self.k} s{self.stride} p{self.pad} {self.res}"
        if self.res == "conv":
            s += f"{self.c_res}"
        s += f"+{self.res_off}" if self.res_off else ""
        s += " relu" if self.relu else ""
        s += f" ksplit{self.ksplit}" if self.ksplit > 1 else ""
        s += f" CSK_TCN16={self.mode}" if self.mode else ""
        s += f" n{self.n}" if self.n != N_SEG else ""
        s += f" {self.tier}" + (f"{self.tap}" if self.tier == "route_tap" else "") if self.tier != "exact" else ""
        return s


def sel_of(case):
    return select(case.c, case.co, case.c_res, case.t, case.v, case.k, case.stride, case.pad, RES_MODE[case.res], case.res_off,
                  case.ksplit, case.mode, n_seg=case.n)


GROUPS = {}


def _add(group, c, co, t, v, **kw):
    if kw.get("res") == "identity":
        kw["c_res"] = co
    table = GROUPS.setdefault(group, [])
    table.append(Case(group, len(table), c, co, t, v, **kw))


def _build():
    # ---- 32x32 family on the default path: compile-time V, stride 1 (NJ 9 on 64-row tiles, 6 on 128-row tiles)
    for v in (25, 18):
        for co in (64, 128):
            g = f"vt_s1-V{v}-co{co}"
            for i, t in enumerate(S1_T):
                c = (12, 20, 3)[i % 3]
                _add(g, c, co, t, v)
                _add(g, c, co, t, v, res="identity")
                _add(g, (12, 20)[i % 2], co, t, v, res="conv", c_res=CRES[i % 6])
            _add(g, 20, co, 21, v, res="conv", c_res=3, relu=1)
            _add(g, 12, co, 11, v, res="identity", n=1)
            if v == 25:                               # more than 64 channels: the default path keeps the 32x32 kernel at V = 25
                _add(g, 128, co, 10, v)
                _add(g, 256, co, 11, v, res="conv", c_res=64, relu=1)
    # ---- stride 2: NJ 14 (generic form) on 64-row tiles, 9 on 128-row tiles
    for v in (25, 18):
        for co in (64, 128):
            g = f"vt_s2-V{v}-co{co}"
            for i, t in enumerate(S2_T):
                c = (20, 3, 12)[i % 3]
                _add(g, c, co, t, v, stride=2)
                _add(g, (12, 20)[i % 2], co, t, v, stride=2, res="conv", c_res=CRES[(i + 1) % 6])
            _add(g, 12, co, 41, v, stride=2, res="conv", c_res=24, relu=1)
            if v == 25:
                _add(g, 256, co, 21, v, stride=2, res="conv", c_res=64)
    # ---- ragged and multiple row tiles
    for co in (12, 70, 256):
        g = f"rows-co{co}"
        for v in (25, 18):
            _add(g, 12, co, 11, v)
            _add(g, 20, co, 21, v, res="identity")
            _add(g, 3, co, 10, v, res="conv", c_res=16)
            _add(g, 12, co, 21, v, stride=2, res="conv", c_res=24)
            _add(g, 20, co, 5, v, stride=2)
        _add(g, 64, co, 9, 25, n=1)                  # (16x16x4 family)
    # ---- run-time V; stride 2 at V = 40 / 64 narrows the tile; V = 12 is the one 64-row shape with 6 sweeps of 9 taps
    for v in (12, 17, 20, 33, 40, 64):
        g = f"runtime-V{v}"
        for j, co in enumerate((64, 128)):
            cs = (3, 8, 12, 20, 64)
            _add(g, cs[j], co, 2, v)
            _add(g, cs[j + 1], co, 11, v, res="identity")
            _add(g, cs[j + 2], co, 21, v, res="conv", c_res=CRES[(v + j) % 6])
            _add(g, cs[j + 3], co, 3, v, stride=2)
            _add(g, cs[j], co, 19, v, stride=2, res="conv", c_res=CRES[(v + j + 1) % 6])
            _add(g, cs[j + 1], co, 41, v, stride=2, res="conv", c_res=CRES[(v + j + 2) % 6])
        _add(g, 12, 70, 21, v, stride=2, relu=1)
    for i, t in enumerate((5, 21, 45)):              # stride 3 at V = 25: the 128-row tile narrows to 96 columns and is kept
        _add("stride3", (12, 20, 64)[i], 128, t, 25, stride=3)
        _add("stride3", (12, 20, 64)[i], 128, t, 25, stride=3, res="conv", c_res=(24, 8, 40)[i])
    # ---- generic k
    for k, pad in ((1, 0), (3, 1), (5, 2)):
        g = f"generic-k{k}"
        for i, v in enumerate((25, 18, 20)):
            for j, co in enumerate((64, 128)):
                cs = (3, 8, 12, 64, 20)
                _add(g, cs[i + j], co, 2 if k < 5 else 3, v, k=k, pad=pad)
                _add(g, cs[i + j + 1], co, 21, v, k=k, pad=pad, res="identity")
                _add(g, cs[i], co, 10, v, k=k, pad=pad, res="conv", c_res=CRES[(i + j + k) % 6])
                _add(g, cs[i + 1], co, 21, v, k=k, pad=pad, stride=2, res="conv", c_res=CRES[(i + j) % 6])
                _add(g, cs[i + 2], co, 41, v, k=k, pad=pad, stride=2)
        _add(g, 12, 70, 11, 25, k=k, pad=pad, relu=1)
    # ---- 9 taps with other paddings: the valid form (pad 0, residual from frame 4 on) and pad 3 (pad * V % 4 != 0 at V = 25:
    # the 16x16x4 gate leaves it to the 32x32 kernel, whatever the channel count)
    for v in (25, 18):
        g = f"k9_pads-V{v}"
        for i, t in enumerate((9, 10, 21, 45)):
            co = (64, 128)[i % 2]
            _add(g, (12, 20)[i % 2], co, t, v, pad=0)
            _add(g, (20, 12)[i % 2], co, t, v, pad=0, res="identity", res_off=4)
            _add(g, (12, 3)[i % 2], co, t, v, pad=0, res="conv", c_res=CRES[i], res_off=4)
        for t in (19, 41):
            _add(g, 12, 128, t, v, pad=0, stride=2, res="conv", c_res=24, res_off=4)
            _add(g, 20, 64, t, v, pad=0, stride=2, res="conv", c_res=8, res_off=4)
        if v == 25:
            for i, t in enumerate((3, 11, 21)):
                _add(g, (8, 64, 8)[i], 64, t, v, pad=3, res=("none", "identity", "conv")[i], c_res=16 if i == 2 else 0)
                _add(g, (64, 8, 64)[i], 128, t, v, pad=3, stride=2, res=("conv", "none", "none")[i], c_res=8 if i == 0 else 0)
    # ---- 16x16x4 family on the default path
    for v in (25, 18):
        g = f"f16_s1-V{v}"
        for i, t in enumerate(S1_T16):
            co = (64, 70, 12, 128)[i % 4]
            c = (8, 64)[i % 2]
            _add(g, c, co, t, v)
            _add(g, (64, 8)[i % 2], co, t, v, res="identity")
            _add(g, c, co, t, v, res="conv", c_res=CRES16[i % 5])
        _add(g, 64, 64, 45, v, res="identity", relu=1)
        _add(g, 8, 70, 37, v, res="conv", c_res=24, relu=1)
        _add(g, 64, 64, 21, v, res="identity", n=1)
        if v == 18:                                   # V = 18: every channel count
            _add(g, 128, 128, 21, v, res="identity")
            _add(g, 256, 64, 10, v, res="conv", c_res=64)
        g = f"f16_s2-V{v}"
        for i, t in enumerate(S2_T16):
            co = (128, 64, 70, 12)[i % 4]
            c = (64, 8, 128)[i % 3]
            _add(g, c, co, t, v, stride=2)
            _add(g, (8, 128, 64)[i % 3], co, t, v, stride=2, res="conv", c_res=CRES16[(i + 2) % 5])
        _add(g, 64, 128, 71, v, stride=2, res="conv", c_res=64, relu=1)
        _add(g, 8, 64, 41, v, stride=2, relu=1)
        if v == 18:
            _add(g, 256, 128, 21, v, stride=2, res="conv", c_res=40)
        g = f"f16_valid-V{v}"
        for i, t in enumerate((9, 10, 21, 45)):
            co = (64, 128)[i % 2]
            _add(g, (8, 64)[i % 2], co, t, v, pad=0)
            _add(g, (64, 8)[i % 2], co, t, v, pad=0, res="identity", res_off=4)
            _add(g, (8, 64)[i % 2], co, t, v, pad=0, res="conv", c_res=CRES16[i], res_off=4)
        for t in (19, 41, 90):
            _add(g, 64, 128, t, v, pad=0, stride=2, res="conv", c_res=16, res_off=4)
    # ---- split-K (csk_tcn_stage_splitk_f32): ranges that divide the 8-channel chunks evenly and not, more ranges asked for than
    # chunks exist, the three residual forms, both tile heights, c_out * Q a multiple of 4 and not, and the nj > 9 fall-back
    sp = "split"
    _add(sp, 40, 64, 11, 25, ksplit=2)
    _add(sp, 40, 64, 11, 25, ksplit=3, res="identity")
    _add(sp, 40, 70, 11, 25, ksplit=5, res="conv", c_res=24)
    _add(sp, 40, 12, 9, 25, ksplit=8, res="identity", relu=1)
    _add(sp, 40, 64, 45, 18, ksplit=32, res="conv", c_res=3)
    _add(sp, 64, 64, 21, 25, ksplit=8, res="conv", c_res=8)
    _add(sp, 64, 64, 10, 18, ksplit=64, res="identity")
    _add(sp, 64, 128, 21, 25, ksplit=64, stride=2, res="conv", c_res=64)
    _add(sp, 64, 128, 10, 20, ksplit=3)
    _add(sp, 128, 128, 10, 18, ksplit=32, res="identity")
    _add(sp, 128, 70, 11, 25, ksplit=5, res="identity", relu=1)
    _add(sp, 128, 256, 19, 18, ksplit=2, stride=2, res="conv", c_res=40)
    _add(sp, 256, 64, 9, 25, ksplit=32)
    _add(sp, 256, 128, 19, 18, ksplit=5, stride=2, res="conv", c_res=16, relu=1)
    _add(sp, 256, 128, 5, 33, ksplit=8, stride=2)
    _add(sp, 40, 64, 11, 12, ksplit=3, res="identity")
    _add(sp, 64, 64, 21, 12, ksplit=2, res="conv", c_res=16)
    _add(sp, 64, 12, 5, 17, ksplit=8, n=1)
    _add(sp, 64, 64, 21, 25, ksplit=2, pad=0, res="identity", res_off=4)
    _add(sp, 40, 128, 21, 25, ksplit=3, pad=0, res="conv", c_res=24, res_off=4)
    _add(sp, 128, 64, 19, 18, ksplit=3, stride=2, res="conv", c_res=24)        # 702 staged positions: the plain 64-row kernel
    _add(sp, 64, 64, 41, 25, ksplit=4, stride=2)                               # 775: the same
    _add(sp, 8, 64, 11, 25, ksplit=2, res="identity")                          # one real chunk: one range, the 16x16x4 family
    # ---- routing: every tap at one shape per family and stride, then each residual form alone
    for fam, c, shapes in (("32", 12, ((25, 1, 21), (18, 2, 41))), ("16", 16, ((25, 1, 37), (18, 2, 71)))):
        for v, stride, t in shapes:
            g = f"route{fam}-s{stride}"
            for r in range(9):
                _add(g, c, 70, t, v, stride=stride, tier="route_tap", tap=r)
            _add(g, c, 70, t, v, stride=stride, res="conv", c_res=24 if fam == "16" else 20, tier="route_conv")
            if stride == 1:
                _add(g, c, 70, t, v, res="identity", tier="route_ident")
                _add(g, c, 70, t, v, pad=0, res="identity", res_off=4, tier="route_ident")
            _add(g, c, 70, t, v, stride=stride, pad=0, res="conv", c_res=24 if fam == "16" else 20, res_off=4, tier="route_conv")
    g = "route32-other"
    for r in range(5):
        _add(g, 3, 12, 11, 20, k=5, pad=2, stride=1 + r % 2, tier="route_tap", tap=r)
    for r in range(3):
        _add(g, 20, 70, 10, 25, k=3, pad=1, stride=1 + r % 2, tier="route_tap", tap=r)
    _add(g, 12, 64, 9, 25, k=1, pad=0, tier="route_tap")
    for r in (0, 4, 8):
        _add(g, 12, 128, 21, 40, stride=2, tier="route_tap", tap=r)          # narrowed tiles
        _add(g, 40, 70, 21, 25, ksplit=3, tier="route_tap", tap=r)           # split-K
        _add(g, 12, 128, 21, 25, stride=3, tier="route_tap", tap=r)
    _add(g, 12, 128, 21, 40, stride=2, res="conv", c_res=20, tier="route_conv")
    _add(g, 40, 70, 21, 25, ksplit=3, res="identity", tier="route_ident")
    _add(g, 40, 70, 21, 25, ksplit=3, res="conv", c_res=20, tier="route_conv")
    _add(g, 12, 70, 41, 25, stride=2, res="identity", tier="route_ident")    # identity residual at stride 2: 32x32 only
    # ---- both families forced at the shapes both support (CSK_TCN16 = 1 / 2 in a child process)
    for mode in (1, 2):
        g = f"forced-{mode}"
        for v in (25, 18):
            for stride, t in ((1, 21), (2, 41)):
                for i, c in enumerate((8, 64, 128, 256)):
                    co = 64 if c <= 64 else 128
                    _add(g, c, co, t, v, stride=stride, mode=mode)
                    _add(g, c, co, t, v, stride=stride, res="conv", c_res=(8, 24, 64, 16)[i], mode=mode)
                    if stride == 1:
                        _add(g, c, co, t, v, res="identity", mode=mode, relu=int(c == 64))
                for r in (0, 4, 8):
                    _add(g, 8, 70, t, v, stride=stride, mode=mode, tier="route_tap", tap=r)
                _add(g, 8, 70, t, v, stride=stride, res="conv", c_res=16, mode=mode, tier="route_conv")
            _add(g, 8, 70, 21, v, res="identity", mode=mode, tier="route_ident")


_build()
ALL_CASES = [c for table in GROUPS.values() for c in table]
DEFAULT_GROUPS = [g for g in GROUPS if not g.startswith("forced-")]

# one NaN in y under ReLU: (case, index of the NaN in y) per family
NAN_CASES = (
    (Case("nan32", 0, 12, 70, 21, 25, res="identity", c_res=70, relu=1), (1, 5, 9, 7)),
    (Case("nan16", 0, 16, 64, 41, 18, stride=2, res="conv", c_res=8, relu=1), (2, 15, 20, 17)),
)


# ------------------------------------------------------------------------------------------------------------------------------
# tiles
# ------------------------------------------------------------------------------------------------------------------------------
def tiles(case, sel=None):
    """per position tile of a sequence: whether its staged activation span lies inside the row (the 16-byte staging form)"""
    sel = sel or sel_of(case)
    q, v, s = case.t_out * case.v, case.v, case.stride
    out = []
    if sel.family == "16":
        span = _ceil_to((15 * s + 9) * v, 4)
        for qt in range((q + 16 * v - 1) // (16 * v)):
            ws = (s * 16 * qt - case.pad) * v
            out.append(ws >= 0 and ws + span <= case.t * v)
        return out
    for q0 in range(0, q, sel.nt):
        qend = min(q0 + sel.nt, q)
        ta, tb = q0 // v, (qend - 1) // v
        fa, span = s * ta - case.pad, (s * (tb - ta) + case.k) * v
        out.append(fa >= 0 and fa * v + 4 * ((span + 3) // 4) <= case.t * v)
    return out


def row_tiles(case, sel=None):
    """(full, ragged) row tiles of the launch: m0 + MT <= c_out or not"""
    sel = sel or sel_of(case)
    n = _ceil_to(case.co, MROWS) // sel.mt
    full = sum(m * sel.mt + sel.mt <= case.co for m in range(n))
    return full, n - full


# ------------------------------------------------------------------------------------------------------------------------------
# operands and references (host)
# ------------------------------------------------------------------------------------------------------------------------------
def _ints(gen, shape, bound):
    return (torch.randint(0, 2 * bound + 1, shape, generator=gen) - bound).float()


def _ids(shape, first=1):
    n = 1
    for d in shape:
        n *= d
    assert first + n <= 1 << 24
    return torch.arange(first, first + n, dtype=torch.float32).view(shape)


@functools.lru_cache(maxsize=None)
def operands(case):
    """y (n, c, t, v), w (co, c, k, 1), bias (co,), and for a residual x (n, c_res, t, v) (+ wres (co, c_res, 1, 1)); never modified"""
    n, c, co, t, v, k = case.n, case.c, case.co, case.t, case.v, case.k
    assert case.res == "none" or case.c_res > 0 and (case.res == "conv" or case.c_res == co)
    d = {}
    if case.tier == "exact":
        g = torch.Generator().manual_seed(977 * (sum(map(ord, case.group)) % 1009) + case.seed)
        d["y"] = _ints(g, (n, c, t, v), ACT)
        d["w"] = _ints(g, (co, c, k, 1), W_MAX)
        d["bias"] = _ints(g, (co,), BIAS)
        if case.res != "none":
            d["x"] = _ints(g, (n, case.c_res, t, v), ACT)
        if case.res == "conv":
            d["wres"] = _ints(g, (co, case.c_res, 1, 1), W_RES)
        return d
    d["y"] = _ids((n, c, t, v))
    d["w"] = torch.zeros((co, c, k, 1))
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


@functools.lru_cache(maxsize=None)
def reference(case):
    """the definition: fp64 conv plus residual, cast to fp32"""
    d = operands(case)
    s = case.stride
    out = F.conv2d(d["y"].double(), d["w"].double(), d["bias"].double(), stride=(s, 1), padding=(case.pad, 0))
    if case.res != "none":
        x = d["x"].double()[:, :, case.res_off::s][:, :, : case.t_out]
        out = out + (x if case.res == "identity" else F.conv2d(x, d["wres"].double()))
    return (torch.relu(out) if case.relu else out).float()


def routing_expected(case):
    """what a routing case must give, read off the ids: y[n, o % c, stride t' + tap - pad, v] (0 in the padding), or the block
    input at frame stride t' + res_off: x[n, o, ...] (identity) / x[n, o % c_res, ...] (one-hot conv)"""
    d = operands(case)
    n, co, v = case.n, case.co, case.v
    rows = torch.arange(co)
    frames = torch.arange(case.t_out) * case.stride
    if case.tier == "route_tap":
        f = frames + case.tap - case.pad
        inside = (f >= 0) & (f < case.t)
        out = d["y"][:, rows % case.c][:, :, f.clamp(0, case.t - 1)] * inside.view(1, 1, -1, 1)
    else:
        out = d["x"][:, rows % case.c_res][:, :, frames + case.res_off]
    assert tuple(out.shape) == (n, co, case.t_out, v)
    return out.contiguous()


def nan_mask(case, idx):
    """outputs that a NaN at y[idx] reaches: its segment and joint, every output channel, the frames whose window covers it"""
    n0, _, f0, v0 = idx
    mask = torch.zeros((case.n, case.co, case.t_out, case.v), dtype=torch.bool)
    for tt in range(case.t_out):
        if 0 <= f0 - (case.stride * tt - case.pad) < case.k:
            mask[n0, :, tt, v0] = True
    return mask


# ------------------------------------------------------------------------------------------------------------------------------
# the operation step by step, with one seeded defect at a time
# ------------------------------------------------------------------------------------------------------------------------------
DEFECTS = ("tap_dropped", "padding_short", "residual_frame", "ragged_channel", "range_twice", "narrow_tile_skipped", "relu_forced")


def applies(defect, case, sel=None):
    """the cases that exist to catch the defect"""
    sel = sel or sel_of(case)
    exact = case.tier == "exact"
    if defect == "tap_dropped":
        return exact
    if defect == "padding_short":
        return exact and case.pad > 0 and case.stride * (case.t_out - 1) - case.pad + case.k - 1 >= case.t
    if defect == "residual_frame":
        return case.res != "none" and case.t >= 2
    if defect == "ragged_channel":
        return exact and (case.c % 8 != 0 or (case.res == "conv" and case.c_res % 8 != 0))
    if defect == "range_twice":
        return sel.split and case.tier in ("exact", "route_tap")           # (the other routing tiers have no conv weights)
    if defect == "narrow_tile_skipped":
        return sel.family == "32" and sel.nt < 16384 // sel.mt
    if defect == "relu_forced":
        return exact and not case.relu
    raise KeyError(defect)


def dropped_tap(case):
    """the tap the defect drops: from seed % k on, the first one that reads inside the row for some output frame"""
    for j in range(case.k):
        r = (case.seed + j) % case.k
        if any(0 <= case.stride * tt + r - case.pad < case.t for tt in range(case.t_out)):
            return r


def model(case, defect=None, sel=None):
    """fp64, cast to fp32.  Defects: one tap (dropped_tap) dropped in the last 8-channel chunk; the first padding frame behind the row
    repeats the last frame; the residual read one frame on; the last channel of a ragged count dropped (conv and residual conv);
    the second channel range of a split launch summed twice; the last position tile of a narrowed launch left out; ReLU applied
    where the launch asks for none."""
    sel = sel or sel_of(case)
    d = operands(case)
    n, c, co, t, v, k, s, pad = case.n, case.c, case.co, case.t, case.v, case.k, case.stride, case.pad
    w = d["w"].double().clone()
    wres = d["wres"].double().clone() if case.res == "conv" else None
    if defect == "tap_dropped":
        w[:, (c - 1) // 8 * 8:, dropped_tap(case)] = 0
    if defect == "ragged_channel":
        if c % 8:
            w[:, c - 1] = 0
        if wres is not None and case.c_res % 8:
            wres[:, case.c_res - 1] = 0
    yp = F.pad(d["y"].double(), (0, 0, pad, pad))
    if defect == "padding_short" and pad > 0:
        yp[:, :, pad + t] = yp[:, :, pad + t - 1]
    out = torch.zeros((n, co, case.t_out, v), dtype=torch.float64)
    frames = torch.arange(case.t_out) * s
    ranges = [(b, min(b + sel.cper, c)) for b in range(0, c, sel.cper)] if sel.split else [(0, c)]
    assert len(ranges) == sel.ksplit
    if defect == "range_twice":
        ranges.append(ranges[1])
    for lo, hi in ranges:                            # partial sums in range order
        for r in range(k):
            out += torch.einsum("oc,nctv->notv", w[:, lo:hi, r, 0], yp[:, lo:hi][:, :, frames + r])
    if case.res != "none":
        fr = frames + case.res_off
        if defect == "residual_frame":
            fr = (fr + 1) % t
        x = d["x"].double()[:, :, fr]
        out += x if case.res == "identity" else torch.einsum("oc,nctv->notv", wres[:, :, 0, 0], x)
    out += d["bias"].double().view(1, -1, 1, 1)
    if defect == "narrow_tile_skipped":
        q = case.t_out * v
        out.view(n, co, q)[:, :, (q - 1) // sel.nt * sel.nt:] = 0
    if case.relu or defect == "relu_forced":
        out = torch.relu(out)
    return out.float()
