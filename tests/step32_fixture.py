"""Cases for the 32x32x2 continual temporal step of csrc/step.hip: tcn_step_kernel<MT, E, HS, SPLIT, K9, OCC> and step_reduce_kernel,
the kernels csk_tcn_step_f32 launches whenever the 16x16x4 family (csrc/step16.hip) does not take the launch -- split-K (latency
mode), k != 9, P = 4, head_step outside 1..2.

``select`` restates, from csk_tcn_step_f32, which of the 15 instantiations a launch gets and how many workgroups it has; every case
also asks the library (csk_tcn_step_f32_tile, host arithmetic only) that step16 does NOT take it.  Three tiers of operands:

exact   integer operands as in tests/step16_fixture.py (weights +-{1..4} never 0, activations 1..7, bias -8..8) with
        sum |w| |x| + |bias| + |res| < 2**24 per output (``admissible``): every partial sum in any order, split or not, is exact in
        fp32, the kernel must give the fp64 ``conv2d`` reference bit for bit.
route   every ring element carries its own integer id in [2**23, 2**24) (odd ids included: the full 24-bit significand), every
        residual element a small id of its own; the weights are one-hot -- output row co picks one (tap, channel), a conv residual
        one residual channel -- so every output names the (slot, channel, position) it came from, and an operand truncated to bf16 or
        xf32 changes the id.
real    torch.rand activations, fan-in scaled normal weights: for the bitwise-invariance tests and the derived fp64 bound.

Layout: ring slots that hold no frame are NaN, positions past N V are NaN, the output ring has one spare slot, the partial buffer is
exactly n_emit * ksplit_eff * c_out * P floats carved out of a larger NaN-filled allocation (tests/test_gpu_step32.py).

``model`` is the same step written out on the host the way the kernel does it, with one seeded defect at a time (``DEFECTS``).

Not exercised: the route of rings of 4 GB or more into the unsplit E > 1 forms, and with it the 64-bit slot offsets of
RingStage::window beyond 2**32 -- multi-GB rings do not belong in a test suite.  P = 4 reaches the same instantiations with a single
clamped position tile; several position tiles of the unsplit forms are covered for E = 1 only (head_step 0 / 3, k != 9).
CPU only: nothing here touches a device."""
import functools
from dataclasses import dataclass, replace

import torch
import torch.nn.functional as F

import _bootstrap
from tests import step16_fixture as s16
from tests import step_split_fixture as ssf

pkg = _bootstrap.load()
from continual_skeletons_amd import fold  # noqa: E402

RES_MODE = s16.RES_MODE
EXACT = s16.EXACT
U = 2.0 ** -24


def _ceil_to(a, b):
    return (a + b - 1) // b * b


@dataclass(frozen=True)
class Case:
    c: int
    co: int
    V: int
    N: int
    k: int
    head_step: int              # 0: a bare CoTemporalConvolution (n_emit 1)
    n_emit: int
    res: str                    # "none" | "ident" | "conv"
    c_res: int
    wrap: bool
    relu: bool
    ksplit: int                 # as requested of the launch
    seed: int
    bare: bool = False          # the ring has exactly k slots (n_emit 1)

    @property
    def id(self):
        return (f"k{self.k}-c{self.c}-o{self.co}-hs{self.head_step}-e{self.n_emit}-{self.res}{self.c_res or ''}-v{self.V}n{self.N}"
                f"{f'-s{self.ksplit}' if self.ksplit > 1 else ''}{'-bare' if self.bare else ''}{'-wrap' if self.wrap else ''}"
                f"{'-relu' if self.relu else ''}")

    @property
    def T(self):                # frames in the ring: exactly n_emit full k-frame windows
        return self.head_step * (self.n_emit - 1) + self.k

    @property
    def NV(self):
        return self.N * self.V

    @property
    def P(self):
        return _ceil_to(self.NV, 4)

    @property
    def res_frames(self):       # residual frame of emission j: the centre of its window
        return [self.head_step * j + (self.k - 1) // 2 for j in range(self.n_emit)]


# ---- geometry: the k-aware sibling of step_split_fixture.launch_geometry ------------------------------------------------------------
def geometry(cs):
    """ring depths and slot arguments of the launch: frame f of the y ring in slot (f + rot) % slots.  For k = 9 and head_step 1 | 2
    these are the values of step_split_fixture.launch_geometry (tests/test_step32_fixture_cpu.py compares them)"""
    slots = cs.T if cs.bare else cs.T + 2
    back = 3 if cs.k >= 4 else 1                                # wrap: the window of emission 0 starts `back` slots before the end
    rot = (slots - back) % slots if cs.wrap else 1 % slots
    head = (cs.k - 1 + rot) % slots
    xs = cs.T + 1
    rc = (cs.k - 1) // 2
    xrot = (xs - 1 - rc) % xs if cs.wrap else 0                 # wrap: the first residual frame in the last slot
    out_slots = cs.n_emit + 1
    return dict(slots=slots, rot=rot, head=head, x_slots=xs, x_rot=xrot, x_slot0=(rc + xrot) % xs, out_slots=out_slots,
                out_slot0=out_slots - 1 if cs.wrap else 0)


def window_wraps(cs):
    """some emission's window crosses the end of the ring"""
    g = geometry(cs)
    return any((g["head"] + j * cs.head_step - (cs.k - 1)) % g["slots"] + cs.k > g["slots"] for j in range(cs.n_emit))


# ---- the selection of csk_tcn_step_f32, restated -------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Sel:
    MT: int
    E: int
    HS: int
    split: bool
    K9: bool
    OCC: int
    eff: int                    # ksplit_eff: the ranges the launch really has
    cper: int
    NP: int                     # positions of a tile
    g: int                      # workgroups gx * gy * gz

    @property
    def key(self):
        return (self.MT, self.E, self.HS, self.split, self.K9, self.OCC)


def split_ranges(c, ksplit):
    """mfma_core.h: cper = round_up(ceil(Cpad / ksplit), 8), ksplit_eff = ceil(c / cper) (1 for an unsplit request)"""
    cpad = _ceil_to(c, 16)
    cper = _ceil_to(-(-cpad // ksplit), 8)
    return (-(-c // cper) if ksplit > 1 else 1), cper


def select_dims(c, co, P, k, head_step, n_emit, ksplit):
    mpad = _ceil_to(co, 64)
    eff, cper = split_ranges(c, ksplit)
    big = mpad % 128 == 0
    MT = 128 if big else 64
    E = 1
    if k == 9:
        if not big and head_step == 1 and eff == 1:
            E = 4 if n_emit % 4 == 0 else 2 if n_emit % 2 == 0 else 1
        if big and 1 <= head_step <= 2:
            E = 2 if n_emit % 2 == 0 else 1
    HS = head_step if E == 2 and big and head_step == 2 else 1
    NP = 16384 // MT // E
    g = -(-P // NP) * (mpad // MT) * (n_emit // E) * eff
    occ = 3 if (not big and E == 4 and eff == 1 and k == 9 and -(-g // 768) < -(-g // 512)) else 2
    return Sel(MT, E, HS, eff > 1, k == 9, occ, eff, cper, NP, g)


def select(cs):
    return select_dims(cs.c, cs.co, cs.P, cs.k, cs.head_step, cs.n_emit, cs.ksplit)


def tile16(cs, lib=None):
    """csk_tcn_step_f32_tile: 0 when the 16x16x4 family does not take the launch"""
    lib = lib or pkg.native.lib()
    g = geometry(cs)
    return lib.csk_tcn_step_f32_tile(g["slots"], cs.head_step, cs.n_emit, g["x_slots"] if cs.res != "none" else 0, g["out_slots"], cs.c, cs.co,
                                     cs.P, cs.k, RES_MODE[cs.res], cs.c_res, cs.ksplit)


def _name(mt, e, hs, split, k9, occ=2):
    return (mt, e, hs, split, k9, occ)


EVERY = frozenset(
    [_name(64, 4, 1, False, True), _name(64, 4, 1, False, True, 3), _name(64, 2, 1, False, True), _name(64, 1, 1, False, True),
     _name(64, 1, 1, False, False), _name(64, 1, 1, True, True), _name(64, 1, 1, True, False),
     _name(128, 2, 1, False, True), _name(128, 2, 2, False, True), _name(128, 1, 1, False, True), _name(128, 1, 1, False, False),
     _name(128, 2, 1, True, True), _name(128, 2, 2, True, True), _name(128, 1, 1, True, True), _name(128, 1, 1, True, False)])
assert len(EVERY) == 15


def smallest_occ3():
    """the smallest (Mpad / 64, n_emit) at P = 4 whose launch takes the 168-register twin: odd Mpad / 64, 512 < g <= 768"""
    for mt in range(1, 64, 2):
        for n in range(4, 65, 4):
            s = select_dims(8, 64 * mt, 4, 9, 1, n, 1)
            if s.OCC == 3:
                assert 512 < s.g <= 768
                return mt, n
    raise AssertionError("no launch at P = 4 takes the OCC = 3 twin")


# ---- case tables -------------------------------------------------------------------------------------------------------------------------
def _cycle(seq, i):
    return seq[i % len(seq)]


def _res(i, co, with_ident=True):
    res = _cycle(("none", "ident", "conv") if with_ident else ("none", "conv"), i)
    return res, (0 if res == "none" else co if res == "ident" else _cycle((3, 16, 24), i // 3))


def build_unsplit_folded():
    """k = 9 at P = 4 (N V = 3: one NaN padding position; 4): the E > 1 forms and the OCC = 3 twin, which a launch below 4 GB reaches
    only here"""
    out, i = [], 0
    forms = [(64, 1, 4), (192, 1, 8), (64, 1, 2), (192, 1, 6),                 # MT = 64: E = 4 (one | two groups), E = 2 (one | three)
             (128, 1, 2), (96, 1, 4), (128, 2, 4), (96, 2, 2),                 # MT = 128: E = 2 at head_step 1 and 2; 96: 32 ragged rows
             (64, 1, 3), (128, 2, 1), (96, 1, 1)]                              # E = 1, K9 at P = 4
    for co, hs, n in forms:
        for c in (16, 20):
            res, c_res = _res(i, co)
            V, N = _cycle(((3, 1), (2, 2)), i // 2 + i)
            out.append(Case(c, co, V, N, 9, hs, n, res, c_res, wrap=i % 2 == 1, relu=i % 3 != 0, ksplit=1, seed=i))
            i += 1
    return out


def build_occ():
    """the 168-register twin <64, 4, 1, ., K9, OCC = 3> at its smallest launch, a ragged last m-tile, and the same emissions one
    group short: the other side of the boundary (OCC = 2)"""
    mt, n = smallest_occ3()
    co = 64 * mt - 23
    hi = Case(8, co, 3, 1, 9, 1, n, "conv", 3, wrap=True, relu=True, ksplit=1, seed=300)
    return [hi, replace(hi, n_emit=n - 4)]


def build_unsplit_e1():
    """k = 9, E = 1 with several position tiles: head_step 3 (and 0, the bare CoTemporalConvolution), both MT, N V = 100 and 428"""
    out, i = [], 0
    for co in (64, 128, 40, 256):
        for hs, n, bare in ((3, 1, False), (3, 3, False), (0, 1, True)):
            res, c_res = _res(i, co)
            V, N = _cycle(((25, 4), (25, 17)), i + i // 3)
            out.append(Case(_cycle((16, 24, 64), i), co, V, N, 9, hs, n, res, c_res, wrap=i % 2 == 0, relu=i % 3 != 1, ksplit=1, seed=400 + i,
                            bare=bare))
            i += 1
    return out


def build_k():
    """k != 9 (K9 = false): k 1, 2, 4, 5, 8 -- t1 / t2 / third segment empty or not in every combination -- both MT, unsplit and split,
    n_emit 1 and 3, the bare ring of exactly k slots and a deeper wrapped one"""
    out, i = [], 0
    for k in (1, 2, 4, 5, 8):
        for co in (64, 128, 40, 96):
            for ksplit in (1, 2):
                for n, bare, wrap in ((1, True, False), (3, False, True)):
                    res, c_res = _res(len(out), co)
                    c = _cycle((64, 20, 40), i) if ksplit > 1 else _cycle((16, 20, 8), i)
                    hs = 1 if n == 1 else _cycle((1, 2), i // 2)
                    V, N = _cycle(((25, 4), (25, 3), (25, 17)), i)
                    out.append(Case(c, co, V, N, k, hs, n, res, c_res, wrap=wrap, relu=i % 3 != 0, ksplit=ksplit, seed=500 + i, bare=bare))
                    i += 1
    return out


def build_split():
    """split-K, k = 9: a single chunk per split (c 16 / 2), the pipelined main loop (64 / 2: cper 32), a partial chunk then a
    padding-only chunk in the last split (20 / 2), a short last split (40 / 4: cper 16, three splits), a request above the effective
    count (16 / 32: two splits) -- crossed with the residual modes, ReLU, wrap, c_out, n_emit 1..4 at head_step 1 and 2, positions"""
    out, i = [], 0
    for c, ksplit in ((16, 2), (64, 2), (20, 2), (40, 4), (16, 32)):
        for hs, n in ((1, 1), (1, 2), (1, 3), (1, 4), (2, 2), (2, 3), (2, 1), (2, 4)):
            co = _cycle((40, 64, 96, 128, 256), i)
            res, c_res = _res(i + i // 3, co)
            V, N = _cycle(((25, 3), (25, 4), (25, 17)), i // 3 + i)
            out.append(Case(c, co, V, N, 9, hs, n, res, c_res, wrap=i % 2 == 1, relu=i % 3 != 0, ksplit=ksplit, seed=700 + i))
            i += 1
    return out


def build_collapse():
    """c = 8 / ksplit 2: the request collapses to one range.  With k = 9 the launch then goes to the 16x16x4 family, with k = 5 it stays
    here; both must equal the reference"""
    return [Case(8, 64, 25, 4, k, 1, 2, "conv", 16, wrap=True, relu=True, ksplit=2, seed=900 + k) for k in (9, 5)]


GROUPS = {"folded": build_unsplit_folded(), "occ": build_occ(), "e1": build_unsplit_e1(), "k": build_k(), "split": build_split()}
CASES = [c for t in GROUPS.values() for c in t]                 # every one of them on the 32x32x2 kernels
COLLAPSE = build_collapse()
assert len({c.id for c in CASES + COLLAPSE}) == len(CASES) + len(COLLAPSE), "duplicate case"


def one_per_instantiation(pool=None):
    """{instantiation: the first case of the tables that reaches it} -- the route and real tiers"""
    first = {}
    for cs in pool or CASES:
        first.setdefault(select(cs).key, cs)
    return first


# ---- operands --------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Ops:
    x: torch.Tensor             # (N, c, T, V)
    w: torch.Tensor             # (co, c, k, 1)
    bias: torch.Tensor          # (co,)
    x_res: torch.Tensor         # (N, c_res, T, V) or None
    w_res: torch.Tensor         # (co, c_res, 1, 1) or None


@functools.lru_cache(maxsize=None)
def operands(cs, tier="exact"):
    g = torch.Generator().manual_seed(1000 + cs.seed)
    sx, sw = (cs.N, cs.c, cs.T, cs.V), (cs.co, cs.c, cs.k, 1)
    sxr, swr = (cs.N, cs.c_res, cs.T, cs.V), (cs.co, cs.c_res, 1, 1)
    has_res, conv = cs.res != "none", cs.res == "conv"
    if tier == "exact":
        return Ops(s16._ints(g, sx, 1, 7), s16._weights(g, sw), s16._ints(g, (cs.co,), -8, 8), s16._ints(g, sxr, 1, 7) if has_res else None,
                   s16._weights(g, swr) if conv else None)
    if tier == "real":
        return Ops(torch.rand(sx, generator=g), torch.randn(sw, generator=g) * (1.0 / (cs.k * cs.c)) ** 0.5, torch.rand(cs.co, generator=g) * 0.2 - 0.1,
                   torch.rand(sxr, generator=g) if has_res else None, torch.randn(swr, generator=g) * (1.0 / cs.c_res) ** 0.5 if conv else None)
    assert tier == "route"
    nx = cs.N * cs.c * cs.T * cs.V
    nr = cs.N * cs.c_res * cs.T * cs.V if has_res else 0
    assert nx + nr + 1 < 2 ** 23                                 # ring id + residual id stays below 2**24
    x = (2 ** 23 + torch.randperm(nx, generator=g)).view(sx).float()
    w = torch.zeros(sw)
    pick = torch.randint(0, cs.c * cs.k, (cs.co,), generator=g)
    pick[: min(cs.co, cs.c * cs.k)] = torch.randperm(cs.c * cs.k, generator=g)[: cs.co]     # every (tap, channel) where the rows allow
    w[torch.arange(cs.co), pick // cs.k, pick % cs.k, 0] = 1.0
    x_res = (1 + torch.randperm(nr, generator=g)).view(sxr).float() if has_res else None
    w_res = None
    if conv:
        w_res = torch.zeros(swr)
        w_res[torch.arange(cs.co), torch.randint(0, cs.c_res, (cs.co,), generator=g), 0, 0] = 1.0
    return Ops(x, w, torch.zeros(cs.co), x_res, w_res)


def _sum(cs, x, w, bias, x_res, w_res):
    if cs.head_step == 0:
        assert cs.n_emit == 1
    y = F.conv2d(x, w, stride=(max(cs.head_step, 1), 1)) + bias[None, :, None, None]       # no padding: emission j is frames hs j .. hs j + k - 1
    assert y.shape[2] == cs.n_emit
    if cs.res == "ident":
        y = y + x_res[:, :, cs.res_frames]
    elif cs.res == "conv":
        y = y + F.conv2d(x_res[:, :, cs.res_frames], w_res)
    return y


def _emissions(cs, y):
    """(N, co, n_emit, V) -> the layout of the emissions: (n_emit, co, N V)"""
    return y.permute(2, 1, 0, 3).reshape(cs.n_emit, cs.co, cs.NV)


@functools.lru_cache(maxsize=None)
def reference(cs, tier="exact"):
    """-> (n_emit, co, N V) fp64: the emitting steps on doubles"""
    o = operands(cs, tier)
    y = _sum(cs, *[None if t is None else t.double() for t in (o.x, o.w, o.bias, o.x_res, o.w_res)])
    return _emissions(cs, torch.relu(y) if cs.relu else y)


@functools.lru_cache(maxsize=None)
def abs_sum(cs, tier="exact"):
    """sum |w| |x| + |bias| + |res terms| per output, fp64, (n_emit, co, N V)"""
    o = operands(cs, tier)
    return _emissions(cs, _sum(cs, *[None if t is None else t.double().abs() for t in (o.x, o.w, o.bias, o.x_res, o.w_res)]))


def admissible(cs, tier="exact"):
    """integer operands and sum |w| |x| + |bias| + |res| < 2**24 for every output"""
    o = operands(cs, tier)
    for t in (o.x, o.w, o.bias, o.x_res, o.w_res):
        assert t is None or (t.dtype == torch.float32 and torch.equal(t, t.round()))
    if tier == "exact":
        assert bool((o.w != 0).all()) and (o.w_res is None or bool((o.w_res != 0).all()))
    bound = float(abs_sum(cs, tier).max())
    assert bound < EXACT
    return bound


def n_terms(cs):
    return cs.k * cs.c + cs.c_res + 2


def bound(cs, tier="real"):
    """(n_terms + 4) 2**-24 sum |term| per output: the form of head_fixture.bound, n_terms = k c + c_res + 2"""
    return (n_terms(cs) + 4) * U * abs_sum(cs, tier)


def bf16_truncated(t):
    """fp32 -> the value of its upper 16 bits"""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


# ---- the launch ------------------------------------------------------------------------------------------------------------------------------
def launch(cs, tier="exact", wide_P=None):
    """host tensors and scalar arguments of the csk_tcn_step_f32 launch.  ``wide_P``: the case's positions (P == N V) repeated along the
    position axis up to wide_P positions"""
    o, P, g = operands(cs, tier), cs.P, geometry(cs)
    idx = None
    if wide_P is not None:
        assert P == cs.NV and wide_P % 4 == 0
        idx = torch.arange(wide_P) % P

    def wide(t):
        return t if idx is None else t[..., idx].contiguous()

    one = torch.ones(cs.co, dtype=torch.float64)
    ring = wide(ssf.ring_of(ssf.channel_major(o.x, P), g["slots"], g["rot"]))
    xres = None if o.x_res is None else wide(ssf.ring_of(ssf.channel_major(o.x_res, P), g["x_slots"], g["x_rot"]))
    t = dict(ring=ring, w=fold.pack_conv_weight(o.w, one), xres=xres, wres=None if o.w_res is None else fold.pack_conv_weight(o.w_res, one),
             bias=fold.pad_vec(o.bias))
    return t, dict(g, P=wide_P or P)


def partial_floats(cs, P=None):
    """the partial-sum buffer of the launch: exactly n_emit * ksplit_eff * c_out * P floats"""
    return cs.n_emit * select(cs).eff * cs.co * (P or cs.P)


# ---- the step written out, with one seeded defect at a time ------------------------------------------------------------------------------
DEFECTS = ("last_split_dropped", "wrap_off_by_one", "res_conv_every_split", "bias_every_split", "ident_from_group_head",
           "ragged_rows_in_slab", "last_tap_skipped", "head_plus_j", "reduce_requested_slabs")


def applies(defect, cs):
    """the cases the tables name as catchers of the defect"""
    sel = select(cs)
    if defect == "last_split_dropped":
        return sel.split
    if defect == "wrap_off_by_one":
        return window_wraps(cs)
    if defect == "res_conv_every_split":
        return sel.split and cs.res == "conv"
    if defect == "bias_every_split":
        return sel.split
    if defect == "ident_from_group_head":
        return sel.E > 1 and cs.res == "ident"
    if defect == "ragged_rows_in_slab":
        return sel.split and cs.co % 64 != 0 and cs.n_emit * sel.eff > 1
    if defect == "last_tap_skipped":
        return cs.k != 9
    if defect == "head_plus_j":
        return cs.head_step >= 2 and cs.n_emit > 1
    if defect == "reduce_requested_slabs":
        return sel.split and cs.ksplit != sel.eff
    raise KeyError(defect)


def model(cs, defect=None, tier="exact"):
    """-> (n_emit, co, N V) fp32: channel ranges per split, emissions folded into tile columns (E per group, window slot of emission jl's
    tap r = first + jl head_step + r modulo the ring), partial slabs then the reduce, on doubles"""
    assert defect is None or defect in DEFECTS
    sel, NV, co, k = select(cs), cs.NV, cs.co, cs.k
    t, g = launch(cs, tier)
    ring, w, bias = t["ring"].double()[..., :NV], t["w"].double(), t["bias"].double()
    xres = None if t["xres"] is None else t["xres"].double()[..., :NV]
    wres = None if t["wres"] is None else t["wres"].double()
    mpad, slots, eff = w.shape[2], g["slots"], sel.eff
    hs = 1 if defect == "head_plus_j" else cs.head_step
    taps = [r for r in range(k) if not (defect == "last_tap_skipped" and k != 9 and r == k - 1)]
    slab_rows = mpad if defect == "ragged_rows_in_slab" else co           # rows between two slabs, and rows a tile column writes
    part = torch.full((cs.n_emit * max(eff, cs.ksplit) * mpad + mpad, NV), float("nan"), dtype=torch.float64)
    out = torch.zeros((cs.n_emit, co, NV), dtype=torch.float64)

    def res_frame(j):
        return xres[(g["x_slot0"] + j * cs.head_step) % g["x_slots"]]

    def finish(j, acc):
        jr = j // sel.E * sel.E if defect == "ident_from_group_head" else j
        v = acc + bias[:co, None] + (res_frame(jr)[:co] if cs.res == "ident" else 0)
        return torch.relu(v) if cs.relu else v

    for grp in range(cs.n_emit // sel.E):
        j0 = grp * sel.E
        first = (g["head"] + j0 * hs - (k - 1)) % slots
        for ks in range(eff):
            lo = ks * sel.cper
            hi = min(cs.c, lo + sel.cper)
            if defect == "last_split_dropped" and sel.split and ks == eff - 1:
                hi = lo
            for jl in range(sel.E):
                j = j0 + jl
                acc = torch.zeros((mpad, NV), dtype=torch.float64)
                for r in taps:
                    i = first + jl * hs + r
                    slot = i % slots
                    if defect == "wrap_off_by_one" and i >= slots:
                        slot = (i + 1) % slots
                    acc += w[r, lo:hi].T @ ring[slot, lo:hi]
                if cs.res == "conv" and (ks == 0 or defect == "res_conv_every_split"):
                    acc += wres[0, : cs.c_res].T @ res_frame(j)[: cs.c_res]
                if not sel.split:
                    out[j] = finish(j, acc[:co])
                    continue
                if defect == "bias_every_split":
                    acc += bias[:mpad, None]
                base = (j * eff + ks) * slab_rows
                part[base: base + slab_rows] = acc[:slab_rows]
    if sel.split:
        nsum = cs.ksplit if defect == "reduce_requested_slabs" else eff
        for j in range(cs.n_emit):
            s = torch.zeros((co, NV), dtype=torch.float64)
            for ks in range(nsum):
                base = (j * nsum + ks) * co
                s += part[base: base + co]
            out[j] = finish(j, s)
    return out.float()
