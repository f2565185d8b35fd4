"""Activation, residual and output pointers OFF the 16-byte boundary: the allocation helper, the classification of every C-ABI entry,
the skew table, the per-entry cases and the host model of the defect, shared by tests/test_gpu_pointer_skew.py and
tests/test_skew_fixture_cpu.py.

The clip kernels move activations as 16-byte vectors and pick their aligned-row fast paths from the dims alone (T * V % 4 == 0).  The
package hands the library any contiguous float32 view (native.require_device_f32, native.ptr), so a caller's tensor may sit at any
multiple of 4 bytes: a batch slice, an ``out=`` view into an arena, a frame of a cycle.  A kernel that used the 16-byte-aligned vector
type on such a pointer could have its address rounded down to the boundary: values shifted by 1 .. 3 positions, or a store that lands
in the neighbour's memory.  Nothing crashes; only a bit-for-bit comparison and guard bands see it.

Skewed        one flat buffer (asserted 16-byte aligned), the tensor a view at GUARD + s floats, s in 0 .. 3, sentinel bands of at
              least GUARD floats on both sides: NaN around an input (a load that strays drags a NaN into the result), a finite
              distinctive value around an output (a store that strays changes a band word); bands_intact() compares bits.
ENTRIES       every name of native.SIGNATURES in exactly one class (takes_any / refuses / reroutes / no_activation_pointer).
SKEWS         (x, x_res, out) offsets in floats; single-operand entries use the projection; CONTROL is (0, 0, 0).
UNITS         per takes_any entry pinned here, the launches: cases of the entry's own fixture -- exact-integer or unique-id operands
              and the fixture's fp64 reference, unchanged -- with both row classes (T * V % 4 == 0 and != 0).
rounded_down  the defect itself on the host: the operation with ONE skewed operand read or written at its address rounded down to 16
              bytes, by slicing the guarded flat buffer; no kernel model.

Weights, packed operands and scratch are the package's own allocations and stay aligned; only caller-visible tensors are skewed.
torch and numpy only; nothing is read from csrc."""
import functools
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from tests import dense_gcn_fixture as dx
from tests import sparse_gcn_fixture as sx
from tests import tcn_direct_fixture as td
from tests import tcn_wino_fixture as tw
from tests import agcn_attention_fixture as af
from tests import head_fixture as hf
from tests import split_fixture as sf
from tests import str_unit_fixture as su

GUARD = 4096
NAN = float("nan")
OUT_SENTINEL = -65521.0                    # finite, an integer no exact-tier result and no id reaches with this sign
SKEWS = ((1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 2, 3), (3, 0, 1), (0, 3, 0), (0, 0, 2))
CONTROL = (0, 0, 0)
ALL_SKEWS = (CONTROL,) + SKEWS


def _bits(t):
    return t.contiguous().view(torch.int32)


class Skewed:
    """a float32 tensor of `shape` at GUARD + s floats of a 16-byte aligned flat buffer.  src given: an INPUT between NaN bands;
    src None: an OUTPUT, the whole buffer (payload included) the finite sentinel"""

    def __init__(self, shape, s, device="cpu", src=None):
        assert s in (0, 1, 2, 3)
        n = int(np.prod(shape))
        self.sentinel = NAN if src is not None else OUT_SENTINEL
        self.buf = torch.full((n + 2 * GUARD + 4,), self.sentinel, device=device, dtype=torch.float32)
        assert self.buf.data_ptr() % 16 == 0, "the flat buffer itself must be 16-byte aligned"
        self.s, self.n, self.lo, self.shape = s, n, GUARD + s, tuple(shape)
        self.t = self.buf[self.lo: self.lo + n].view(self.shape)
        assert self.t.data_ptr() % 16 == 4 * s and self.t.is_contiguous()
        assert self.lo >= GUARD and self.buf.numel() - (self.lo + n) >= GUARD
        if src is not None:
            self.t.copy_(torch.as_tensor(src, dtype=torch.float32).reshape(self.shape))
        self._want = _bits(torch.full((1,), self.sentinel, dtype=torch.float32)).item()

    def bands_intact(self):
        """every guard word is still bitwise the sentinel"""
        b = _bits(self.buf)
        return bool((b[: self.lo] == self._want).all()) and bool((b[self.lo + self.n:] == self._want).all())

    def rounded_down(self):
        """the tensor at this one's address rounded down to 16 bytes: what a 16-byte-aligned access would touch"""
        return self.buf[GUARD: GUARD + self.n].view(self.shape)

    def host(self):
        return self.t.detach().cpu().clone()


# ------------------------------------------------------------------------------------------------------------------------------
# classification of the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
TAKES_ANY, REFUSES, REROUTES, NO_POINTER = "takes_any", "refuses", "reroutes", "no_activation_pointer"


class Entry(NamedTuple):
    cls: str
    pinned: str = ""       # takes_any: "here" (UNITS / the package tests of test_gpu_pointer_skew.py), or the suite that runs it skewed, or
                           # "" (not run at a skewed pointer by any test yet)
    operand: str = ""      # refuses: the operand and the alignment that trigger the guard
    message: str = ""      # refuses: fragment of the library's message
    note: str = ""


HERE = "here"
ENTRIES = {
    # ---- plan, ABI, probe and pure host queries
    "csk_abi_version": Entry(NO_POINTER),
    "csk_stream_overlap_probe": Entry(NO_POINTER, note="its buffers are the probe's own scratch"),
    "csk_tcn_step_f32_tile": Entry(NO_POINTER), "csk_tcn_step_f32_route": Entry(NO_POINTER), "csk_tcn_step_bf16x3_tile": Entry(NO_POINTER),
    "csk_co_stack_step_f32_route": Entry(NO_POINTER, note="reads the blocks' scalar fields only"),
    "csk_str_unit_f32_route": Entry(NO_POINTER),
    "csk_co_plan_create": Entry(NO_POINTER), "csk_co_plan_destroy": Entry(NO_POINTER), "csk_co_plan_update_weights": Entry(NO_POINTER),
    "csk_co_plan_set_fusion": Entry(NO_POINTER), "csk_co_plan_set_delays": Entry(NO_POINTER),
    # ---- alignment picks the kernel (or the path inside it); every path computes the same sums
    "csk_gcn_stage_f32_route": Entry(REROUTES, note="dense V = 18 adjacency: dense2 at 8-byte aligned x, dense128 / general otherwise; "
                                                     "sparse: the 16x16x4 tiles need 16-byte aligned x and y"),
    "csk_gcn_stage_f32_tile": Entry(REROUTES, note="0 (not the 16x16x4 tiles) unless x and y are 16-byte aligned"),
    "csk_gcn_stage_splitk_f32_route": Entry(REROUTES, note="a request that collapses to one range answers as csk_gcn_stage_f32_route"),
    "csk_agcn_stage_framewise_f32_route": Entry(REROUTES, note="even V: 0 unless x is 8-byte aligned"),
    "csk_derive_modality_f32": Entry(REROUTES, "tests/test_gpu_modality.py", note="16-byte vectors when x and out are aligned, scalars otherwise"),
    "csk_derive_modality_frames_f32": Entry(REROUTES, "tests/test_gpu_modality.py", note="the same, over every frame and prev"),
    # ---- documented guards
    "csk_tcn_step_f32": Entry(REFUSES, operand="ring / x_res at any of 4, 8, 12 bytes", message="state pointers must be 16-byte aligned"),
    "csk_tcn_step_bf16x3": Entry(REFUSES, operand="ring / x_res / out at any of 4, 8, 12 bytes", message="state pointers must be 16-byte aligned"),
    "csk_co_block_step_f32": Entry(REFUSES, operand="xin / y_ring / out at any of 4, 8, 12 bytes", message="state pointers must be 16-byte aligned"),
    "csk_co_stack_step_f32": Entry(REFUSES, operand="a block's xin / y_ring / out at any of 4, 8, 12 bytes",
                                   message="state pointers must be 16-byte aligned"),
    "csk_fc_f32": Entry(REFUSES, operand="feat at any of 4, 8, 12 bytes when C % 4 == 0", message="16-byte aligned when C is a multiple of 4"),
    "csk_co_head_clip_f32": Entry(REFUSES, operand="pooled at any of 4, 8, 12 bytes when C % 4 == 0",
                                  message="16-byte aligned when C is a multiple of 4", note="h, entries and logits take any 4-byte alignment"),
    "csk_agcn_embed_attention_f32": Entry(REFUSES, operand="x at 4 or 12 bytes when V is even", message="activation rows must be 8-byte aligned"),
    "csk_agcn_stage_framewise_f32": Entry(REFUSES, operand="x at 4 or 12 bytes when V is even", message="8-byte aligned rows"),
    # ---- the clip kernels pinned here
    "csk_gcn_stage_f32": Entry(TAKES_ANY, HERE, note="which kernel runs may change with the alignment (see its _route entry)"),
    "csk_gcn_stage_splitk_f32": Entry(TAKES_ANY, HERE),
    "csk_conv1x1_f32": Entry(TAKES_ANY, HERE),
    "csk_tcn_stage_f32": Entry(TAKES_ANY, HERE), "csk_tcn_stage_splitk_f32": Entry(TAKES_ANY, HERE),
    "csk_tcn_stage_wino_f32": Entry(TAKES_ANY, HERE), "csk_tcn_stage_wino_ext_f32": Entry(TAKES_ANY, HERE),
    "csk_tcn_stage_wino_valid_f32": Entry(TAKES_ANY, HERE), "csk_tcn_stage_wino_valid_res_f32": Entry(TAKES_ANY, HERE),
    "csk_block_few_channels_f32": Entry(TAKES_ANY, HERE, note="through SpatioTemporalBlock(fuse_few_channels=True)"),
    "csk_input_norm_f32": Entry(TAKES_ANY, HERE), "csk_pool_fc_f32": Entry(TAKES_ANY, HERE, note="logits = NULL: the pool alone; with logits "
                                                                                                  "its FC reads the feat it wrote"),
    "csk_input_norm_frames_f32": Entry(TAKES_ANY, HERE, note="through forward_cycle with each frame at its own skew"),
    # ---- takes any 4-byte alignment by its code; run skewed by the suite named, or by none yet
    "csk_pool_scaled_f32": Entry(TAKES_ANY, HERE),
    "csk_select_people_f32": Entry(TAKES_ANY, "tests/test_gpu_keypoints.py"),
    "csk_select_people_frames_f32": Entry(TAKES_ANY, "tests/test_gpu_keypoints.py"),
    "csk_co_scrub_streams_f32": Entry(TAKES_ANY, "tests/test_gpu_stream_reset.py"),
    "csk_co_move_streams_f32": Entry(TAKES_ANY, "tests/test_gpu_stream_move.py"),
    "csk_co_prime_pack_f32": Entry(TAKES_ANY, "tests/test_gpu_stream_prime.py"),
    "csk_tcn_stage_bf16x3": Entry(TAKES_ANY, HERE, note="non-exact tier: the fixture's D / 2 bound and the bits of the (0, 0, 0) launch; packed weights guarded"),
    "csk_gcn_stage_bf16x3": Entry(TAKES_ANY, HERE, note="as csk_tcn_stage_bf16x3"),
    "csk_str_unit_f32": Entry(TAKES_ANY, HERE, note="x and y skewed, the scratch is the package's own; packed weights guarded"),
    "csk_agcn_attention_f32": Entry(TAKES_ANY, HERE, note="non-exact tier: the fixture's bound and the bits of the (0, 0, 0) launch"),
    "csk_prenorm_f32": Entry(TAKES_ANY, note="picks 16 / 8 / 4-byte accesses per address inside the kernel"),
    "csk_prenorm_frames_f32": Entry(TAKES_ANY, note="as csk_prenorm_f32"),
    "csk_ntu_intake_f32": Entry(TAKES_ANY, note="scalar accesses"),
    "csk_fuse_rank_f32": Entry(TAKES_ANY, note="strided scalar accesses"),
    "csk_co_spatial_pool_f32": Entry(TAKES_ANY, note="continual state: the package's own rings"),
    "csk_co_window_mean_f32": Entry(TAKES_ANY, note="continual state: the package's own rings"),
    "csk_co_head_step_f32": Entry(TAKES_ANY, note="continual state: the package's own rings"),
    "csk_co_plan_cycle": Entry(TAKES_ANY, HERE, note="the caller's frames reach the pre-pass frame entries (forward_cycle test); all else is the plan's"),
}

# entries whose takes_any class is asserted by launches of UNITS (kernel level); the other "here" entries run through the package tests
KERNEL_LEVEL = ("csk_gcn_stage_f32", "csk_gcn_stage_splitk_f32", "csk_conv1x1_f32", "csk_tcn_stage_f32", "csk_tcn_stage_splitk_f32",
                "csk_tcn_stage_wino_f32", "csk_tcn_stage_wino_ext_f32", "csk_tcn_stage_wino_valid_f32", "csk_tcn_stage_wino_valid_res_f32",
                "csk_tcn_stage_bf16x3", "csk_gcn_stage_bf16x3", "csk_str_unit_f32", "csk_agcn_attention_f32", "csk_input_norm_f32",
                "csk_pool_fc_f32", "csk_pool_scaled_f32")


# ------------------------------------------------------------------------------------------------------------------------------
# the launches
# ------------------------------------------------------------------------------------------------------------------------------
class Norm(NamedTuple):      # csk_input_norm_f32: x [N, C, T, V, M] -> h [N M, C, T, V]
    name: str
    n: int
    c: int
    t: int
    v: int
    m: int


class Pool(NamedTuple):      # csk_pool_fc_f32 (logits NULL) / csk_pool_scaled_f32: h [(n m), c, t v] -> feat [n, c]
    name: str
    n: int
    m: int
    c: int
    t: int
    v: int
    scale: float


class Unit(NamedTuple):
    entry: str
    kind: str          # "tcn" / "wino" / "gcn" / "conv" (as their fixtures' cases), "bf" (split_fixture.Case), "str" (str_unit_fixture.Case),
                       # "att" (agcn_attention_fixture.Att), "norm" (Norm), "pool" (Pool)
    case: object
    ksplit: int = 1    # gcn: the ranges asked of csk_gcn_stage_splitk_f32 (tcn: the case's own field)

    @property
    def name(self):
        c = self.case
        base = c.id if self.kind == "bf" else su.name(c) if self.kind == "str" else c.name
        return f"{base}" + (f" ksplit{self.ksplit}" if self.kind == "gcn" and self.ksplit > 1 else "")

    @property
    def exact(self):
        """exact tier: fp64's bits; otherwise the fixture's bound and the bits of the (0, 0, 0) launch"""
        return self.kind not in ("bf", "att")

    @property
    def rows_whole_quads(self):
        c = self.case
        if self.kind in ("tcn", "wino", "norm", "pool"):
            return (c.t * c.v) % 4 == 0
        return ((c.T if self.kind in ("bf", "att") else c.frames) * c.V) % 4 == 0

    @property
    def operands(self):
        """names of the skewed operands, in the order (x, x_res, out) of the skew table"""
        if self.kind in ("tcn", "wino"):
            return ("x", "x_res", "out") if self.case.res != "none" else ("x", "out")
        if self.kind == "bf" and self.case.kernel == "tcn":
            return ("x", "x_res", "out") if self.case.res != "none" else ("x", "out")
        return ("x", "out")                  # the graph conv's (and the S-TR unit's) residual is x itself


WINO_ENTRY = {"id": "csk_tcn_stage_wino_f32", "ext": "csk_tcn_stage_wino_ext_f32", "valid": "csk_tcn_stage_wino_valid_f32",
              "valid_res": "csk_tcn_stage_wino_valid_res_f32"}


def _tcn_units():
    """The routing tier (unique ids, one-hot weights) of tcn_direct_fixture at both row classes: per family and stride one tap, the
    conv residual alone and (stride 1) the identity residual alone; split-K the same on the 32x32 kernel.  T: V = 25 -> 20 / 52 whole
    quads, 21 / 37 not; V = 18 -> 36 / 72 whole quads, 41 / 71 not.  Every length leaves a front-border, an interior or back-border
    and a ragged last tile (tcn_direct_fixture.tiles; asserted in test_skew_fixture_cpu.py)."""
    out = []
    for fam, c, cres, shapes in (("32", 12, 20, ((25, 1, (20, 21)), (18, 2, (36, 41)))), ("16", 16, 24, ((25, 1, (52, 37)), (18, 2, (72, 71))))):
        for v, stride, ts in shapes:
            for t in ts:
                g = f"route{fam}-s{stride}"
                out.append(td.Case(g, 100 + t, c, 70, t, v, stride=stride, tier="route_tap", tap=1 + 5 * (t % 2)))
                out.append(td.Case(g, 200 + t, c, 70, t, v, stride=stride, res="conv", c_res=cres, tier="route_conv"))
                if stride == 1:
                    out.append(td.Case(g, 300 + t, c, 70, t, v, res="identity", c_res=70, tier="route_ident"))
    units = [Unit("csk_tcn_stage_f32", "tcn", c) for c in out]
    for t in (20, 21):
        g = "route32-other"
        units.append(Unit("csk_tcn_stage_splitk_f32", "tcn", td.Case(g, 100 + t, 40, 70, t, 25, ksplit=3, tier="route_tap", tap=4)))
        units.append(Unit("csk_tcn_stage_splitk_f32", "tcn", td.Case(g, 200 + t, 40, 70, t, 25, ksplit=3, res="identity", c_res=70, tier="route_ident")))
        units.append(Unit("csk_tcn_stage_splitk_f32", "tcn", td.Case(g, 300 + t, 40, 70, t, 25, ksplit=3, res="conv", c_res=20, tier="route_conv")))
    return units


def _wino_units():
    """The routing tier of tcn_wino_fixture: per kernel (padded stride 1, valid, stride 2) one tap and each residual form alone, at a
    frame count with whole-quad rows and one without, V = 25 and 18"""
    cases = []
    for t in (52, 29):                                   # padded stride 1, V = 25
        cases.append(tw.Case("route-s1", 100 + t, "id", 12, 64, t, 25, res="identity", c_res=64, tier="route_tap", tap=2))
        cases.append(tw.Case("route-s1", 200 + t, "ext", 12, 64, t, 25, tier="route_tap", tap=7))
        cases.append(tw.Case("route-s1", 300 + t, "id", 12, 64, t, 25, res="identity", c_res=64, tier="route_res"))
    for t in (36, 35):                                   # ... V = 18 (35 * 18 % 4 == 2)
        cases.append(tw.Case("route-s1", 400 + t, "id", 12, 128, t, 18, res="identity", c_res=128, tier="route_tap", tap=5))
        cases.append(tw.Case("route-s1", 500 + t, "ext", 12, 128, t, 18, tier="route_tap", tap=0))
    for v, ts in ((18, (26, 25)), (25, (20, 31))):       # valid
        for t in ts:
            cases.append(tw.Case("route-valid", 100 + t, "valid", 12, 128, t, v, tier="route_tap", tap=3))
            cases.append(tw.Case("route-valid", 200 + t, "valid", 12, 128, t, v, res="identity", c_res=128, tier="route_res"))
            cases.append(tw.Case("route-valid", 300 + t, "valid_res", 12, 128, t, v, res="conv", c_res=48, tier="route_res"))
    for v, ts in ((25, (52, 35)), (18, (36, 43))):       # stride 2
        for t in ts:
            cases.append(tw.Case("route-s2", 100 + t, "ext", 12, 128, t, v, stride=2, tier="route_tap", tap=6))
            cases.append(tw.Case("route-s2", 200 + t, "ext", 12, 128, t, v, stride=2, res="conv", c_res=24, tier="route_res"))
    return [Unit(WINO_ENTRY[c.entry], "wino", c) for c in cases]


def _gcn_units():
    """sparse_gcn_fixture cases (exact tier), rows packed (no pads: the row class follows from T * V alone): both tile heights, both
    residuals, V = 25 and 18, c_in = 3 (element-wise staging) and >= 8 (16-byte staging), several position tiles with a ragged last one"""
    I, C = dx.RES_IDENTITY, dx.RES_CONV
    cs = [sx.sp(25, 52, 64, 64, I, 2), sx.sp(25, 47, 64, 64, I, 2),                      # 1300 / 1175 positions: five tiles of 256
          sx.sp(25, 20, 8, 64, C, 2), sx.sp(25, 11, 3, 64, C, 2),
          sx.sp(18, 36, 128, 128, I, 1, (1, 1, 3)), sx.sp(25, 47, 128, 128, I, 2),         # 128-row tiles of 128 positions
          sx.sp(18, 10, 40, 128, C, 2, ell_w=4), sx.sp(18, 15, 40, 130, C, 1, (1, 1, 3))]
    units = [Unit("csk_gcn_stage_f32", "gcn", c) for c in cs]
    for c, ks in ((sx.sp(25, 12, 64, 64, I, 3), 4), (sx.sp(25, 11, 64, 64, I, 3), 4),
                  (sx.sp(18, 10, 128, 64, C, 2, (1, 1, 3)), 6), (sx.sp(18, 15, 128, 128, I, 2, (1, 1, 3)), 6)):
        units.append(Unit("csk_gcn_stage_splitk_f32", "gcn", c, ks))
    for v, ci, co, fr in ((25, 16, 96, 16), (25, 17, 48, 31), (18, 40, 384, 10), (18, 3, 48, 31)):
        units.append(Unit("csk_conv1x1_f32", "conv", dx.Conv(f"conv-V{v}-ci{ci}-co{co}-T{fr}", v, ci, co, fr, 2, 0, 0)))
    return units


def _more_units():
    """bf16x3 (split_fixture: designed pieces, hot pairs in chunk 0, where the first elements of x live), the S-TR unit (dense layout,
    designed tie sets), the A-GCN attention (clip form, integer embeddings), input norm and the two pools (head_fixture)"""
    u = []
    for t in (20, 21):
        u.append(Unit("csk_tcn_stage_bf16x3", "bf", sf.Case("tcn", 64, 64, 25, t, 2, 1, hot=((4, 0),), res="ident", c_res=64)))
        u.append(Unit("csk_gcn_stage_bf16x3", "bf", sf.Case("gcn", 64, 128, 25, t, 2, hot=((1, 0),), res="conv", res_hot=(0,))))
    for t in (40, 41):
        u.append(Unit("csk_tcn_stage_bf16x3", "bf", sf.Case("tcn", 128, 128, 25, t, 2, 2, hot=((7, 0),), res="conv", res_hot=(0,), c_res=64)))
    for t in (30, 15):
        u.append(Unit("csk_tcn_stage_bf16x3", "bf", sf.Case("tcn", 130, 70, 18, t, 2, 2, hot=((3, 0),))))
        u.append(Unit("csk_gcn_stage_bf16x3", "bf", sf.Case("gcn", 128, 128, 18, t, 2, hot=((2, 0),), res="ident")))
    for c in (su.Case(48, 64, 18, 3, 16, "dense", 0), su.Case(48, 64, 18, 3, 15, "dense", 0),       # 288 / 270 columns: two column tiles
              su.Case(64, 64, 25, 3, 12, "dense", 1), su.Case(64, 64, 25, 3, 11, "dense", 1)):      # 300 / 275, the skip connection
        u.append(Unit("csk_str_unit_f32", "str", c))
    for T, inter, V, n in ((64, 6, 18, 2), (63, 6, 18, 2), (64, 16, 25, 2), (65, 16, 25, 2)):        # around the 64-frame chunk
        u.append(Unit("csk_agcn_attention_f32", "att", af.Att(f"att-T{T}-i{inter}-V{V}", n, inter, T, V, 0, 0)))
    for n, c, t, v, m in ((2, 3, 16, 25, 2), (2, 3, 5, 25, 2), (1, 2, 10, 18, 1), (3, 4, 7, 18, 3)):
        u.append(Unit("csk_input_norm_f32", "norm", Norm(f"norm-N{n}-C{c}-T{t}-V{v}-M{m}", n, c, t, v, m)))
    for t, v in ((4, 25), (3, 25), (36, 18), (57, 9)):                                             # 100 / 75 / 648 / 513 positions
        u.append(Unit("csk_pool_fc_f32", "pool", Pool(f"pool-fc-T{t}-V{v}", 3, 2, 5, t, v, 1.0)))
        u.append(Unit("csk_pool_scaled_f32", "pool", Pool(f"pool-scaled-T{t}-V{v}", 3, 2, 5, t, v, 0.75)))
    return u


UNITS = _tcn_units() + _wino_units() + _gcn_units() + _more_units()


def units_of(entry):
    return [u for u in UNITS if u.entry == entry]


# ------------------------------------------------------------------------------------------------------------------------------
# operands and references: the fixtures' own, unchanged; apply() is the same definition as a function of the activation operands
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_operands(unit):
    """-> dict: "x" (the activations the kernel reads), "x_res" (temporal convs: the block input, where there is a residual), as float32
    tensors in the layout the launch gets, plus the fixture's own operands under "ops" """
    c = unit.case
    if unit.kind in ("tcn", "wino"):
        d = (td if unit.kind == "tcn" else tw).operands(c)
        out = dict(ops=d, x=d["y"])
        if "x" in d:
            out["x_res"] = d["x"]
        return out
    if unit.kind == "bf":
        fx = sf.build(c)
        out = dict(ops=fx, x=fx.x, an=sf.analyse(fx))
        if c.kernel == "tcn" and c.res != "none":
            out["x_res"] = fx.x_res
        return out
    if unit.kind == "str":
        ops = su.exact_operands(c, "designed")
        su.admissible(c, ops)
        return dict(ops=ops, x=torch.from_numpy(np.ascontiguousarray(ops["x"], dtype=np.float32)))
    if unit.kind == "att":
        E, a_sum = af.att_operands(c.n, c.inter, c.T, c.V, 0)
        af.admissible(E, c.inter)
        return dict(ops=dict(a_sum=a_sum), x=torch.from_numpy(E))
    if unit.kind == "norm":
        rng = np.random.default_rng(c.n + 10 * c.t + 100 * c.v)
        x = hf.exact_operand(rng, (c.n, c.c, c.t, c.v, c.m))
        scale, shift = hf.distinct_affine(rng, c.m * c.v * c.c)
        return dict(ops=dict(scale=scale, shift=shift), x=torch.from_numpy(x))
    if unit.kind == "pool":
        rng = np.random.default_rng(c.t * c.v)
        k, rows = hf.exact_mean_rows(rng, c.n * c.c, c.m * c.t * c.v)
        h = np.ascontiguousarray(np.transpose(rows.reshape(c.n, c.c, c.m, c.t * c.v), (0, 2, 1, 3))).reshape(c.n * c.m, c.c, c.t * c.v)
        return dict(ops=dict(k=k.reshape(c.n, c.c)), x=torch.from_numpy(h))
    ops = dx.operands(c, "exact") if unit.kind == "gcn" else dx.conv_operands(c, "exact")
    return dict(ops=ops, x=torch.from_numpy(ops["x"]))


def out_shape(unit):
    c = unit.case
    if unit.kind in ("tcn", "wino"):
        return (c.n, c.co, c.t_out, c.v)
    if unit.kind == "bf":
        return (c.N, c.co, c.t_out, c.V)
    if unit.kind == "att":
        return (c.n, 3, c.V, c.V)
    if unit.kind == "norm":
        return (c.n * c.m, c.c, c.t, c.v)
    if unit.kind == "pool":
        return (c.n, c.c)
    return (c.n_seg, c.c_out, c.frames, c.V)


@functools.lru_cache(maxsize=None)
def expected(unit):
    """the fixture's reference: exact units a float32 tensor (the bits), the others fp64"""
    c = unit.case
    h = host_operands(unit)
    if unit.kind == "tcn":
        return td.routing_expected(c) if c.tier != "exact" else td.reference(c)
    if unit.kind == "wino":
        return (tw.routing_expected(c) if c.tier != "exact" else tw.reference(c)).float()
    if unit.kind == "bf":
        return h["an"]["want"]
    if unit.kind == "str":
        ops = h["ops"]
        want = su.y64(c, ops, su.o64(c, su.qkv64(c, ops)[0])[0])[0]
        assert su.is_f32(want), unit.name
        return torch.from_numpy(want.astype(np.float32)).view(out_shape(unit))
    if unit.kind == "att":
        return torch.from_numpy(af.reference(h["x"].numpy(), h["ops"]["a_sum"], c.inter)[0])
    if unit.kind == "norm":
        return torch.from_numpy(hf.ref_input_norm(h["x"].numpy(), h["ops"]["scale"], h["ops"]["shift"]).astype(np.float32))
    if unit.kind == "pool":
        s = hf.ref_pool_sum(h["x"].numpy(), c.n, c.m)
        assert np.array_equal(hf.ref_pool(h["x"].numpy(), c.n, c.m), h["ops"]["k"]), unit.name
        return torch.from_numpy(np.asarray(hf.exact_pool_bits(s, c.m * c.t * c.v, c.scale), dtype=np.float32))
    ops = h["ops"]
    want, mag = dx.reference(c, ops) if unit.kind == "gcn" else dx.conv_reference(c, ops)
    assert float(mag.max()) < 2 ** 24, unit.name
    return torch.from_numpy(want.astype(np.float32))


def apply(unit, x, x_res=None):
    """the definition on doubles as a function of the activation operands (what rounded_down feeds moved operands to); with the
    fixture's own operands it is expected(unit) (test_skew_fixture_cpu.py)"""
    c, d = unit.case, host_operands(unit)["ops"]
    if unit.kind in ("tcn", "wino"):
        s = c.stride
        out = F.conv2d(x.double(), d["w"].double(), d["bias"].double(), stride=(s, 1), padding=(c.pad, 0))
        if c.res != "none":
            xr = x_res.double()[:, :, c.res_off::s][:, :, : c.t_out]
            out = out + (xr if c.res == "identity" else F.conv2d(xr, d["wres"].double()))
        return (torch.relu(out) if c.relu else out).float()
    with np.errstate(invalid="ignore"):
        if unit.kind == "bf":
            if c.kernel == "tcn":
                out = sf.conv64(d.w, x, c.stride, sf.PAD_TCN)
                if c.res == "ident":
                    out = out + x_res.double()
                elif c.res == "conv":
                    out = out + sf.conv64(d.w_res, x_res, c.stride, 0)
                return out
            src = [d.adj[r].argmax(0) for r in range(3)]
            out = sf.conv64(d.groups[0].w, torch.cat([x[..., j] for j in src], 1), 1, 0)
            return out + (x.double() if c.res == "ident" else sf.conv64(d.w_res, x, 1, 0))
        if unit.kind == "str":
            ops = dict(d, x=x.numpy().reshape(np.shape(d["x"])))
            return torch.from_numpy(su.y64(c, ops, su.o64(c, su.qkv64(c, ops)[0])[0])[0].astype(np.float32)).view(out_shape(unit))
        if unit.kind == "att":
            return torch.from_numpy(af.reference(x.numpy(), d["a_sum"], c.inter)[0])
        if unit.kind == "norm":
            return torch.from_numpy(hf.ref_input_norm(x.numpy(), d["scale"], d["shift"]).astype(np.float32))
        if unit.kind == "pool":
            s = hf.ref_pool_sum(x.numpy(), c.n, c.m)
            return torch.from_numpy(np.asarray((s.astype(np.float32) / np.float32(c.m * c.t * c.v)) * np.float32(c.scale), dtype=np.float32))
        ops = dict(d, x=x.numpy())
        want = (dx.reference(c, ops) if unit.kind == "gcn" else dx.conv_reference(c, ops))[0]
    return torch.from_numpy(want.astype(np.float32))


def matches(unit, got):
    """the check of the unit's tier on a float32 result: the reference's bits, or finite and inside the fixture's own bound"""
    want = expected(unit)
    if unit.exact:
        return same_bits(got, want)
    if not bool(torch.isfinite(got).all()):
        return False
    if unit.kind == "bf":
        an = host_operands(unit)["an"]
        return int((got.double()[~an["nz"]] != 0).sum()) == 0 and sf.rel_err(got, an["want"], an["nz"]) <= an["tol"]
    c, h = unit.case, host_operands(unit)
    bnd = af.reference(h["x"].numpy(), h["ops"]["a_sum"], c.inter)[1]
    return bool((np.abs(got.double().numpy() - want.numpy()) <= bnd).all())


def skew_of(unit, skew):
    """the projection of an (x, x_res, out) triple on the unit's operands -> {operand: offset in floats}"""
    full = dict(zip(("x", "x_res", "out"), skew))
    return {k: full[k] for k in unit.operands}


def rounded_down(unit, skew, which):
    """The defect on the host: operand `which` accessed at its address rounded down to 16 bytes, every other operand where it is.
    -> (the output tensor as the caller sees it, all guard bands intact)"""
    h, sk = host_operands(unit), skew_of(unit, skew)
    x = Skewed(h["x"].shape, sk["x"], src=h["x"])
    xr = Skewed(h["x_res"].shape, sk["x_res"], src=h["x_res"]) if "x_res" in sk else None
    out = Skewed(out_shape(unit), sk["out"])
    res = apply(unit, x.rounded_down() if which == "x" else x.t, None if xr is None else (xr.rounded_down() if which == "x_res" else xr.t))
    (out.rounded_down() if which == "out" else out.t).copy_(res.float())
    return out.host(), all(g.bands_intact() for g in (x, xr, out) if g is not None)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))
