"""co_stack16_kernel (csrc/step16.hip) at the C ABI -- csk_co_block_step_f32 and csk_co_stack_step_f32 only -- against the fp64 clip
reference of tests/co_stack_fixture.py, driven cycle by cycle through wrapping rings.  Every test asserts FIRST, through
csk_co_stack_step_f32_route (the function the launcher switches on), that the call is the one fused launch (or the per-block launches,
or the family's two stages) the case is there for; after every launch the guard bands and every ring slot the cycle does not write must
keep their NaN bits.  Exact tier: torch.equal, tolerance 0.  Bound tier: stage by stage from what the device left in the rings, under
the bounds DESIGN.md derives for the graph conv and the step; the achieved error / bound goes to the parity report.
tests/test_co_stack_fixture_cpu.py proves the cases on the CPU."""
import ctypes

import pytest
import torch

import _bootstrap
from tests import co_stack_fixture as fx
from tests.helpers import check_parity

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native = pkg.native
DEV = "cuda:0"
NAN_BITS = 0x7FC00000


def _launch(c, k, st, packed, per_block=False):
    """cycle k through the entry the case names (``per_block``: one csk_co_stack_step_f32 call of one block per block)"""
    lib, stream = native.lib(), native.stream_of(st.x[0])
    arr = fx.block_args(c, k, st, packed)
    if per_block:
        for i in range(c.n):
            native.check(lib.csk_co_stack_step_f32(1, ctypes.cast(ctypes.byref(arr[i]), ctypes.c_void_p), c.n_skel, c.V, c.P, stream),
                         "csk_co_stack_step_f32")
    elif c.entry == "block":
        a = arr[0]
        cnt = (ctypes.c_int32 * 3)(*packed["ell_cnt"])
        native.check(lib.csk_co_block_step_f32(a.xin, a.xin_slots, a.xin_slot0, a.c_in, a.gcn_w, a.gcn_bias, a.ell_src, a.ell_val,
                                               ctypes.cast(cnt, ctypes.c_void_p), a.ell_w, a.gcn_res_mode, a.y_ring, a.y_slots, a.y_slot0,
                                               a.tcn_w, a.tcn_bias, a.res_mode, a.x_res_slot0, a.out, a.out_slots, a.out_slot0, a.c_out,
                                               c.n_skel, c.V, c.P, stream), "csk_co_block_step_f32")
    else:
        native.check(lib.csk_co_stack_step_f32(c.n, ctypes.cast(arr, ctypes.c_void_p), c.n_skel, c.V, c.P, stream), "csk_co_stack_step_f32")
    torch.cuda.synchronize()


def _guards_intact(st):
    return all(bool((fx._bits(b[: fx.GUARD]) == NAN_BITS).all()) and bool((fx._bits(b[-fx.GUARD:]) == NAN_BITS).all()) for b in st.bufs)


def _drive(c, ops, ref, after, snapshots=True, per_block=False):
    """the case's cycles on the device; ``after(st, k)`` compares after every launch"""
    st, packed = fx.init_state(c, ops, ref, device=DEV), fx.pack_ops(c, ops, DEV)
    for k in range(c.cycles):
        fx.prepare_cycle(c, ops, st, k)
        before = [b.clone() for b in st.bufs] if snapshots else None
        _launch(c, k, st, packed, per_block)
        assert _guards_intact(st), f"cycle {k}: a guard band was written"
        if snapshots:
            assert fx.untouched(c, before, st, k) is None, fx.untouched(c, before, st, k)
        after(st, k)
    return st


@pytest.mark.parametrize("c", fx.CASES, ids=lambda c: c.id)
def test_cycles_equal_the_fp64_clip_reference(c):
    """one dense block over the fused domain, stacks of 2 - 4 sparse blocks, the two-stage routes and the stack edges: y and out of
    every block and frame equal the reference bit for bit, in every cycle (positions below n_skel V; nothing about the padding)"""
    assert c.tier != "real" and fx.route(c) == (0, c.want_route())
    ops = fx.make_ops(c)
    ref = fx.reference(c, ops)

    def after(st, k):
        bad = fx.compare_exact(c, ref, st, k)
        assert bad is None, bad
    _drive(c, ops, ref, after)


@pytest.mark.parametrize("c", fx.PRODUCTION, ids=lambda c: c.id)
def test_production_width_stack_equals_the_reference_of_its_base_skeletons(c):
    """512 workgroups, two per CU, in different stages side by side (what stage_handoff is for): 2048 / 2047 skeletons repeat a
    7-skeleton exact case (expanded on the device); 3 blocks, 2 cycles; every skeleton equals its base skeleton's reference"""
    assert fx.route(c) == (0, [1, c.V, 512, 1, 1, 1, -1])
    ops = fx.make_ops(c)
    ref = fx.reference(c, ops)

    def after(st, k):
        bad = fx.compare_exact(c, ref, st, k)
        assert bad is None, bad
    _drive(c, ops, ref, after, snapshots=False)


@pytest.mark.parametrize("c", fx.BOUND, ids=lambda c: c.id)
def test_real_valued_stack_stage_by_stage_under_the_derived_bounds(c):
    """dense real-valued stacks at 64 channels: every stage against fp64 of the slots the device itself read -- graph conv within
    (4 + 3 c_pad + 4) 2^-24 sum |term|, step within (9 c + c_res + 6) 2^-24 sum |term|"""
    assert fx.route(c) == (0, c.want_route()) and c.whole
    ops = fx.make_ops(c)
    ref = fx.reference(c, ops)
    worst = {}

    def after(st, k):
        for i, stage, ratio in fx.stage_ratios(c, ops, st, k):
            worst[(i, stage)] = max(worst.get((i, stage), 0.0), ratio) if ratio == ratio else ratio
    _drive(c, ops, ref, after)
    assert len(worst) == 2 * c.n
    print({f"{i}{s}": round(r, 4) for (i, s), r in worst.items()})
    zero = torch.zeros(1)
    for (i, stage), ratio in sorted(worst.items()):
        # (the compared quantity is err / bound: the tolerance is 1)
        check_parity(torch.tensor([ratio]), zero, tol=1.0, case=c.id, block=i, stage=stage, quantity="err / derived bound")


@pytest.mark.parametrize("pair", fx.INVARIANCE, ids=lambda p: p[0].id)
def test_a_skeleton_does_not_depend_on_the_others_in_the_launch(pair):
    """real-valued data: the same three skeletons alone (one ragged workgroup) and inside 11 (several workgroups): the same bits"""
    small, big = pair
    assert fx.route(small) == (0, small.want_route()) and fx.route(big) == (0, big.want_route()) and small.grid < big.grid
    ops = fx.make_ops(big)
    ref = fx.reference(big, ops)
    ops3 = fx.Ops(ops.x[:, :, :3], ops.A, ops.gw, ops.gb, ops.tw, ops.tb)
    ref3 = [{k: v[:, :, :3] for k, v in stage.items()} for stage in ref]
    kept = {}

    def keep(tag, c):
        def after(st, k):
            kept[(tag, k)] = [r.clone() for r in st.x[1:] + st.y]
        return after
    _drive(big, ops, ref, keep("big", big))
    _drive(small, ops3, ref3, keep("small", small))
    for k in range(small.cycles):
        for a, b in zip(kept[("small", k)], kept[("big", k)]):
            a, b = a[:, :, : small.Q], b[:, :, : small.Q]
            assert torch.equal(fx._bits(a), fx._bits(b))
            live = a[~torch.isnan(a)]
            assert live.numel() and not torch.equal(live, live.round())


@pytest.mark.parametrize("c", fx.BOUND[2:4], ids=lambda c: c.id)
def test_one_launch_gives_the_bits_of_the_per_block_calls(c):
    """the one kernel-against-kernel check, on top of the references: the fused stack and one call per block on the same rings"""
    assert fx.route(c)[1][0] == 1 and all(fx.route(c, blocks=[i]) == (0, [1, c.nb, c.grid, 1, -1, -1, -1]) for i in range(c.n))
    ops = fx.make_ops(c)
    ref = fx.reference(c, ops)
    kept = {}

    def keep(tag):
        def after(st, k):
            kept[(tag, k)] = [b.clone() for b in st.bufs]
        return after
    _drive(c, ops, ref, keep("one"))
    _drive(c, ops, ref, keep("each"), per_block=True)
    for k in range(c.cycles):
        assert all(torch.equal(fx._bits(a), fx._bits(b)) for a, b in zip(kept[("one", k)], kept[("each", k)]))
