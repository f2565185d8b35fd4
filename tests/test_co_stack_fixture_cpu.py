"""tests/co_stack_fixture.py without a GPU: every exact case is admissible at every stage of every block (integers, sum |term| <
2**24, the ReLU condition), the real-valued cases keep their derived bounds below half of the smallest term, the host model of the
cycle reproduces the clip reference through the rings and every seeded defect fails every case named for it, the cases reach every
answer of csk_co_stack_step_f32_route (the function the launcher switches on), every wrap kind and every grid residue, and the query
refuses what the entry refuses, with the same message."""
import ast
import ctypes
import os

import pytest
import torch

import _bootstrap
from tests import co_stack_fixture as fx

pkg = _bootstrap.load()
native = pkg.native
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT_CASES = fx.CASES + fx.PRODUCTION[::3]
_memo = {}


def _ops_ref(c):
    if c.id not in _memo:
        ops = fx.make_ops(c)
        _memo[c.id] = (ops, fx.reference(c, ops))
    return _memo[c.id]


@pytest.mark.parametrize("c", EXACT_CASES, ids=lambda c: c.id)
def test_exact_case_is_admissible_at_every_stage(c):
    ops, ref = _ops_ref(c)
    top = fx.admissible(c, ops)
    assert top < fx.EXACT
    assert len(ref) == c.n and tuple(ref[-1]["out"].shape) == (c.T, c.chans[-1], c.S, c.V)
    # the rings hold what the kernel is handed: integers or NaN, NaN padding, NaN guards
    st = fx.init_state(c, ops, ref)
    fx.prepare_cycle(c, ops, st, 0)
    for buf in st.bufs:
        real = buf[~torch.isnan(buf)]
        assert torch.equal(real, real.round()) and bool(torch.isnan(buf[: fx.GUARD]).all()) and bool(torch.isnan(buf[-fx.GUARD:]).all())
    assert all(bool(torch.isnan(r[:, :, c.Q:]).all()) for r in st.x + st.y)
    s = fx.slots_of(c, 0)
    for i in range(c.n):
        assert all(bool(torch.isnan(st.y[i][(s[i]["y"] + f) % c.ys[i]]).all()) for f in range(4))
        assert all(bool(torch.isnan(st.x[i + 1][(s[i]["out"] + f) % c.xs[i + 1]]).all()) for f in range(4))
        assert not bool(torch.isnan(st.x[i][s[i]["xres"]][:, : c.Q]).any())
    packed = fx.pack_ops(c, ops)
    assert packed["ell_cnt"] == [1, 1, 4] and packed["ell_w"] == 4
    for i, b in enumerate(packed["blocks"]):
        assert float(b["gw"].abs().sum()) == float(ops.gw[i].abs().sum()) and float(b["tw"].abs().sum()) == float(ops.tw[i].abs().sum())


def test_sparse_weights_use_every_channel_and_tap_and_differ_per_block():
    for c in (c for c in fx.CASES if c.tier == "sparse"):
        ops, _ = _ops_ref(c)
        for i in range(c.n):
            gw, tw = ops.gw[i], ops.tw[i]
            assert bool(((gw != 0).sum(1) == 1).all()) and bool(((tw != 0).sum((1, 2)) == 2).all()), c.id
            assert bool((gw != 0).any(2).any(0).all()) and bool((tw != 0).any(0).any(1).all()) and bool((tw != 0).any(0).any(0).all()), c.id
            rows = {tuple(r.nonzero().flatten().tolist()) for r in tw}
            assert len(rows) == tw.shape[0], c.id                                   # the non-zero positions differ per row
            if i and gw.shape == ops.gw[i - 1].shape:
                assert not torch.equal(gw != 0, ops.gw[i - 1] != 0) and not torch.equal(tw != 0, ops.tw[i - 1] != 0), c.id
        assert set(ops.A.unique().tolist()) == {0.0, 1.0}


@pytest.mark.parametrize("c", fx.BOUND + [b for pair in fx.INVARIANCE for b in pair], ids=lambda c: c.id)
def test_real_case_bounds_are_below_half_the_smallest_term(c):
    ops, _ = _ops_ref(c)
    rows = fx.margin(c, ops)
    assert len(rows) == 2 * c.n
    for i, stage, bound, small in rows:
        assert 0 < bound < small / 2, (c.id, i, stage, bound, small)
    assert fx.gcn_depth(64) == 200 and fx.step_depth(64, True) == 646 and fx.step_depth(64, False) == 582


@pytest.mark.parametrize("c", fx.CASES + fx.BOUND, ids=lambda c: c.id)
def test_host_model_gives_the_reference_and_every_seeded_defect_fails(c):
    """the cycle model drives the rings exactly as the GPU test drives the device; clean, the case's own comparison passes (the ring
    placement of the fixture is right); with a defect it fails on every case named for the defect"""
    ops, ref = _ops_ref(c)
    assert fx.host_run(c, ops, ref) is None
    for d in fx.DEFECTS:
        if fx.named_for(c, d):
            assert fx.host_run(c, ops, ref, d) is not None, (c.id, d)


def test_every_defect_has_cases_in_both_tiers():
    for d in fx.DEFECTS:
        assert sum(fx.named_for(c, d) for c in fx.CASES) >= 3, d
        if d != "ragged":
            assert any(fx.named_for(c, d) for c in fx.BOUND), d
    assert any(fx.named_for(c, "ragged") for c in fx.BOUND)


def test_every_route_wrap_kind_and_grid_residue_is_reached():
    lib = native.lib()
    every = fx.CASES + fx.BOUND + fx.PRODUCTION + [b for pair in fx.INVARIANCE for b in pair]
    for c in every:                                                   # the route is the case's, in every cycle
        for k in range(c.cycles):
            assert fx.route(c, k, lib) == (0, c.want_route()), (c.id, k)
    routes = [c.want_route() for c in fx.CASES]
    assert {r[0] for r in routes} == {0, 1} and {r[1] for r in routes} == {0, 18, 25}
    assert {tuple(r[3:]) for r in routes} >= {(1, -1, -1, -1), (1, 1, -1, -1), (1, 1, 1, -1), (1, 1, 1, 1), (0, -1, -1, -1), (0, 0, -1, -1),
                                              (0, 1, 1, 1)}
    fused = [c for c in fx.CASES if c.whole]
    assert {(c.chans[0], r) for c in fused if c.n == 1 for r in c.res} >= {(16, "none"), (16, "ident"), (32, "ident"), (48, "none"), (64, "ident")}
    assert {c.chans[0] for c in fused} == {16, 32, 48, 64} and {c.entry for c in fused} == {"block", "stack"}
    for V, nb in ((25, 25), (18, 18)):
        cs = [c for c in fused if c.V == V]
        assert {c.nb for c in cs} == {nb} and {c.n for c in cs} == {1, 2, 3, 4}
        grids = {c.grid for c in cs}
        assert grids >= {1, 2, 3, 8} and (V == 18 or 9 in grids)
        assert any(c.Q % (4 * nb) == 0 and c.P == c.Q for c in cs) and any(c.Q % (4 * nb) for c in cs)      # whole and ragged tiles
        assert any(c.P - c.Q >= 4 and c.Q == 4 * nb for c in cs)                                           # a tile of padding only
    assert {c.grid % 8 for c in fused} >= {0, 1, 2, 3}
    v4 = {c.P: c.nb for c in fused if c.V == 4}
    assert v4 == {18432: 18, 18436: 25}                               # either side of the width's choice
    # every wrap kind, in different cycles of one case, and deeper rings whose slot counts are no multiples of 4
    for c in fused:
        kinds = [fx.wraps_of(c, k) for k in range(c.cycles)]
        if c.cycles >= 4 and c.xs[0] == 8:
            assert set().union(*kinds) == {"xin", "y", "window", "res", "out"}, c.id
            assert c.ys[0] == 12 and c.xs[-1] == 4 and all(x == 8 for x in c.xs[:-1])
    deep = [c for c in fused if c.xs[0] % 4 and c.ys[0] % 4 and c.xs[-1] % 4]
    assert len(deep) >= 3 and all(set().union(*[fx.wraps_of(c, k) for k in range(c.cycles)]) >= {"xin", "y", "window", "out"} for c in deep)
    # the two-stage form: graph-conv runs of 1, 2, 3 and 4 frames; c_out 8 and 40, a conv gcn_residual, V = 7
    fall = [c for c in fx.CASES if not any(c.fused)]
    assert {r for c in fall for k in range(c.cycles) for i in range(c.n) for r in fx.gcn_runs(c, k, i)} == {1, 2, 3, 4}
    assert {c.chans[-1] for c in fall} >= {8, 40} and any(c.gcn_res(0) == "conv" for c in fall) and any(c.V == 7 for c in fall)
    # stack edges: alternating block residuals, a stack whose first block is not fusable
    assert any(c.n >= 3 and set(c.res) == {"none", "ident"} and c.whole for c in fx.CASES)
    assert any(c.fused == (0, 1, 1, 1) for c in fx.CASES)
    assert {(c.V, c.n_skel) for c in fx.PRODUCTION} == {(V, s) for V in (25, 18) for s in (2048, 2047)}
    assert all(c.n == 3 and c.cycles == 2 and c.base_skel == 7 and c.grid == 512 for c in fx.PRODUCTION)
    assert {(c.n, c.V) for c in fx.BOUND} == {(n, V) for n in (2, 3, 4) for V in (25, 18)} and all(c.cycles == 3 and c.chans[0] == 64 for c in fx.BOUND)


def test_query_refuses_what_the_entry_refuses_with_the_same_message():
    lib = native.lib()
    assert len(native.SIGNATURES["csk_co_stack_step_f32_route"]) == 6 and native.CO_ROUTE_WORDS == 7
    c = next(c for c in fx.CASES if c.id == "stack3-c64-v18-s7")
    out = (ctypes.c_int32 * native.CO_ROUTE_WORDS)()

    def both(mutate=None, n=None, n_skel=c.n_skel, V=c.V, P=c.P):
        arr = fx.block_args(c, 0)
        if mutate:
            mutate(arr)
        n = len(arr) if n is None else n
        p = ctypes.cast(arr, ctypes.c_void_p)
        rc_e = lib.csk_co_stack_step_f32(n, p, n_skel, V, P, None)
        msg_e = lib.csk_last_error()
        rc_q = lib.csk_co_stack_step_f32_route(n, p, n_skel, V, P, out)
        return rc_e, msg_e, rc_q, lib.csk_last_error()

    def st(field, value, i=1):
        return lambda arr: setattr(arr[i], field, value)

    bad = [(dict(n=0), b"blocks expected"), (dict(n=5), b"blocks expected"), (dict(P=c.P + 2), b"bad dims"), (dict(P=c.Q - 4), b"bad dims"),
           (dict(n_skel=0), b"bad dims"), (dict(V=1), b"bad dims"), (dict(V=43, P=43 * 8, n_skel=8), b"longer than 128"),
           (dict(mutate=st("xin_slot0", 2)), b"does not read what block 0 emits"), (dict(mutate=st("c_in", 32)), b"does not read"),
           (dict(mutate=st("y_slots", 11)), b"too shallow"), (dict(mutate=st("y_slot0", 12)), b"slot index out of range"),
           (dict(mutate=st("x_res_slot0", -1, 0)), b"slot index out of range"), (dict(mutate=st("res_mode", 2, 2)), b"none or identity"),
           (dict(mutate=st("gcn_res_mode", 0, 2)), b"identity or conv"), (dict(mutate=st("tcn_w", None, 2)), b"null pointer"),
           (dict(mutate=st("y_ring", 0x100004, 0)), b"16-byte aligned"), (dict(mutate=st("ell_w", 0, 0)), b"skeleton-sparse"),
           (dict(mutate=st("c_out", 128, 2)), b"bad dims")]
    for kw, text in bad:
        rc_e, msg_e, rc_q, msg_q = both(**kw)
        assert rc_e == rc_q == -1 and msg_e == msg_q and text in msg_q, (kw, msg_e, msg_q)
    assert lib.csk_co_stack_step_f32_route(3, ctypes.cast(fx.block_args(c, 0), ctypes.c_void_p), c.n_skel, c.V, c.P, None) == -1
    assert b"null route" in lib.csk_last_error()
    assert lib.csk_co_stack_step_f32_route(3, None, c.n_skel, c.V, c.P, out) == -1 and b"blocks expected" in lib.csk_last_error()
    # what moves a call off the one launch: a ring of 4 GB, c_out no multiple of 16 (asked per block), a dense column
    wide = fx.Case(**{**c.__dict__, "n_skel": 1 << 21, "P_": 18 << 21})
    assert fx.route(wide) == (0, [0, 0, 0, 0, 0, 0, -1])
    arr = fx.block_args(c, 0)
    assert fx.route(c, arr=arr) == (0, c.want_route())


def test_fixture_takes_nothing_from_the_product_but_fold_native_and_the_graphs():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "co_stack_fixture.py")).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.module and node.module.startswith("continual_skeletons_amd"):
            names |= {a.name for a in node.names}
        if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id == "pkg":
            names.add(node.attr)
    assert names <= {"fold", "native", "graph"}, names
    assert not any(isinstance(n, ast.Call) and getattr(n.func, "id", "") == "open" for n in ast.walk(tree))
