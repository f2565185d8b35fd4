"""tests/skew_fixture.py proven on the CPU: ENTRIES covers native.SIGNATURES exactly, every entry pinned at kernel level has both row
classes and the tiles it claims, the fixtures' references are reused unchanged, the rounded-down defect is visible on every launch,
skew and operand, and the documented alignment guards fire -- before any launch -- on stand-in pointers 0x1000 + 4 s."""
import ctypes as C

import pytest
import torch

import _bootstrap
from tests import skew_fixture as sk
from tests import tcn_direct_fixture as td
from tests import tcn_wino_fixture as tw

pkg = _bootstrap.load()
native = pkg.native


def test_entries_cover_the_abi_exactly():
    assert set(sk.ENTRIES) == set(native.SIGNATURES), (set(native.SIGNATURES) - set(sk.ENTRIES), set(sk.ENTRIES) - set(native.SIGNATURES))
    for name, e in sk.ENTRIES.items():
        assert e.cls in (sk.TAKES_ANY, sk.REFUSES, sk.REROUTES, sk.NO_POINTER), name
        if e.cls == sk.REFUSES:
            assert e.operand and e.message, name
        if e.cls == sk.NO_POINTER:
            assert not e.pinned, name
    assert {u.entry for u in sk.UNITS} == set(sk.KERNEL_LEVEL)
    assert all(sk.ENTRIES[n] == sk.Entry(sk.TAKES_ANY, sk.HERE, note=sk.ENTRIES[n].note) for n in sk.KERNEL_LEVEL)


def test_skew_table():
    assert sk.SKEWS == ((1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 2, 3), (3, 0, 1), (0, 3, 0), (0, 0, 2)) and sk.CONTROL == (0, 0, 0)
    for i in range(3):                       # every operand sees every non-zero offset, and a zero beside skewed neighbours
        assert {s[i] for s in sk.SKEWS} == {0, 1, 2, 3}


@pytest.mark.parametrize("s", (0, 1, 2, 3))
def test_allocation_helper(s):
    src = torch.arange(1, 31, dtype=torch.float32).view(2, 3, 5)
    a = sk.Skewed((2, 3, 5), s, src=src)
    assert a.t.data_ptr() % 16 == 4 * s and a.buf.data_ptr() % 16 == 0 and torch.equal(a.t, src) and a.bands_intact()
    assert bool(torch.isnan(a.buf[: a.lo]).all()) and a.lo >= sk.GUARD and a.buf.numel() - a.lo - a.n >= sk.GUARD
    assert a.rounded_down().data_ptr() == a.t.data_ptr() - 4 * s
    o = sk.Skewed((2, 3, 5), s)
    assert o.bands_intact() and bool((o.buf == sk.OUT_SENTINEL).all())
    for idx in (o.lo - 1, o.lo + o.n, 0, o.buf.numel() - 1):                  # one changed word on either side is seen, bitwise
        o.buf[idx] = -0.0 if idx == 0 else 1.0
        assert not o.bands_intact()
        o.buf[idx] = sk.OUT_SENTINEL
        assert o.bands_intact()
    a.buf[a.lo - 1] = 0.0                                                    # a NaN band: any non-NaN, and another NaN pattern
    assert not a.bands_intact()


@pytest.mark.parametrize("entry", sk.KERNEL_LEVEL)
def test_both_row_classes_and_the_tiles(entry):
    units = sk.units_of(entry)
    assert any(u.rows_whole_quads for u in units) and any(not u.rows_whole_quads for u in units), entry
    for u in units:
        c = u.case
        if u.kind == "tcn":
            sel = td.sel_of(c)
            assert sel.split == (c.ksplit > 1) and sel.family == ("16" if c.group.startswith("route16") else "32"), u.name
            inner = td.tiles(c, sel)
            assert len(inner) >= 2 and not inner[0] and (c.t_out * c.v) % sel.nt, (u.name, inner)     # a border tile, a ragged last one
        if u.kind == "wino":
            assert not tw.sel_of(c).reject, u.name                              # the gate takes it: the Winograd kernel runs
    if entry == "csk_tcn_stage_f32":
        fams = {(td.sel_of(u.case).family, u.case.stride, u.case.res) for u in units}
        assert fams >= {(f, s, r) for f in ("32", "16") for s in (1, 2) for r in ("none", "conv")} | {(f, 1, "identity") for f in ("32", "16")}
        assert any(any(td.tiles(u.case)) for u in units if u.rows_whole_quads)                       # an interior tile on whole-quad rows
    if entry.startswith("csk_tcn_stage_wino"):
        assert {u.case.v for u in units} == {18, 25}


def test_apply_is_the_fixtures_reference():
    """the function of the operands that rounded_down uses is the fixture's reference, bit for bit, on the fixture's own operands"""
    for u in sk.UNITS:
        h = sk.host_operands(u)
        got = sk.apply(u, h["x"], h.get("x_res"))
        assert (sk.same_bits(got, sk.expected(u)) if u.exact else torch.equal(got, sk.expected(u))) and sk.matches(u, got.float()), u.name
        assert bool(torch.isfinite(sk.expected(u)).all()) and tuple(sk.expected(u).shape) == sk.out_shape(u), u.name
        assert bool((sk.expected(u) != sk.OUT_SENTINEL).all()), u.name               # the sentinel is no value of any result


@pytest.mark.parametrize("entry", sk.KERNEL_LEVEL)
def test_the_rounded_down_defect_is_visible(entry):
    """every launch, every non-zero skew, ONE operand at its address rounded down: the result differs from the reference or a guard
    band changed; and the same model with nothing rounded down gives the reference with the bands intact"""
    for u in sk.units_of(entry):
        for skew in sk.SKEWS:
            off = sk.skew_of(u, skew)
            got, intact = sk.rounded_down(u, skew, None)
            assert intact and sk.matches(u, got), (u.name, skew)
            for which in u.operands:
                if off[which] == 0:
                    continue
                got, intact = sk.rounded_down(u, skew, which)
                assert not (intact and sk.matches(u, got)), (u.name, skew, which)
                if which == "out":
                    assert not intact, (u.name, skew)                             # the store lands in the lower band


# ---- the guards of the `refuses` entries, on stand-in pointers: nothing is launched -----------------------------------------------
FAKE = 0x1000


def _p(v):
    """a pointer argument; None: the stand-in FAKE as it is NOW (the GPU test points it at a real, large, aligned device buffer)"""
    return C.c_void_p(FAKE if v is None else v)


def _err():
    return native.lib().csk_last_error().decode()


def _tcn_step(ring=None, x_res=None, partial=None, ksplit=1):
    return native.lib().csk_tcn_step_f32(_p(ring), 16, 0, 1, 4, _p(None), _p(x_res), 16, 0, 1, None, _p(None), _p(None), 16, 0, 64, 64, 200, 9,
                                         1, 64, 1, ksplit, partial, None)


def _tcn_step_split(ring=None, x_res=None, out=None, w=None):
    return native.lib().csk_tcn_step_bf16x3(_p(ring), 16, 0, 1, 4, _p(w), _p(x_res), 16, 0, 1, None, _p(None), _p(out), 16, 0, 64, 64, 200, 9,
                                            1, 64, 1, None)


def _co_block(xin=None, y_ring=None, out=None, V=25, P=200):
    cnt = (C.c_int32 * 3)(1, 1, 4)
    f = _p(None)
    return native.lib().csk_co_block_step_f32(_p(xin), 16, 0, 64, f, f, f, f, C.cast(cnt, C.c_void_p), 4, 1, _p(y_ring), 16, 0, f, f, 1, 12,
                                              _p(out), 16, 0, 64, 8, V, P, None)


def _co_stack(xin=None, V=25, P=200):
    b = (native.CoBlockArgs * 1)()
    a = b[0]
    xin = FAKE if xin is None else xin
    a.xin, a.xin_slots, a.xin_slot0, a.c_in, a.ell_w, a.gcn_res_mode = xin, 16, 0, 64, 4, 1
    for name in ("gcn_w", "gcn_bias", "ell_src", "ell_val", "y_ring", "tcn_w", "tcn_bias", "out"):
        setattr(a, name, FAKE)
    a.ell_cnt[0], a.ell_cnt[1], a.ell_cnt[2] = 1, 1, 4
    a.y_slots, a.y_slot0, a.res_mode, a.x_res_slot0, a.out_slots, a.out_slot0, a.c_out = 16, 0, 1, 12, 16, 0, 64
    return native.lib().csk_co_stack_step_f32(1, C.cast(b, C.c_void_p), 8, V, P, None)


def _fc(feat=None, c=8):
    return native.lib().csk_fc_f32(_p(feat), _p(None), _p(None), _p(None), 2, c, 5, None)


def _head_clip(pooled=None, c=256, logits=None):
    return native.lib().csk_co_head_clip_f32(_p(None), 7, 5, _p(None), 4, 3, 3, _p(None), _p(None), _p(pooled), _p(logits), 2, 2, c,
                                             25, 60, None)


def _embed_attention(x=None, V=18):
    f = _p(None)
    return native.lib().csk_agcn_embed_attention_f32(_p(x), f, f, f, f, None, 2, 64, 16, 4, V, 0, 1000, 100, None)     # no scratch: the LAST check


def _framewise(x=None, V=18):
    f = _p(None)
    return native.lib().csk_agcn_stage_framewise_f32(_p(x), f, f, f, f, f, f, 2, 64, 64, 16, 5, V, 64 * 5 * V, 5 * V, 64 * 5 * V, 5 * V, 1, None)


def _framewise_route(x=None, V=18):
    return native.lib().csk_agcn_stage_framewise_f32_route(_p(x), 2, 64, 64, 16, 5, V, 64 * 5 * V, 5 * V, 1)


# entry -> (call with the guarded operand at `ptr`, offsets in floats that must be refused, a call with that operand aligned that trips a
# LATER host check -- so the control passes the guard without launching anything -- and that later check's message)
GUARDS = {
    "csk_tcn_step_f32": (lambda p: _tcn_step(ring=p), (1, 2, 3), lambda: _tcn_step(ksplit=2, partial=_p(FAKE + 4)), "partial-sum buffer must be"),
    "csk_tcn_step_bf16x3": (lambda p: _tcn_step_split(out=p), (1, 2, 3), lambda: _tcn_step_split(w=FAKE + 8), "packed weights must be"),
    "csk_co_block_step_f32": (lambda p: _co_block(y_ring=p), (1, 2, 3), lambda: _co_block(V=43, P=344), "longer than 128"),
    "csk_co_stack_step_f32": (lambda p: _co_stack(xin=p), (1, 2, 3), lambda: _co_stack(V=43, P=344), "longer than 128"),
    "csk_co_head_clip_f32": (lambda p: _head_clip(pooled=p), (1, 2, 3), lambda: _head_clip(c=1 << 20), "channels"),
    "csk_agcn_embed_attention_f32": (lambda p: _embed_attention(x=p), (1, 3), lambda: _embed_attention(), "scratch"),
}


def test_guard_table_names_the_refusing_entries():
    assert set(GUARDS) | {"csk_fc_f32", "csk_agcn_stage_framewise_f32"} == {n for n, e in sk.ENTRIES.items() if e.cls == sk.REFUSES}


@pytest.mark.parametrize("entry", sorted(GUARDS))
def test_guard_fires_before_any_launch(entry):
    call, offsets, control, later = GUARDS[entry]
    frag = sk.ENTRIES[entry].message
    for s in offsets:
        assert call(FAKE + 4 * s) == -1 and frag in _err(), (entry, s, _err())
    assert control() == -1 and later in _err() and frag not in _err(), (entry, _err())       # aligned: past the guard, stopped later


def test_other_second_operands_are_guarded_too():
    frag = "state pointers must be 16-byte aligned"
    for s in (1, 2, 3):
        for rc in (_tcn_step(x_res=FAKE + 4 * s), _tcn_step_split(ring=FAKE + 4 * s), _tcn_step_split(x_res=FAKE + 4 * s),
                   _co_block(xin=FAKE + 4 * s), _co_block(out=FAKE + 4 * s)):
            assert rc == -1 and frag in _err(), (s, _err())
    assert _embed_attention(x=FAKE + 8) == -1 and "scratch" in _err()                        # even V: 8 bytes suffice
    assert _embed_attention(x=FAKE + 4, V=25) == -1 and "scratch" in _err()                  # odd V: no guard


def test_fc_guard():
    """csk_fc_f32 has no host check behind its guard: an aligned call launches, so its control runs on the device
    (tests/test_gpu_pointer_skew.py::test_fc_refuses_and_leaves_the_output_alone); here the guard alone, at both channel counts.  The
    control of csk_agcn_stage_framewise_f32 is its route query (the one copy of the rule the launcher switches on)"""
    frag = sk.ENTRIES["csk_fc_f32"].message
    for s in (1, 2, 3):
        assert _fc(feat=FAKE + 4 * s) == -1 and frag in _err()
        assert _fc(feat=FAKE + 4 * s, c=256) == -1 and frag in _err()


def test_framewise_guard_and_route():
    frag = sk.ENTRIES["csk_agcn_stage_framewise_f32"].message
    want = 16 * 1000 + 18 * 10
    assert _framewise_route() == want and _framewise_route(x=FAKE + 8) == want               # the aligned control: host arithmetic only
    for s in (1, 3):
        assert _framewise_route(x=FAKE + 4 * s) == 0
        assert _framewise(x=FAKE + 4 * s) == -1 and frag in _err()
    assert _framewise_route(x=FAKE + 4, V=25) == 16 * 1000 + 250                             # odd V: any 4-byte alignment


def test_gcn_routes_follow_the_alignment():
    """the `reroutes` queries: the sparse stage leaves the 16x16x4 tiles when x or y is off 16 bytes, the dense V = 18 stage leaves
    dense2 when x is off 8 bytes; both are host arithmetic"""
    from tests import dense_gcn_fixture as dx
    lib = native.lib()
    for co, base in dx.LEAVE_BASE.items():
        assert dx.route_query(lib, base) == base.route and dx.family(base.route) == dx.DENSE2
        assert dx.route_query(lib, base, x=dx.ALIGNED + 8) == base.route
        for s in (1, 3):
            assert dx.family(dx.route_query(lib, base, x=dx.ALIGNED + 4 * s)) in (dx.DENSE128, dx.GENERAL)
    for u in sk.units_of("csk_gcn_stage_f32"):
        aligned = dx.route_query(lib, u.case)
        assert dx.family(aligned) in (dx.SPARSE2, dx.TILE16), u.name
        for s in (1, 2, 3):
            for kw in (dict(x=dx.ALIGNED + 4 * s), dict(y=dx.ALIGNED + 4 * s)):
                assert dx.route_query(lib, u.case, **kw) == u.case.route, (u.name, kw)       # off the boundary: always sparse2
