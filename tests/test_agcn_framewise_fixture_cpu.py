"""Host-side checks of tests/agcn_framewise_fixture.py and of the frame-wise clip pass's host logic: the case table reaches every
instantiation csk_agcn_stage_framewise_f32 can launch (through its route query -- host arithmetic, no GPU), shapes outside the built set
are reported, the exact tier is exact, every seeded defect breaks the derived bound, and the head's index map of
``CoAGcn.clip_as_steps_map`` is what stepping gives."""
import ctypes as C

import numpy as np
import pytest

import _bootstrap
from tests import agcn_framewise_fixture as fx

pkg = _bootstrap.load()
native = pkg.native


def _route(c, x=0x1000, seg_pad=None, **kw):
    a = dict(n_seg=c.n_seg, c_in=c.c_in, c_out=c.c_out, inter=fx.inter_of(c), T=c.T, V=c.V, res=2 if c.conv_res else 1)
    a.update(kw)
    chan = a["T"] * a["V"]
    seg = a["c_in"] * chan + (c.seg_pad if seg_pad is None else seg_pad)
    return native.lib().csk_agcn_stage_framewise_f32_route(C.c_void_p(x), a["n_seg"], a["c_in"], a["c_out"], a["inter"], a["T"], a["V"], seg,
                                                           chan, a["res"])


def test_case_table_reaches_every_instantiation():
    """The table holds the shapes the issue names; the route query maps it onto all twelve instantiations (print with -s)."""
    seen = {}
    for c in fx.CASES:
        r = _route(c)
        assert r == fx.route_of(c), (c.name, r)
        seen.setdefault(r, []).append(c.name)
    for r in fx.ALL_ROUTES:
        print(f"agcn_stage_framewise_kernel<{r // 1000}, {r // 10 % 100}, {bool(r % 10)}>: {len(seen.get(r, []))} cases, e.g. {seen.get(r, ['-'])[0]}")
    assert sorted(seen) == fx.ALL_ROUTES
    for V in (18, 25):
        ts = {c.T for c in fx.CASES if c.V == V}
        assert {1, fx.FT[V] - 1, fx.FT[V], fx.FT[V] + 1, 2 * fx.FT[V] + 3} <= ts
        assert {c.n_seg for c in fx.CASES if c.V == V} == {1, 3}
        assert any(c.seg_pad for c in fx.CASES if c.V == V)
        assert {(64, 64), (64, 128), (128, 128), (256, 256)} <= {(c.c_in, c.c_out) for c in fx.CASES if c.V == V}
    assert set(fx.PER_INSTANTIATION) == {(i, V, r) for i in fx.INTERS for V in (18, 25) for r in (False, True)}


def test_route_reports_what_is_not_built_and_bad_dims():
    c = fx.CASES[0]
    assert _route(c, V=20) == 0 and _route(c, inter=8, c_in=32, c_out=32) == 0 and _route(c, inter=16, c_out=128, res=2) == 0
    c18 = next(k for k in fx.CASES if k.V == 18)
    assert _route(c18, x=0x1004) == 0 and _route(c18, seg_pad=1) == 0           # even V: rows 8-byte aligned
    c25 = next(k for k in fx.CASES if k.V == 25)
    assert _route(c25, x=0x1004, seg_pad=1) == fx.route_of(c25)
    for kw, msg in ((dict(n_seg=0), b"bad dims"), (dict(T=0), b"bad dims"), (dict(res=0), b"res_mode must be identity or conv"),
                    (dict(c_in=32, res=1), b"identity residual needs c_in == c_out")):
        assert _route(c, **kw) == -1 and msg in native.lib().csk_last_error()
    # the launcher refuses an unbuilt shape with the project's error code and a message, before anything is launched
    f = C.c_void_p(0x1000)
    rc = native.lib().csk_agcn_stage_framewise_f32(f, f, f, f, f, f, f, 1, 64, 64, 16, 4, 20, 64 * 80, 80, 64 * 80, 80, 1, None)
    assert rc == -1 and b"built for V in {18, 25}" in native.lib().csk_last_error()
    rc = native.lib().csk_agcn_stage_framewise_f32(f, None, f, f, f, f, f, 1, 64, 64, 16, 4, 18, 64 * 72, 72, 64 * 72, 72, 1, None)
    assert rc == -1 and b"null pointer" in native.lib().csk_last_error()


@pytest.mark.parametrize("c", [c for c in fx.CASES if c.T == 2 * fx.FT[c.V] + 3 or c.seg_pad], ids=lambda c: c.name)
def test_exact_tier_is_exact_and_defects_break_the_bound(c):
    inter = fx.inter_of(c)
    ops = fx.operands(c, "exact")
    fx.admissible(c, ops)
    y = fx.definition(ops, inter, c.conv_res, adj=ops["adj_exact"])
    assert np.array_equal(y, f64_round(y)) and (y > 0).any() and (y == 0).any()
    # the attention's own definition gives 1 / V + a_sum: the construction is the definition up to the rounding of 1 / V
    assert np.abs(fx.definition(ops, inter, c.conv_res) - y).max() <= 1e-5 * max(1.0, y.max())
    ops = fx.operands(c, "positive")
    y = fx.definition(ops, inter, c.conv_res)
    b = fx.bound(c, ops, y)
    assert (y > 0).all() and float((b / y).max()) < 1e-3
    for d in fx.DEFECTS:
        if d == "neighbour_frame" and c.T == 1:
            continue
        err = np.abs(fx.definition(ops, inter, c.conv_res, defect=d) - y)
        worst = float((err / b).max())
        print(f"{c.name} {d}: largest err / bound = {worst:.1f}")
        assert worst > 4.0, (c.name, d, worst)


def f64_round(y):
    return np.float64(np.float32(y))


def _model(V, pool_size=-1, pool_padding=-1, T=300):
    A = pkg.ntu_graph().A if V == 25 else pkg.kinetics_graph().A
    return pkg.CoAGcn(A, input_shape=(3, T, V, 2), pool_size=pool_size, pool_padding=pool_padding).eval()


@pytest.mark.parametrize("pool", [(-1, -1), (4, 0), (7, 2)])
def test_head_index_map_is_the_stepping_rule(pool):
    """For T in {76, 80, 96, 300} and both pad_end values: the number of predictions and the feature frames behind each equal what
    prime_counts (frames the steps emit), prime_clip_frames (frames the flush completes) and the head's step rule give."""
    m = _model(25, *pool)
    for T in (76, 80, 96, 300):
        for pad_end in (False, True):
            emitted, clip = m.prime_counts(T)[-1], m.prime_clip_frames(T)[-1]
            assert 0 <= emitted <= clip
            want = fx.head_map_by_stepping(emitted, clip - emitted, m.pool_size, m.pool_padding, pad_end)
            got = m.clip_as_steps_map(T, pad_end)
            print(f"T={T} pad_end={pad_end} pool={m.pool_size}/{m.pool_padding}: {got[0]} feature frames, {len(got[1])} predictions")
            assert got == want, (T, pad_end, got, want)
            assert all(0 <= a <= b and b - a < m.pool_size for a, b in got[1])
    assert m.clip_as_steps_map(0, True) == (0, [(a, b) for a, b in fx.head_map_by_stepping(0, 0, m.pool_size, m.pool_padding, False)[1]])
