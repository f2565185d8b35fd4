"""The cases of tests/test_gpu_step32.py, checked without a GPU (tests/step32_fixture.py): every exact and route case is admissible,
the selection restated from csk_tcn_step_f32 reaches exactly the 15 instantiations of tcn_step_kernel and the tables reach all of
them, no case moves to the 16x16x4 family (asked of the library), the workgroup counts cover the XCD-contiguous work-item order,
``model`` equals the fp64 reference and every seeded defect is caught by the cases named for it, and truncating a result to bf16
breaks the derived bound of the real tier."""
import pytest
import torch

import _bootstrap
from tests import step16_fixture as s16
from tests import step32_fixture as fx
from tests import step_split_fixture as ssf

pkg = _bootstrap.load()
ROUTE = fx.one_per_instantiation()


@pytest.mark.parametrize("cs", fx.CASES + fx.COLLAPSE, ids=lambda c: c.id)
def test_case_is_admissible(cs):
    bound = fx.admissible(cs)
    want = fx.reference(cs)
    assert tuple(want.shape) == (cs.n_emit, cs.co, cs.NV) and float(want.abs().max()) <= bound
    assert torch.equal(want, want.round()) and torch.equal(want.float().double(), want)        # the cast to fp32 is exact
    assert float((want != 0).double().mean()) > 0.8                                           # the ReLU leaves the values to compare
    t, g = fx.launch(cs)
    for v in t.values():                                                                       # every operand handed over is an integer
        if v is not None:
            real = v[~torch.isnan(v)]
            assert torch.equal(real, real.round())
    assert float(t["w"].abs().sum()) == float(fx.operands(cs).w.abs().sum())                   # the image holds the weights and zeros
    assert tuple(t["w"].shape) == (cs.k, (cs.c + 15) // 16 * 16, (cs.co + 63) // 64 * 64)
    assert 0 <= g["head"] < g["slots"] and g["slots"] >= cs.k - 1 + (cs.n_emit - 1) * cs.head_step + 1
    assert (g["slots"] == cs.k) == cs.bare
    n_nan_slots = int(torch.isnan(t["ring"][:, 0, 0]).sum())
    assert n_nan_slots == g["slots"] - cs.T                                                    # slots that hold no frame are NaN
    assert bool(torch.isnan(t["ring"][..., cs.NV:]).all()) and cs.P - cs.NV in (0, 1, 2, 3)
    if cs.wrap and cs.k >= 2 and not cs.bare:
        assert fx.window_wraps(cs)


@pytest.mark.parametrize("cs", list(ROUTE.values()), ids=lambda c: c.id)
def test_route_case_names_its_source(cs):
    """ids in [2**23, 2**24) on the ring, small ids on the residual, one-hot weights: exact sums, and a bf16 operand changes them"""
    fx.admissible(cs, "route")
    o, want = fx.operands(cs, "route"), fx.reference(cs, "route")
    assert int(o.x.unique().numel()) == o.x.numel() and float(o.x.min()) >= 2 ** 23 and float(o.x.max()) < 2 ** 24
    assert bool((o.x % 2 == 1).any()) and bool(((o.w != 0).sum((1, 2, 3)) == 1).all())
    assert o.x_res is None or int(o.x_res.unique().numel()) == o.x_res.numel()
    assert torch.equal(want.float().double(), want)
    if cs.res == "none":                                                    # every output IS the id of one ring element
        assert set(want.flatten().tolist()) <= set(o.x.double().flatten().tolist())
    trunc = fx.Ops(fx.bf16_truncated(o.x), o.w, o.bias, o.x_res, o.w_res)
    y = fx._sum(cs, *[None if t is None else t.double() for t in (trunc.x, trunc.w, trunc.bias, trunc.x_res, trunc.w_res)])
    assert float((fx._emissions(cs, y) != want).double().mean()) > 0.9


def test_geometry_is_launch_geometry_for_nine_taps():
    """the k-aware geometry leaves the k = 9 results of step_split_fixture.launch_geometry unchanged"""
    seen = 0
    for sc in s16.STEP_CASES:
        cs = fx.Case(sc.c, sc.co, sc.V, sc.N, 9, sc.head_step, sc.n_emit, sc.res, sc.c_res, sc.wrap, sc.relu, 1, sc.seed)
        assert cs.T == sc.T and cs.res_frames == sc.res_frames and fx.geometry(cs) == ssf.launch_geometry(sc), sc.id
        seen += 1
    assert seen == len(s16.STEP_CASES) > 0


def _sweep():
    lib = pkg.native.lib()
    keys, taken16 = set(), 0
    mt_occ, n_occ = fx.smallest_occ3()
    for k in range(1, 10):
        for hs in range(4):
            for n in range(1, 65):
                slots = k - 1 + (n - 1) * hs + 1
                for co in (64, 128, 64 * mt_occ, 64 * mt_occ + 64):
                    for c, ksplit in ((8, 1), (16, 1), (16, 2), (64, 4), (64, 32), (8, 2)):
                        for P in (4, 100):
                            t = lib.csk_tcn_step_f32_tile(slots, hs, n, 0, n, c, co, P, k, 0, 0, ksplit)
                            assert t >= 0
                            if t:
                                taken16 += 1
                                continue
                            keys.add(fx.select_dims(c, co, P, k, hs, n, ksplit).key)
    return keys, taken16


def test_reachable_set_is_the_fifteen_and_the_tables_reach_them():
    keys, taken16 = _sweep()
    assert keys == set(fx.EVERY) and len(keys) == 15 and taken16 > 0
    lib = pkg.native.lib()
    for cs in fx.CASES:
        assert fx.tile16(cs, lib) == 0, cs.id                              # no case moves to the 16x16x4 family
    assert {fx.select(cs).key for cs in fx.CASES} == set(fx.EVERY)
    assert set(ROUTE) == set(fx.EVERY) and len(ROUTE) == 15
    nine, five = fx.COLLAPSE
    assert fx.select(nine).eff == 1 == fx.select(five).eff and fx.tile16(nine, lib) // 1000 == 18 and fx.tile16(five, lib) == 0
    assert fx.select(five).key == (64, 1, 1, False, False, 2)
    # the 168-register twin and the other side of its boundary
    hi, lo = fx.GROUPS["occ"]
    assert fx.select(hi).key == (64, 4, 1, False, True, 3) and fx.select(lo).key == (64, 4, 1, False, True, 2)
    assert 512 < fx.select(hi).g <= 768 and fx.select(lo).g <= 512 and (hi.co + 63) // 64 % 2 == 1 and hi.co % 64
    assert fx.smallest_occ3() == ((hi.co + 63) // 64, hi.n_emit) == (33, 64)
    size = sum(v.numel() for v in fx.launch(hi)[0].values() if v is not None)
    assert 4 * size < 3 << 20 and 4 * (hi.n_emit + 1) * hi.co * hi.P < 3 << 20              # operands, and the output ring


def test_split_ranges_and_table_coverage():
    assert [fx.split_ranges(c, s) for c, s in ((16, 2), (64, 2), (20, 2), (40, 4), (16, 32), (8, 2))] == [(2, 8), (2, 32), (2, 16), (3, 16), (2, 8), (1, 8)]
    sp = fx.GROUPS["split"]
    assert {(c.c, c.ksplit) for c in sp} == {(16, 2), (64, 2), (20, 2), (40, 4), (16, 32)}
    for grp in ({c for c in sp}, {c for c in fx.GROUPS["k"] if c.ksplit > 1}):
        assert {c.res for c in grp} == {"none", "ident", "conv"} and {c.relu for c in grp} == {False, True}
        assert {c.wrap for c in grp} == {False, True}
    assert {c.c_res for c in sp if c.res == "conv"} == {3, 16, 24}
    assert {c.co for c in sp} == {40, 64, 96, 128, 256} and {c.NV for c in sp} == {75, 100, 425}
    assert {c.P for c in sp} == {76, 100, 428}
    assert {(c.head_step, c.n_emit) for c in sp} >= {(hs, n) for hs in (1, 2) for n in (1, 2, 3, 4)}
    assert any(fx.select(c).E == 2 and c.n_emit == 4 for c in sp)                                  # bz / ksplit and bz % ksplit both in play
    ks = fx.GROUPS["k"]
    assert {c.k for c in ks} == {1, 2, 4, 5, 8} and {c.n_emit for c in ks} == {1, 3}
    for k in (1, 2, 4, 5, 8):
        mine = [c for c in ks if c.k == k]
        assert any(c.bare and fx.geometry(c)["slots"] == k for c in mine) and any(c.wrap and not c.bare for c in mine)
        assert {(fx.select(c).MT, fx.select(c).split) for c in mine} == {(64, False), (64, True), (128, False), (128, True)}
        if k > 1:
            assert any(not c.bare and fx.window_wraps(c) for c in mine)
        else:                                                               # a one-slot window cannot wrap: the emissions' slots do
            assert any(fx.geometry(c)["head"] + (c.n_emit - 1) * c.head_step >= fx.geometry(c)["slots"] for c in mine)
    fo = fx.GROUPS["folded"]
    assert {c.P for c in fo} == {4} and {c.NV for c in fo} == {3, 4} and {c.co for c in fo} == {64, 192, 128, 96}
    e1 = fx.GROUPS["e1"]
    assert {c.head_step for c in e1} == {0, 3} and {c.NV for c in e1} == {100, 425} and {fx.select(c).MT for c in e1} == {64, 128}
    assert all(fx.select(c).E == 1 and fx.select(c).K9 and not fx.select(c).split for c in e1)
    assert any(-(-c.P // fx.select(c).NP) > 1 for c in e1)                                           # several position tiles


def test_workgroup_counts_cover_the_xcd_order():
    """xcd_contiguous_id treats launches below 8 workgroups, above 8 and with a remainder modulo 8 differently"""
    gs = {fx.select(c).g for c in fx.CASES}
    assert any(g < 8 for g in gs) and any(g > 8 and g % 8 for g in gs) and any(g > 8 and g % 8 == 0 for g in gs), sorted(gs)
    assert 1 in gs and max(gs) == fx.select(fx.GROUPS["occ"][0]).g


@pytest.mark.parametrize("cs", fx.CASES + fx.COLLAPSE[1:], ids=lambda c: c.id)
def test_model_equals_the_reference(cs):
    assert torch.equal(fx.model(cs).double(), fx.reference(cs))


@pytest.mark.parametrize("defect", fx.DEFECTS)
def test_seeded_defect_is_caught_by_its_cases(defect):
    # (the OCC pair is the largest case: its forms are in the folded group as well)
    named = [cs for cs in fx.CASES if fx.applies(defect, cs) and cs not in fx.GROUPS["occ"]]
    assert named, defect
    for cs in named:
        got = fx.model(cs, defect)
        assert not torch.equal(got.double(), fx.reference(cs)), (defect, cs.id)


@pytest.mark.parametrize("cs", list(ROUTE.values()), ids=lambda c: c.id)
def test_bf16_truncation_breaks_the_derived_bound(cs):
    """the bound of the real tier cannot pass vacuously: the fp32-rounded reference, truncated to bf16, misses it on most outputs, and
    the fp32-rounded reference itself meets it"""
    want, bnd = fx.reference(cs, "real"), fx.bound(cs)
    assert bool(((want.float().double() - want).abs() <= bnd).all())
    broken = (fx.bf16_truncated(want.float()).double() - want).abs() > bnd
    live = want != 0                                                        # (a ReLU zero truncates to itself)
    assert float(live.double().mean()) > 0.3 and float(broken[live].double().mean()) > 0.8
    assert float(want.abs().max()) > 0.1 and not torch.equal(want, want.round())
