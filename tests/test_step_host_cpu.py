"""The host path of the continual temporal step without a GPU (tests/step_host_fixture.py): csk_tcn_step_f32_route -- what the launcher of
csrc/step.hip switches on -- against the Python restatement of the rule (step32_fixture.select_dims) over every case of the 32x32x2 and the
16x16x4 suites; every refusal of the two entries and their queries, return code and text, against the table recorded before the entries
shared one check; and the two _tile queries over a grid of launch shapes against the values recorded with it."""
import pytest

import _bootstrap
from tests import step16_fixture as s16
from tests import step32_fixture as s32
from tests import step_host_fixture as hx

pkg = _bootstrap.load()
TILE16, TILE32 = 1, 2


def code_of(sel):
    return sel.MT * 100000 + sel.E * 10000 + sel.HS * 1000 + sel.split * 100 + sel.K9 * 10 + sel.OCC


def _route_of_case(lib, cs):
    g = s32.geometry(cs)
    return hx.route(lib, slots=g["slots"], head_step=cs.head_step, n_emit=cs.n_emit, x_res_slots=g["x_slots"] if cs.res != "none" else 0,
                    out_slots=g["out_slots"], c=cs.c, c_out=cs.co, P=cs.P, k=cs.k, res_mode=s32.RES_MODE[cs.res], c_res=cs.c_res, ksplit=cs.ksplit)


def test_route_is_the_python_model_on_every_32x32x2_case():
    lib = pkg.native.lib()
    seen = set()
    for cs in s32.CASES + s32.COLLAPSE:
        rc, words = _route_of_case(lib, cs)
        tile, sel = s32.tile16(cs, lib), s32.select(cs)
        assert rc == 0, (cs.id, lib.csk_last_error())
        if tile:                                                            # the collapsed k = 9 request: the 16x16x4 family
            assert words == [TILE16, tile, 0] and cs is s32.COLLAPSE[0], cs.id
            continue
        assert words == [TILE32, code_of(sel), sel.g], (cs.id, words, sel)
        seen.add(sel.key)
    assert seen == set(s32.EVERY) and {code_of(s32.select(cs)) for cs in s32.CASES} == {m * 100000 + e * 10000 + h * 1000 + s * 100 + k * 10 + o
                                                                                         for m, e, h, s, k, o in s32.EVERY}


def test_route_is_the_tile_query_on_every_16x16x4_case():
    lib = pkg.native.lib()
    launches = [(sc, None) for sc in s16.STEP_CASES] + [(w.sc, s16.wide_P(w)) for w in s16.WIDE]
    tiles = set()
    for sc, P in launches:
        g = s16.ssf.launch_geometry(sc)
        tile = s16.step_tile(sc, P, lib)
        rc, words = hx.route(lib, slots=g["slots"], head_step=sc.head_step, n_emit=sc.n_emit, x_res_slots=g["x_slots"] if sc.res != "none" else 0,
                             out_slots=g["out_slots"], c=sc.c, c_out=sc.co, P=P or sc.P, k=9, res_mode=s16.RES_MODE[sc.res], c_res=sc.c_res, ksplit=1)
        assert rc == 0 and tile > 0 and words == [TILE16, tile, 0], (sc.id, words, tile)
        tiles.add(tile)
    assert len(tiles) == 16                                                 # every instantiation of tcn_step16_kernel


def test_route_over_the_sweep_of_the_fifteen():
    """the sweep of tests/test_step32_fixture_cpu.py, thinned to every fourth n_emit and the boundary of the OCC = 3 twin: wherever the
    16x16x4 family does not take the launch the library names the instantiation and the grid the model names"""
    lib = pkg.native.lib()
    mt_occ, n_occ = s32.smallest_occ3()
    keys = set()
    for k in (1, 5, 9):
        for hs in range(4):
            for n in sorted({1, 2, 3, 4, 6, 8, 12, 16, 60, 64, n_occ, n_occ - 4}):
                slots = k - 1 + (n - 1) * hs + 1
                for co in (64, 128, 64 * mt_occ, 64 * mt_occ + 64):
                    for c, ksplit in ((8, 1), (16, 1), (16, 2), (64, 4), (64, 32), (8, 2)):
                        for P in (4, 100):
                            rc, words = hx.route(lib, slots=slots, head_step=hs, n_emit=n, x_res_slots=0, out_slots=n, c=c, c_out=co, P=P, k=k,
                                                 res_mode=0, c_res=0, ksplit=ksplit)
                            tile = lib.csk_tcn_step_f32_tile(slots, hs, n, 0, n, c, co, P, k, 0, 0, ksplit)
                            assert rc == 0 and tile >= 0
                            if tile:
                                assert words == [TILE16, tile, 0]
                                continue
                            sel = s32.select_dims(c, co, P, k, hs, n, ksplit)
                            assert words == [TILE32, code_of(sel), sel.g], (k, hs, n, co, c, ksplit, P, words, sel)
                            keys.add(sel.key)
    assert keys == set(s32.EVERY)


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
def test_the_table_is_the_fixtures_rows_and_reaches_every_refusing_site():
    gold = hx.golden()["refusals"]
    assert [(r["fn"], r["site"], r["change"]) for r in gold] == [(fn, site, change) for fn, site, change in hx.ROWS]
    assert all(r["rc"] == -1 and r["text"].startswith("tcn_step") for r in gold)
    for fn, sites in hx.SITES.items():
        reached = {r["site"] for r in gold if r["fn"] == fn}
        unreachable = {s for f, s in hx.UNREACHABLE if f == fn}
        assert reached | unreachable == set(sites) and not reached & unreachable, fn
    assert [len(hx.SITES[f]) for f in (hx.F32, hx.BF, hx.TILE, hx.BF_TILE)] == [19, 16, 8, 1] and len(hx.UNREACHABLE) == 2
    # one change per row, but for the rings a change of n_emit, head_step or k needs; a stand-in pointer is never a real address
    assert all(len(r["change"]) == 1 or len(set(r["change"]) - {"slots", "out_slots"}) == 1
               or r["site"] in ("no_x_res", "ident_c_res", "partial_align", "grid", "ring_4gb") for r in gold)


@pytest.mark.parametrize("fn", [hx.F32, hx.BF, hx.TILE, hx.BF_TILE])
def test_refusals_are_the_recorded_ones(fn):
    lib = pkg.native.lib()
    rows = [r for r in hx.golden()["refusals"] if r["fn"] == fn]
    assert rows
    for r in rows:
        assert hx.call(lib, fn, r["change"]) == (r["rc"], r["text"]), r


def test_the_route_query_refuses_what_the_tile_query_refuses():
    lib = pkg.native.lib()
    rows = [r for r in hx.golden()["refusals"] if r["fn"] == hx.TILE]
    for r in rows:
        rc, _ = hx.route(lib, **r["change"])
        assert (rc, lib.csk_last_error().decode()) == (r["rc"], r["text"]), r
    a = hx.BASE[hx.TILE]
    assert lib.csk_tcn_step_f32_route(*[a[n] for n in hx.ARGS[hx.TILE]], None) == -1 and lib.csk_last_error() == b"tcn_step_route: null route"
    big = {k: v for k, v in hx.ROWS_GRID.items() if k in hx.ARGS[hx.TILE]}                         # the launch the entry refuses for its grid
    assert s32.select_dims(a["c"], big["c_out"], big["P"], 9, 1, big["n_emit"], 1).g >= 1 << 31
    assert hx.route(lib, **big) == (0, [TILE32, 12821012, -1])
    assert hx.route(lib) == (0, [TILE16, 18410, 0]) and lib.csk_tcn_step_f32_tile(*[a[n] for n in hx.ARGS[hx.TILE]]) == 18410


# ---- the tile sweep --------------------------------------------------------------------------------------------------------------------
def test_tile_queries_over_the_grid_are_the_recorded_ones():
    gold = hx.golden()
    assert gold["sweep"] == {k: list(v) for k, v in hx.SWEEP.items()} and len(hx.sweep_points()) == 4 * 5 * 8 * 2 * 2 * 2
    assert gold["sweep"] == dict(c_out=[4, 64, 128, 256], P=[8, 52, 100, 400, 25600], n_emit=list(range(1, 9)), head_step=[1, 2], ksplit=[1, 4], k=[3, 9])
    f32, bf = hx.sweep_tiles(pkg.native.lib())
    assert f32 == gold["f32_tile"] and bf == gold["bf16x3_tile"] and len(f32) == len(bf) == 1280
    assert min(f32) == 0 and len(set(f32)) > 8 and set(bf) == {25, 18, 13, 9}                   # both families, every width
