"""tests/dense_gcn_fixture.py without a GPU: every case is admissible (integer operands, sums below 2^24, ReLU share; float tier:
bound below half a term), the case tables reach every kernel instantiation they claim -- proven through the host-only query
csk_gcn_stage_f32_route, the function the launcher switches on -- and a plain fp32 model of the stage fails both tiers under one
seeded defect at a time."""
import numpy as np
import pytest

import _bootstrap
from tests import dense_gcn_fixture as fx

pkg = _bootstrap.load()
f32 = np.float32


def _all_stage_cases():
    lib = pkg.native.lib()
    return [c for g, cs in fx.EXACT_GROUPS.items() for c in (fx.boundary_routes(lib) if g == "boundary" else cs)]


def test_every_case_takes_the_route_it_claims():
    lib = pkg.native.lib()
    for c in _all_stage_cases() + fx.FLOAT_CASES:
        assert fx.route_query(lib, c) == c.route, (c.name, fx.route_query(lib, c), lib.csk_last_error())
    # the misaligned launches differ from their base case in the alignment alone
    for c in fx.LEAVE_CASES:
        assert fx.route_query(lib, c._replace(x_off=0, x_pad=0, ell_off=0)) == fx.LEAVE_BASE[c.c_out].route


def test_case_tables_reach_every_instantiation():
    routes = {c.route for c in _all_stage_cases()}
    dense2 = {fx.DENSE2 * fx.UNIT + mt * 1000 + V * 10 + cr for mt in (64, 128) for V in (18, 25) for cr in (0, 1)}
    dense128 = {fx.DENSE128 * fx.UNIT + cr for cr in (0, 1)}
    general = {fx.GENERAL * fx.UNIT + k for k in (1283, 1284, 645, 646)}
    assert len(dense2) == 8 and dense2 | dense128 | general <= routes
    assert any(fx.family(r) in (fx.SPARSE2, fx.TILE16) for r in routes)                  # the sparse side of the boundary
    for route in dense2:                                                                    # each with both adjacency forms, all frame counts
        cs = [c for c in fx.DENSE2_CASES if c.route == route]
        ft = fx.DENSE2_FT[cs[0].V]
        for adj in ("seg", "frame"):
            assert {c.frames for c in cs if c.adj == adj} >= {1, ft - 1, ft, ft + 1, 2 * ft + 3}, (route, adj)
    for V in (18, 25):
        cs = [c for c in fx.DENSE2_CASES if c.V == V]
        assert {c.c_in for c in cs} >= {3, 8, 20, 40} and {c.c_out for c in cs} >= {40, 100, 130, 192, 256}
    # dense128: V 20 / 19 / 4 / 32, both residuals each, a last tile of one frame
    assert {(c.V, c.res) for c in fx.DENSE128_CASES} == {(V, r) for V in (20, 19, 4, 32) for r in (fx.RES_IDENTITY, fx.RES_CONV)}
    assert any(c.frames % (128 // c.V) == 1 and c.frames > 1 for c in fx.DENSE128_CASES)
    # general: shared and per-segment adjacencies, and a per-frame one at a V gcn_dense.hip does not take
    assert {c.adj for c in fx.GENERAL_CASES} == {"shared", "seg", "frame"}
    # leaving dense2: three ways, each to dense128 and to general <64, 5>
    assert sorted(fx.family(c.route) for c in fx.LEAVE_CASES) == [fx.DENSE128] * 3 + [fx.GENERAL] * 3
    # conv1x1: 64- and 128-row tiles, the c_in and c_out of the issue, a ragged last position tile everywhere
    assert {fx.tile_rows(c.c_out) for c in fx.CONV_CASES} == {64, 128}
    assert {c.c_in for c in fx.CONV_CASES} == {3, 16, 17, 40} and {c.c_out for c in fx.CONV_CASES} >= {96, 384}
    assert all((c.frames * c.V) % (16384 // fx.tile_rows(c.c_out)) != 0 for c in fx.CONV_CASES)


def test_exact_cases_are_admissible():
    for c in _all_stage_cases():
        ops = fx.operands(c, "exact")
        pre, mag = fx.reference(c, ops, relu=False)
        fx.admissible_exact(c, ops, pre, mag)
        assert fx.is_integral_f32(pre)
        a = ops["adj"]
        if c.adj != "ell":                                # dense, from a small set with 0, not symmetric, different everywhere
            assert set(np.unique(a).tolist()) == {-1.0, 0.0, 1.0, 2.0}
            assert not np.array_equal(a, np.swapaxes(a, 2, 3)) and not np.array_equal(a[:, 0], a[:, 1])
            assert a.shape[0] == 1 or not np.array_equal(a[0], a[1])
    for c in fx.CONV_CASES:
        ops = fx.conv_operands(c, "exact")
        y, mag = fx.conv_reference(c, ops)
        fx.admissible_exact(c, ops, y, mag, relu=False)
        assert (y < 0).any() and (y > 0).any()


def test_leave_cases_share_their_base_operands():
    for c in fx.LEAVE_CASES:
        a, b = fx.operands(c, "exact"), fx.operands(fx.LEAVE_BASE[c.c_out], "exact")
        assert all(np.array_equal(a[k], b[k]) for k in a)


def test_boundary_cases_differ_in_the_entries_that_count():
    refs = [fx.reference(c, fx.operands(c, "exact"))[0] for c in fx.BOUNDARY_CASES]
    assert not np.array_equal(refs[0], refs[1]) and not np.array_equal(refs[0], refs[2])
    ops = [fx.operands(c, "exact") for c in fx.BOUNDARY_CASES]
    assert all(np.array_equal(ops[0][k], o[k]) for o in ops for k in ("x", "w", "bias", "ell_src", "ell_val_full"))   # ONE graph
    assert (ops[0]["ell_val_full"] != 0).all()
    for c, o in zip(fx.BOUNDARY_CASES, ops):               # ... of which the kernel gets the entries that count; the rest is NaN
        for r in range(3):
            assert np.array_equal(o["ell_val"][0, r, :, :c.ell_cnt[r]], o["ell_val_full"][0, r, :, :c.ell_cnt[r]])
            assert np.isnan(o["ell_val"][0, r, :, c.ell_cnt[r]:]).all()


def test_float_cases_keep_the_bound_below_half_a_term():
    for c in fx.FLOAT_CASES:
        ops = fx.operands(c, "float")
        _, mag = fx.reference(c, ops)
        bnd, term = fx.margin(c, ops, mag)
        assert bnd < term / 2, (c.name, bnd, term)
    for c in fx.CONV_FLOAT:
        ops = fx.conv_operands(c, "float")
        _, mag = fx.conv_reference(c, ops)
        bnd, term = fx.margin(c, ops, mag)
        assert bnd < term / 2, (c.name, bnd, term)
    assert {fx.family(c.route) for c in fx.FLOAT_CASES} == {fx.DENSE2, fx.DENSE128, fx.GENERAL}


@pytest.mark.parametrize("defect", fx.DEFECTS)
def test_plain_fp32_model_fails_under_each_seeded_defect(defect):
    """the defect-free model passes both tiers; with the defect it fails the bit comparison AND the float bound"""
    for c in fx.FLOAT_CASES:
        if defect == "next_matrix" and fx.n_matrices(c) == 1:
            continue
        ft = 128 // c.V
        for tier in ("exact", "float"):
            ops = fx.operands(c, tier)
            want, mag = fx.reference(c, ops)
            good, bad = fx.model_f32(c, ops), fx.model_f32(c, ops, defect, tile_frames=ft)
            if tier == "exact":
                assert np.array_equal(good, want.astype(f32)) and not np.array_equal(bad, want.astype(f32)), (c.name, defect)
            else:
                bnd = fx.bound(c, mag)
                assert (np.abs(good - want) <= bnd).all() and (np.abs(bad - want) > bnd).any(), (c.name, defect)
