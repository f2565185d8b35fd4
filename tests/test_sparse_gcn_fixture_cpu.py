"""tests/sparse_gcn_fixture.py without a GPU: every case takes the route it claims (host-only queries csk_gcn_stage_f32_route and
csk_gcn_stage_splitk_f32_route, the function the launcher switches on), the tables reach the 4 + 4 instantiations of
gcn_stage_sparse2_kernel and the branch points listed in the fixture's docstring, exact cases are admissible, float cases keep the
derived bound below half a term, and a plain fp32 model of the stage fails both tiers under one seeded defect at a time."""
import numpy as np
import pytest

import _bootstrap
from tests import dense_gcn_fixture as dx
from tests import sparse_gcn_fixture as fx

pkg = _bootstrap.load()
f32 = np.float32
ALL_SPLITS = fx.SPLIT_CASES + fx.FLOAT_SPLITS
ALL_CASES = fx.UNSPLIT_CASES + fx.FLOAT_CASES + [s.c for s in ALL_SPLITS]


def test_every_case_takes_the_route_it_claims():
    lib = pkg.native.lib()
    for c in ALL_CASES:
        assert dx.family(c.route) == dx.SPARSE2 and c.route == fx.sparse_route(c)
        assert dx.route_query(lib, c) == c.route, (c.name, dx.route_query(lib, c), lib.csk_last_error())
        # aligned or not, at most 256 workgroups: the cost model of the 16x16x4 tiles keeps the 32x32x2 kernel
        assert fx.workgroups(c) <= 256, c.name
        assert dx.route_query(lib, c._replace(x_off=0, x_pad=0, y_pad=0, seg_pad=0)) == c.route, c.name
        assert fx.split_query(lib, c, 1) == c.route, c.name                  # ksplit = 1 is the unsplit stage
    for s in ALL_SPLITS:
        assert fx.split_query(lib, s.c, s.ksplit) == fx.split_route(s.c, s.ksplit), (s.c.name, s.ksplit, lib.csk_last_error())
        assert fx.workgroups(s.c, s.ksplit) <= 256, s.c.name


def test_tables_reach_all_eight_instantiations():
    unsplit = {dx.SPARSE2 * dx.UNIT + mt * 10 + cr for mt in (64, 128) for cr in (0, 1)}
    assert {c.route for c in fx.UNSPLIT_CASES} == unsplit and {c.route for c in fx.FLOAT_CASES} == unsplit
    for table in (fx.SPLIT_CASES, fx.FLOAT_SPLITS):
        routes = {fx.split_route(s.c, s.ksplit) for s in table}
        assert {(r & fx.SPLIT_MT128 != 0, r & fx.SPLIT_CONVRES != 0) for r in routes if r & fx.SPLIT_BIT} == {(a, b) for a in (False, True)
                                                                                                               for b in (False, True)}
        assert sum(not r & fx.SPLIT_BIT for r in routes) == 1                 # the collapsed request
    assert len(fx.FLOAT_CASES) == 4 and len(fx.FLOAT_SPLITS) == 5


def test_tables_reach_the_tile_and_staging_branch_points():
    cs = fx.UNSPLIT_CASES
    by_mt = {mt: [c for c in cs if dx.tile_rows(c.c_out) == mt] for mt in (64, 128)}
    # Q around one tile (127 and 257 are primes above 64), one ragged tile below 64 positions, one frame, last tiles of 1 .. 3
    assert {c.frames * c.V for c in by_mt[64]} >= {255, 256, 258} and {c.frames * c.V for c in by_mt[128]} >= {126, 128, 129}
    for mt, group in by_mt.items():
        nt = 16384 // mt
        assert any(c.frames * c.V < 64 and c.frames > 1 for c in group) and any(c.frames == 1 for c in group)
        assert {c.frames * c.V % nt for c in group if c.frames * c.V > nt} >= {1, 2, 3}, mt
        assert any(t.q0 % c.V for c in group for t in fx.tiles(c))           # tiles are not frame aligned
        # the widest span of the class, from the definition: 12 / 7 frames at V = 25, 16 / 8 at V = 18
        for V in (18, 25):
            widest = max(t.span for c in group if c.V == V for t in fx.tiles(c))
            assert widest == fx.max_span(V, mt) and widest <= fx.ldb(V, mt), (V, mt, widest)
        # both staging forms, each inside a multi-chunk K loop; the vector form with span % 4 != 0, x one float off, odd stride
        forms = {(t.vec, dx.cpad(c.c_in) // fx.KCG >= 4) for c in group for t in fx.tiles(c)}
        assert forms >= {(True, True), (False, True)}, mt
        assert any(t.vec and t.span % 4 for c in group for t in fx.tiles(c))
        assert any(t.vec and c.x_off == 1 for c in group for t in fx.tiles(c))
        assert any(t.vec and dx.strides(c)[0] % 2 for c in group for t in fx.tiles(c))
        assert any(not t.vec and c.c_in >= fx.KCG for c in group for t in fx.tiles(c))     # the last tile of a segment
        assert any(c.c_in < fx.KCG and len(fx.tiles(c)) > 1 for c in group)                # c_in = 3, every tile
        # full and ragged row tiles, identity and conv residual
        assert any(fx.row_tiles(c)[0] for c in group) and any(fx.row_tiles(c)[1] for c in group)
        assert {fx.row_tiles(c) for c in group} >= ({(2, 1), (3, 0), (0, 1)} if mt == 64 else {(2, 0), (0, 1)})    # c_out 130, 192 / 256
        assert {c.res for c in group} == {dx.RES_IDENTITY, dx.RES_CONV}
    assert fx.max_span(25, 64) == 300 and fx.max_span(25, 128) == 175
    assert any(c.V == 25 and c.frames == 52 for c in by_mt[64]) and any(c.V == 25 and c.frames == 47 for c in by_mt[128])
    # the staging limits themselves
    assert any(fx.ldb(c.V, 64) == 320 and max(t.span for t in fx.tiles(c)) == 320 for c in by_mt[64])
    assert any(fx.ldb(c.V, 128) == 160 for c in by_mt[128])
    assert all(fx.ldb(c.V, dx.tile_rows(c.c_out)) <= (320 if dx.tile_rows(c.c_out) == 64 else 192) for c in cs)
    assert {c.V for c in cs} >= {18, 25} and any(c.V % 2 and c.V not in (18, 25) for c in cs)
    # K loop, epilogue, layout, adjacency
    assert {c.c_in for c in cs} >= {3, 8, 16, 17, 40, 64, 128, 256}
    assert {c.c_out for c in cs} >= {40, 64, 100, 128, 130, 192, 256}
    assert {c.y_pad for c in cs} == {0, 1, 3} and {c.seg_pad for c in cs} == {0, 4} and {c.n_seg for c in cs} == {1, 2, 3, 5}
    assert any(fx.workgroups(c) % 8 for c in cs)
    assert {c.ell_cnt for c in cs} == {(1, 1, 4), (1, 1, 3), (1, 0, 4), (0, 1, 2), (0, 0, 0), (1, 1, 1)}
    assert all(c.ell_w == 1 for c in cs if c.ell_cnt == (1, 1, 1)) and any(c.ell_w == 5 for c in cs)
    assert all(c.frames * c.V <= 1400 and max(c.c_in, c.c_out) <= 256 and c.frames * c.V * c.n_seg <= 3 * 1400 for c in ALL_CASES)


def test_tables_reach_the_split_branch_points():
    sc = fx.SPLIT_CASES
    shape = {(s.c.c_in, s.ksplit): (fx.cper_ranges(s.c.c_in, s.ksplit), fx.chunks_of_ranges(s.c, s.ksplit)) for s in sc}
    assert shape[(256, 32)] == ((8, 32), [1] * 32)                            # nchunks = 1 inside a split
    assert shape[(128, 6)] == ((24, 6), [3] * 5 + [1])                        # a short last range
    assert shape[(40, 4)] == ((16, 3), [2, 2, 2])                             # fewer ranges than asked
    assert shape[(3, 4)][0] == (8, 1)                                         # collapses: the unsplit kernel
    assert any(s.c.c_out == 70 for s in sc)
    live = [s for s in sc if fx.cper_ranges(s.c.c_in, s.ksplit)[1] > 1]
    assert {dx.tile_rows(s.c.c_out) for s in live} == {64, 128} and {s.c.res for s in live} == {1, 2} and {s.c.V for s in live} == {18, 25}
    assert any(dx.strides(s.c)[2] % 2 for s in live)                          # odd y_chan_stride under the partial rows
    assert any(len(fx.tiles(s.c)) > 1 for s in live) and any(fx.row_tiles(s.c)[1] for s in live)


def test_exact_cases_are_admissible():
    """integer operands, sum |term| < 2^24, ReLU clips 20 % .. 80 % -- (0, 0, 0) included: bias + residual keep both signs"""
    seen = set()
    for c in fx.UNSPLIT_CASES + [s.c for s in fx.SPLIT_CASES]:
        ops = dx.operands(c, "exact")
        pre, mag = dx.reference(c, ops, relu=False)
        dx.admissible_exact(c, ops, pre, mag)
        assert dx.is_integral_f32(pre)
        a, src = ops["adj"][0], ops["ell_src"]
        assert src.min() >= 0 and src.max() < c.V                              # tails included: the kernel may load them
        if sum(c.ell_cnt) > 1 and c.V > 2:
            assert not np.array_equal(a, np.swapaxes(a, 1, 2))                 # not symmetric
        if c.ell_cnt[0] and c.ell_cnt[1]:
            assert not np.array_equal(a[0], a[1])
        if c.ell_w > 1:
            assert any(len(set(src[r, w].tolist())) > 1 for r in range(3) for w in range(c.V))
        seen.add(c.ell_cnt)
    assert (0, 0, 0) in seen


def test_float_cases_keep_the_bound_below_half_a_term():
    for c, ksplit in [(c, 1) for c in fx.FLOAT_CASES] + [(s.c, s.ksplit) for s in fx.FLOAT_SPLITS]:
        ops = dx.operands(c, "float")
        _, mag = dx.reference(c, ops)
        bnd, term = fx.margin(c, ops, mag, ksplit)
        assert bnd < term / 2 and term >= 0.125, (c.name, bnd, term)
        assert c.c_in <= fx.FLOAT_MAX_C_IN.get(c.route, 40), c.name
        R, ranges = (4 if c.res == dx.RES_CONV else 3), fx.cper_ranges(c.c_in, ksplit)[1]
        assert fx.depth(c, ksplit) == 4 + R * dx.cpad(c.c_in) + 2 + (ranges if ranges > 1 else 0) + 2
        assert np.isnan(ops["ell_val"]).any() or c.ell_w == max(c.ell_cnt)


MODEL_CASES = [(c, 1) for c in fx.FLOAT_CASES] + [(s.c, s.ksplit) for s in fx.FLOAT_SPLITS]


def test_every_defect_has_a_model_case():
    for defect in fx.DEFECTS:
        assert sum(fx.applies(defect, c, k) for c, k in MODEL_CASES) >= 2, defect


@pytest.mark.parametrize("defect", fx.DEFECTS)
def test_plain_fp32_model_fails_under_each_seeded_defect(defect):
    """the defect-free model passes both tiers; with the defect it fails the bit comparison AND the float bound"""
    for c, ksplit in MODEL_CASES:
        if not fx.applies(defect, c, ksplit):
            continue
        for tier in ("exact", "float"):
            ops = dx.operands(c, tier)
            want, mag = dx.reference(c, ops)
            good, bad = fx.model_f32(c, ops, None, ksplit), fx.model_f32(c, ops, defect, ksplit)
            if tier == "exact":
                assert np.array_equal(good, want.astype(f32)) and not np.array_equal(bad, want.astype(f32)), (c.name, defect)
            else:
                bnd = fx.bound(c, mag, ksplit)
                assert (np.abs(good - want) <= bnd).all() and not (np.abs(bad - want) <= bnd).all(), (c.name, defect)
