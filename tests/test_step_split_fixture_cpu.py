"""The step cases of tests/test_gpu_step_bf16x3.py, checked without a GPU (tests/step_split_fixture.py): what
tests/test_split_fixture_cpu.py asserts for the clip cases, for every derived step case -- the operands are their designed
pieces in the packed images, the sequential fp32 restatement of the six piece products stays under the case's tolerance, and
the result without any ONE of the six piece products of the hot (tap slot, 16-channel chunk) pair misses it at every output
that products reach.  The tolerance is the clip fixture's own D / 2; no number is introduced here."""
import pytest
import torch

import _bootstrap
from tests import split_fixture as sf
from tests import step_split_fixture as ssf

pkg = _bootstrap.load()
from continual_skeletons_amd import fold  # noqa: E402


def test_cases_cover_the_matrix():
    cs = ssf.CASES
    seen = {(c.case.ci, c.case.stride, c.case.res, c.case.V, c.n_emit) for c in cs}
    for ci in (16, 24, 64):
        for stride in (1, 2):
            for res in ("none", "ident", "conv"):
                if res == "ident" and stride == 2:
                    continue
                for V in (25, 18):
                    for n_emit in (1, 4):
                        assert (ci, stride, res, V, n_emit) in seen
            hot = {c.case.hot[0] for c in cs if c.case.ci == ci and c.case.stride == stride and c.case.hot and c.case.res == "none"}
            assert hot >= {(s, ch) for s in range(9) for ch in range(sf.n_chunks(ci))}
    assert all(c.case.co == 128 and c.case.kernel == "tcn" for c in cs)
    assert {c.P for c in cs} >= {100, 72} and any(c.P > 288 and c.P % 288 and c.P % 144 for c in cs)    # several tiles, a partial last one
    assert {c.wrap for c in cs} == {False, True}
    for c in cs:                                                  # a wrapping case really wraps: the window, the residual and the output ring
        g = ssf.launch_geometry(c)
        w0 = (g["head"] - 8) % g["slots"]
        assert (w0 + 8 >= g["slots"]) == c.wrap
        assert 0 <= g["head"] < g["slots"] and g["slots"] >= 9 + (c.n_emit - 1) * c.case.stride


def test_tiles_of_the_cases():
    """the tile a launch picks (host arithmetic of csk_tcn_step_bf16x3): the matrix runs on the narrow tiles (18 / 9 column
    blocks), the WIDE launches on every wide instantiation, each with a partial last tile"""
    tile = pkg.native.lib().csk_tcn_step_bf16x3_tile
    assert {tile(c.n_emit, 128, c.P) for c in ssf.CASES + ssf.MIXED} == {18, 9}
    for w in ssf.WIDE:
        assert w.sc.P == 100 and tile(w.sc.n_emit, 128, w.sc.P) == (9 if w.sc.n_emit % 2 == 0 else 18)
        assert tile(w.sc.n_emit, 128, w.P) == w.blocks and w.P % (16 * w.blocks), w.id
    assert {(w.blocks, 2 - w.sc.n_emit % 2, w.sc.case.stride) for w in ssf.WIDE} == {(25, 1, 1), (25, 1, 2), (13, 2, 1), (13, 2, 2)}
    assert {w.sc.case.res for w in ssf.WIDE} == {"none", "ident", "conv"} and {w.sc.wrap for w in ssf.WIDE} == {False, True}
    assert tile(1, 128, 102) == -1 and b"bad dims" in pkg.native.lib().csk_last_error()
    # the 1024-stream NTU cycle: every covered layer runs a wide tile
    assert [tile(e, co, 1024 * 2 * 25) for e, co in ((2, 128), (1, 256))] == [13, 25]


@pytest.mark.parametrize("sc", ssf.MIXED, ids=lambda c: c.id)
def test_mixed_case_is_admissible_and_bites(sc):
    """a temporal pair and a residual-conv chunk in one accumulator (two pairs): what tests/test_split_fixture_cpu.py asserts for
    the clip fixture's two-pair cases, cut to the emissions"""
    fx = sf.build(sc.case)
    an = ssf.analyse(sc, fx)
    tol = an["tol"]
    assert sc.case.n_hot == 2 and 1e-6 < tol < 6e-6 and bool(an["with_terms"].all()) and an["bound"] <= tol
    lo, hi = sc.t_lo, sc.t_lo + sc.n_emit
    assert sf.rel_err(sf.restate32(fx)[:, :, lo:hi], an["want"], an["nz"]) <= tol / 2
    for name, dropped in an["drops"].items():
        rel = ((dropped - an["want"]) / an["want"]).abs()
        assert float(rel.min()) > tol, (name, float(rel.min()), tol)
    for g in fx.groups:                                           # either phase lost altogether: half the output
        part = sf.conv64(g.w, g.x, g.stride, g.pad)[:, :, lo:hi]
        assert float((part / an["want"]).abs().min()) > 0.25


@pytest.mark.parametrize("sc", ssf.CASES, ids=lambda c: c.id)
def test_step_case_is_exact_on_the_way_in_admissible_and_bites(sc):
    case = sc.case
    fx = sf.build(case)
    for val, pieces in ((fx.w, fx.wp), (fx.x, fx.xp), (fx.w_res, fx.w_resp), (fx.x_res, fx.x_resp)):
        if val is not None:
            for got, p in zip(fold.split3_bf16(val), pieces):
                assert torch.equal(got.float(), p)
    an = ssf.analyse(sc, fx)
    tol = an["tol"]
    assert tuple(an["want"].shape) == (case.N, case.co, sc.n_emit, case.V)
    assert float(an["want"].abs().max()) <= sf.REF_CAP and 1e-6 < tol < 6e-6
    assert bool(an["with_terms"].all())                           # every emission has a full window: products reach every output
    assert an["bound"] <= tol
    lo, hi = sc.t_lo, sc.t_lo + sc.n_emit
    r32 = sf.restate32(fx)[:, :, lo:hi]
    assert sf.rel_err(r32, an["want"], an["nz"]) <= tol / 2
    # the check bites: without any one of the six piece products of the hot pair every output misses the tolerance
    prods = ssf.pair_products(sc, fx)
    add = 0.0 if fx.addend is None else fx.addend.double()[:, :, lo:hi]
    assert sf.rel_err(sum(prods.values()) + add, an["six"], an["nz"]) <= 1e-12       # the pair IS the case's products
    for pq, prod in prods.items():
        rel = (prod / an["want"]).abs()
        assert float(rel.min()) > tol, (pq, float(rel.min()), tol)
