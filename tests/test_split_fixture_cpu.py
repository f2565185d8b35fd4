"""The fixtures of tests/test_gpu_bf16x3_pieces.py, checked without a GPU (tests/split_fixture.py): the designed pieces survive
fold.split3_bf16 and fold.pack_conv_weight_split bit for bit; for every case of the matrix the worst-case accumulation bound and
a sequential fp32 restatement of the six piece products stay under the case's tolerance D / 2 (D / 4 for the restatement),
and the fp64 emulation with any one second-order product left out misses D / 2 at every output that products reach."""
import pytest
import torch
import torch.nn.functional as F

import _bootstrap
from tests import split_fixture as sf

pkg = _bootstrap.load()
from continual_skeletons_amd import fold  # noqa: E402

ALL = sf.CASES + sf.DENSE
# the neglected products ml, lm, ll relative to an element product of operands >= 1: m < 2^-8, l <= 63 * 2^-23
THIRD = 2 * 2.0 ** -8 * 63 * 2.0 ** -23 + (63 * 2.0 ** -23) ** 2


def _bits(p):
    b = p.to(torch.bfloat16)
    assert torch.equal(b.float(), p), "piece is not bf16-exact"
    return b.view(torch.int16)


def _expected_image(wp, stride):
    """[chunk][slot][piece][half][row][8 channels] (include/cskel.h) filled element range by element range from the pieces."""
    co, ci, k = wp[0].shape
    taps = sf.tap_order(stride, k)
    slots, mpad, nch = -(-len(taps) // 3) * 3, -(-co // sf.MT) * sf.MT, sf.n_chunks(ci)
    img = torch.zeros((nch, slots, 3, 2, mpad, 8), dtype=torch.int16)
    for pc in range(3):
        bits = _bits(wp[pc])
        for slot, tap in enumerate(taps):
            for c in range(nch):
                for h in range(2):
                    lo = sf.KS * c + 8 * h
                    n = max(0, min(8, ci - lo))
                    img[c, slot, pc, h, :co, :n] = bits[:, lo: lo + n, tap]
    return img.reshape(-1)


def test_designed_operands_are_what_the_docstring_says():
    x, (h, m, l) = sf.designed((4, 33, 7), 11)
    assert torch.equal(h.double() + m.double() + l.double(), x.double())
    assert h.min() >= 1.0 and h.max() < 1.25 and m.min() >= 1.5 * 2.0 ** -9 and m.max() < 2.0 ** -8
    assert l.min() >= 32 * 2.0 ** -23 and l.max() <= 63 * 2.0 ** -23
    for p in (h, m, l):
        assert torch.equal(p.to(torch.bfloat16).float(), p)
    assert x.unique().numel() > 0.9 * x.numel()                   # values are (nearly all) distinct: a positional error shows
    for e in (0, 3, 5):                                           # a power-of-two scale is exact for the value and for every piece
        got = fold.split3_bf16(x * 2.0 ** -e)
        for g, p in zip(got, (h, m, l)):
            assert torch.equal(g.float(), p * 2.0 ** -e)


def test_conv64_is_the_plain_convolution():
    g = torch.Generator().manual_seed(5)
    for stride, pad, k, t in ((1, 4, 9, 13), (2, 4, 9, 12), (2, 4, 9, 1), (2, 0, 1, 7)):
        w = torch.randn(6, 5, k, generator=g)
        w[:, 2] = 0
        x = torch.randn(2, 5, t, 3, generator=g)
        want = F.conv2d(x.double(), w.double().unsqueeze(-1), stride=(stride, 1), padding=(pad, 0))
        assert torch.allclose(sf.conv64(w, x, stride, pad), want, rtol=0, atol=1e-13)


def test_six_products_are_the_exact_product_up_to_third_order():
    fx = sf.build(sf.DENSE[0])
    an = sf.analyse(fx)
    assert sf.rel_err(an["six"], an["want"], an["nz"]) <= 3.2e-8


def test_permutation_adjacency_passes_the_split_gate_and_copies_values():
    for V in (18, 25):
        a = sf.permutations(V)
        assert a.sum(1).max() == 1 and set(a.unique().tolist()) == {0.0, 1.0}       # at most one non-zero per column
        m = pkg.GraphConvolution(128, 128, a.numpy()).eval()
        m.precision = "bf16x3"
        ops = m._fold()
        assert [int(c) for c in ops["ell_cnt_host"]] == [1, 1, 1] and ops["ell_w"] == 1
        assert m._split_applies(ops)
        assert torch.equal(ops["ell_val"], torch.ones(3, V, 1))
        x = torch.rand(2, 3, 4, V)
        for r in range(3):
            assert torch.equal(torch.einsum("nctv,vw->nctw", x, a[r]), x[..., ops["ell_src"][r, :, 0].long()])
            assert torch.equal(ops["ell_src"][r, :, 0].long(), a[r].argmax(0))


def test_cases_cover_the_matrix():
    sf.assert_matrix_covered(sf.CASES, sf.DENSE)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_case_is_exact_on_the_way_in_admissible_and_bites(case):
    fx = sf.build(case)
    # (1) the operands are their designed pieces, for the host split and in the packed images; padding is zero
    for val, pieces in ((fx.w, fx.wp), (fx.x, fx.xp), (fx.w_res, fx.w_resp), (fx.x_res, fx.x_resp)):
        if val is not None:
            for got, p in zip(fold.split3_bf16(val), pieces):
                assert torch.equal(got.float(), p)
    w_img, r_img = sf.pack_images(fx, fold)
    assert w_img.dtype == torch.int16 and torch.equal(w_img, _expected_image(fx.wp, case.stride if case.kernel == "tcn" else 1))
    if r_img is not None:
        want_img = _expected_image(fx.w_resp, 1)
        assert torch.equal(r_img, want_img)
        assert not bool(want_img.view(sf.n_chunks(fx.w_res.shape[1]), 3, -1)[:, 1:].any())     # slots 1 and 2 of the K = 1 image
    # (2) reference, tolerance, admissibility -- all from the fixture
    an = sf.analyse(fx)
    assert float(an["want"].abs().max()) <= sf.REF_CAP
    if an["D"] is None:                                           # no product reaches any output: the kernel must be exact
        assert an["tol"] == 0.0 and not case.hot and not case.res_hot and not case.dense or case.T == 1
        assert torch.equal(sf.restate32(fx).double(), an["want"])
        return
    tol = an["tol"]
    assert 1e-6 < tol < 6e-6
    assert sf.rel_err(an["six"], an["want"], an["nz"]) <= THIRD < tol / 8
    r32 = sf.restate32(fx)
    assert not bool(r32[~an["nz"]].any())
    assert sf.rel_err(r32, an["want"], an["nz"]) <= tol / 2         # D / 4
    if not case.dense:
        assert an["bound"] <= tol, (an["bound"], tol)
    # (3) the check bites: the fp64 emulation without any one second-order product misses D / 2 wherever products reach
    for name, dropped in an["drops"].items():
        rel = ((dropped - an["want"]) / an["want"])[an["with_terms"]].abs()
        assert float(rel.min()) > tol, (name, float(rel.min()), tol)
