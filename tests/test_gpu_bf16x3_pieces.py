"""The "bf16x3" kernels (csrc/split_core.h, tcn_split.hip, gcn_split.hip) against fp64 at a tolerance that a lost piece product
misses.  Operands are designed from their bf16 pieces, weights are non-zero in one to three (tap slot, 16-channel chunk) pairs,
and the tolerance of a case is D / 2 relative per output, D being the smallest shift that leaving out mm, hl or lh causes in
an fp64 emulation of the same fixture (tests/split_fixture.py; tests/test_split_fixture_cpu.py checks the fixtures, their
admissibility and that each single-product drop fails, without a GPU).  Outputs that no term reaches must be exactly zero.
The stages are launched directly -- blocks.tcn_stage(split=True), csk_gcn_stage_bf16x3 -- on images packed with a unit scale,
zero bias, ReLU off (temporal conv) or a positive pre-activation (graph conv)."""
import pytest
import torch

import _bootstrap
from tests import split_fixture as sf

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
from continual_skeletons_amd import blocks, fold, native  # noqa: E402

DEV = "cuda:0"
RES_MODE = {"none": 0, "ident": 1, "conv": 2}          # CSK_RES_* (include/cskel.h)


def _dev(t):
    return None if t is None else t.to(DEV)


def _launch(fx):
    """Run the case's stage on its fixture; the output buffer starts as NaN (an element left unwritten fails the comparison)."""
    case = fx.case
    w_img, r_img = sf.pack_images(fx, fold)
    w_img, r_img = _dev(w_img), _dev(r_img)
    bias = fold.pad_vec(torch.zeros(case.co)).to(DEV)
    x = fx.x.to(DEV)
    out = torch.full((case.N, case.co, case.t_out, case.V), float("nan"), device=DEV)
    if case.kernel == "tcn":
        blocks.tcn_stage(x, w_img, bias, case.co, sf.K_TCN, case.stride, sf.PAD_TCN, relu=False, res_mode=RES_MODE[case.res],
                         x_res=_dev(fx.x_res), w_res=r_img, out=out, split=True)
    else:
        src, val, cnt, ew = fold.ell_from_dense(fx.adj)
        assert [int(c) for c in cnt] == [1, 1, 1]                  # within the <= 1 / 1 / 4 gate of GraphConvolution._split_applies
        src, val = src.to(DEV), val.to(DEV)
        rc = native.lib().csk_gcn_stage_bf16x3(native.ptr(x), native.ptr(out), native.ptr(w_img), native.ptr(r_img), native.ptr(bias),
                                               native.ptr(src), native.ptr(val), native.ptr(cnt), ew, case.N, case.ci, case.co, case.T,
                                               case.V, RES_MODE[case.res], native.stream_of(x))
        native.check(rc, "csk_gcn_stage_bf16x3")
    torch.cuda.synchronize()
    return out.cpu()


def test_sweep_covers_the_matrix():
    sf.assert_matrix_covered(sf.CASES, sf.DENSE)


def test_permutation_adjacency_takes_the_split_kernel():
    m = pkg.GraphConvolution(64, 128, sf.permutations(25).numpy()).eval()
    m.precision = "bf16x3"
    m.refold()
    assert m._split_applies(m._packed_ops(torch.device(DEV)))


@pytest.mark.parametrize("case", sf.CASES, ids=lambda c: c.id)
def test_hot_pairs_vs_fp64(case):
    fx = sf.build(case)
    an = sf.analyse(fx)
    assert an["D"] is None or an["bound"] <= an["tol"]
    sf.check_case(_launch(fx), an, case=case.id, n_hot=case.n_hot, template=case.template)


@pytest.mark.parametrize("case", sf.DENSE, ids=lambda c: c.id)
def test_dense_vs_fp64(case):
    """The one dense comparison per kernel (C_in 64: K = 576 / 192), at D / 2 of its own fixture.  Unlike the hot cases this one
    DEPENDS ON ROUND-TO-NEAREST ACCUMULATION in the matrix pipe: its admissibility rests on the sequential fp32 restatement
    (8.9e-7 at K = 576 against D / 2 = 2.4e-6), not on the rounding-mode-agnostic worst case, which K = 576 exceeds.  If this test
    alone fails while test_hot_pairs_vs_fp64 passes, the finding is about accumulation, not about a lost product.
    Measured on an MI355X: 2.26e-6 of 2.42e-6 at K = 576 (temporal conv), 7.7e-7 of 2.38e-6 at K = 192 (graph conv) -- the
    temporal conv is 2.5 times the restatement, so the pipe's accumulation is not a round-to-nearest sequential sum, and the
    margin of this case is thin; the hot cases (at most 3.6e-7 of at least 1.6e-6) are the ones that carry the claim."""
    fx = sf.build(case)
    an = sf.analyse(fx)
    sf.check_case(_launch(fx), an, case=case.id, n_hot="dense", template=case.template)
