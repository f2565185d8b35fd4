"""Multi-stream logit fusion + top-k on the GPU vs the numpy oracle: bit-exact fusion."""
import numpy as np
import pytest
import torch

import _bootstrap
from oracle import stgcn_oracle as o

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
DEV = "cuda:0"


@pytest.mark.parametrize("n_streams", [1, 2, 4])
@pytest.mark.parametrize("method", ["add", "maximum"])
@pytest.mark.parametrize("steps", [0, 3])
def test_fusion_and_topk(n_streams, method, steps):
    rng = np.random.default_rng(10 * n_streams + steps)
    n, classes = 517, 60
    shape = (n, classes, steps) if steps else (n, classes)
    preds = [rng.standard_normal(shape).astype(np.float32) for _ in range(n_streams)]
    targets = rng.integers(0, classes, n)
    want = o.fuse_preds(preds, np.add if method == "add" else np.maximum)
    dev = [torch.from_numpy(p).to(DEV) for p in preds]
    got = pkg.fusion.aggregate_preds(dev, method).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    accs = pkg.fusion.topk_accuracies(dev, targets, (1, 3, 5), method)
    assert np.allclose(accs, o.topk_accuracies_np(want, targets), atol=1e-7)


@pytest.mark.parametrize("dims", ["2d", "3d"])
def test_fusion_equals_the_reference_fixture_g10(dims):
    """csk_fuse_rank_f32 against G10 = outputs of the reference's own aggregate_preds (scripts/multi_stream_eval.py:33-42,
    executed by tests/golden/make_golden.py): bit-exact for add and maximum over 1-4 streams, 2-D and 3-D predictions."""
    from tests.helpers import load_golden
    a, _ = load_golden("g10_fusion")
    dev = [torch.from_numpy(a[f"{dims}/pred{i}"]).to(DEV) for i in range(4)]
    for n in (1, 2, 3, 4):
        for name in ("add", "maximum"):
            want = a[f"{dims}/{name}{n}"]
            want = want[:, :, 0] if want.ndim == 3 else want
            got = pkg.fusion.aggregate_preds(dev[:n], name).cpu().numpy()
            assert got.shape == want.shape and np.array_equal(got, want), (dims, name, n)


def test_fusion_errors():
    a = torch.rand(4, 60, device=DEV)
    with pytest.raises(AssertionError):
        pkg.fusion.aggregate_preds([a, torch.rand(4, 61, device=DEV)])
    with pytest.raises(ValueError):
        pkg.fusion.aggregate_preds([a] * 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.fusion.aggregate_preds([a.cpu()])


def _tie_cases():
    from tests import nan_cone_fixture as fx
    return fx.TIE_CASES


@pytest.mark.parametrize("case", _tie_cases(), ids=lambda c: c.id)
def test_fusion_rank_with_ties(case):
    """Integer-valued logits in [-2, 2]: classes tie with the target all the time (tests/test_nan_cone_fixture_cpu.py: in at least
    half the samples), so "a class outranks the target only when it scores STRICTLY higher" decides the rank.  N no multiple of 4,
    60 and 400 classes, targets at class 0 and at the last class; fused values, rank and top-1/3/5 exactly the definition's."""
    from tests import nan_cone_fixture as fx
    preds, targets = fx.tie_operands(case)
    fused, rank, accs = fx.tie_reference(case, preds, targets)
    assert fx.tie_fraction(fused, targets) >= 0.5
    dev = [torch.from_numpy(p).to(DEV) for p in preds]
    got_fused, got_rank = pkg.fusion._launch(dev, case.method, targets=targets)
    assert np.array_equal(got_fused.cpu().numpy(), fused)
    assert np.array_equal(got_rank.cpu().numpy().astype(np.int64), rank)
    # hit counts from integer data: the device's ranks give exactly the definition's counts, and the definition's accuracies are
    # those counts over n (one fp64 division)
    hits = [int((got_rank.cpu().numpy().astype(np.int64) < k).sum()) for k in (1, 3, 5)]
    assert hits == [int((rank < k).sum()) for k in (1, 3, 5)] and accs == [h / case.n for h in hits]
    # the package forms its mean on the device in fp32: the same expression on the definition's ranks, same device, bit for bit
    want_accs = [float((torch.from_numpy(rank).to(DEV) < k).float().mean()) for k in (1, 3, 5)]
    assert pkg.fusion.topk_accuracies(dev, targets, (1, 3, 5), case.method) == want_accs
