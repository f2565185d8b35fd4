"""tests/nan_cone_fixture.py on the host: the cones are non-empty, nested, confined to the poisoned sequence and equal to what
the really poisoned fp64 reference gives; the case lists hold the seam, edge and middle-sequence positions; the restated
Winograd transforms equal the direct conv and keep (stride 1) or exceed by exactly the documented frames (stride 2) its cone."""
import numpy as np
import pytest
import torch

from tests import nan_cone_fixture as fx

ALL_BLOCKS = fx.BLOCK_CASES + fx.MOD_CASES + fx.SIX_CASES


def _other_sequences_clear(mask, n0):
    keep = torch.ones(mask.shape[0], dtype=torch.bool)
    keep[n0] = False
    return not bool(mask[keep].any())


@pytest.mark.parametrize("case", ALL_BLOCKS, ids=lambda c: c.id)
def test_block_cone(case):
    must, may = fx.block_masks(case)
    assert tuple(must.shape) == tuple(may.shape) == case.out_shape
    assert bool(must.any())
    assert not bool((must & ~may).any())
    assert _other_sequences_clear(may, case.poison[0])
    got = torch.isnan(fx.block_reference(case, fx.block_input(case)))
    assert not bool((must & ~got).any())                 # sparse op: the reference holds at least the structural cone
    assert torch.equal(got, may)                         # and, with its dense matmul, exactly the dense one
    assert not bool(torch.isnan(fx.block_reference(case, fx.block_input(case, clean=True))).any())
    if case.res == "identity" and case.pad < 0:
        n0, c0, t0, v0 = case.poison
        assert bool(must[n0, c0, t0, v0])                # the identity residual carries it straight through


@pytest.mark.parametrize("case", fx.AGCN_CASES + list(fx.AGCN_STEP_CASES), ids=lambda c: c.id)
def test_adaptive_graph_conv_cone(case):
    must, may = fx.agcn_masks(case)
    n0, _, t0, _ = case.poison
    assert bool(must.any()) and not bool((must & ~may).any())
    assert _other_sequences_clear(may, n0)
    want = torch.zeros(case.out_shape, dtype=torch.bool)
    if case.form == "clip":
        want[n0] = True                                  # the attention sums over every frame of the sequence
    else:
        want[n0, :, t0] = True                           # the whole frame: the softmax must not skip the NaN
    assert torch.equal(may, want)
    got = torch.isnan(fx.agcn_reference(case, fx.agcn_input(case)))
    assert torch.equal(got, may)                         # dense op: exactly the cone
    assert not bool(torch.isnan(fx.agcn_reference(case, fx.agcn_input(case, clean=True))).any())


@pytest.mark.parametrize("case", fx.HEAD_CASES, ids=lambda c: c.id)
def test_head_cone(case):
    must, may = fx.head_masks(case)
    h, w, b = fx.head_operands(case)
    want = torch.zeros((case.N, case.classes), dtype=torch.bool)
    want[case.poison[0] // case.M] = True                # exactly that row of logits, every class
    assert torch.equal(must, want) and torch.equal(may, want)
    h[case.poison] = float("nan")
    assert torch.equal(torch.isnan(fx.head_reference(case, h, w, b)), may)


@pytest.mark.parametrize("case", fx.CO_HEAD_CASES, ids=lambda c: c.id)
def test_continual_head_cone(case):
    """the step head and the clip-as-steps head: the NaN's row of logits, every class, for exactly the predictions whose pooling
    window (zero-initialised, ``window`` entries) holds the poisoned feature frame -- the head has finite memory"""
    must, may = fx.co_head_masks(case)
    h, w, b = fx.co_head_operands(case)
    n_pred, t0 = case.steps - case.first_entry, case.poison[2]
    want = torch.zeros((n_pred, case.N, case.classes), dtype=torch.bool)
    for k in range(n_pred):
        e = case.first_entry + k
        want[k, case.poison[0] // case.M] = e - case.window < t0 <= e
    assert bool(must.any()) and torch.equal(must, want) and torch.equal(may, want)
    assert torch.equal(torch.isnan(fx.co_head_reference(case, fx.co_head_poisoned(case, h), w, b)), may)
    assert not bool(torch.isnan(fx.co_head_reference(case, h, w, b)).any())


def test_continual_head_cases_cover_filling_sliding_and_last_frames():
    kinds = set()
    for c in fx.CO_HEAD_CASES:
        t0 = c.poison[2]
        kinds.add("first" if t0 == 0 else "last" if t0 == c.steps - 1 else "slides out" if t0 + c.window < c.steps else "mid")
        assert 0 < c.poison[0] // c.M < c.N - 1 or c.N < 3            # a stream that is neither first nor last
    assert {"first", "last", "slides out"} <= kinds and {c.window for c in fx.CO_HEAD_CASES} >= {1}


def test_poison_positions_cover_the_seams_and_edges():
    for cases in (fx.BLOCK_CASES, fx.MOD_CASES, fx.AGCN_CASES):
        frames = {c.poison[2] for c in cases}
        assert {0, 15, 16, fx.T - 1} <= frames
        for V in (25, 18):
            joints = {c.poison[3] for c in cases if c.V == V}
            assert {0, V - 1} <= joints
        assert any(c.poison[1] == 0 for c in cases) and any(c.poison[1] == c.ci - 1 and c.ci > 1 for c in cases)
        assert any(0 < c.poison[0] < c.N - 1 for c in cases)
        key = lambda c: (c.geometry, getattr(c, "form", ""))  # noqa: E731
        for k in {key(c) for c in cases}:
            assert len({c.poison for c in cases if key(c) == k}) == 3
        assert {c.N for c in cases} == {3, 4}
    assert {c.N for c in fx.SIX_CASES} == {6} and any(0 < c.poison[0] < 5 for c in fx.SIX_CASES)
    assert {(c.ci, c.co, c.stride, c.res) for c in fx.BLOCK_CASES} == set(fx.LAYER_ROWS)
    assert 0 < fx.CO_POISONED < fx.CO_STREAMS - 1 and fx.CO_POISON_FRAME % 4 != 0


# ---- Winograd ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,t", [(1, 20), (1, 21), (2, 20), (2, 21), (2, 23)])
def test_restated_winograd_equals_the_direct_conv(stride, t):
    rng = np.random.default_rng(t + stride)
    y = rng.integers(-3, 4, (5, t, 3)).astype(np.float64)
    w = rng.integers(-4, 5, (4, 5, 9)).astype(np.float64)               # integers: halves in the image, exact sums in fp64
    assert np.array_equal(fx.wino(y, w, stride), fx.direct(y, w, stride))


@pytest.mark.parametrize("t", [20, 21])
def test_winograd_f23_keeps_the_direct_cone(t):
    """Y0 uses d0 .. d2 and Y1 d1 .. d3 of every 3-tap group: frame for frame the direct window -- structurally and on a really
    poisoned input"""
    rng = np.random.default_rng(t)
    w = rng.standard_normal((4, 2, 9))
    for t0 in range(t):
        assert fx.wino_frames(t0, t, 1) == fx.direct_frames(t0, t, 1), t0
        y = rng.standard_normal((2, t, 3))
        y[1, t0, 2] = np.nan
        got = np.isnan(fx.wino(y, w, 1))
        assert np.array_equal(got, np.isnan(fx.direct(y, w, 1)))
        assert sorted(set(np.nonzero(got)[1].tolist())) == fx.direct_frames(t0, t, 1)


def extra_wino_s2(t0, t):
    return sorted(set(fx.wino_frames(t0, t, 2)) - set(fx.direct_frames(t0, t, 2)))


@pytest.mark.parametrize("t", [20, 21, 23])
def test_winograd_stride2_exceeds_the_direct_cone_by_the_zero_tap_frames(t):
    """FINDING (module docstring of the fixture): the 2-tap groups carry d2 against a zero tap, so input frames 2 t' + 5 and
    2 t' + 6 reach the EVEN output frame t' -- one output frame in front of the direct cone, same sequence, same joint.  Nothing
    else is added and nothing of the direct cone is lost; the restated transform on a poisoned input gives exactly these frames."""
    t_out = (t - 1) // 2 + 1
    rng = np.random.default_rng(t)
    w = rng.standard_normal((4, 2, 9))
    seen = False
    for t0 in range(t):
        reach, window = fx.wino_frames(t0, t, 2), fx.direct_frames(t0, t, 2)
        assert set(window) <= set(reach)
        want_extra = sorted(tt for tt in range(0, t_out, 2) if t0 - 2 * tt in (5, 6))
        assert extra_wino_s2(t0, t) == want_extra, t0
        seen = seen or bool(want_extra)
        y = rng.standard_normal((2, t, 3))
        y[0, t0, 1] = np.nan
        got = np.isnan(fx.wino(y, w, 2))
        assert sorted(set(np.nonzero(got)[1].tolist())) == reach
        assert not got[:, :, [0, 2]].any()                               # the joint is kept
    assert seen


@pytest.mark.parametrize("case", [c for c in fx.BLOCK_CASES + fx.SIX_CASES if c.stride == 2], ids=lambda c: c.id)
def test_stride2_winograd_block_mask_is_the_dense_cone_plus_the_named_frames(case):
    must, may = fx.block_masks(case)
    wide = fx.may_wino_s2(case)
    n0, _, t0, _ = case.poison
    assert not bool((may & ~wide).any()) and _other_sequences_clear(wide, n0)
    extra = (wide & ~may).any(0).any(0).any(-1).nonzero().flatten().tolist()
    assert extra == extra_wino_s2(t0, fx.T)


# ---- the continual oracle and the tie fixture ----------------------------------------------------------------------------------
def test_tie_cases_tie():
    assert {c.classes for c in fx.TIE_CASES} == {60, 400} and any(c.n % 4 for c in fx.TIE_CASES)
    assert {c.streams for c in fx.TIE_CASES} == {1, 2, 3, 4} and {c.steps > 0 for c in fx.TIE_CASES} == {False, True}
    for case in fx.TIE_CASES:
        preds, targets = fx.tie_operands(case)
        fused, rank, _ = fx.tie_reference(case, preds, targets)
        assert targets[0] == 0 and targets[1] == case.classes - 1
        assert fx.tie_fraction(fused, targets) >= 0.5, case.id
        assert np.array_equal(fused, np.round(fused)) and fused.dtype == np.float32
        assert int(rank.max()) > 0
