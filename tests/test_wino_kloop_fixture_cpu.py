"""CPU side of tests/test_gpu_wino_kloop.py: the integer operands of its cases keep every partial sum exact in fp32, the shapes
produce the chunk counts and tile kinds the GPU tests are there to pin, and the fixture's fp64 reference is the oracle's temporal
conv on the same data."""
import itertools

import torch

from oracle import stgcn_oracle as o
from tests import wino_kloop_fixture as fx


def test_partial_sums_stay_exact_in_fp32():
    assert fx.partial_sum_bound() < 2 ** 24, fx.partial_sum_bound()
    ev = range(-fx.W_EVEN, fx.W_EVEN + 1, 2)         # even conv weights: every F(2, 3) image value is an integer
    assert all((a + s * b + c) % 2 == 0 for a, b, c in itertools.product(ev, ev, ev) for s in (1, -1))
    for case in fx.cases()[:6]:
        d = fx.operands(case, 1)
        for k in ("y", "w", "bias", "x", "wres"):
            assert k not in d or torch.equal(d[k], d[k].round())


def test_cases_cover_chunk_counts_shapes_and_residual_patterns():
    cs = fx.cases()
    assert {c[2] // 8 for c in cs} == {1, 2, 3}                           # the peel alone, one trip + peel, two trips + peel
    assert {c[3] for c in cs} == {64, 128}
    assert {c[6] // 8 for c in cs if c[0] == "s2" and c[5] == "conv"} == {2, 3}
    assert {(c[0], c[5]) for c in cs} == {("s1", "identity"), ("s2", "none"), ("s2", "conv"), ("valid", "identity"), ("valid", "conv")}
    assert all(c[4] >= 9 for c in cs if c[0] == "valid")


def test_shapes_have_border_only_and_interior_tiles_in_both_workgroup_shapes():
    for mw in (1, 2):
        for v, t in fx.SHAPES:
            s1, valid = fx.tiles("s1", t, v, mw), fx.tiles("valid", t + 8, v, mw)
            if t == 7:
                assert t % 2 == 1 and not any(s1), (v, t, mw)             # odd, and every tile a border tile
            else:
                assert any(s1) and not s1[0] and not s1[-1], (v, t, mw)   # interior tiles between the border tiles
                assert any(valid), (v, t, mw)
                assert any(fx.tiles("s2", 2 * t - 1, v, mw)), (v, t, mw)
        assert len(fx.tiles("s1", 40, 25, mw)) > 1                         # more than one workgroup per sequence


def test_reference_is_the_oracles_temporal_conv():
    for case in (c for c in fx.cases() if c[1:4] == (25, 16, 64) or c[1:4] == (18, 24, 128)):
        d = fx.operands(case, 5)
        stride, pad = fx.stride_pad(d["form"])
        co = d["co"]
        sd = {"t_conv.weight": d["w"].double(), "t_conv.bias": d["bias"].double(), "bn.weight": torch.ones(co, dtype=torch.float64),
              "bn.bias": torch.zeros(co, dtype=torch.float64), "bn.running_mean": torch.zeros(co, dtype=torch.float64),
              "bn.running_var": torch.full((co,), 1.0 - o.BN_EPS, dtype=torch.float64)}
        want = o.temporal_conv(d["y"].double(), sd, "", stride=stride, padding=pad)
        got = fx.conv64(d)
        assert got.shape == want.shape
        assert float((got - want).abs().max()) < 1e-9 and torch.equal(got, want.round())
        # without a residual the reference is ReLU of that conv
        if d["res"] == "none":
            assert torch.equal(fx.reference(d), torch.relu(got).float())
