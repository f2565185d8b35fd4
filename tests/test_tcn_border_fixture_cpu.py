"""CPU side of tests/test_gpu_tcn_border_tiles.py: the integer operands of its cases keep every partial sum exact in fp32, and the
shapes really produce what the GPU tests are there to pin -- border tiles, interior tiles, sequences that are all border, and the
16 / 16 + 8 / lone 8 channel chunks of the stride-2 residual phase."""
import itertools

from tests import tcn_border_fixture as fx


def test_partial_sums_stay_exact_in_fp32():
    worst = max(fx.partial_sum_bound(c, r) for c in fx.C_IN for r in (0,) + fx.S2_CRES + fx.VALID_CRES)
    assert worst < 2 ** 24, worst
    # even conv weights: every F(2, 3) image value (w0 +- w1 + w2) / 2 is an integer
    ev = range(-fx.W_EVEN, fx.W_EVEN + 1, 2)
    assert all((a + s * b + c) % 2 == 0 for a, b, c in itertools.product(ev, ev, ev) for s in (1, -1))


def _kinds(form, ts):
    seen = {}
    for t, v, co in itertools.product(ts, fx.JOINTS, fx.C_OUT):
        seen[(t, v, co)] = [tl["interior"] for tl in fx.tiles(form, t, v, co)]
    return seen


def test_stride1_shapes_have_border_and_interior_tiles():
    seen = _kinds("s1", fx.S1_T)
    for (t, v, co), kinds in seen.items():
        if t <= 10:
            assert not any(kinds), (t, v, co)                       # T <= 10: the whole sequence is border
        assert not kinds[0] and not kinds[-1]                       # pad 4: both ends of every sequence are border
    for v, co in itertools.product(fx.JOINTS, fx.C_OUT):
        assert any(seen[(40, v, co)]), (v, co)                      # interior tiles between border tiles at T = 40
        assert not any(seen[(11, v, co)]), (v, co)                  # ... none yet at T = 11, in two or three tiles at V = 25
    assert len(seen[(11, 25, 64)]) == 2 and len(seen[(11, 25, 128)]) == 3
    assert any(t % 2 for t in fx.S1_T)


def test_stride2_shapes_have_border_and_interior_tiles_and_a_remainder_chunk():
    seen = _kinds("s2", fx.S2_T)
    for (t, v, co), kinds in seen.items():
        assert not kinds[0] and not kinds[-1], (t, v, co)
        if t <= 22:
            assert not any(kinds), (t, v, co)                       # all border, in one, two or three tiles
    for v in fx.JOINTS:                                             # T_in = 61: interior tiles in the tall shape, and at V = 25 in the wide one
        assert any(seen[(61, v, 128)]) and not all(seen[(61, v, 128)]), v
    assert any(seen[(61, 25, 64)])
    assert {len(k) for (t, v, co), k in seen.items() if t <= 22} == {1, 2, 3}
    assert [fx.res_chunks(c) for c in fx.S2_CRES] == [[8], [8], [16], [16, 8], [16, 16, 8]]


def test_valid_shapes_have_interior_tiles():
    seen = _kinds("valid", fx.VALID_T)
    assert all(len(k) >= 1 for k in seen.values())
    assert all(any(seen[(30, v, co)]) for v in fx.JOINTS for co in fx.C_OUT)


def test_embedding_turns_border_tiles_into_interior_tiles():
    """the long rows of the interior / border agreement test: some output frame lies in a border tile of the short launch and in
    an interior tile of the launch on the zero-embedded row"""
    for form, (t, front, back), stride in (("s1", fx.LONG_S1, 1), ("s2", fx.LONG_S2, 2)):
        assert front % (2 * stride) == 0                             # frame pairs of the two launches line up
        shift = front // stride
        for v, co in itertools.product(fx.JOINTS, fx.C_OUT):
            short = {f for tl in fx.tiles(form, t, v, co) if not tl["interior"] for f in tl["frames"]}
            long_ = {f - shift for tl in fx.tiles(form, front + t + back, v, co) if tl["interior"] for f in tl["frames"]}
            assert short & long_, (form, v, co)
