"""tests/agcn_attention_fixture.py without a GPU: every case is admissible (integer embeddings, logit sums below 2^24, spans of at
most 8), the fused table reaches all twelve instantiations at every frame count, a plain fp32 model of the operation meets the bound
and each seeded defect moves some output by at least four times the bound."""
import numpy as np
import pytest

from tests import agcn_attention_fixture as fx


def _all_embeddings():
    for c in fx.ATT_CLIP:
        yield c.name, fx.att_operands(c.n, c.inter, c.T, c.V, 0), c.inter
    for c in fx.ATT_STEP:
        yield c.name, fx.att_operands(c.groups * c.spg, c.inter, 1, c.V, 1), c.inter
    for c in fx.EMB_CASES:
        x, w, b, a_sum = fx.emb_operands(c)
        assert set(np.unique(w).tolist()) <= {-1.0, 0.0, 1.0} and (np.abs(w).sum(axis=1) <= 2).all()
        E = fx.embed(x, w, b)
        yield c.name, ((fx.per_frame_view(E) if c.per_frame else E), a_sum), c.inter


def test_every_case_is_admissible_and_the_model_meets_the_bound():
    for name, (E, a_sum), inter in _all_embeddings():
        fx.admissible(E, inter)
        want, bnd = fx.reference(E, a_sum, inter)
        assert want.shape == bnd.shape and float(bnd.max()) < 2e-5 and float(bnd.min()) > 0, name
        assert (np.abs(fx.model_f32(E, a_sum, inter) - want) <= bnd).all(), name


def test_tables_cover_the_issue():
    assert {c.T for c in fx.ATT_CLIP} >= {1, 2, 63, 64, 65, 130} and {c.inter for c in fx.ATT_CLIP} >= {3, 6, 16, 20}
    assert {c.V for c in fx.ATT_CLIP} >= {2, 18, 25, 31, 32} and any(c.off for c in fx.ATT_CLIP)
    assert any(c.spg > 1 and c.group_pad and (3 * c.groups * c.spg) % 4 for c in fx.ATT_STEP)
    inst = {}
    for c in fx.EMB_CASES:
        inst.setdefault(fx.instantiation(c), []).append(c)
    assert len(inst) == 12 and set(inst) == {(i, 3 if i == 16 else 1, V, cl) for i in (16, 32, 64) for V in (18, 25) for cl in (False, True)}
    for (inter, np_, V, clip), cs in inst.items():
        assert {c.frames for c in cs} == {1, fx.FT[V], fx.FT[V] + 1, 3 * fx.FT[V] + 2}
    assert {c.c_in for c in fx.EMB_CASES} == {3, 16, 40}


def test_pair_major_image_is_the_conv_image_reordered():
    c = fx.EMB_CASES[0]
    x, w, b, _ = fx.emb_operands(c)
    pm, pb = fx.pair_major(w, b, c.inter)
    cv, cb = fx.conv_image(w, b)
    for i in range(3):
        for k in range(c.inter):
            assert np.array_equal(pm[:, i * 2 * c.inter + k], cv[:, i * c.inter + k]) and pb[i * 2 * c.inter + k] == cb[i * c.inter + k]
            assert np.array_equal(pm[:, i * 2 * c.inter + c.inter + k], cv[:, (3 + i) * c.inter + k])


@pytest.mark.parametrize("defect", fx.DEFECTS)
def test_each_seeded_defect_moves_an_output_by_four_bounds(defect):
    for name, (E, a_sum), inter in _all_embeddings():
        if defect == "next_segment" and E.shape[0] == 1:
            continue
        want, bnd = fx.reference(E, a_sum, inter)
        bad = fx.model_f32(E, a_sum, inter, defect)
        assert (np.abs(bad - want) >= 4 * bnd).any(), (name, defect)
