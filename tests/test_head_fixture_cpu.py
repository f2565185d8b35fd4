"""CPU side of tests/test_gpu_head_kernels.py: the exact-tier operands keep every partial sum exact in fp32, the float-tier bound
is smaller than half of any term, the case tables reach the kernels' branch points, and -- the evidence that the GPU tests would
notice a subtly wrong kernel -- a plain fp32 model of every reduction passes every case while the same model with one seeded
defect fails."""
from fractions import Fraction

import numpy as np
import pytest

from tests import head_fixture as fx

f32 = np.float32


# ---- plain fp32 models of the operations (sequential sums), with the seeded defects -------------------------------------------
def _seq_sum(terms):
    """left-to-right fp32 sum over the last axis"""
    return np.cumsum(terms.astype(f32), axis=-1, dtype=f32)[..., -1]


def _defective_terms(terms, defect):
    if defect == "drop_last":
        return terms[..., :-1] if terms.shape[-1] > 1 else np.zeros_like(terms)
    if defect == "double":
        mid = terms.shape[-1] // 2
        return np.concatenate([terms, terms[..., mid: mid + 1]], axis=-1)
    return terms


def model_pool(h, n, m, scale, defect=None):
    nm, c, tv = h.shape
    terms = np.transpose(h.reshape(n, m, c, tv), (0, 2, 1, 3)).reshape(n, c, m * tv)
    return _seq_sum(_defective_terms(terms, defect)) / f32(m * tv) * f32(scale)


def model_spatial(h, n, mv, defect=None):
    terms = np.transpose(h[:, : n * mv].reshape(h.shape[0], n, mv), (1, 0, 2))
    return _seq_sum(_defective_terms(terms, defect)) / f32(mv)


def model_fc(feat, w, b, defect=None):
    terms = _defective_terms(feat[:, None, :].astype(f32) * w[None, :, :].astype(f32), defect)
    out = _seq_sum(terms) + b[None, :].astype(f32)
    if defect == "bias_skip_64":
        out[:, 64:] = _seq_sum(terms)[:, 64:]
    return out


def model_window(ring, head, count, window, defect=None):
    shift = 1 if defect == "slot_off_by_one" else 0
    terms = np.stack([ring[(head - age - shift) % window] for age in range(count - 1, -1, -1)], axis=-1)
    return _seq_sum(_defective_terms(terms, defect)) / f32(count if defect == "divide_by_count" else window)


def model_input_norm(x, scale, shift, defect=None):
    n, c, t, v, m = x.shape
    out = np.empty((n * m, c, t, v), dtype=f32)
    for mi in range(m):
        for vi in range(v):
            for ci in range(c):
                ch = (vi * m + mi) * c + ci if defect == "permute_mvc" else fx.norm_channel(c, v, mi, vi, ci)
                out[mi::m, ci, :, vi] = fx.fma_f32(x[:, ci, :, vi, mi], scale[ch], shift[ch])
    return out


def model_head(w, b, frames, n, c, mv, window, defect=None):
    """the continual head step by step -> [(ring, pooled or None, logits or None)] per step"""
    ring = np.zeros((window, n, c), dtype=f32)
    out = []
    for (step, head, count, emit, zero), h in zip(fx.head_steps(window), frames):
        ring[head] = 0 if zero else model_spatial(h, n, mv, defect if defect in ("drop_last", "double") else None)
        pooled = logits = None
        if emit:
            pooled = model_window(ring, head, count, window, defect if defect in ("slot_off_by_one", "divide_by_count") else None)
            logits = model_fc(pooled, w, b, defect if defect == "bias_skip_64" else None)
        out.append((ring.copy(), pooled, logits))
    return out


# ---- the checks the GPU tests make, on a model --------------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


def _same_bits(got, want, what):
    if not np.array_equal(np.asarray(got, dtype=f32), np.asarray(want, dtype=f32)):
        raise Mismatch(what)


def _within(got, want64, terms_abs_sum, n_terms, what):
    if not np.all(np.abs(fx.f64(got) - want64) <= fx.bound(terms_abs_sum, n_terms)):
        raise Mismatch(what)


def _pool_cases(run):
    for tv in fx.POOL_TV:
        for m in fx.POOL_M:
            for n, c in fx.POOL_NC:
                h = fx.exact_operand(np.random.default_rng(tv * 100 + m * 10 + n), (n * m, c, tv))
                for scale in fx.POOL_SCALES:
                    _same_bits(run(h, n, m, scale), fx.exact_pool_bits(fx.ref_pool_sum(h, n, m), m * tv, scale), ("pool", tv, m, n, c, scale))
    for tv in fx.POOL_FLOAT_TV:
        m = fx.POOL_FLOAT_M
        for n, c in fx.POOL_NC:
            h = fx.float_operand(np.random.default_rng(tv + n), (n * m, c, tv))
            for scale in fx.POOL_SCALES:
                _within(run(h, n, m, scale), fx.ref_pool(h, n, m, scale), fx.ref_pool(np.abs(h), n, m, scale), m * tv, ("pool", tv, n, c, scale))


def _fc_operands(tier, n, c, classes):
    rng = np.random.default_rng(c * 1000 + classes + n)
    if tier == "exact":
        return fx.exact_operand(rng, (n, c)), fx.exact_operand(rng, (classes, c)), fx.exact_operand(rng, (classes,), fx.BIAS_AMP)
    return fx.float_operand(rng, (n, c)), fx.float_operand(rng, (classes, c)), fx.float_operand(rng, (classes,))


def _fc_cases(run):
    for c in fx.FC_C:
        for classes in fx.FC_CLASSES:
            for n in fx.FC_N:
                feat, w, b = _fc_operands("exact", n, c, classes)
                _same_bits(run(feat, w, b), fx.ref_fc(feat, w, b), ("fc", c, classes, n))
                feat, w, b = _fc_operands("float", n, c, classes)
                _within(run(feat, w, b), fx.ref_fc(feat, w, b), fx.ref_fc(np.abs(feat), np.abs(w), np.abs(b)), c + 1, ("fc", c, classes, n))


def _spatial_cases(run):
    for mv in fx.SPATIAL_MV:
        for n, c in fx.SPATIAL_NC:
            p = fx.spatial_p(n, mv)
            h = fx.exact_operand(np.random.default_rng(mv + n), (c, p))
            _same_bits(run(h, n, mv), fx.exact_pool_bits(fx.ref_spatial_sum(h, n, mv), mv), ("spatial", mv, n, c))
            h = fx.float_operand(np.random.default_rng(mv + n), (c, p))
            _within(run(h, n, mv), fx.ref_spatial_sum(h, n, mv) / mv, fx.ref_spatial_sum(np.abs(h), n, mv) / mv, mv, ("spatial", mv, n, c))


def _window_cases(run):
    for window in fx.WINDOWS:
        ring_i = fx.exact_operand(np.random.default_rng(window), (window, fx.WINDOW_ELEMS))
        ring_f = fx.float_operand(np.random.default_rng(window), (window, fx.WINDOW_ELEMS))
        for head, count in fx.window_states(window):
            _same_bits(run(ring_i, head, count, window), fx.exact_pool_bits(fx.ref_window_sum(ring_i, head, count, window), window),
                       ("window", window, head, count))
            want = fx.ref_window_sum(ring_f, head, count, window) / window
            _within(run(ring_f, head, count, window), want, want, count, ("window", window, head, count))


def _head_cases(defect=None):
    for tier, cases in (("exact", fx.HEAD_EXACT), ("float", fx.HEAD_FLOAT)):
        for n, c, mv, classes, window in cases:
            w, b, frames = fx.head_operands(tier, n, c, mv, classes, window, seed=c + window)
            ring64 = np.zeros((window, n, c))
            for (step, head, count, emit, zero), h, (ring, pooled, logits) in zip(fx.head_steps(window), frames,
                                                                                 model_head(w, b, frames, n, c, mv, window, defect)):
                what = (tier, n, c, mv, classes, window, step)
                if tier == "exact":
                    ring64[head] = 0 if zero else fx.ref_spatial_sum(h, n, mv) / mv
                    _same_bits(ring, ring64, what)
                    if emit:
                        want = fx.ref_window_sum(ring64, head, count, window) / window
                        _same_bits(pooled, want, what)
                        _same_bits(logits, fx.ref_fc(want, w, b), what)
                else:                                                   # stage by stage, each on the operands the stage read
                    if not zero:
                        _within(ring[head], fx.ref_spatial_sum(h, n, mv) / mv, fx.ref_spatial_sum(h, n, mv) / mv, mv, what)
                    if emit:
                        want = fx.ref_window_sum(ring, head, count, window) / window
                        _within(pooled, want, want, count, what)
                        want = fx.ref_fc(pooled, w, b)
                        _within(logits, want, want, c + 1, what)


def _norm_cases(run):
    for shape in fx.NORM_DENSE + (fx.NORM_STRIDED,):
        n, c, t, v, m = shape
        rng = np.random.default_rng(sum(shape))
        x = rng.standard_normal(shape).astype(f32)
        scale, shift = fx.distinct_affine(rng, m * v * c)
        _same_bits(run(x, scale, shift), fx.ref_input_norm(x, scale, shift), ("input_norm", shape))


# ---- tests --------------------------------------------------------------------------------------------------------------------
def test_exact_tier_partial_sums_stay_below_2_to_24():
    amp2 = fx.INT_AMP * fx.INT_AMP
    assert max(fx.POOL_TV) * max(fx.POOL_M) * fx.INT_AMP < 2 ** 24
    assert max(fx.SPATIAL_MV) * fx.INT_AMP < 2 ** 24 and max(fx.WINDOWS) * fx.INT_AMP < 2 ** 24
    assert max(fx.FC_C) * amp2 + fx.BIAS_AMP < 2 ** 24
    p = fx.POOL_FC_CASE
    assert p["m"] * p["tv"] * (fx.K_AMP + p["m"] * p["tv"] // 2) < 2 ** 24 and p["c"] * fx.K_AMP * fx.INT_AMP + fx.BIAS_AMP < 2 ** 24
    for n, c, mv, classes, window in fx.HEAD_EXACT:
        assert window in (4, 8, 16)
        assert mv * (fx.K_AMP + mv // 2) < 2 ** 24                       # spatial sums: integers
        assert window * fx.K_AMP * window < 2 ** 24                      # window sums, and pooled in units of 1 / window
        assert (c * fx.K_AMP * fx.INT_AMP + fx.BIAS_AMP) * window < 2 ** 24      # FC partial sums in units of 1 / window


def test_exact_tier_head_values_are_the_dyadics_claimed():
    """the spatial mean of every row is its integer k, pooled is a multiple of 1 / window, the logits are multiples of 1 / window
    that fp32 holds exactly"""
    for n, c, mv, classes, window in fx.HEAD_EXACT:
        w, b, frames = fx.head_operands("exact", n, c, mv, classes, window, seed=c + window)
        ring = np.zeros((window, n, c))
        for (step, head, count, emit, zero), h in zip(fx.head_steps(window), frames):
            ring[head] = 0 if zero else fx.ref_spatial_sum(h, n, mv) / mv
            assert np.all(ring[head] == np.round(ring[head])) and np.abs(ring[head]).max() <= fx.K_AMP
            if not zero:
                assert np.isnan(h[:, n * mv:]).all() and h.shape[1] % 4 == 0 and h.shape[1] > n * mv
            pooled = fx.ref_window_sum(ring, head, count, window) / window
            logits = fx.ref_fc(pooled, w, b)
            for a in (pooled, logits):
                assert np.all(a * window == np.round(a * window)) and np.all(a.astype(f32).astype(np.float64) == a)
    rng = np.random.default_rng(0)
    for nn in (1, 2, 18, 25, 36, 50, 100):
        k, x = fx.exact_mean_rows(rng, 7, nn)
        assert np.all(x == np.round(x)) and np.array_equal(x.astype(np.float64).sum(1), nn * k.astype(np.float64))
    p = fx.POOL_FC_CASE
    assert fx.zero_sum(p["m"] * p["tv"]).sum() == 0


def test_float_tier_bound_is_below_half_of_any_term():
    def ok(terms, what):
        n_terms, smallest, worst = fx.margin(terms)
        assert n_terms <= fx.MAX_FLOAT_TERMS, (what, n_terms)
        assert smallest > 2 * worst, (what, n_terms, smallest, worst)

    for tv in fx.POOL_FLOAT_TV:
        m = fx.POOL_FLOAT_M
        for n, c in fx.POOL_NC:
            h = fx.float_operand(np.random.default_rng(tv + n), (n * m, c, tv))
            for scale in fx.POOL_SCALES:
                ok(np.transpose(h.reshape(n, m, c, tv), (0, 2, 1, 3)).reshape(n, c, m * tv) * scale / (m * tv), ("pool", tv, n, c))
    for c in fx.FC_C:
        for classes in fx.FC_CLASSES:
            for n in fx.FC_N:
                feat, w, b = _fc_operands("float", n, c, classes)
                terms = np.concatenate([feat[:, None, :].astype(np.float64) * w[None], np.broadcast_to(b[None, :, None], (n, classes, 1))], -1)
                ok(terms, ("fc", c, classes, n))
    for mv in fx.SPATIAL_MV:
        for n, c in fx.SPATIAL_NC:
            h = fx.float_operand(np.random.default_rng(mv + n), (c, fx.spatial_p(n, mv)))
            ok(h[:, : n * mv].reshape(c, n, mv) / mv, ("spatial", mv))
    for window in fx.WINDOWS:
        ring = fx.float_operand(np.random.default_rng(window), (window, fx.WINDOW_ELEMS))
        ok(np.moveaxis(ring, 0, -1) / window, ("window", window))
    for n, c, mv, classes, window in fx.HEAD_FLOAT:                     # the head's three stages, each a sum of its own
        w, b, frames = fx.head_operands("float", n, c, mv, classes, window, seed=c + window)
        steps = model_head(w, b, frames, n, c, mv, window)
        ok(np.stack([h[:, : n * mv].reshape(c, n, mv) for h in frames if h is not None]) / mv, ("head spatial", c))
        ring, pooled, _ = [s for s in steps if s[1] is not None][-1]    # the last emitting step: a full window
        ok(np.moveaxis(ring, 0, -1) / window, ("head window", window))
        ok(np.concatenate([pooled[:, None, :].astype(np.float64) * w[None], np.broadcast_to(b[None, :, None], (n, classes, 1))], -1), ("head fc", c))
    for shapes in (fx.POOL_FLOAT_TV, ):
        assert max(shapes) * fx.POOL_FLOAT_M <= fx.MAX_FLOAT_TERMS


def test_case_tables_reach_the_branch_points():
    # a 64-lane strided walk that keeps eight loads in flight while lane + 7 * 64 < TV: some TV splits the lanes
    assert any(0 + 448 < tv <= 63 + 448 for tv in fx.POOL_TV)
    assert any(tv <= 448 for tv in fx.POOL_TV) and any(tv > 511 + 512 for tv in fx.POOL_TV)
    assert {tv % 64 for tv in fx.POOL_TV} >= {0, 1, 63}
    assert all(n * c % 4 for n, c in fx.POOL_NC) and any(n * c > 4 for n, c in fx.POOL_NC)
    # the ring walk takes the entries older than the newest eight at a time: a second pass needs count - 1 >= 9
    assert any(w - 1 >= 9 for w in fx.WINDOWS) and any(w - 1 >= 9 for *_, w in fx.HEAD_FLOAT) and 1 in fx.WINDOWS
    assert any(w - 1 > 16 for *_, w in fx.HEAD_FLOAT)                    # ... and a third
    # FC: 64 classes per wave, four waves per block
    ktiles = lambda classes: (classes + 63) // 64       # noqa: E731
    assert any(n * ktiles(k) % 4 for n in fx.FC_N for k in fx.FC_CLASSES) and any(n * ktiles(k) > 4 for n in fx.FC_N for k in fx.FC_CLASSES)
    assert any(k % 64 for k in fx.FC_CLASSES) and any(k % 64 == 0 for k in fx.FC_CLASSES) and any(k > 64 for k in fx.FC_CLASSES)
    assert any(c % 4 for c in fx.FC_C) and any(c % 4 == 0 for c in fx.FC_C) and any(c % 4 and c > 64 for c in fx.FC_C)
    heads = fx.HEAD_EXACT + fx.HEAD_FLOAT
    assert any(c % 4 and c > 64 for _, c, *_ in heads) and any(c > 512 for _, c, *_ in heads) and any(c % 64 == 0 for _, c, *_ in heads)
    assert any(k > 64 for _, _, _, k, _ in heads) and any(mv > 64 for mv in fx.SPATIAL_MV) and any(mv < 64 for mv in fx.SPATIAL_MV)
    # steps: silent ones, one zero feature, filling / full / wrapped windows
    for window in {w for *_, w in heads}:
        steps = fx.head_steps(window)
        assert len(steps) == 2 * window + 3 and sum(z for *_, z in steps) == 1
        assert any(not e for _, _, _, e, _ in steps) and any(e and cnt < window for _, _, cnt, e, _ in steps if window > 2)
        assert max(s for s, *_ in steps) // window == 2
        assert all(cnt >= 1 for _, _, cnt, _, _ in steps)
    # input norm: the large case needs a second trip of the grid-stride loop; padded rows really have padding
    assert np.prod(fx.NORM_LARGE) > fx.NORM_GRID_THREADS and all(np.prod(s) < fx.NORM_GRID_THREADS for s in fx.NORM_DENSE)
    assert all(fx.frames_p(n, m, v) % 4 == 0 and fx.frames_p(n, m, v) >= n * m * v + 8 for n, _, v, m in fx.FRAMES_SHAPES)
    assert all(fx.spatial_p(n, mv) % 4 == 0 and fx.spatial_p(n, mv) > n * mv for mv in fx.SPATIAL_MV for n, _ in fx.SPATIAL_NC)


def test_fma_reference_rounds_once():
    """fp32(x scale + shift) in one rounding: against exact rational arithmetic on random operands, and on a constructed case where
    rounding the fp64 sum a second time goes the other way (fp64 gives 2^24 + 3, a tie; the exact value lies just below it)"""
    def round_f32(q):
        if q == 0:
            return 0.0
        sign, a = (-1 if q < 0 else 1), abs(q)
        e = a.numerator.bit_length() - a.denominator.bit_length()
        e = e if a >= Fraction(2) ** e else e - 1                       # 2^e <= a < 2^(e + 1)
        step = Fraction(2) ** (e - 23)
        k, rem = divmod(a, step)
        k = int(k) + (1 if rem * 2 > step or (rem * 2 == step and int(k) % 2) else 0)
        return sign * float(k * step)

    x, s = f32(1 + 2.0 ** -23), f32(1 - 2.0 ** -23)
    for sg in (1.0, -1.0):
        got = fx.fma_f32(f32(sg) * x, s, f32(sg * (2.0 ** 24 + 2)))
        assert float(got) == sg * (2.0 ** 24 + 2)
        assert float(f32(np.float64(sg * x) * np.float64(s) + sg * (2.0 ** 24 + 2))) == sg * (2.0 ** 24 + 4)    # the double rounding
    rng = np.random.default_rng(5)
    a, b, c = (rng.standard_normal(2000).astype(f32) for _ in range(3))
    got = fx.fma_f32(a, b, c)
    for i in range(a.size):
        assert float(got[i]) == round_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))), i


def test_plain_models_pass_every_case():
    _pool_cases(model_pool)
    _fc_cases(model_fc)
    _spatial_cases(model_spatial)
    _window_cases(model_window)
    _head_cases()
    _norm_cases(model_input_norm)


@pytest.mark.parametrize("defect,cases", [
    ("drop_last", lambda d: _pool_cases(lambda *a: model_pool(*a, defect=d))),
    ("double", lambda d: _pool_cases(lambda *a: model_pool(*a, defect=d))),
    ("drop_last", lambda d: _spatial_cases(lambda *a: model_spatial(*a, defect=d))),
    ("double", lambda d: _spatial_cases(lambda *a: model_spatial(*a, defect=d))),
    ("drop_last", lambda d: _fc_cases(lambda *a: model_fc(*a, defect=d))),
    ("double", lambda d: _fc_cases(lambda *a: model_fc(*a, defect=d))),
    ("bias_skip_64", lambda d: _fc_cases(lambda *a: model_fc(*a, defect=d))),
    ("slot_off_by_one", lambda d: _window_cases(lambda *a: model_window(*a, defect=d))),
    ("divide_by_count", lambda d: _window_cases(lambda *a: model_window(*a, defect=d))),
    ("double", lambda d: _window_cases(lambda *a: model_window(*a, defect=d))),
    ("drop_last", _head_cases), ("double", _head_cases), ("slot_off_by_one", _head_cases), ("divide_by_count", _head_cases),
    ("bias_skip_64", _head_cases),
    ("permute_mvc", lambda d: _norm_cases(lambda *a: model_input_norm(*a, defect=d))),
])
def test_a_seeded_defect_fails(defect, cases):
    with pytest.raises(Mismatch):
        cases(defect)


@pytest.mark.parametrize("tier", ["exact", "float"])
def test_each_defect_fails_in_each_tier_of_the_head(tier, monkeypatch):
    """the two tiers do not lean on each other: every defect of the head is caught by the exact cases alone and by the float cases
    alone"""
    monkeypatch.setattr(fx, "HEAD_FLOAT" if tier == "exact" else "HEAD_EXACT", ())
    _head_cases()
    for defect in ("drop_last", "double", "slot_off_by_one", "divide_by_count", "bias_skip_64"):
        with pytest.raises(Mismatch):
            _head_cases(defect)
