"""The degenerate-geometry cases of the skeleton pre-normalisation (tests/prenorm_edge_fixture.py), proved without a GPU:
every case takes the branch outcome it declares and keeps its distance from the thresholds, every outcome of both stages is
reached, the bound holds for the oracle under a matrix error of 2^-30, the host model of the kernel passes what the device test
asks and every seeded defect of it fails, and the oracle reproduces what the reference's own function wrote for these cases
(tests/golden/g19_prenorm_edges.npz, make_golden_prenorm_edges.py).  Run with -s for the tables."""
import os

import numpy as np
import pytest

from tests import prenorm_edge_fixture as fx
from tests import prenorm_oracle as po
from tests.helpers import GOLDEN

GROUP_NAMES = tuple(fx.GROUPS)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def world():
    """Per group: ids, cases, x, the oracle's output, its matrices, the bound -- computed once, never written to."""
    out = {}
    for group, g in fx.GROUPS.items():
        ids, x = fx.batch(group)
        d = dict(ids=ids, cases=[fx.BY_ID[i] for i in ids], x=x, joints=g["joints"], want=fx.oracle(x, g["joints"]),
                 mats=fx.matrices(x, g["joints"]), bound=fx.bound(x), centred=fx.centred(x)[0])
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[group] = d
    return out


# ---- the table ------------------------------------------------------------------------------------------------------------------
def test_shapes_values_and_exact_bones(world):
    assert len(fx.CASES) <= 64
    for group, w in world.items():
        g = fx.GROUPS[group]
        assert w["x"].shape == (len(w["ids"]), 3, fx.T, g["V"], g["M"]) and w["x"].dtype == np.float32
        assert 1 not in g["joints"] or group == "ntu"
        z0, z1, x0, x1 = g["joints"]
        for c, x in zip(w["cases"], w["x"]):
            assert fx.whole_sums_nonzero(x), c.id
            anchors = np.zeros(x.shape[1:], dtype=bool)
            anchors[0, [z0, z1, x0, x1, 1], 0] = True
            if c.id.endswith("_far"):
                anchors[1, g["V"] - 3, 0] = True
            if c.id != "rounded_x":
                assert np.abs(x.transpose(1, 2, 3, 0)[~anchors]).max() <= 8.0, c.id
            assert not po.null_mask(x.transpose(1, 0, 2, 3))[~anchors].any(), c.id          # null joints: the intended anchors only
            s1 = po.centre(x[:, 0]).astype(np.float64)
            raw = x[:, 0].astype(np.float64)
            if "z" in c.exact and "null" not in c.id:         # the fp32 centred difference is the difference of the raw joints, exactly
                assert np.array_equal(s1[:, z1, 0] - s1[:, z0, 0], raw[:, z1, 0] - raw[:, z0, 0]), c.id
            if "x" in c.exact and "null" not in c.id:
                assert np.array_equal(s1[:, x0, 0] - s1[:, x1, 0], raw[:, x0, 0] - raw[:, x1, 0]), c.id
    far = fx.BY_ID["z_angle0_far"].x_in
    assert fx.radius(far[None])[0].max() >= 64.0 and fx.radius(fx.BY_ID["x_angle0_far"].x_in[None])[0].max() >= 64.0


def test_every_case_takes_the_outcome_it_declares_with_margin(world):
    """Margins are a condition: a threshold pair sits 10 to 12 % from 1e-6, a quantity a case names in ``close`` at least 5 %,
    every other one at least a factor of 2 -- a libm ulp or the reference's fp32 sums cannot flip a branch."""
    reached = {"z": set(), "x": set()}
    print()
    for group, w in world.items():
        for c, x in zip(w["cases"], w["x"]):
            q = fx.quantities(x[:, 0], w["joints"])
            got = fx.outcome(q["z"]), fx.outcome(q["x"])
            print(f"{c.id:26s} z {got[0]:7s} {q['z'][0]:.3e} {q['z'][1]:.3e} {q['z'][2]:.3e}   x {got[1]:7s} {q['x'][0]:.3e} {q['x'][1]:.3e} {q['x'][2]:.3e}"
                  f"   {'reference' if c.reference_exact else 'oracle only'}")
            assert got == (c.z, c.x), (c.id, got)
            reached["z"].add(got[0])
            reached["x"].add(got[1])
            n_pair = 0
            for st in "zx":
                for name, val in zip(("bone", "axis", "angle"), q[st]):
                    ratio = abs(val) / fx.EPS
                    if ratio == 0.0 or ratio >= 2.0 or ratio <= 0.5:
                        continue
                    if c.pair is not None:
                        assert 0.10 <= abs(ratio - 1.0) <= 0.12, (c.id, st, name, ratio)
                        n_pair += name == c.pair
                    else:
                        assert name in c.close and abs(ratio - 1.0) >= 0.05, (c.id, st, name, ratio)
            assert (c.pair is None) == (n_pair == 0), c.id
    assert reached["z"] == set(fx.OUTCOMES) and reached["x"] == set(fx.OUTCOMES), reached
    lo, hi = fx.BY_ID["z_bone_lo"], fx.BY_ID["z_bone_hi"]
    assert (lo.z, hi.z) == ("bone0", "rotate") and (fx.BY_ID["x_bone_lo"].x, fx.BY_ID["x_bone_hi"].x) == ("bone0", "rotate")


def test_rounded_x_exists_only_because_of_the_rounding():
    """Exact z-rotated anchors: 1.4e-7 off the x axis, under the threshold by a factor of 5.  Rounded to fp32: 7.6e-6, over it
    by more than 2, and an angle over it by more than 2.  Neither anchor is within 4e-8 of the rounding boundary."""
    c = fx.BY_ID["rounded_x"]
    z0, z1, x0, x1 = fx.GROUPS["ntu"]["joints"]
    s1 = po.centre(c.x_in[:, 0])
    rz, _ = po.align(s1[:, z1, 0] - s1[:, z0, 0], po.Z_AXIS)
    exact = rz @ s1[:, x0, 0].astype(np.float64) - rz @ s1[:, x1, 0].astype(np.float64)
    q = fx.quantities(c.x_in[:, 0], (z0, z1, x0, x1))
    assert abs(exact[1]) + abs(exact[2]) <= 2e-7 and q["x"][1] >= 5e-6 and q["x"][2] >= 5e-6
    for j in (x0, x1):
        v = float(rz[2] @ s1[:, j, 0].astype(np.float64))
        r = float(np.float32(v))
        assert abs(abs(v - r) - 2.0 ** -18) >= 3.9e-8          # half an ulp of [64, 128) is 2^-18


def test_the_clamp_is_unreachable_from_fp32_bones():
    """A bounded seeded search (4e5 bones, half of them a few binades off an axis, a quarter on it) finds no fp32 bone whose
    unclamped fp64 cosine exceeds 1 in magnitude; the fixture's docstring says why there is none.  So no clamp case."""
    assert len(fx.clamp_search()) == 0


# ---- the bound ----------------------------------------------------------------------------------------------------------------------
def _ratio(got, want, bound):
    """Largest |got - want| / bound over elements with a bound > 0; where the bound is 0 (null joints, joints at the centre)
    the value must be 0, else inf (of either sign: a row of negative entries times +0 sums to -0; null joints are +0, checked on the device)."""
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    zero = np.broadcast_to(bound == 0, err.shape)
    if got[zero].any():
        return float("inf")
    return float((err[~zero] / np.broadcast_to(bound, err.shape)[~zero]).max())


def test_bound_holds_under_a_matrix_error_of_2_to_the_minus_30(world):
    rng = np.random.default_rng(30)
    print()
    for group, w in world.items():
        worst = 0.0
        for _ in range(8):
            mats = w["mats"] + fx.ROT_TOL * rng.choice([-1.0, 1.0], size=w["mats"].shape)
            worst = max(worst, _ratio(fx.apply(w["x"], mats), w["want"], w["bound"]))
        assert np.array_equal(_bits(fx.apply(w["x"], w["mats"])), _bits(w["want"]))
        print(f"{group}: oracle with matrices +-2^-30 against itself: max err / bound = {worst:.3f}")
        assert worst <= 1.0


# ---- the host model and its defects ---------------------------------------------------------------------------------------------------
def _verdict(c, got, mats, w, n):
    """What tests/test_gpu_prenorm_edges.py asks of the device, on sample n: (passes, fails by a factor of 10 or by a bit)."""
    want, bound = w["want"][n], w["bound"][n]
    ident = [c.z != "rotate", c.x != "rotate"]
    eye_ok = all(np.array_equal(mats[i], np.eye(3)) for i in range(2) if ident[i])
    rot_err = max([float(np.abs(mats[i] - w["mats"][n, i]).max()) for i in range(2) if not ident[i]] or [0.0])
    if all(ident):
        same = np.array_equal(_bits(got), _bits(w["centred"][n]))
        return same and eye_ok, not same
    ratio = _ratio(got, want, bound) if np.isfinite(got).all() else np.inf
    return ratio <= 1.0 and eye_ok and rot_err <= fx.ROT_TOL, ratio >= 10.0


def test_host_model_passes_and_every_defect_is_caught(world):
    caught = {d: [] for d in fx.DEFECTS}
    print()
    for group, w in world.items():
        got, mats = fx.model_clip(w["x"], w["joints"])
        for n, c in enumerate(w["cases"]):
            ok, _ = _verdict(c, got[n], mats[n], w, n)
            assert ok, (c.id, "the model without a defect")
        for d in fx.DEFECTS:
            bad, bad_mats = fx.model_clip(w["x"], w["joints"], d)
            if d in fx.EQUIVALENT:
                assert np.array_equal(_bits(bad), _bits(got)) and np.array_equal(bad_mats, mats), d
                continue
            for n, c in enumerate(w["cases"]):
                ok, far_out = _verdict(c, bad[n], bad_mats[n], w, n)
                if far_out:
                    assert not ok
                    caught[d].append(c.id)
    for d, ids in caught.items():
        print(f"{d:22s} {'equivalent: changes no bit (fixture docstring)' if d in fx.EQUIVALENT else ' '.join(ids)}")
    assert all(caught[d] for d in fx.DEFECTS if d not in fx.EQUIVALENT), [d for d in caught if not caught[d]]
    # the defects are caught where they were aimed
    for d, cid in (("antiparallel_pi", "z_antiparallel"), ("antiparallel_pi", "x_antiparallel"), ("l2_bone", "z_bone_hi"), ("l2_axis", "x_axis_hi"),
                   ("thresholds_1e-5", "z_axis_hi"), ("thresholds_1e-7", "x_axis_lo"), ("no_angle_shortcut", "z_angle0_far"),
                   ("null_not_zeroed", "null_x0_nonzero"), ("null_other_order", "null_x0_assoc"), ("xbone_unrotated", "generic"),
                   ("xbone_unrounded", "rounded_x"), ("centre_nonnull_only", "kin_centre_null_nonzero"), ("centre_nonnull_only", "null_z1_nonzero")):
        assert cid in caught[d], (d, cid)


# ---- the golden file ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUP_NAMES)
def test_oracle_reproduces_the_reference_on_the_reference_exact_cases(world, group):
    """Within 1e-6 absolute, test_prenorm_cpu.py's figure; the file holds exactly the cases the table marks, and their inputs."""
    g = np.load(os.path.join(GOLDEN, "g19_prenorm_edges.npz"))
    ids, x = fx.batch(group, only=lambda c: c.reference_exact)
    assert [str(i) for i in g[f"{group}/ids"]] == ids and np.array_equal(_bits(g[f"{group}/x"]), _bits(x))
    want = g[f"{group}/want"]
    assert want.dtype == np.float32 and np.abs(want).max() <= 8.0
    kinds = {fx.BY_ID[i].id.split("_", 1)[-1] for i in ids}
    if group == "ntu":
        assert {"antiparallel", "on_axis", "bone_lo", "bone_hi", "axis_lo", "axis_hi", "right_p1", "angle0", "x0_assoc"} <= kinds
        assert not any(i.startswith(("z_near", "x_near")) for i in ids)
    pick = [w for w, i in enumerate(world[group]["ids"]) if i in ids]
    err = np.abs(world[group]["want"][pick].astype(np.float64) - want).reshape(len(ids), -1).max(axis=1)
    print(f"\n{group}: {len(ids)} cases, max |oracle - reference| = {err.max():.3e} ({ids[int(err.argmax())]}), |want| max {np.abs(want).max():.3f}")
    assert err.max() <= 1e-6
