"""Skeleton pre-normalisation at its degenerate geometries: the case table, the fp64 reference with its per-element bound,
and a host model of the kernel with one seeded defect (test infrastructure).

``align_to_axis`` (csrc/prenorm.hip, restating rotation.py:10-50) decides three things per stage, in this order:
  bone0   sum|d| < 1e-6            the angle is 0
  axis0   sum|d x e_k| < 1e-6      the matrix is the identity (also for a bone antiparallel to e_k: angle pi, left alone)
  angle0  |angle| < 1e-6           the matrix is the identity
  rotate  otherwise
and ``latch_rotations`` decides three more in front of it: which of the four anchor joints are null (``(a + b) + c == 0`` in
fp32), that the centre is joint 1 of the main body null or not, and that the x-bone comes from the z-rotated anchors *after*
their rounding to fp32.  A case is one sample (3, T = 3, V, M) whose frame 0 is built around one of these decisions; all other
joints and frames are seeded multiples of 2^-6 with |x| <= 2.5.  Anchors are small-integer multiples of powers of two (the
tiny ones of U = 2^-30), the centre has zeros or multiples of U where the bone is tiny, so that the fp32 centred differences
are exactly the intended bone (``Case.exact`` names the stages for which test_prenorm_edge_fixture_cpu.py asserts that).

Two shape groups: ``ntu`` (V, M) = (25, 2) with the reference's joints (0, 1, 8, 4) -- the centre joint 1 is the upper z
anchor -- and ``kin`` (18, 1) with joints (8, 0, 5, 2), none of which is the centre.

Bound.  Per output element 3 * 2^-23 * r, r the fp64 L2 norm of that joint's centred position: a stage is one fp32 rounding
of an exact-to-fp64 dot; device and oracle matrices differ by libm ulps, so a stage can differ by one flipped rounding,
<= 2^-23 r per component; the first stage's flip passes through the orthogonal Rx (gain <= sqrt 3 per component), the second
stage adds one flip: (1 + sqrt 3) 2^-23 r = 2.73 * 2^-23 r; the rest pays for a matrix error of up to 2^-30.

Not separable, and said so rather than hidden:
  * ``no_bone_shortcut`` is an equivalent mutant.  sum|d x e_k| is a sub-sum of sum|d|, so a bone under the bone threshold
    is under the axis threshold too and the matrix is the identity whatever the angle came out as (NaN included: the axis
    test is the first operand of the ``||``).  The CPU test asserts that this defect changes no bit of any case.
  * a rounded-x case in which the x stage ends in axis0 cannot tell rounded from unrounded anchors: an off-axis part of 1e-16
    is under 1e-6 both ways.  ``zrot_xaxis0`` is kept as that geometry (spine on y, shoulders on x); ``rounded_x`` is the case
    that separates them: anchors ~95 from the centre whose exact z-rotated difference is 1.4e-7 off the x axis (axis0) while
    their fp32 roundings fall on either side of a rounding boundary and leave 7.6e-6, so the stage *rotates*, by 6e-6 rad,
    only because of the rounding.
"""
import math
from collections import namedtuple

import numpy as np

from tests import prenorm_oracle as po

T = 3
U = 2.0 ** -30
EPS = 1e-6
GROUPS = {"ntu": dict(V=25, M=2, joints=(0, 1, 8, 4)), "kin": dict(V=18, M=1, joints=(8, 0, 5, 2))}
OUTCOMES = ("bone0", "axis0", "angle0", "rotate")
BOUND_ULPS = 3.0
ROT_TOL = 2.0 ** -30
C_BIG, C_TINY = (0.5, -0.25, 0.875), (64 * U, 32 * U, 96 * U)
DEF_Z, DEF_X = (0.5, -0.25, 1.0), (1.0, 0.5, -0.25)          # the other stage's bone: well inside [20, 160] degrees
P_Z, P_X = (0.25, 0.5, -0.5), (-0.5, 0.25, 0.5)              # the lower anchor of a default bone (kin z; both groups x)
FAR = (40.0, -40.0, 33.0)                                    # r ~ 65 from the centre

Case = namedtuple("Case", "id group z x reference_exact close exact pair x_in")


def _seeded(seed, v, m):
    x = np.random.default_rng(seed).integers(-128, 129, size=(3, T, v, m)).astype(np.float32) / np.float32(64)
    x[0][((x[0] + x[1]) + x[2]) == 0] += np.float32(0.5)      # no null joint by accident
    return x


def whole_sums_nonzero(sample):
    """The fp32 sums of a whole sample, person and frame that the reference tests against 0 (preprocess.py:16-39, in its
    (M, T, V, C) view): all non-zero, so that its padding step and its skips act on all-zero data only -- here on none."""
    s = np.transpose(sample, [3, 1, 2, 0])
    return bool(s.sum() != 0 and all(p.sum() != 0 and all(f.sum() != 0 for f in p) for p in s))


def _centre_for(bone):
    return tuple(C_BIG[i] if float(bone[i] * 1024).is_integer() else C_TINY[i] for i in range(3))


def _case(cid, group, z, x, bz=None, bx=None, raw=None, far=False, reference_exact=True, close=(), pair=None, sx1=None, seed=[1900]):
    """``bz`` / ``bx``: the stage's bone as centred anchor difference (None: the default rotating geometry); ``raw``: role ->
    raw coordinates that replace what the geometry gives (roles z0 z1 x0 x1 c)."""
    g = GROUPS[group]
    v, m = g["V"], g["M"]
    raw = dict(raw or {})
    while True:                                               # the next seed with which no whole-frame sum cancels (1e8 - 1e8)
        seed[0] += 1
        xin = _place(_seeded(seed[0], v, m), g, bz, bx, raw, far, sx1)
        if whole_sums_nonzero(xin):
            break
    exact = ("z" if bz is not None else "") + ("x" if bx is not None and bz is not None else "")
    return Case(cid, group, z, x, reference_exact, tuple(close), exact, pair, xin)


def _place(xin, g, bz, bx, raw, far, sx1):
    v, m, (z0, z1, x0, x1) = g["V"], g["M"], g["joints"]
    focus = bz if bz is not None and any(bz) else bx if bx is not None else bz if bz is not None else DEF_Z
    c = np.array(raw.get("c", _centre_for(focus)), dtype=np.float32)
    if z1 == 1 and "z1" in raw:
        c = np.array(raw["z1"], dtype=np.float32)
    s = {}
    if z1 == 1:                                               # ntu: the upper z anchor is the centre itself
        s["z0"] = -np.array(DEF_Z if bz is None else bz)
    else:
        s["z0"] = np.array(P_Z if bz is None else (0.0, 0.0, 0.0))
        s["z1"] = s["z0"] + np.array(DEF_Z if bz is None else bz)
    s["x1"] = np.array(sx1 if sx1 is not None else (P_X if bx is None else (0.0, 0.0, 0.0)))
    s["x0"] = s["x1"] + np.array(DEF_X if bx is None else bx)
    joint = dict(z0=z0, z1=z1, x0=x0, x1=x1)
    xin[:, 0, 1, 0] = c
    for role, val in s.items():
        xin[:, 0, joint[role], 0] = (c.astype(np.float64) + val).astype(np.float32)
    for role, val in raw.items():
        if role != "c":
            xin[:, 0, joint[role], 0] = np.array(val, dtype=np.float32)
    if far:
        xin[:, 1, v - 3, 0] = np.array(FAR, dtype=np.float32)
    return xin


ROUNDED_X_BONE = (1.0 + 2.0 ** -22, 0.0, -0.75)              # Rz of the bone (0.75, 0, 1) turns it to (1.25, 0, 0.6 * 2^-22)


def _rounded_x_anchor():
    """The lower x anchor of ``rounded_x``: the first of a seeded sequence of positions (x ~ 2, z ~ 95: z-rotated z' ~ 77,
    one fp32 ulp there is 7.6e-6) whose two z-rotated anchors, 1.4e-7 apart off the axis, fall on either side of an fp32
    rounding boundary and at least 4e-8 from it -- no libm ulp in Rz (7e-15 there) moves either across."""
    rz, _ = po.align((0.75, 0.0, 1.0), po.Z_AXIS)
    rng = np.random.default_rng(1999)
    for _ in range(20000):
        b = np.array([2.05 + int(rng.integers(0, 2 ** 20)) * 2.0 ** -22, int(rng.integers(-128, 129)) / 64.0,
                      85.0 + int(rng.integers(0, 20 * 1024)) / 1024.0])
        b = b.astype(np.float32).astype(np.float64)
        z4, z8 = float(rz[2] @ b), float(rz[2] @ (b + ROUNDED_X_BONE))
        t4, t8 = float(np.float32(z4)), float(np.float32(z8))
        mid = (t4 + t8) / 2.0
        if t4 != t8 and min(abs(z4 - mid), abs(z8 - mid)) >= 4e-8:
            return tuple(b)
    raise RuntimeError("no anchor position found")


def _build():
    cases = []
    add = lambda *a, **k: cases.append(_case(*a, **k))        # noqa: E731
    zero3, nz_null = (0.0, 0.0, 0.0), (1.0, -1.0, 0.0)
    a_lo, a_hi = 483, 591                                     # 2 * 483 U = 0.8997e-6, 2 * 591 U = 1.1008e-6
    add("generic", "ntu", "rotate", "rotate")
    # ---- the z stage (the x stage is the default rotating geometry, or a vanishing bone) and its x twin (the z stage is a vanishing bone)
    for st in "zx":
        k = 2 if st == "z" else 0
        def vec(along, off1, off2):                           # components: along the target axis, and the two others
            out = [0.0, 0.0, 0.0]
            out[k], out[(k + 1) % 3], out[(k + 2) % 3] = along, off1, off2
            return tuple(out)

        def put(name, own, bone=None, **kw):
            if st == "z":                                     # an identity z stage shows in bits only next to an identity x stage
                still = own == "angle0" or "len1" in name
                add(f"z_{name}", "ntu", own, "bone0" if still else "rotate", bz=bone, bx=zero3 if still else None, **kw)
            else:
                add(f"x_{name}", "ntu", "bone0", own, bz=zero3, bx=bone, **kw)

        put("null_both_zero", "bone0", zero3, raw={"z0": zero3, "z1": zero3} if st == "z" else {"x0": zero3, "x1": zero3})
        put("equal", "bone0", zero3)
        put("bone_lo", "bone0", vec(0.0, a_lo * U, a_lo * U), pair="bone")
        put("bone_hi", "rotate", vec(0.0, a_hi * U, a_hi * U), pair="bone")
        put("on_axis", "axis0", vec(1.0, 0.0, 0.0))
        put("antiparallel", "axis0", vec(-1.0, 0.0, 0.0))
        put("tiny_oblique", "axis0", vec(430 * U, 430 * U, 430 * U), close=("bone", "axis"))
        put("axis_lo", "axis0", vec(1288 * U, a_lo * U, a_lo * U), pair="axis")
        put("axis_hi", "rotate", vec(1288 * U, a_hi * U, a_hi * U), pair="axis")
        put("axis_len1_lo", "axis0", vec(2.0, a_lo * U, a_lo * U), pair="axis")
        put("axis_len1_hi", "angle0", vec(2.0, a_hi * U, a_hi * U), pair="axis")
        put("angle0", "angle0", vec(1.5, 859 * U, 859 * U), close=("axis", "angle"))
        put("angle0_far", "angle0", vec(1.5, 859 * U, 859 * U), close=("axis", "angle"), far=True,
            reference_exact=False)                            # identity there too, but |want| ~ 65 is past the golden's cap of 8
        for sign, tag in ((1.0, "p"), (-1.0, "m")):
            put(f"right_{tag}1", "rotate", vec(0.0, sign, 0.0))
            put(f"right_{tag}2", "rotate", vec(0.0, 0.0, sign))
            # oracle-only: the reference's fp32 unit vector moves the angle near 0 and pi (make_golden_prenorm.py)
            put(f"near_{tag}", "rotate", vec(sign, 2.0 ** -10, 0.0), reference_exact=False)
    # ---- null anchors: each in turn, all-zero and non-zero with a zero fp32 sum
    for role in ("z0", "z1", "x0", "x1"):
        zo = "bone0" if role == "z0" else "rotate"            # ntu: the other z anchor is the centre, s = 0 null or not
        add(f"null_{role}_zero", "ntu", zo, "rotate", raw={role: zero3})
        add(f"null_{role}_nonzero", "ntu", zo, "rotate", raw={role: nz_null})
    add("null_x0_assoc", "ntu", "rotate", "rotate", raw={"x0": (1.0, 1e8, -1e8)})      # null as (a + b) + c, not as a + (b + c)
    # ---- the x-bone is formed from the z-rotated, fp32-rounded anchors
    add("zrot_xaxis0", "ntu", "rotate", "axis0", bz=(0.0, 1.0, 0.0), bx=(2.0, 0.0, 0.0), sx1=(-1.0, 0.5, 0.25), reference_exact=False)
    add("rounded_x", "ntu", "rotate", "rotate", bz=(0.75, 0.0, 1.0), bx=ROUNDED_X_BONE, sx1=_rounded_x_anchor(), reference_exact=False)
    # ---- (18, 1): the centre joint is no anchor
    add("kin_generic", "kin", "rotate", "rotate")
    add("kin_z_antiparallel", "kin", "axis0", "rotate", bz=(0.0, 0.0, -1.0))
    add("kin_x_antiparallel", "kin", "bone0", "axis0", bz=zero3, bx=(-1.0, 0.0, 0.0))
    add("kin_z_bone_hi", "kin", "rotate", "rotate", bz=(a_hi * U, a_hi * U, 0.0), pair="bone")
    add("kin_z_right", "kin", "rotate", "rotate", bz=(0.0, -1.0, 0.0))
    add("kin_null_z1_nonzero", "kin", "rotate", "rotate", raw={"z1": nz_null})
    add("kin_null_x1_zero", "kin", "rotate", "rotate", raw={"x1": zero3})
    add("kin_centre_null_zero", "kin", "rotate", "rotate", raw={"c": zero3})
    add("kin_centre_null_nonzero", "kin", "rotate", "rotate", raw={"c": nz_null})
    return cases


CASES = _build()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def batch(group, only=None):
    """(ids, x (N, 3, T, V, M) fp32) of a shape group; ``only``: a predicate on the case."""
    sel = [c for c in CASES if c.group == group and (only is None or only(c))]
    return [c.id for c in sel], np.stack([c.x_in for c in sel])


# ---- what a frame 0 decides, from the oracle's own intermediate quantities --------------------------------------------------
def quantities(frame, joints):
    """frame 0 (3, V, M) -> {"z": (sum|d|, sum|axis|, angle), "x": ...} and the fp32 bones, by the oracle's functions."""
    z0, z1, x0, x1 = joints
    null, s1 = po.null_mask(frame), po.centre(frame)
    dz = (s1[:, z1, 0] - s1[:, z0, 0]).astype(np.float64)
    rz, az = po.align(dz, po.Z_AXIS)
    s2 = po.rotate(rz, s1, null)
    dx = (s2[:, x0, 0] - s2[:, x1, 0]).astype(np.float64)
    _, ax = po.align(dx, po.X_AXIS)
    l1 = lambda v: float(np.abs(v).sum())                     # noqa: E731
    return dict(z=(l1(dz), l1(np.cross(dz, po.Z_AXIS)), az), x=(l1(dx), l1(np.cross(dx, po.X_AXIS)), ax), dz=dz, dx=dx)


def outcome(q):
    bone, axis, angle = q
    return "bone0" if bone < EPS else "axis0" if axis < EPS else "angle0" if abs(angle) < EPS else "rotate"


def centred(x):
    """(N, 3, T, V, M) fp32 -> the centred, masked input in fp32 numpy: what both stages being the identity must return."""
    x = np.asarray(x, dtype=np.float32)
    s1 = x - x[:, :, :, 1:2, 0:1]
    null = po.null_mask(x.transpose(0, 2, 1, 3, 4))          # (N, T, V, M)
    s1[np.broadcast_to(null[:, None], s1.shape)] = 0.0
    return s1, null


def radius(x):
    """(N, T, V, M) fp64: L2 norm of every joint's centred position (0 for a null joint)."""
    s1, _ = centred(x)
    return np.sqrt((s1.astype(np.float64) ** 2).sum(axis=1))


def bound(x):
    """(N, 1, T, V, M): the per-element bound, broadcast over the three channels."""
    return (BOUND_ULPS * 2.0 ** -23 * radius(x))[:, None]


def matrices(x, joints):
    """(N, 2, 3, 3) fp64: what the oracle latches per sample (Rz, Rx)."""
    return np.stack([np.stack(po.latch(x[n, :, 0], joints[:2], joints[2:])[:2]) for n in range(x.shape[0])])


def matrix_exact(m):
    """All nine entries 0 or +-1 in fp64: no libm ulp can move them, and a stage with this matrix is exact in fp32."""
    return bool(np.isin(m, (0.0, 1.0, -1.0)).all())


def apply(x, mats):
    """The oracle's two stages with given matrices (N, 2, 3, 3): centre, mask, rotate, round, rotate, round."""
    s1, null = centred(x)
    out = np.empty_like(s1)
    for n in range(x.shape[0]):
        out[n] = po.rotate(mats[n, 1], po.rotate(mats[n, 0], s1[n], null[n]), null[n])
    return out


def oracle(x, joints):
    return po.pre_normalize_clip(x, joints[:2], joints[2:])


# ---- the kernel's latch and normalise restated on the host, with one defect ----------------------------------------------------
DEFECTS = ("antiparallel_pi", "l2_bone", "l2_axis", "thresholds_1e-5", "thresholds_1e-7", "no_bone_shortcut", "no_angle_shortcut",
           "null_not_zeroed", "null_other_order", "xbone_unrotated", "xbone_unrounded", "centre_nonnull_only")
EQUIVALENT = ("no_bone_shortcut",)                           # module docstring: changes no bit of any input whatever


def _is_null(a, b, c, defect):
    a, b, c = np.float32(a), np.float32(b), np.float32(c)
    return bool((a + (b + c) if defect == "null_other_order" else (a + b) + c) == 0)


def _align(d, k, defect):
    """align_to_axis of csrc/prenorm.hip in fp64 numpy (k = 2: onto z, k = 0: onto x)."""
    dx, dy, dz = (float(v) for v in d)
    eps = {"thresholds_1e-5": 1e-5, "thresholds_1e-7": 1e-7}.get(defect, EPS)
    ax, ay, az = (dy, -dx, 0.0) if k == 2 else (0.0, dz, -dy)
    norm = (lambda *v: math.sqrt(sum(t * t for t in v))) if defect in ("l2_bone", "l2_axis") else None
    bone = norm(dx, dy, dz) if defect == "l2_bone" else abs(dx) + abs(dy) + abs(dz)
    axis = norm(ax, ay, az) if defect == "l2_axis" else abs(ax) + abs(ay) + abs(az)
    angle, cosine = 0.0, 1.0
    if bone >= eps or defect == "no_bone_shortcut":
        length = math.sqrt(dx * dx + dy * dy + dz * dz)
        cosine = (dz if k == 2 else dx) / length if length > 0 else float("nan")
        cosine = -1.0 if cosine < -1.0 else (1.0 if cosine > 1.0 else cosine)
        angle = math.acos(cosine) if cosine == cosine else float("nan")
    m = np.eye(3)
    if axis < eps:
        if defect == "antiparallel_pi" and bone >= eps and cosine < 0:
            m = np.diag([1.0, -1.0, -1.0]) if k == 2 else np.diag([-1.0, -1.0, 1.0])
        return m
    if abs(angle) < eps and defect != "no_angle_shortcut":
        return m
    inv = math.sqrt(ax * ax + ay * ay + az * az)
    a, s = math.cos(angle / 2.0), math.sin(angle / 2.0)
    b, c, d_ = -(ax / inv) * s, -(ay / inv) * s, -(az / inv) * s
    return np.array([[a * a + b * b - c * c - d_ * d_, 2 * (b * c + a * d_), 2 * (b * d_ - a * c)],
                     [2 * (b * c - a * d_), a * a + c * c - b * b - d_ * d_, 2 * (c * d_ + a * b)],
                     [2 * (b * d_ + a * c), 2 * (c * d_ - a * b), a * a + d_ * d_ - b * b - c * c]])


def _rot3(m, v):
    v = np.asarray(v, dtype=np.float64)
    return np.array([(m[i, 0] * v[0] + m[i, 1] * v[1]) + m[i, 2] * v[2] for i in range(3)])


def _centre_of(frame, defect):
    c = frame[:, 1, 0].astype(np.float32)
    if defect == "centre_nonnull_only" and _is_null(*c, None):
        return np.zeros(3, dtype=np.float32)
    return c


def model_latch(frame, joints, defect=None):
    """latch_rotations: frame 0 (3, V, M) fp32 -> (2, 3, 3) fp64."""
    c = _centre_of(frame, defect)
    s, null = [], []
    for j in joints:
        raw = frame[:, j, 0].astype(np.float32)
        null.append(_is_null(*raw, defect))
        s.append(np.zeros(3, dtype=np.float32) if null[-1] and defect != "null_not_zeroed" else raw - c)
    rz = _align((s[1] - s[0]).astype(np.float64), 2, defect)
    if defect == "xbone_unrotated":
        t = [v.astype(np.float64) for v in s[2:]]
    elif defect == "xbone_unrounded":
        t = [_rot3(rz, v) for v in s[2:]]
    else:
        t = [_rot3(rz, v).astype(np.float32) for v in s[2:]]
    t = [np.zeros(3, dtype=t[i].dtype) if null[2 + i] and defect != "null_not_zeroed" else t[i] for i in range(2)]
    bone = (t[0] - t[1]).astype(np.float64)
    return np.stack([rz, _align(bone, 0, defect)])


def model_clip(x, joints, defect=None):
    """The clip entry on (N, 3, T, V, M): latch from frame 0, then normalise4 on every joint.  -> (out, mats)."""
    x = np.asarray(x, dtype=np.float32)
    out, mats = np.zeros_like(x), []
    for n in range(x.shape[0]):
        m = model_latch(x[n, :, 0], joints, defect)
        mats.append(m)
        for t in range(x.shape[2]):
            c = _centre_of(x[n, :, t], defect)
            s1 = x[n, :, t] - c[:, None, None]
            a, b, cc = x[n, 0, t], x[n, 1, t], x[n, 2, t]
            null = ((a + (b + cc)) if defect == "null_other_order" else ((a + b) + cc)) == 0
            s1[:, null] = 0.0
            out[n, :, t] = po.rotate(m[1], po.rotate(m[0], s1, null), null)
    return out, np.stack(mats)


def clamp_search(n=200000, seed=1905):
    """Bounded seeded search for an fp32 bone whose unclamped fp64 cosine against z or x exceeds 1 in magnitude: random bones,
    and bones a few ulps off an axis.  -> list of offending bones (empty: a square of an fp32 number is exact in fp64, the sum
    under the root is then >= d_k^2 and a correctly rounded root of it >= |d_k|)."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    d[n // 2:, :2] *= np.float32(2.0) ** rng.integers(-40, -10, size=(n - n // 2, 1)).astype(np.float32)
    d[3 * n // 4:, :2] = 0.0
    d = np.concatenate([d, d[:, ::-1]]).astype(np.float64)
    length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    keep = length > 0
    bad = (np.abs(d[keep][:, 2] / length[keep]) > 1.0) | (np.abs(d[keep][:, 0] / length[keep]) > 1.0)
    return d[keep][bad]
