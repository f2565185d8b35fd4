"""numpy restatement of the skeleton pre-normalisation (test infrastructure; DESIGN.md section 3c, include/cskel.h).

The reference's ``datasets/data_preparation/preprocess.py:14-93`` centres every frame on the main body's joint 1 and rotates
the clip so that the zaxis bone of the first frame lies on z and the xaxis line on x (``rotation.py:10-50``).
tests/golden/g14_prenorm.npz holds what that function itself wrote and tests/test_prenorm_cpu.py checks this restatement
against it.  Here the matrices are fp64 from the fp32 bone on, and every stage is rounded to fp32 once, as the reference
stores each stage into its fp32 array.  Not restated: the padding of null frames (it looks ahead), and the ``== 0`` tests on
whole-person / whole-frame sums, which act here on all-zero data only."""
import math

import numpy as np

Z_AXIS, X_AXIS = (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)


def rotation_matrix(axis, theta):
    """fp64 quaternion form of rotation.py:10-29, with its identity shortcuts."""
    axis = np.asarray(axis, dtype=np.float64)
    if np.abs(axis).sum() < 1e-6 or abs(theta) < 1e-6:
        return np.eye(3)
    axis = axis / math.sqrt(float(np.dot(axis, axis)))
    a = math.cos(theta / 2.0)
    b, c, d = -axis * math.sin(theta / 2.0)
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c + a * d), 2 * (b * d - a * c)],
                     [2 * (b * c - a * d), a * a + c * c - b * b - d * d, 2 * (c * d + a * b)],
                     [2 * (b * d + a * c), 2 * (c * d - a * b), a * a + d * d - b * b - c * c]])


def angle_to(d, target):
    """fp64 angle between the bone ``d`` and a unit axis (rotation.py:37-50); 0 for a vanishing bone."""
    d = np.asarray(d, dtype=np.float64)
    if np.abs(d).sum() < 1e-6:
        return 0.0
    u = d / math.sqrt(float(np.dot(d, d)))
    return math.acos(min(1.0, max(-1.0, float(np.dot(u, np.asarray(target))))))


def align(d, target):
    """Rotation that turns the fp32 bone ``d`` onto ``target``: (matrix, angle)."""
    d = np.asarray(d, dtype=np.float32).astype(np.float64)
    angle = angle_to(d, target)
    return rotation_matrix(np.cross(d, np.asarray(target)), angle), angle


def null_mask(x):
    """(..., 3, V, M) -> (..., V, M) bool: joint is null iff (x0 + x1) + x2 == 0 in fp32."""
    x = np.asarray(x, dtype=np.float32)
    return ((x[..., 0, :, :] + x[..., 1, :, :]) + x[..., 2, :, :]) == 0


def centre(frame):
    """(3, V, M) frame -> s1: minus the main body's joint 1 of the same frame, null joints +0."""
    frame = np.asarray(frame, dtype=np.float32)
    s1 = frame - frame[:, 1:2, 0:1]
    s1[:, null_mask(frame)] = 0.0
    return s1


def rotate(m, s, null):
    """fp32(m . fp64(s)) per joint of a (3, ...) stage -- a three-term fp64 dot, one rounding; null joints stay +0."""
    s = s.astype(np.float64)
    out = np.stack([(m[i, 0] * s[0] + m[i, 1] * s[1]) + m[i, 2] * s[2] for i in range(3)]).astype(np.float32)
    out[:, null] = 0.0
    return out


def latch(frame, zaxis=(0, 1), xaxis=(8, 4)):
    """(3, V, M) first frame of a sample / stream -> (Rz, Rx, angle_z, angle_x)."""
    null = null_mask(frame)
    s1 = centre(frame)
    rz, az = align(s1[:, zaxis[1], 0] - s1[:, zaxis[0], 0], Z_AXIS)
    s2 = rotate(rz, s1, null)
    rx, ax = align(s2[:, xaxis[0], 0] - s2[:, xaxis[1], 0], X_AXIS)
    return rz, rx, az, ax


def normalise_frame(frame, rz, rx, use_mask=True, centre_of=None):
    """One (3, V, M) frame with latched matrices.  ``use_mask`` / ``centre_of`` (a frame whose centre is taken instead of
    the frame's own) exist for the tests' wrong-on-purpose variants."""
    null = null_mask(frame) if use_mask else np.zeros(frame.shape[1:], dtype=bool)
    s1 = np.asarray(frame, dtype=np.float32) - (frame if centre_of is None else centre_of)[:, 1:2, 0:1]
    s1[:, null] = 0.0
    return rotate(rx, rotate(rz, s1, null), null)


def pre_normalize_clip(x, zaxis=(0, 1), xaxis=(8, 4)):
    """Clip form, (N, 3, T, V, M) fp32 -> the same shape: matrices from frame 0 of each sample, whole clip at once."""
    x = np.asarray(x, dtype=np.float32)
    out = np.empty_like(x)
    for n in range(x.shape[0]):
        rz, rx, _, _ = latch(x[n, :, 0], zaxis, xaxis)
        null = null_mask(x[n].transpose(1, 0, 2, 3))                           # (T, V, M)
        s1 = x[n] - x[n, :, :, 1:2, 0:1]
        s1[:, null] = 0.0
        out[n] = rotate(rx, rotate(rz, s1, null), null)
    return out


def pre_normalize_steps(x, first=None, zaxis=(0, 1), xaxis=(8, 4)):
    """Step form over a sequence (N, 3, T, V, M), frame by frame: a stream latches its matrices on every frame where
    ``first[n, t]`` (bool (N, T); default: t == 0 only) and uses them until the next such frame."""
    x = np.asarray(x, dtype=np.float32)
    n_, _, t_, _, _ = x.shape
    if first is None:
        first = np.zeros((n_, t_), dtype=bool)
        first[:, 0] = True
    out = np.empty_like(x)
    for n in range(n_):
        rz = rx = None
        for t in range(t_):
            if first[n, t] or rz is None:
                rz, rx, _, _ = latch(x[n, :, t], zaxis, xaxis)
            out[n, :, t] = normalise_frame(x[n, :, t], rz, rx)
    return out


def latched_angles(x, zaxis=(0, 1), xaxis=(8, 4)):
    """(N, 2) degrees: the two angles each sample latches from its frame 0."""
    return np.array([[math.degrees(a) for a in latch(x[n, :, 0], zaxis, xaxis)[2:]] for n in range(x.shape[0])])
