#!/usr/bin/env python
"""Generate tests/golden/g14_prenorm.npz by running the REFERENCE's own ``pre_normalization``.

``datasets/data_preparation/preprocess.py:14-93`` is imported from the reference checkout (with ``rotation.py`` next to it)
and called, unmodified and never copied, on tiny synthetic joint clips (``tqdm`` is stubbed by name only where it is not
installed).  Nothing of the reference travels as code: the fixture holds data only -- per tag the input ``x`` and what the
function returned, ``want``:
  ntu  (3, 3, 6, 25, 2)  the skeleton the reference pre-normalises (ntu60_prep.py:179 / ntu120_prep.py:219)
  kin  (2, 3, 5, 18, 1)  the reference does NOT pre-normalise Kinetics; this tag only shows that the function is V-agnostic
Values are seeded standard-normal fp32.  The NTU input holds one sample whose second person is all zero, one null frame of
a present second person with non-null frames after it, and one null joint of person 0 -- and no leading or trailing null
frame and no empty sample, so the reference's padding step (which looks ahead and is not reproduced on the device) is a
no-op and the output is a function of frame t and frame 0 only.  The seed is advanced until both latched angles of every
sample lie in [20, 160] degrees (near 0 or pi the reference's fp32 unit vector moves the angle by up to ~3.5e-4 rad) and
|want| <= 8; the angles are computed with the reference's own ``rotation.py``.

usage: python tests/golden/make_golden_prenorm.py --reference DIR [--verify]
``--verify`` regenerates everything and demands arrays bit-identical to the committed fixture.
"""
import argparse
import contextlib
import io
import math
import os
import sys
import types

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g14_prenorm.npz")
SHAPES = {"ntu": (3, 3, 6, 25, 2), "kin": (2, 3, 5, 18, 1)}
BASE_SEED = {"ntu": 1400, "kin": 1450}
ZAXIS, XAXIS = (0, 1), (8, 4)


def joint_input(tag, seed):
    x = np.random.default_rng(seed).standard_normal(SHAPES[tag]).astype(np.float32)
    if tag == "ntu":
        x[1, :, :, :, 1] = 0.0          # sample 1: the second person is absent
        x[0, :, 2, :, 1] = 0.0          # sample 0: one null frame of a present second person, non-null frames after it
        x[2, :, 3, 7, 0] = 0.0          # sample 2: one null joint of the main body
    return x


def _import_reference(reference):
    prep = os.path.join(reference, "datasets", "data_preparation")
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:                # a name only: the function uses it to draw a progress bar
            stub = types.ModuleType("tqdm")
            stub.tqdm = lambda it, *a, **k: it
            sys.modules["tqdm"] = stub
    sys.path.insert(0, prep)
    try:
        import preprocess
        import rotation
    finally:
        sys.path.remove(prep)
    return preprocess, rotation


def _angles(rotation, x):
    """Degrees of the two angles the reference latches per sample, by its own rotation.py on frame 0 of the main body."""
    out = []
    for n in range(x.shape[0]):
        body = x[n, :, 0, :, 0].T.copy()                                        # (V, 3)
        body = (body - body[1:2]) * (body.sum(-1, keepdims=True) != 0)
        dz = body[ZAXIS[1]] - body[ZAXIS[0]]
        az = rotation.angle_between(dz, [0, 0, 1])
        mz = rotation.rotation_matrix(np.cross(dz, [0, 0, 1]), az)
        turned = np.stack([np.dot(mz, j) for j in body]).astype(np.float32)
        ax = rotation.angle_between(turned[XAXIS[0]] - turned[XAXIS[1]], [1, 0, 0])
        out.append((math.degrees(az), math.degrees(ax)))
    return np.array(out)


def generate(reference):
    preprocess, rotation = _import_reference(reference)
    arrays = {}
    for tag in SHAPES:
        for seed in range(BASE_SEED[tag], BASE_SEED[tag] + 50):
            x = joint_input(tag, seed)
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                want = np.ascontiguousarray(preprocess.pre_normalization(x.copy(), zaxis=list(ZAXIS), xaxis=list(XAXIS)))
            ang = _angles(rotation, x)
            if ang.min() >= 20.0 and ang.max() <= 160.0 and np.abs(want).max() <= 8.0:
                break
        else:
            raise RuntimeError(f"{tag}: no admissible seed")
        assert want.dtype == np.float32 and want.shape == x.shape
        arrays[f"{tag}/x"], arrays[f"{tag}/want"] = x, want
        arrays[f"{tag}/seed"] = np.array([seed], dtype=np.int64)
    return arrays


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of LukasHedegaard/continual-skeletons")
    ap.add_argument("--verify", action="store_true")
    args = ap.parse_args()
    arrays = generate(os.path.abspath(args.reference))
    if args.verify:
        stored = np.load(OUT)
        assert sorted(stored.files) == sorted(arrays), (stored.files, sorted(arrays))
        for k, a in arrays.items():
            assert stored[k].dtype == a.dtype and np.array_equal(stored[k].view(np.uint8), a.view(np.uint8)), f"{k} differs"
        print(f"{os.path.basename(OUT)}: {len(arrays)} arrays regenerated by the reference's function, bit-identical")
        return
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
