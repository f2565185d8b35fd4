#!/usr/bin/env python
"""Generate tests/golden/g18_ntu_intake.npz by running the REFERENCE's own NTU pipeline on tiny synthetic recordings.

Per case, synthetic bodies ``(T, 4, 25, 3)`` fp32 are written to a temporary ``.skeleton`` text file (every value as
``repr(float(v))``, which reads back to the same fp32) and go through the reference's code, imported from the reference checkout,
unmodified and never copied:
  1. ``datasets/data_preparation/ntu60_prep.py:111-128`` ``read_xyz`` parses the file and keeps the two bodies with the largest
     motion energy;
  2. the generator places what it returned at the front of a zero fp32 array of ``FRAMES_OUT`` frames -- what ``gendata``
     (``:169-177``) does with ``max_frame`` = 300, restated here because ``gendata`` walks a dataset directory;
  3. ``preprocess.py:14-93`` ``pre_normalization`` pads the null frames, centres and rotates.  The padded intermediate is the
     array the function hands to ``tqdm`` at the start of its second loop; the generator's stand-in for ``tqdm`` copies it there.
Nothing of the reference travels as code: the fixture holds data only -- per case ``bodies``, ``want_selected`` (after 2),
``want_padded`` (inside 3) and ``want_final`` (what 3 returned), the last three ``(3, FRAMES_OUT, 25, 2)``.

The cases, each the smallest that takes one branch (``CASES`` below): four bodies whose energy order is not slot order; one body;
an exact duplicate pair plus a mirrored copy (x negated: the same energy bit for bit from other data, so the tie rule shows in
the output -- it goes to the HIGHER slot); an empty clip; a main body with leading null frames and a gap (compacted); a null
frame in the middle behind a present frame 0 (kept); a tail that is no multiple of L; L = 1; T = FRAMES_OUT (the one case with
T = 12, the others have T <= 10); two persons with different L; a second person who appears late.

Conditions, asserted here and again by tests/test_ntu_intake_cpu.py: apart from the designed ties any two energies of a clip
differ by at least 1e-6 relative (with the reference's own ``get_nonzero_std``), so no fp64 summation order decides a rank.  A
case's seed is advanced until both angles that ``pre_normalization`` latches lie in [20, 160] degrees (near 0 or pi the
reference's fp32 unit vector moves the angle) and |want_final| <= 8, as in make_golden_prenorm.py.

usage: python tests/golden/make_golden_ntu_intake.py --reference DIR [--verify]
``--verify`` regenerates everything and demands arrays bit-identical to the committed fixture.
"""
import argparse
import contextlib
import io
import math
import os
import sys
import tempfile
import types

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g18_ntu_intake.npz")
P, V, FRAMES_OUT, KEPT = 4, 25, 12, 2
ZAXIS, XAXIS = (0, 1), (8, 4)
MIN_GAP = 1e-6

# name -> (T, {slot: (scale, frames present | "dup:slot" | "mirror:slot")}); a body is offset + scale * standard normal
CASES = {
    "order": (8, {0: (0.6, range(8)), 1: (1.2, range(8)), 2: (0.4, range(8)), 3: (0.9, range(8))}),
    "one": (6, {0: (1.0, range(6))}),
    "tie": (7, {0: (0.3, range(7)), 1: (1.0, range(7)), 2: "dup:1", 3: "mirror:1"}),
    "empty": (5, {}),
    "compact": (10, {0: (0.5, range(10)), 2: (1.1, (2, 3, 5, 6, 7))}),
    "gap": (8, {0: (1.0, (0, 1, 3, 4, 5)), 1: (0.5, range(8))}),
    "tail": (5, {1: (1.0, range(5)), 3: (0.6, range(5))}),
    "one_frame": (4, {1: (1.0, (0,))}),
    "full": (12, {0: (0.7, range(12)), 1: (1.0, range(12))}),
    "two_lengths": (9, {0: (1.0, range(7)), 3: (0.6, range(4))}),
    "late": (8, {0: (1.0, range(8)), 2: (0.5, (5, 6, 7))}),
}
BASE_SEED = 1800


def bodies_of(case, seed):
    t, spec = CASES[case]
    rng = np.random.default_rng(seed)
    b = np.zeros((t, P, V, 3), dtype=np.float32)
    for slot in sorted(spec):
        what = spec[slot]
        if isinstance(what, str):
            kind, src = what.split(":")
            b[:, slot] = b[:, int(src)]
            if kind == "mirror":
                b[:, slot, :, 0] = -b[:, slot, :, 0]
            continue
        scale, present = what
        body = (rng.standard_normal(3) + scale * rng.standard_normal((t, V, 3))).astype(np.float32)
        for f in present:
            b[f, slot] = body[f]
    return b


def write_skeleton_file(path, bodies):
    """The NTU RGB+D text format as read_skeleton_filter parses it: frames, per frame the bodies up to the last tracked slot (an
    untracked slot in front of it as zeros, which is what read_xyz leaves for a missing one), per body 10 fields, per joint 12."""
    lines = [str(bodies.shape[0])]
    for frame in bodies:
        tracked = [p for p in range(frame.shape[0]) if frame[p].any()]
        n = tracked[-1] + 1 if tracked else 0
        lines.append(str(n))
        for p in range(n):
            lines.append(" ".join(["0"] * 9 + ["2"]))
            lines.append(str(frame.shape[1]))
            for joint in frame[p]:
                lines.append(" ".join([repr(float(c)) for c in joint] + ["0"] * 9))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def _import_reference(reference):
    prep = os.path.join(reference, "datasets", "data_preparation")
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:                # a name only: the functions use it to draw a progress bar
            stub = types.ModuleType("tqdm")
            stub.tqdm = lambda it, *a, **k: it
            sys.modules["tqdm"] = stub
    sys.path.insert(0, prep)
    try:
        import ntu60_prep
        import preprocess
        import rotation
    finally:
        sys.path.remove(prep)
    return ntu60_prep, preprocess, rotation


def _angles(rotation, padded):
    """Degrees of the two angles pre_normalization latches, by the reference's own rotation.py on frame 0 of the main body of the
    padded clip (3, T, V, M); None for an empty clip."""
    body = padded[:, 0, :, 0].T.astype(np.float32).copy()                       # (V, 3)
    if not body.any():
        return None
    body = (body - body[1:2]) * (body.sum(-1, keepdims=True) != 0)
    dz = body[ZAXIS[1]] - body[ZAXIS[0]]
    az = rotation.angle_between(dz, [0, 0, 1])
    mz = rotation.rotation_matrix(np.cross(dz, [0, 0, 1]), az)
    turned = np.stack([np.dot(mz, j) for j in body]).astype(np.float32)
    ax = rotation.angle_between(turned[XAXIS[0]] - turned[XAXIS[1]], [1, 0, 0])
    return math.degrees(az), math.degrees(ax)


def _gap(energy):
    e = np.unique(np.asarray(energy, dtype=np.float64))
    return min(((b - a) / b for a, b in zip(e, e[1:])), default=np.inf)


def run_reference(ntu60_prep, preprocess, bodies, tmp):
    """(want_selected, want_padded, want_final, energies) of one recording, by the reference's functions."""
    path = os.path.join(tmp, "S001C001P001R001A001.skeleton")
    write_skeleton_file(path, bodies)
    data = ntu60_prep.read_xyz(path, max_body=P, num_joint=V)                  # (3, T, V, 2) fp64
    fp = np.zeros((1, 3, FRAMES_OUT, V, KEPT), dtype=np.float32)
    fp[0, :, 0:data.shape[1], :, :] = data
    selected = fp[0].copy()
    handed = []

    def tqdm(it, *a, **k):                  # pre_normalization hands its working array (N, M, T, V, C) to tqdm at every loop
        handed.append(np.array(it, copy=True))
        return it

    saved = preprocess.tqdm
    preprocess.tqdm = tqdm
    try:
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            final = np.ascontiguousarray(preprocess.pre_normalization(fp, zaxis=list(ZAXIS), xaxis=list(XAXIS)))
    finally:
        preprocess.tqdm = saved
    assert len(handed) == 4 and np.array_equal(handed[0].transpose(0, 4, 2, 3, 1)[0], selected)
    padded = np.ascontiguousarray(handed[1].transpose(0, 4, 2, 3, 1)[0])       # at the start of the second loop: padded, not centred
    energy = [float(ntu60_prep.get_nonzero_std(bodies[:, p].astype(np.float64))) for p in range(P)]
    return selected, padded, final[0], energy


def generate(reference):
    ntu60_prep, preprocess, rotation = _import_reference(reference)
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, case in enumerate(CASES):
            for seed in range(BASE_SEED + 50 * i, BASE_SEED + 50 * (i + 1)):
                bodies = bodies_of(case, seed)
                selected, padded, final, energy = run_reference(ntu60_prep, preprocess, bodies, tmp)
                assert _gap(energy) >= MIN_GAP, (case, energy)
                ang = _angles(rotation, padded)
                if (ang is None or (min(ang) >= 20.0 and max(ang) <= 160.0)) and np.abs(final).max() <= 8.0:
                    break
            else:
                raise RuntimeError(f"{case}: no admissible seed")
            for name, a in (("bodies", bodies), ("want_selected", selected), ("want_padded", padded), ("want_final", final)):
                assert a.dtype == np.float32 and (name == "bodies" or a.shape == (3, FRAMES_OUT, V, KEPT))
                arrays[f"{case}/{name}"] = a
            arrays[f"{case}/seed"] = np.array([seed], dtype=np.int64)
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
        print(f"{os.path.basename(OUT)}: {len(arrays)} arrays regenerated by the reference's functions, bit-identical")
        return
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
