#!/usr/bin/env python
"""Generate tests/golden/g15_keypoints.npz by running the REFERENCE's own ``Feeder_kinetics.__getitem__``.

``datasets/data_preparation/kinetics400_prep.py:20-138`` is imported from the reference checkout and called, unmodified and
never copied (``tqdm`` is stubbed by name only where it is not installed), on a handful of tiny synthetic OpenPose JSON files
and a label file written into a temporary directory.  Nothing of the reference travels as code: the fixture holds data only
-- per sample ``s<i>``
  s<i>/k     (T_used, 5, 18, 3) fp32   the people of the JSON file, (x, y, score) per joint, absent people all zero
  s<i>/want  (3, T_used, 18, 2) fp32   what the feeder returned, cast to fp32 as ``gendata`` casts it, cropped to the
                                       populated frames (the generator asserts that the other 300 - T_used are all zero)
Coordinates and scores are multiples of 1/1024 in [0, 1], so the JSON text, fp64 and fp32 hold them exactly.  The frames hold
what the intake can get wrong (``PLANS``): 0, 1, 2, 3 and 5 people; the best-scored person in slot 3 or 4; the order of the top
two swapping between consecutive frames; joints with score 0 whose x / y are not 0; a joint with y == 0.5 and a score (the
reference's -0.0); a joint with x == 0.5.  Admissible means: in every frame the score sums of the people with any non-zero
score are pairwise distinct, so that ties occur only among all-zero people, where every order gives the same output; the seed
is advanced until that holds.

usage: python tests/golden/make_golden_keypoints.py --reference DIR [--verify]
``--verify`` regenerates everything and demands arrays bit-identical to the committed fixture.
"""
import argparse
import json
import os
import sys
import tempfile
import types

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g15_keypoints.npz")
P_IN, V, M_OUT = 5, 18, 2
BASE_SEED = 1500
# per sample, per frame: the strength rank of the person in each filled slot (0 = weakest; the slots beyond are empty)
PLANS = [
    [(4, 3, 2, 1, 0), (3, 4, 2, 1, 0), (4, 3, 0, 1, 2), (0, 1, 2, 4, 3), (0, 1, 2, 3, 4), (1, 0, 2)],     # top two swap at 0 -> 1; best in slot 3, 4
    [(1, 0), (0, 1), (0,), (), (2, 0, 1), (1, 0, 2), (0, 3, 1, 4, 2)],                                  # 2, 1, 0, 3, 5 people; swaps
    [(), (0,), (0, 1), (1, 0)],                                                                         # starts with an empty frame
]


def sample_people(plan, seed):
    """(T_used, 5, 18, 3) fp32 for one sample: slot p of frame t holds a person whose joint scores lie in the band of its
    strength rank, with a few joints undetected (score 0, coordinates kept) and the exact-half coordinates."""
    rng = np.random.default_rng(seed)
    k = np.zeros((len(plan), P_IN, V, 3), dtype=np.float64)
    for t, ranks in enumerate(plan):
        for p, rank in enumerate(ranks):
            k[t, p, :, 0] = rng.integers(1, 1025, V) / 1024.0
            k[t, p, :, 1] = rng.integers(1, 1025, V) / 1024.0
            k[t, p, :, 2] = rng.integers(64 + 180 * rank, 64 + 180 * rank + 120, V) / 1024.0
            k[t, p, rng.choice(V, 2, replace=False), 2] = 0.0         # undetected joints whose x / y are not 0
    for t, ranks in enumerate(plan):
        if ranks:
            best = int(np.argmax(ranks))
            k[t, best, 3, 1], k[t, best, 3, 2] = 0.5, 0.25            # y == 0.5 with a score: -(0.5 - 0.5) = -0.0
            k[t, best, 5, 0], k[t, best, 5, 2] = 0.5, 0.375           # x == 0.5: +0.0 with a score
    return k.astype(np.float32)


def admissible(k):
    """Every frame: the fp64 score sums of the people with any non-zero score are pairwise distinct."""
    for frame in k.astype(np.float64):
        sums = [person[:, 2].sum() for person in frame if person[:, 2].any()]
        if len(set(sums)) != len(sums):
            return False
    return True


def _import_reference(reference):
    prep = os.path.join(reference, "datasets", "data_preparation")
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:                # a name only: the module uses it to draw a progress bar
            stub = types.ModuleType("tqdm")
            stub.tqdm = lambda it, *a, **k: it
            sys.modules["tqdm"] = stub
    sys.path.insert(0, prep)
    try:
        import kinetics400_prep
    finally:
        sys.path.remove(prep)
    return kinetics400_prep


def _write_json(path, k, label_index):
    """The people of ``k`` as an OpenPose-style file: per frame the filled slots in order, pose = x0, y0, x1, y1, ..."""
    frames = []
    for t, frame in enumerate(k):
        people = [p for p in range(P_IN) if frame[p].any()]
        assert people == list(range(len(people)))                     # the filled slots are the leading ones
        skeletons = [{"pose": [float(c) for joint in frame[p, :, :2] for c in joint], "score": [float(s) for s in frame[p, :, 2]]}
                     for p in people]
        frames.append({"frame_index": t, "skeleton": skeletons})
    with open(path, "w") as f:
        json.dump({"data": frames, "label": "synthetic", "label_index": label_index}, f)


def generate(reference):
    prep = _import_reference(reference)
    people = []
    for i, plan in enumerate(PLANS):
        for seed in range(BASE_SEED + 100 * i, BASE_SEED + 100 * i + 50):
            k = sample_people(plan, seed)
            if admissible(k):
                break
        else:
            raise RuntimeError(f"sample {i}: no admissible seed")
        people.append((k, seed))
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "kinetics_val")
        os.mkdir(data)
        labels = {}
        for i, (k, _) in enumerate(people):
            _write_json(os.path.join(data, f"s{i}.json"), k, 7 + i)
            labels[f"s{i}"] = {"has_skeleton": True, "label_index": 7 + i}
        label_path = os.path.join(tmp, "kinetics_val_label.json")
        with open(label_path, "w") as f:
            json.dump(labels, f)
        feeder = prep.Feeder_kinetics(data_path=data, label_path=label_path, num_person_in=P_IN, num_person_out=M_OUT)
        assert len(feeder) == len(people)
        for j, name in enumerate(feeder.sample_name):
            i = int(name[1:].split(".")[0])
            k, seed = people[i]
            got, label = feeder[j]
            assert label == 7 + i and got.shape == (3, prep.max_frame, V, M_OUT) and got.dtype == np.float64
            t_used = k.shape[0]
            assert not got[:, t_used:].any(), "the unpopulated frames must be all zero"
            arrays[f"s{i}/k"] = k
            arrays[f"s{i}/want"] = np.ascontiguousarray(got[:, :t_used].astype(np.float32))      # gendata's cast (its fp array is fp32)
            arrays[f"s{i}/seed"] = np.array([seed], dtype=np.int64)
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
        print(f"{os.path.basename(OUT)}: {len(arrays)} arrays regenerated by the reference's feeder, bit-identical")
        return
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
