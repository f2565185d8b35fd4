#!/usr/bin/env python
"""Generate tests/golden/g13_modalities.npz by running the REFERENCE's own data-preparation scripts.

``datasets/data_preparation/bone_data_prep.py`` and ``motion_data_prep.py`` are plain scripts: they read
``./data/<dataset>/{train,val}_data_joint.npy`` for five datasets, and write the bone, joint-motion and bone-motion files
next to them.  This generator writes tiny synthetic joint files (N = 2, C = 3, T = 6, M = 2; V = 25 for the four NTU sets,
18 for Kinetics) into a temporary directory and executes the two scripts themselves, unmodified and never copied, with
that directory as the working directory (``tqdm`` is stubbed by name only where it is not installed).  Nothing of the
reference travels as code: the fixture holds data only -- for one NTU set and for Kinetics, the input and the three
files the scripts wrote, and the parent tables read from the bone script's ``paris`` table (the four NTU entries are
checked to be identical and to give identical results for identical input).

usage: python tests/golden/make_golden_modalities.py --reference DIR [--verify]
``--verify`` regenerates everything and demands arrays bit-identical to the committed fixture.
"""
import argparse
import contextlib
import io
import os
import runpy
import sys
import tempfile
import types

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g13_modalities.npz")
NTU_SETS = ("ntu60/xview", "ntu60/xsub", "ntu120/xset", "ntu120/xsub")
DATASETS = NTU_SETS + ("kinetics",)
N, C, T, M = 2, 3, 6, 2
STORED = {"ntu": ("ntu60/xsub", "val"), "kinetics": ("kinetics", "val")}       # fixture tag -> (dataset, set) kept in the file


def joint_input(dataset, part):
    """Synthetic joint file of a dataset: every NTU set gets the SAME values (so that their results can be compared),
    train and val differ.  O(1) normal values with full mantissas: every subtraction rounds."""
    v = 18 if dataset == "kinetics" else 25
    seed = (1 if dataset == "kinetics" else 0) * 2 + (part == "val")
    return np.random.default_rng(1300 + seed).standard_normal((N, C, T, v, M)).astype(np.float32)


def generate(reference):
    scripts = os.path.join(reference, "datasets", "data_preparation")
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:                # a name only: the scripts use it to draw a progress bar
            stub = types.ModuleType("tqdm")
            stub.tqdm = lambda it, *a, **k: it
            sys.modules["tqdm"] = stub
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        for dataset in DATASETS:
            os.makedirs(os.path.join(tmp, "data", dataset))
            for part in ("train", "val"):
                np.save(os.path.join(tmp, "data", dataset, f"{part}_data_joint.npy"), joint_input(dataset, part))
        os.chdir(tmp)
        try:
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                bone_globals = runpy.run_path(os.path.join(scripts, "bone_data_prep.py"), run_name="__main__")
                runpy.run_path(os.path.join(scripts, "motion_data_prep.py"), run_name="__main__")
        finally:
            os.chdir(here)

        def load(dataset, part, kind):
            return np.array(np.load(os.path.join(tmp, "data", dataset, f"{part}_data_{kind}.npy")))

        paris = bone_globals["paris"]
        assert all(paris[d] == paris[NTU_SETS[0]] for d in NTU_SETS), "the reference's NTU bone tables differ"
        for d in NTU_SETS[1:]:
            for part in ("train", "val"):
                for kind in ("bone", "joint_motion", "bone_motion"):
                    assert np.array_equal(load(d, part, kind), load(NTU_SETS[0], part, kind)), (d, part, kind)
        arrays = {}
        for tag, (dataset, part) in STORED.items():
            base = 0 if dataset == "kinetics" else 1           # bone_data_prep.py:160-162: the NTU pairs are 1-based
            v = 18 if dataset == "kinetics" else 25
            parents = np.full((v,), -1, dtype=np.int32)
            for v1, v2 in paris[dataset]:
                assert parents[v1 - base] == -1, f"joint {v1} listed twice"
                parents[v1 - base] = v2 - base
            assert (parents >= 0).all()
            arrays[f"{tag}/parents"] = parents
            arrays[f"{tag}/joint"] = joint_input(dataset, part)
            assert np.array_equal(load(dataset, part, "joint"), arrays[f"{tag}/joint"])
            for kind in ("bone", "joint_motion", "bone_motion"):
                arrays[f"{tag}/{kind}"] = load(dataset, part, kind)
                assert arrays[f"{tag}/{kind}"].dtype == np.float32 and arrays[f"{tag}/{kind}"].shape == arrays[f"{tag}/joint"].shape
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
        print(f"{os.path.basename(OUT)}: {len(arrays)} arrays regenerated by the reference's scripts, bit-identical")
        return
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
