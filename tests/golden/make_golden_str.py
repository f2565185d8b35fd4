#!/usr/bin/env python3
"""Generate the S-TR golden vectors (G11, G12) under tests/golden/ by executing the REFERENCE's own classes.

Runs only where the reference project is available (see make_golden.py).  Nothing here travels as code: the outputs
are data (inputs, state_dicts, expected outputs) stored as .npz.  The name-only stubs of make_golden.py are reused, plus
two more that models/s_tr/s_tr.py imports: ``optimizers.SgdMultiStepLR`` and ``datasets.datasets.GraphDatasets`` (names
only, no arithmetic).

  G11  GcnUnitAttention (s_tr.py:271-477) at 32 -> 32 (skip) and 16 -> 32 (no skip), V = 25 and V = 18, T = 6, N = 2,
       closed-form input (g11_input); BN, data_bn, running statistics and conv biases randomised.
  G12  a whole STr (s_tr.py:480-550) built the way make_golden._whole_model builds StGcn: closed-form weights and input,
       NTU shape (V = 25, 60 classes) and Kinetics shape (V = 18, 400 classes), N = 1; logits + layer 1/5/8/10 taps.

usage: python tests/golden/make_golden_str.py [--verify]      (--verify: regenerate and demand bit-identical arrays)
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
from closed_form import closed_form_input  # noqa: E402

OUT = mg.OUT
G11_VARIANTS = {"eq25": (32, 32, 25), "neq25": (16, 32, 25), "eq18": (32, 32, 18), "neq18": (16, 32, 18)}   # (C_in, C_out, V)
G12_VARIANTS = {"ntu": (25, 60, 1, 121), "kin": (18, 400, 1, 122)}                                         # (V, classes, n, seed)
G12_GCN_BN_SCALE = 0.5


def g11_input(ci, v, salt):
    """The G11 input (2, ci, 6, v) in [-1, 1): closed form, so the fixture stores the output only."""
    return torch.from_numpy(closed_form_input((2, ci, 6, v), salt=float(salt)) * 2 - 1)


def _ref():
    if "models.s_tr.s_tr" not in sys.modules:
        if "models.base" not in sys.modules:
            mg._install_stubs()
        m = types.ModuleType("optimizers")
        m.SgdMultiStepLR = type("SgdMultiStepLR", (), {})
        sys.modules["optimizers"] = m
        if "datasets.datasets" not in sys.modules:
            d = types.ModuleType("datasets.datasets")
            d.GraphDatasets = type("GraphDatasets", (), {})
            sys.modules["datasets.datasets"] = d
    from datasets import kinetics, ntu_rgbd
    from models.s_tr.s_tr import GcnUnitAttention, STr
    return types.SimpleNamespace(A_ntu=ntu_rgbd.graph.A, A_kin=kinetics.graph.A, GcnUnitAttention=GcnUnitAttention, STr=STr)


def generate():
    R = _ref()
    torch.set_num_threads(4)
    out = {}
    for j, (tag, (ci, co, v)) in enumerate(G11_VARIANTS.items()):
        g = mg._seeded(1110 + j)
        m = R.GcnUnitAttention(ci, co, R.A_ntu if v == 25 else R.A_kin, num_point=v).eval()
        mg.randomise(m, g)
        x = g11_input(ci, v, 1110 + j)
        with torch.no_grad():
            y = m(x)
        out[f"g11_str_unit_{tag}"] = dict(y=y.numpy(), meta=np.array([ci, co, v, 1110 + j]), **mg.sd_np(m))
    for tag, (v, classes, n, seed) in G12_VARIANTS.items():
        out[f"g12_str_{tag}"] = mg._whole_model(R, R.STr, R.A_ntu if v == 25 else R.A_kin, v, classes, n, seed,
                                                G12_GCN_BN_SCALE)
    return out


def verify():
    bad = []
    for name, arrays in generate().items():
        d = np.load(os.path.join(OUT, name + ".npz"))
        same = set(d.files) == set(arrays) and all(np.array_equal(np.asarray(arrays[k]), d[k]) for k in d.files)
        print(f"  {name:28s} regenerates bit-identically: {same}")
        if not same:
            bad.append(name)
    if bad:
        print("MISMATCH:", bad)
        raise SystemExit(1)
    print("all S-TR fixtures verified against the reference")


def main():
    if "--verify" in sys.argv[1:]:
        return verify()
    for name, arrays in generate().items():
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"wrote {path}: {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
