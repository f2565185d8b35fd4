#!/usr/bin/env python
"""Generate tests/golden/g15_stgcn_mod.npz by running the REFERENCE's own ``StGcnMod`` class (models/st_gcn_mod/st_gcn_mod.py).

The class is imported from the reference checkout under the name-only import stubs of make_golden.py (two more names
that only the "*" model's base-class list mentions are added here) and built without its Ride shell, exactly as make_golden.py
builds ``StGcn`` for G6: closed-form weights with randomised BatchNorm and graph_attn (closed_form.py) and a
closed-form input, so that both sides regenerate them from an index formula.  Two shapes, (N, C, T, V, M) = (1, 3, 88, 25, 2)
(NTU, 60 classes) and (1, 3, 88, 18, 2) (Kinetics, 400 classes): ten unpadded blocks leave 88 - 80 = 8 feature frames.  Stored per
shape under ``<tag>/``: the logits in full, every 97th element of the layer 1, 5, 8 and 10 activations and their absolute maxima,
and what the tests need to rebuild weights and input (key names, shapes, seed, salt).  Nothing of the reference travels as code:
the fixture holds data only.

usage: python tests/golden/make_golden_mod.py --reference DIR [--verify]
``--verify`` regenerates everything and demands arrays bit-identical to the committed fixture.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from closed_form import closed_form_input, closed_form_state_dict  # noqa: E402

OUT = os.path.join(HERE, "g15_stgcn_mod.npz")
T = 88
VARIANTS = {"ntu": (25, 60, 1, 151), "kin": (18, 400, 1, 152)}      # tag: (V, classes, n, seed)
TAPS = (1, 5, 8, 10)
SUB = 97                                                           # the taps are 27 times shorter than G6's: every 97th element


def _ref(reference):
    import make_golden
    make_golden.REF = reference
    make_golden._install_stubs()
    empty = lambda: type("_Stub", (), {})                          # noqa: E731  names of StGcnMod's base-class list only
    sys.modules["ride.optimizers"].SgdOneCycleOptimizer = empty()
    sys.modules["datasets.datasets"].GraphDatasets = empty()
    from datasets import kinetics, ntu_rgbd
    from models.st_gcn_mod.st_gcn_mod import StGcnMod
    return types.SimpleNamespace(A_ntu=ntu_rgbd.graph.A, A_kin=kinetics.graph.A, StGcnMod=StGcnMod)


def _one(R, V, classes, n, seed):
    torch.manual_seed(seed)
    cls = R.StGcnMod
    net = cls.__new__(cls)
    nn.Module.__init__(net)
    net.input_shape = (3, T, V, 2)
    net.num_classes = classes
    net.graph = types.SimpleNamespace(A=R.A_ntu if V == 25 else R.A_kin)
    cls.__init__(net, {})
    net.eval()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    gen = closed_form_state_dict(shapes, salt0=float(seed))
    net.load_state_dict({k: (torch.from_numpy(gen[k]) if k in gen else v) for k, v in net.state_dict().items()})
    x = torch.from_numpy(closed_form_input((n, 3, T, V, 2), salt=15.0 + seed))
    taps = {}
    hooks = [net.layers[f"layer{i}"].register_forward_hook(lambda mod, inp, out, i=i: taps.__setitem__(i, out)) for i in TAPS]
    with torch.no_grad():
        logits = net(x)
    for h in hooks:
        h.remove()
    out = dict(logits=logits.numpy(), n=np.array(n), t=np.array(T), v=np.array(V), salt=np.array(15.0 + seed), seed=np.array(float(seed)),
               nparams=np.array(sum(p.numel() for p in net.parameters())), sd_keys=np.array(list(shapes.keys())),
               sd_shapes=np.array([str(list(v)) for v in shapes.values()]))
    for i, t in taps.items():
        out[f"layer{i}_sub"] = t.numpy().reshape(-1)[::SUB].copy()
        out[f"layer{i}_shape"] = np.array(t.shape)
        out[f"layer{i}_absmax"] = np.array(float(t.abs().max()))
    return out


def generate(reference):
    R = _ref(reference)
    torch.set_num_threads(4)
    arrays = {}
    for tag, (V, classes, n, seed) in VARIANTS.items():
        arrays.update({f"{tag}/{k}": v for k, v in _one(R, V, classes, n, seed).items()})
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--verify", action="store_true")
    args = ap.parse_args()
    arrays = generate(os.path.abspath(args.reference))
    if args.verify:
        d = np.load(OUT)
        same = set(d.files) == set(arrays) and all(np.array_equal(np.asarray(arrays[k]), d[k]) for k in d.files)
        print(f"g15_stgcn_mod regenerates bit-identically: {same}")
        raise SystemExit(0 if same else 1)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
