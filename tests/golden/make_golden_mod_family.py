#!/usr/bin/env python
"""Generate tests/golden/g16_agcn_mod.npz and g17_str_mod.npz by running the REFERENCE's own ``AGcnMod``
(models/a_gcn_mod/a_gcn_mod.py) and ``STrMod`` (models/s_tr_mod/s_tr_mod.py).

As make_golden_mod.py does for ``StGcnMod``: the classes are imported from the reference checkout under the name-only import stubs
of make_golden.py (plus ``optimizers.SgdMultiStepLR``, a name of STrMod's base-class list) and built without their Ride shell,
with closed-form weights and input (closed_form.py), so that both sides regenerate them from an index formula.  Two shapes per
model, (N, C, T, V, M) = (2, 3, 88, 25, 2) (NTU, 60 classes) and (2, 3, 88, 18, 2) (Kinetics, 400 classes): ten unpadded blocks
leave 88 - 80 = 8 feature frames.  Stored per shape under ``<tag>/``: the logits in full, every 97th element of the layer 1, 5, 8
and 10 activations, their shapes and absolute maxima, and what the tests need to rebuild weights and input (key names, shapes,
seed, salt).  Outputs and shape tables only: nothing of the reference travels as code.

usage: python tests/golden/make_golden_mod_family.py --reference DIR [--verify]
``--verify`` regenerates everything and prints the largest absolute difference to the committed fixtures (0.0 is demanded).
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

T, N = 88, 2
# tag: (V, classes, seed, gcn_bn_scale).  A-GCN* multiplies every joint by s_i[v] = 1 + sum_w (A + graph_attn)_i[v, w], about V + 2
# with graph_attn ~ U(.5, 1.5): the graph conv's BN scales down by as much so that activations stay O(1) through ten blocks (as G8)
FIXTURES = {"AGcnMod": ("g16_agcn_mod.npz", {"ntu": (25, 60, 161, 0.04), "kin": (18, 400, 162, 0.055)}),
            "STrMod": ("g17_str_mod.npz", {"ntu": (25, 60, 171, 1.0), "kin": (18, 400, 172, 1.0)})}
TAPS = (1, 5, 8, 10)
SUB = 97


def _ref(reference):
    import make_golden
    make_golden.REF = reference
    make_golden._install_stubs()
    empty = lambda: type("_Stub", (), {})                          # noqa: E731  names of the base-class lists only
    sys.modules["ride.optimizers"].SgdOneCycleOptimizer = empty()
    sys.modules["datasets.datasets"].GraphDatasets = empty()
    opt = types.ModuleType("optimizers")
    opt.SgdMultiStepLR = empty()
    sys.modules["optimizers"] = opt
    from datasets import kinetics, ntu_rgbd
    from models.a_gcn_mod.a_gcn_mod import AGcnMod
    from models.s_tr_mod.s_tr_mod import STrMod
    return types.SimpleNamespace(A_ntu=ntu_rgbd.graph.A, A_kin=kinetics.graph.A, AGcnMod=AGcnMod, STrMod=STrMod)


def _one(R, cls, V, classes, seed, gcn_bn_scale):
    torch.manual_seed(seed)
    net = cls.__new__(cls)
    nn.Module.__init__(net)
    net.input_shape = (3, T, V, 2)
    net.num_classes = classes
    net.graph = types.SimpleNamespace(A=R.A_ntu if V == 25 else R.A_kin)
    cls.__init__(net, {})
    net.eval()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    gen = closed_form_state_dict(shapes, salt0=float(seed), gcn_bn_scale=gcn_bn_scale)
    net.load_state_dict({k: (torch.from_numpy(gen[k]) if k in gen else v) for k, v in net.state_dict().items()})
    x = torch.from_numpy(closed_form_input((N, 3, T, V, 2), salt=15.0 + seed))
    taps = {}
    hooks = [net.layers[f"layer{i}"].register_forward_hook(lambda mod, inp, out, i=i: taps.__setitem__(i, out)) for i in TAPS]
    with torch.no_grad():
        logits = net(x)
    for h in hooks:
        h.remove()
    out = dict(logits=logits.numpy(), n=np.array(N), t=np.array(T), v=np.array(V), salt=np.array(15.0 + seed), seed=np.array(float(seed)),
               nparams=np.array(sum(p.numel() for p in net.parameters())), gcn_bn_scale=np.array(gcn_bn_scale), sd_keys=np.array(list(shapes.keys())),
               sd_shapes=np.array([str(list(v)) for v in shapes.values()]))
    for i, t in taps.items():
        out[f"layer{i}_sub"] = t.numpy().reshape(-1)[::SUB].copy()
        out[f"layer{i}_shape"] = np.array(t.shape)
        out[f"layer{i}_absmax"] = np.array(float(t.abs().max()))
    return out


def generate(reference):
    R = _ref(reference)
    torch.set_num_threads(4)
    files = {}
    for name, (fname, variants) in FIXTURES.items():
        arrays = {}
        for tag, (V, classes, seed, scale) in variants.items():
            arrays.update({f"{tag}/{k}": v for k, v in _one(R, getattr(R, name), V, classes, seed, scale).items()})
        files[fname] = arrays
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--verify", action="store_true")
    args = ap.parse_args()
    files = generate(os.path.abspath(args.reference))
    worst = 0.0
    for fname, arrays in files.items():
        path = os.path.join(HERE, fname)
        if args.verify:
            d = np.load(path)
            if set(d.files) != set(arrays):
                raise SystemExit(f"{fname}: the set of arrays differs")
            for k in d.files:
                a, b = np.asarray(arrays[k]), d[k]
                if a.dtype.kind in "US":
                    worst = max(worst, 0.0 if np.array_equal(a, b) else float("inf"))
                else:
                    worst = max(worst, float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if a.shape == b.shape else float("inf"))
        else:
            np.savez_compressed(path, **arrays)
            print(f"wrote {path}: {os.path.getsize(path) / 1e3:.1f} kB")
    if args.verify:
        print(f"g16_agcn_mod / g17_str_mod regenerate with max |difference| {worst}")
        raise SystemExit(0 if worst == 0.0 else 1)


if __name__ == "__main__":
    main()
