"""CPU oracle of the unpadded "*" models (test infrastructure): ST-GCN* / CoST-GCN* composed from the block oracles of
oracle/stgcn_oracle.py -- ``st_block(..., temporal_padding=0)`` and ``CoBlockOracle(..., padding=0)`` -- over the layer table of
models/st_gcn_mod/st_gcn_mod.py:28-45 / models/cost_gcn_mod/cost_gcn_mod.py:29-40, and the loader of the fixture
tests/golden/g15_stgcn_mod.npz (the reference's own StGcnMod, tests/golden/make_golden_mod.py)."""
import math
import os

import numpy as np
import torch

from oracle import stgcn_oracle as o

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def mod_layer_table(c_in=3):
    """(in, out, stride, residual): the channels and residuals of ST-GCN, stride 1 in every block."""
    return [(ci, co, 1, res) for (ci, co, _, res) in o.layer_table(c_in)]


def mod_geometry(c_in=3):
    """receptive field / padding / stride of ten 9-tap blocks with padding 0 (the sums of models/base.py:86-97)."""
    r, p, s = 1, 0, 1
    for (_, _, st, _) in mod_layer_table(c_in):
        r, p, s = r + 8 * s, p + 0 * s, s * st
    return r, p, s


def mod_pool_defaults(t=300, c_in=3):
    r, p, s = mod_geometry(c_in)
    size = math.ceil((t - r + 2 * p + 1) / s)
    return size, max(0, size - math.ceil((t - r + p + 1) / s))


def stgcn_mod_features(x, sd, taps=None):
    """(N, C, T, V, M) -> layer-10 activations (N * M, 256, T - 80, V)."""
    h = o.stgcn_pre(x, sd)
    for i, (_, _, stride, res) in enumerate(mod_layer_table(x.shape[1])):
        h = o.st_block(h, sd, f"layers.layer{i + 1}.", stride, res, temporal_padding=0)
        if taps is not None:
            taps[f"layer{i + 1}"] = h
    return h


def stgcn_mod_forward(x, sd, taps=None):
    """StGcnMod.forward (models/st_gcn_mod/st_gcn_mod.py:54-71)."""
    return o.stgcn_head(stgcn_mod_features(x, sd, taps), sd, x.shape[0], x.shape[4])


class CoStGcnModOracle(o.CoStGcnOracle):
    """CoStGcnMod frame by frame: the driver of CoStGcnOracle over ten ``CoBlockOracle(padding=0)`` of stride 1."""

    def __init__(self, sd, c_in=3, pool_size=220, pool_padding=0):
        self.sd = sd
        self.blocks = [o.CoBlockOracle(sd, f"layers.layer{i + 1}.", st, res, padding=0)
                       for i, (_, _, st, res) in enumerate(mod_layer_table(c_in))]
        self.pool_size, self.pool_padding = pool_size, pool_padding
        self.clean_state()


def g15(tag):
    """-> (arrays, regular-layout state dict, input (N, 3, 88, V, 2)) of the fixture's NTU ("ntu") or Kinetics ("kin") model."""
    from closed_form import closed_form_input, closed_form_state_dict

    d = np.load(os.path.join(GOLDEN, "g15_stgcn_mod.npz"))
    a = {k[len(tag) + 1:]: d[k] for k in d.files if k.startswith(tag + "/")}
    v, t = int(a["v"]), int(a["t"])
    shapes = {str(k): tuple(eval(str(s))) for k, s in zip(a["sd_keys"], a["sd_shapes"])}
    gen = closed_form_state_dict(shapes, salt0=float(a["seed"]))
    A = torch.from_numpy((o.ntu_graph() if v == 25 else o.kinetics_graph()).astype(np.float32))
    sd = {k: (A.clone() if k.endswith(".A") else torch.from_numpy(gen[k])) for k in shapes}
    x = torch.from_numpy(closed_form_input((int(a["n"]), 3, t, v, 2), salt=float(a["salt"])))
    return a, sd, x
