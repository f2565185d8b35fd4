"""CPU oracle of the A-GCN* and S-TR* models (test infrastructure; pure torch, no package code).

``adaptive_graph_conv_mod`` restates AdaptiveGraphConvolutionMod.forward (models/a_gcn_mod/a_gcn_mod.py:48-64) literally -- the
per-frame softmax, both einsums -- and ``folded_graph_conv_mod`` is the form the device runs: the plain graph conv of
oracle/stgcn_oracle.py with the diagonal adjacency diag(s_i), s_i[v] = 1 + sum_w (A + graph_attn)_i[v, w].  The "*" stacks are
composed from oracle/stgcn_oracle.py (``st_block(..., temporal_padding=0)``, ``CoBlockOracle(..., padding=0)``) and the attention
unit of tests/str_oracle.py over the table of tests/mod_oracle.py, as tests/mod_oracle.py composes ST-GCN*.  ``g16`` / ``g17`` load
the fixtures tests/golden/g16_agcn_mod.npz / g17_str_mod.npz (the reference's own AGcnMod / STrMod,
tests/golden/make_golden_mod_family.py)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import stgcn_oracle as o
from tests import mod_oracle as mo
from tests import str_oracle as so

GOLDEN = mo.GOLDEN


def adaptive_graph_conv_mod(x, sd, p=""):
    """AdaptiveGraphConvolutionMod.forward, op for op.  x: (N, C, T, V)."""
    inter_c = sd[p + "a_conv.0.weight"].shape[0]                                        # a_gcn_mod.py:15
    A = sd[p + "A"] + sd[p + "graph_attn"]                                              # a_gcn_mod.py:50
    hidden = None
    for i in range(3):                                                                  # a_gcn_mod.py:52
        A1 = F.conv2d(x, sd[f"{p}a_conv.{i}.weight"], sd[f"{p}a_conv.{i}.bias"]).permute(0, 3, 1, 2).contiguous()   # :53  N V C T
        A2 = F.conv2d(x, sd[f"{p}b_conv.{i}.weight"], sd[f"{p}b_conv.{i}.bias"])        # a_gcn_mod.py:54  N C T V
        A1 = torch.softmax(torch.einsum("nvct,nctw->nvwt", A1, A2) / inter_c, dim=-2)   # a_gcn_mod.py:56-58, nn.Softmax(-2) of :46
        A1 = A1 + A[i].unsqueeze(0).unsqueeze(-1)                                       # a_gcn_mod.py:59
        z = F.conv2d(torch.einsum("nctv,nvwt->nctv", x, A1), sd[f"{p}g_conv.{i}.weight"], sd[f"{p}g_conv.{i}.bias"])   # :60
        hidden = z + hidden if hidden is not None else z                                # a_gcn_mod.py:61
    hidden = o._bn(hidden, sd, p + "bn.")                                               # a_gcn_mod.py:62
    if (p + "gcn_residual.0.weight") in sd:                                             # a_gcn_mod.py:33-41, 63
        r = o._bn(F.conv2d(x, sd[p + "gcn_residual.0.weight"], sd[p + "gcn_residual.0.bias"]), sd, p + "gcn_residual.1.")
    else:
        r = x
    return F.relu(hidden + r)                                                           # a_gcn_mod.py:64


def row_sums(sd, p=""):
    """s_i[v] = 1 + sum_w (A + graph_attn)_i[v, w] in float64, rounded once: (3, V) float32."""
    return (1.0 + (sd[p + "A"].double() + sd[p + "graph_attn"].double()).sum(-1)).float()


def folded_graph_conv_mod(x, sd, p=""):
    """The same module as oracle/stgcn_oracle.py's plain graph conv on the diagonal adjacency diag(s_i): ``graph_conv`` multiplies
    A by graph_attn (models/base.py:262), so it is handed A = diag(s_i) and graph_attn = 1."""
    s = row_sums(sd, p)
    alt = dict(sd)
    alt[p + "A"] = torch.diag_embed(s)
    alt[p + "graph_attn"] = torch.ones_like(alt[p + "A"])
    return o.graph_conv(x, alt, p)


def gcn(x, sd, p=""):
    """The graph conv a block's keys describe: A-GCN*'s, the S-TR attention unit, or GraphConvolution."""
    if (p + "a_conv.0.weight") in sd:
        return adaptive_graph_conv_mod(x, sd, p)
    return so.gcn(x, sd, p)


def mod_features(x, sd, taps=None, gcn=gcn):
    """(N, C, T, V, M) -> layer-10 activations (N * M, 256, T - 80, V) of AGcnMod / STrMod (the keys decide)."""
    h = o.stgcn_pre(x, sd)
    for i, (_, _, stride, res) in enumerate(mo.mod_layer_table(x.shape[1])):
        h = o.st_block(h, sd, f"layers.layer{i + 1}.", stride, res, temporal_padding=0, gcn=gcn)
        if taps is not None:
            taps[f"layer{i + 1}"] = h
    return h


def mod_forward(x, sd, taps=None, gcn=gcn):
    """AGcnMod.forward (a_gcn_mod.py:107-124) / STrMod.forward (models/s_tr_mod/s_tr_mod.py:63-80)."""
    return o.stgcn_head(mod_features(x, sd, taps, gcn), sd, x.shape[0], x.shape[4])


class CoModOracle(o.CoStGcnOracle):
    """CoAGcnMod / CoSTrMod frame by frame: CoStGcnOracle's driver over ten ``CoBlockOracle(padding=0)`` of stride 1 with the
    dispatcher above (models/coa_gcn_mod/coa_gcn_mod.py:31-42, models/cos_tr_mod/cos_tr_mod.py:30-41)."""

    def __init__(self, sd, c_in=3, pool_size=220, pool_padding=0):
        self.sd = sd
        self.blocks = [o.CoBlockOracle(sd, f"layers.layer{i + 1}.", st, res, padding=0, gcn=gcn)
                       for i, (_, _, st, res) in enumerate(mo.mod_layer_table(c_in))]
        self.pool_size, self.pool_padding = pool_size, pool_padding
        self.clean_state()


def _load(name, tag):
    from closed_form import closed_form_input, closed_form_state_dict

    d = np.load(os.path.join(GOLDEN, name))
    a = {k[len(tag) + 1:]: d[k] for k in d.files if k.startswith(tag + "/")}
    v, t = int(a["v"]), int(a["t"])
    shapes = {str(k): tuple(eval(str(s))) for k, s in zip(a["sd_keys"], a["sd_shapes"])}
    gen = closed_form_state_dict(shapes, salt0=float(a["seed"]), gcn_bn_scale=float(a["gcn_bn_scale"]))
    A = torch.from_numpy((o.ntu_graph() if v == 25 else o.kinetics_graph()).astype(np.float32))
    sd = {k: (A.clone() if k.endswith(".A") else torch.from_numpy(gen[k])) for k in shapes}
    x = torch.from_numpy(closed_form_input((int(a["n"]), 3, t, v, 2), salt=float(a["salt"])))
    return a, sd, x


def g16(tag):
    """-> (arrays, regular-layout state dict, input (2, 3, 88, V, 2)) of the AGcnMod fixture, ``tag`` "ntu" or "kin"."""
    return _load("g16_agcn_mod.npz", tag)


def g17(tag):
    """The same of the STrMod fixture."""
    return _load("g17_str_mod.npz", tag)
