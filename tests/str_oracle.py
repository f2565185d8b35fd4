"""CPU restatement of the S-TR spatial-attention unit (test infrastructure; pure torch, fp32, no package code).

``str_unit`` is GcnUnitAttention.forward (models/s_tr/s_tr.py:424-477) in the configuration STr / CoSTr build
(only_attention, no relative / adjacency / more_channels, data_normalization, skip_conn, bn_flag; Nh = 8,
dk = C_out / 4, dv = C_out), written op for op in the reference's order.  ``gcn`` dispatches between it and the plain
graph conv of oracle/stgcn_oracle.py by the keys present, so the unchanged ``stgcn_forward`` / ``co_stgcn_steps_pad_end`` /
``CoBlockOracle`` restate STr / CoSTr when handed ``gcn=gcn``.
"""
from typing import Dict

import torch
import torch.nn.functional as F
from torch import Tensor

from oracle import stgcn_oracle as o

NH = 8


def str_unit(x: Tensor, sd: Dict[str, Tensor], p: str = "") -> Tensor:
    """GcnUnitAttention.forward.  x: (N, C_in, T, V) -> (N, C_out, T, V)."""
    n, c, t, v = x.shape
    x_sum = x                                                                        # s_tr.py:430
    xb = x.permute(0, 1, 3, 2).reshape(n, c * v, t)                                  # s_tr.py:432-435 (data_bn)
    xb = F.batch_norm(xb, sd[p + "data_bn.running_mean"], sd[p + "data_bn.running_var"], sd[p + "data_bn.weight"],
                      sd[p + "data_bn.bias"], False, 0.0, o.BN_EPS)
    xb = xb.reshape(n, c, v, t).permute(0, 1, 3, 2)
    xa = xb.permute(0, 2, 1, 3).reshape(-1, c, 1, v)                                 # s_tr.py:440: one frame per row
    qkv = F.conv2d(xa, sd[p + "attention_conv.qkv_conv.weight"], sd[p + "attention_conv.qkv_conv.bias"])   # s_tr.py:200
    dv = sd[p + "attention_conv.attn_out.weight"].shape[0]
    dk = (qkv.shape[1] - dv) // 2
    q, k, vv = torch.split(qkv, [dk, dk, dv], dim=1)                                 # s_tr.py:216
    b = qkv.shape[0]
    q = q.reshape(b, NH, dk // NH, 1, v) * (dk // NH) ** -0.5                        # s_tr.py:217-222 (split_heads_2d)
    k = k.reshape(b, NH, dk // NH, 1, v)
    vv = vv.reshape(b, NH, dv // NH, 1, v)
    fq, fk, fv = q.reshape(b, NH, dk // NH, v), k.reshape(b, NH, dk // NH, v), vv.reshape(b, NH, dv // NH, v)   # s_tr.py:225-227
    logits = torch.matmul(fq.transpose(2, 3), fk)                                    # s_tr.py:148
    weights = F.softmax(logits, dim=-1)                                              # s_tr.py:169
    att = torch.matmul(weights, fv.transpose(2, 3))                                  # s_tr.py:181
    att = att.reshape(b, NH, 1, v, dv // NH).permute(0, 1, 4, 2, 3).reshape(b, dv, 1, v)   # s_tr.py:183-189 (combine_heads_2d)
    att = F.conv2d(att, sd[p + "attention_conv.attn_out.weight"], sd[p + "attention_conv.attn_out.bias"])   # s_tr.py:192
    att = att.reshape(n, t, -1, v).permute(0, 2, 1, 3)                               # s_tr.py:446
    y = att + x_sum if c == dv else att                                              # s_tr.py:467-470
    y = F.batch_norm(y, sd[p + "bn.running_mean"], sd[p + "bn.running_var"], sd[p + "bn.weight"], sd[p + "bn.bias"],
                     False, 0.0, o.BN_EPS)                                           # s_tr.py:471-472
    return F.relu(y)                                                                 # s_tr.py:473


def gcn(x: Tensor, sd: Dict[str, Tensor], p: str = "") -> Tensor:
    """The graph conv a block's keys describe: the attention unit (layers 4-10 of STr / CoSTr) or GraphConvolution."""
    if (p + "attention_conv.qkv_conv.weight") in sd:
        return str_unit(x, sd, p)
    return o.graph_conv(x, sd, p)


def folded_unit(x: Tensor, ops: Dict[str, Tensor]) -> Tensor:
    """The unit recomputed in fp64 from the FOLDED operands of csk_str_unit_f32 (GcnUnitAttention._fold): data_bn as the
    [C_in][V] affine, q scale inside w_qkv, BN inside w_out / b_out, the skip as res_scale * x."""
    n, c, t, v = x.shape
    dk, dv = ops["dk"], ops["dv"]
    xd = x.double()
    xh = xd * ops["s_in"].double().view(1, c, 1, v) + ops["t_in"].double().view(1, c, 1, v)
    rows = 2 * dk + dv
    qkv = torch.einsum("km,nktv->nmtv", ops["w_qkv"].double()[:, :rows], xh) + ops["b_qkv"].double()[:rows].view(1, rows, 1, 1)
    q = qkv[:, :dk].reshape(n, NH, dk // NH, t, v)
    k = qkv[:, dk:2 * dk].reshape(n, NH, dk // NH, t, v)
    vv = qkv[:, 2 * dk:].reshape(n, NH, dv // NH, t, v)
    w = torch.softmax(torch.einsum("nhdti,nhdtj->nhtij", q, k), dim=-1)
    att = torch.einsum("nhtij,nhdtj->nhdti", w, vv).reshape(n, dv, t, v)
    y = torch.einsum("km,nktv->nmtv", ops["w_out"].double()[:, :dv], att) + ops["b_out"].double()[:dv].view(1, dv, 1, 1)
    if ops["res_scale"] is not None:
        y = y + ops["res_scale"].double().view(1, dv, 1, 1) * xd
    return torch.relu(y).float()


class CoSTrOracle:
    """CoSTr stepping (forward_step) as ten CoBlockOracles with the dispatcher, fed by the oracle's input norm; returns
    the layer-10 emission of each step (features before the head).  CoStGcnOracle takes no ``gcn``, hence this."""

    def __init__(self, sd: Dict[str, Tensor], c_in: int = 3):
        self.sd = sd
        self.blocks = [o.CoBlockOracle(sd, f"layers.layer{i + 1}.", s, r, padding=4, gcn=gcn)
                       for i, (_, _, s, r) in enumerate(o.layer_table(c_in))]

    def features_steps(self, x: Tensor, pad_end: bool = True):
        """x: (N, C, T, V, M) -> list of (N*M, 256, V) emissions of layer 10 (block flushes in stack order as pad_end)."""
        h = o.stgcn_pre(x, self.sd)                                                  # (N*M, C, T, V)
        for blk in self.blocks:
            h = blk.forward_steps(h, pad_end=pad_end)
        return h
