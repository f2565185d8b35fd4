"""S-TR / CoS-TR: the spatial-attention graph unit and the two model drivers around it.

Counterpart of ``GcnUnitAttention`` (models/s_tr/s_tr.py:271-477), ``STr`` (s_tr.py:480-550) and ``CoSTr``
(models/cos_tr/cos_tr.py) in the configuration those models build: ``only_attention=True, relative=False,
adjacency=False, more_channels=False, data_normalization=True, skip_conn=True, bn_flag=True, kernel_size=1, stride=1,
Nh=8, dk_factor=0.25``, ``dv = out_channels`` -- any other value of these flags raises ``NotImplementedError`` at
construction.  Inference only (``drop_connect`` acts in training alone).

Per frame the unit computes multi-head self-attention over the V joints (s_tr.py:424-477, 134-230):
    y = ReLU(BN(attn_out(attention(qkv_conv(data_bn(x)))) + x))        (+ x only when C_in == C_out)
Three HIP launches (csrc/str.hip, ``csk_str_unit_f32``): data_bn + QKV GEMM, attention, output projection + epilogue.
data_bn (a per-(c, v) affine, not foldable into the conv) is applied while x is staged, ``dkh^-0.5`` is folded into the q
rows, the unit's BN into the output projection, and the skip becomes ``s_c * x`` in the epilogue.  Both GEMMs are exact
fp32 MFMA; ``set_precision(net, "bf16x3")`` does not touch the unit (it acts on the temporal convs only).

The same module serves the clip path (``forward``) and the continual rings (``stage``), so a ``CoSTr`` stack never reaches
``CoSpatioTemporalBlock._foreign_gcn_stage``.  It has no ``plan_operands``: ``CoSTr`` runs the Python step engine
(``CoStGcn._build_plan`` leaves such stacks to it).
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import fold, native
from .blocks import _check_input, _Folded
from .continual import CoStGcn, CoStGcnMod
from .models import StGcn, StGcnMod, use_wino_valid_res

NH = 8


def conv_init(module):
    """he_normal of the reference (s_tr.py:264-269); used there only by the ``only_attention=False`` form."""
    n = module.out_channels
    for k in module.kernel_size:
        n = n * k
    module.weight.data.normal_(0, math.sqrt(2.0 / n))


class SpatialAttention(nn.Module):
    """Parameter container of s_tr.py:19-131 in the built configuration: ``qkv_conv`` (C_in -> 2 dk + dv) and
    ``attn_out`` (dv -> dv), both 1x1.  Never called: the unit's kernels read its weights."""

    def __init__(self, in_channels, dk, dv, Nh=NH):
        super().__init__()
        assert dk % Nh == 0 and dv % Nh == 0, "dk and dv must be divisible by Nh (s_tr.py:75-80)"
        self.in_channels, self.dk, self.dv, self.Nh = in_channels, dk, dv, Nh
        self.qkv_conv = nn.Conv2d(in_channels, 2 * dk + dv, kernel_size=1, stride=1, padding=0)
        self.attn_out = nn.Conv2d(dv, dv, kernel_size=1, stride=1)


_BUILT = dict(only_attention=True, relative=False, adjacency=False, more_channels=False, data_normalization=True,
              skip_conn=True, bn_flag=True, kernel_size=1, stride=1, Nh=NH, dk_factor=0.25)


class GcnUnitAttention(_Folded):
    """models/s_tr/s_tr.py:271-477 (same constructor, keyword names, parameters, buffers and state_dict keys:
    ``A``, ``data_bn.*``, ``bn.*``, ``attention_conv.qkv_conv.*``, ``attention_conv.attn_out.*``)."""

    def __init__(self, in_channels, out_channels, A, num=4, dv_factor=0.25, dk_factor=0.25, Nh=8, complete=True,
                 relative=False, only_attention=True, layer=0, more_channels=False, drop_connect=True,
                 data_normalization=True, skip_conn=True, adjacency=False, num_point=25, padding=0, kernel_size=1, stride=1,
                 bn_flag=True, t_dilation=1, last_graph=False, visualization=True, *args, **kwargs):
        super().__init__()
        given = dict(only_attention=only_attention, relative=relative, adjacency=adjacency, more_channels=more_channels,
                     data_normalization=data_normalization, skip_conn=skip_conn, bn_flag=bn_flag, kernel_size=kernel_size,
                     stride=stride, Nh=Nh, dk_factor=dk_factor)
        off = {k: v for k, v in given.items() if v != _BUILT[k]}
        if off:
            raise NotImplementedError(
                f"GcnUnitAttention is built for the configuration STr / CoSTr use ({_BUILT}); got {off}")
        self.relu = nn.ReLU()
        self.visualization = visualization
        self.in_channels = in_channels
        self.more_channels = more_channels
        self.drop_connect = drop_connect
        self.data_normalization = data_normalization
        self.skip_conn = skip_conn
        self.num_point = num_point
        self.adjacency = adjacency
        self.last_graph = last_graph
        self.out_channels = out_channels
        self.num = num
        self.data_bn = nn.BatchNorm1d(self.in_channels * self.num_point)
        self.bn = nn.BatchNorm2d(out_channels)
        self.only_attention = only_attention
        self.bn_flag = bn_flag
        self.layer = layer
        self.A = nn.Parameter(torch.from_numpy(np.asarray(A).astype(np.float32)))   # never read in this configuration
        self.attention_conv = SpatialAttention(in_channels, int(out_channels * dk_factor), int(out_channels), Nh)

    @property
    def has_skip(self) -> bool:
        return self.skip_conn and self.in_channels == self.out_channels          # s_tr.py:467-470

    def _fold(self):
        """Packed operands of csk_str_unit_f32 (include/cskel.h), folded in float64 and rounded once."""
        sd = {k: v.detach().cpu() for k, v in self.state_dict().items()}
        att = self.attention_conv
        dk, dv = att.dk, att.dv
        s_in, t_in = fold.bn_affine(sd["data_bn.weight"], sd["data_bn.bias"], sd["data_bn.running_mean"],
                                    sd["data_bn.running_var"], self.data_bn.eps)
        qscale = torch.ones(2 * dk + dv, dtype=torch.float64)
        qscale[:dk] = float(dk // att.Nh) ** -0.5                                  # s_tr.py:222
        w_qkv = fold.pack_conv_weight(sd["attention_conv.qkv_conv.weight"], qscale)[0]
        b_qkv = torch.zeros(w_qkv.shape[1], dtype=torch.float64)
        b_qkv[: 2 * dk + dv] = sd["attention_conv.qkv_conv.bias"].double() * qscale
        sc, sh = fold.bn_affine(sd["bn.weight"], sd["bn.bias"], sd["bn.running_mean"], sd["bn.running_var"], self.bn.eps)
        w_out = fold.pack_conv_weight(sd["attention_conv.attn_out.weight"], sc)[0]
        b_out = torch.zeros(w_out.shape[1], dtype=torch.float64)
        b_out[:dv] = sd["attention_conv.attn_out.bias"].double() * sc + sh
        return dict(w_qkv=w_qkv.contiguous(), b_qkv=b_qkv.float().contiguous(),
                    s_in=s_in.float().contiguous(), t_in=t_in.float().contiguous(),
                    w_out=w_out.contiguous(), b_out=b_out.float().contiguous(),
                    res_scale=sc.float().contiguous() if self.has_skip else None,
                    c_in=self.in_channels, c_out=self.out_channels, V=self.num_point, dk=dk, dv=dv)

    def scratch_floats(self, n_seg: int, frames: int) -> int:
        """qkv + attention-output images of one launch (csk_str_unit_f32 ``scratch``)."""
        att = self.attention_conv
        return n_seg * (2 * att.dk + 2 * att.dv) * frames * self.num_point

    def forward(self, x):
        """(N, C_in, T, V) -> (N, C_out, T, V): every frame attends over its own joints (s_tr.py:424-477)."""
        self._require_eval()
        _check_input(x, self.in_channels, "GcnUnitAttention input")
        n, c, t, v = x.shape
        if v != self.num_point:
            raise RuntimeError(f"input has V={v} joints, the unit was built for num_point={self.num_point}")
        y = torch.empty((n, self.out_channels, t, v), device=x.device, dtype=torch.float32)
        self.stage(x, y, n_seg=n, frames=t, x_strides=(c * t * v, t * v), y_strides=(self.out_channels * t * v, t * v))
        return y

    def stage(self, x, y, n_seg, frames, x_strides, y_strides):
        """Launch on explicit views / strides: element (seg, c, f, v) at seg * seg_stride + c * chan_stride + f * V + v (the
        clip layout, or the continual engine's channel-major ring slots with frames = skeletons)."""
        ops = self._packed_ops(x.device)
        floats = self.scratch_floats(n_seg, frames)
        scratch = torch.empty((max(floats, 1),), device=x.device, dtype=torch.float32)
        rc = native.lib().csk_str_unit_f32(
            native.ptr(x), native.ptr(y), native.ptr(scratch), floats, native.ptr(ops["w_qkv"]), native.ptr(ops["b_qkv"]),
            native.ptr(ops["s_in"]), native.ptr(ops["t_in"]), native.ptr(ops["w_out"]), native.ptr(ops["b_out"]),
            native.ptr(ops["res_scale"]), n_seg, ops["c_in"], ops["c_out"], frames, ops["V"], x_strides[0], x_strides[1],
            y_strides[0], y_strides[1], native.stream_of(x))
        native.check(rc, "csk_str_unit_f32")


ATTENTION_LAYERS = range(3, 10)      # layers 4-10 (s_tr.py:507-518; cos_tr.py:31-41); layers 1-3 keep GraphConvolution


class STr(StGcn):
    """models/s_tr/s_tr.py:480-550 without the Ride shell: StGcn's layer table and head, ``GcnUnitAttention`` as the graph
    conv of layers 4-10.  Same state_dict keys as the reference."""

    def __init__(self, graph_A, input_shape=(3, 300, 25, 2), num_classes=60):
        v = input_shape[2]

        def graph_conv(in_channels, out_channels, A):
            return GcnUnitAttention(in_channels, out_channels, A, num_point=v)

        super().__init__(graph_A, input_shape, num_classes,
                         GraphConv=[graph_conv if i in ATTENTION_LAYERS else None for i in range(10)])


class CoSTr(CoStGcn):
    """models/cos_tr/cos_tr.py without the Ride shell: CoStGcn with ``GcnUnitAttention`` in layers 4-10.  The reference's
    factory passes ``bn_momentum`` positionally, i.e. as ``num`` (cos_tr.py:25-28); that is reproduced (no shape depends
    on it).  State-dict keys, ``map_state_dict`` and ``map_loaded_weights`` are CoStGcn's (cos_tr.py:50-85 is the same
    key map).  Steps run on the Python engine (no native plan for attention stacks)."""

    def __init__(self, graph_A, input_shape=(3, 300, 25, 2), num_classes=60, pool_size=-1, pool_padding=-1):
        v = input_shape[2]

        def co_graph_conv(in_channels, out_channels, A, bn_momentum=0.1):
            return GcnUnitAttention(in_channels, out_channels, A, bn_momentum, num_point=v)

        super().__init__(graph_A, input_shape, num_classes, pool_size, pool_padding,
                         CoGraphConv=[co_graph_conv if i in ATTENTION_LAYERS else None for i in range(10)])


class STrMod(StGcnMod):
    """S-TR*: models/s_tr_mod/s_tr_mod.py -- StGcnMod's table, geometry and refusals with ``GcnUnitAttention`` in layers 4-10.
    Layers 5 and 8 run the valid Winograd form with the conv residual (csk_tcn_stage_wino_valid_res_f32)."""

    def __init__(self, graph_A, input_shape=(3, 300, 25, 2), num_classes=60):
        v = input_shape[2]

        def graph_conv(in_channels, out_channels, A):
            return GcnUnitAttention(in_channels, out_channels, A, num_point=v)

        super().__init__(graph_A, input_shape, num_classes,
                         GraphConv=[graph_conv if i in ATTENTION_LAYERS else None for i in range(10)])
        use_wino_valid_res(self)


class CoSTrMod(CoStGcnMod):
    """CoS-TR*: models/cos_tr_mod/cos_tr_mod.py -- CoStGcnMod with ``GcnUnitAttention`` in layers 4-10 (``bn_momentum`` lands in
    ``num`` as in CoSTr).  The ``window_size`` arguments of the reference's blocks -- halved in layers 6-10 although the stride is
    1 -- are metadata no computation reads, and are not reproduced.  Steps run on the Python engine, as CoSTr's."""

    def __init__(self, graph_A, input_shape=(3, 300, 25, 2), num_classes=60, pool_size=-1, pool_padding=-1):
        v = input_shape[2]

        def co_graph_conv(in_channels, out_channels, A, bn_momentum=0.1):
            return GcnUnitAttention(in_channels, out_channels, A, bn_momentum, num_point=v)

        super().__init__(graph_A, input_shape, num_classes, pool_size, pool_padding,
                         CoGraphConv=[co_graph_conv if i in ATTENTION_LAYERS else None for i in range(10)])
        use_wino_valid_res(self)
