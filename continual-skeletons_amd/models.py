"""Model drivers around the block library: the callers on either side of the hot path.

``StGcn`` is the counterpart of ``models/st_gcn/st_gcn.py:20-65`` minus the Ride/Lightning shell
(CLI, training, datasets are out of scope): same layer table, same attribute names
(``data_bn``, ``layers.layerK``, ``fc``) and therefore the same ``state_dict`` keys, so published
ST-GCN checkpoints load unchanged.  ``forward`` = input-norm kernel -> 10 fused blocks -> pool+fc kernels.
"""
import torch
import torch.nn as nn

from . import fold, native
from .blocks import SpatioTemporalBlock, _Folded, init_weights
from .input_stage import InputChain
from .keypoints import KeypointIntake
from .modality import InputModality
from .ntu_intake import NtuIntake
from .prenorm import PreNorm


def layer_table(c_in, unpadded=False):
    """(in, out, stride, residual) of the ten blocks (models/st_gcn/st_gcn.py:30-39).  ``unpadded``: the table of the "*"
    models (models/st_gcn_mod/st_gcn_mod.py:28-45) -- the same channels and residuals, stride 1 in every block (the blocks
    then take temporal padding 0: ``MOD_TEMPORAL_PADDING``)."""
    down = 1 if unpadded else 2
    return [
        (c_in, 64, 1, False), (64, 64, 1, True), (64, 64, 1, True), (64, 64, 1, True),
        (64, 128, down, True), (128, 128, 1, True), (128, 128, 1, True),
        (128, 256, down, True), (256, 256, 1, True), (256, 256, 1, True),
    ]


MOD_TEMPORAL_PADDING = 0      # temporal padding of every block of the "*" models; a block then shortens the clip by k - 1 = 8 frames
MOD_MIN_FRAMES = 10 * 8 + 1   # receptive field of the ten unpadded 9-tap blocks: shorter clips leave no output frame
MOD_CONV_RESIDUAL_LAYERS = (5, 8)   # the "*" blocks that change the channel count: 1 x 1 conv + BN residual on the centred shrink


def use_wino_valid_res(net, layers=MOD_CONV_RESIDUAL_LAYERS):
    """Route the conv-residual blocks ``layers`` of a "*" model through csk_tcn_stage_wino_valid_res_f32 (the A-GCN* / S-TR* models
    call it in their constructors; StGcnMod / CoStGcnMod keep the direct kernels there).  Which layers are listed follows the
    measurement in profiles/r17_mod_family.md."""
    for i in layers:
        net.layers[f"layer{i}"].wino_valid_res = True
    return net


def per_layer(factory):
    """A graph-conv factory for all ten layers, or a sequence of ten (None entries: the model's default) -> list of ten."""
    if isinstance(factory, (list, tuple)):
        if len(factory) != 10:
            raise ValueError(f"a per-layer graph-conv list needs 10 entries, got {len(factory)}")
        return list(factory)
    return [factory] * 10


class StGcn(InputChain, _Folded):
    unpadded = False     # StGcnMod: the "*" layer table (stride 1, temporal padding 0, centred residual shrink)
    STAGES = (NtuIntake, KeypointIntake, PreNorm, InputModality)     # the input pre-passes, in order (input_stage.py)

    def __init__(self, graph_A, input_shape=(3, 300, 25, 2), num_classes=60, GraphConv=None):
        """graph_A: (3, V, V) adjacency; input_shape = (C, T, V, M) as datasets/datasets.py:128-134.  ``GraphConv``: the
        graph-conv factory of every block, or a sequence of ten (one per layer; None = GraphConvolution) -- S-TR keeps the
        plain graph conv in layers 1-3 (models/s_tr/s_tr.py:507-518)."""
        super().__init__()
        pad = {"temporal_padding": MOD_TEMPORAL_PADDING} if self.unpadded else {}
        (num_channels, num_frames, num_vertices, num_skeletons) = input_shape
        self.input_shape = tuple(input_shape)
        self._init_stages()
        self.num_classes = num_classes
        convs = per_layer(GraphConv)
        self.data_bn = nn.BatchNorm1d(num_skeletons * num_channels * num_vertices)
        self.layers = nn.ModuleDict({
            f"layer{i + 1}": SpatioTemporalBlock(ci, co, graph_A, stride=s, residual=r, **pad,
                                                 **({} if convs[i] is None else {"GraphConv": convs[i]}))
            for i, (ci, co, s, r) in enumerate(layer_table(num_channels, self.unpadded))
        })
        self.fc = nn.Linear(256, num_classes)
        init_weights(self.data_bn, bs=1)
        init_weights(self.fc, bs=num_classes)

    def _fold(self):
        s, t = fold.fold_data_bn({k: v for k, v in self.state_dict().items() if k.startswith("data_bn.")})
        return dict(scale=s, shift=t)

    def _watched(self):       # only the driver's own folded tensors; blocks keep their own caches
        return [self.data_bn]

    def features(self, x):
        h = self.input_norm(self._prepare_clip(x))      # the pre-passes on channel-first input; all off: x itself
        return self._through_blocks(h, lambda blk, h: blk(h))       # through __call__: hooks and a subclass's forward hold

    def head(self, h, n, m):
        """mean over (T, V), mean over M, fc (models/st_gcn/st_gcn.py:60-64)."""
        nm, c, t, v = h.shape
        feat = torch.empty((n, c), device=h.device, dtype=torch.float32)
        logits = torch.empty((n, self.num_classes), device=h.device, dtype=torch.float32)
        rc = native.lib().csk_pool_fc_f32(native.ptr(h), native.ptr(self.fc.weight.detach()), native.ptr(self.fc.bias.detach()),
                                          native.ptr(feat), native.ptr(logits), n, m, c, t * v, self.num_classes,
                                          native.stream_of(h))
        native.check(rc, "csk_pool_fc_f32")
        return logits

    def forward(self, x):
        self._require_eval()
        x = self._intake_clip(x)        # the intake that is on (input_stage.py); none: x itself
        n, c, t, v, m = x.shape
        return self.head(self.features(x), n, m)

    def set_latency_mode(self, split_k: int = 4, gcn_split_k: int = None, max_sequences: int = None):
        """Small-batch clip inference: split the K loops of every block over workgroups for forwards of at most
        ``max_sequences`` sequences (N * M; default 6), the default kernels above that (blocks.set_clip_latency_mode)."""
        from .blocks import CLIP_SPLIT_MAX_SEQUENCES, set_clip_latency_mode
        return set_clip_latency_mode(self, split_k, gcn_split_k, CLIP_SPLIT_MAX_SEQUENCES if max_sequences is None else max_sequences)


class StGcnMod(StGcn):
    """ST-GCN*: models/st_gcn_mod/st_gcn_mod.py -- the ten blocks with stride 1, temporal padding 0 and the centred residual shrink
    (``layer_table(c, unpadded=True)``); data_bn and the head are StGcn's, and so are the ``state_dict`` keys.  Every block shortens
    the clip by 8 frames: (N, C, T, V, M) -> layer-10 features of T - 80 frames, so T >= 81.  The identity-residual blocks (layers
    2-4, 6-7, 9-10) run the valid form of the Winograd temporal conv (csk_tcn_stage_wino_valid_f32), layers 1, 5 and 8 the direct
    kernels.  The "bf16x3" precision and the clip latency mode are not built for the unpadded blocks: both raise."""

    unpadded = True

    def __init__(self, graph_A, input_shape=(3, 300, 25, 2), num_classes=60, GraphConv=None):
        super().__init__(graph_A, input_shape, num_classes, GraphConv=GraphConv)

    def features(self, x):
        if x.dim() != 5 or x.shape[2] < MOD_MIN_FRAMES:
            raise ValueError(f"{type(self).__name__} needs (N, C, T, V, M) clips of T >= {MOD_MIN_FRAMES} frames (ten unpadded 9-tap blocks, 8 frames "
                             f"each), got {tuple(x.shape)}")
        if any(b.precision != "f32" or b.clip_split_k > 1 for b in self.layers.values()):
            raise NotImplementedError(f"{type(self).__name__} runs the exact fp32 default kernels only (no 'bf16x3' precision, no clip latency mode)")
        return super().features(x)

    def set_latency_mode(self, *args, **kwargs):
        raise NotImplementedError("the clip latency mode is not built for the unpadded '*' blocks; the model is unchanged")
