"""A-GCN adaptive graph convolution and the (Co)AGCN model drivers (BASELINE.json configs[3]).

Counterpart of ``AdaptiveGraphConvolution`` (models/a_gcn/a_gcn.py:12-69), ``AGcn`` (a_gcn.py:72-145) and
``CoAGcn`` (models/coa_gcn/coa_gcn.py).  The graph conv aggregates with a PER-SAMPLE dense adjacency
    adj_i = softmax_{dim=-2}( a_i(x)^T b_i(x) / (inter*T) ) + (A + graph_attn)_i        (a_gcn.py:50-63)
``AdaptiveGraphConvolution._adjacency`` forms the dense column-wise adjacency values and owns the choice between its two routes:
the two-launch one -- the six 1x1 embedding convs as ONE ``csk_conv1x1_f32``, then ``csk_agcn_attention_f32`` -- and the fused
``csk_agcn_embed_attention_f32`` (embedding convs and logits in one launch) at the shapes it is built for.  ``_graph_conv`` applies
them: the general GCN stage kernel with ``adj_seg_stride`` (aggregation on VALU from LDS-staged tables, channel mixing on MFMA).
Three callers state a geometry each.  ``forward``, clip mode: one V x V matrix per sample over all T.  ``stage``, continual mode
(CoAGCN): T = 1, i.e. per-frame attention -- clip != step by design (a_gcn.py:60-61, coa_gcn.py:31).  ``forward_framewise``: a
whole clip at the steps' arithmetic, one matrix per (sample, frame) -- the frame-wise kernel ``csk_agcn_stage_framewise_f32``
(adjacencies never reach memory) where it is built and measured faster, else the per-frame launches on chunks of frames.
"""
import torch
import torch.nn as nn

from . import blocks, fold, native
from .blocks import GraphConvolution, _check_input, init_weights
from .continual import CoStGcn, CoStGcnMod
from .models import StGcn, StGcnMod, use_wino_valid_res


class AdaptiveGraphConvolution(GraphConvolution):
    def __init__(self, in_channels, out_channels, A, bn_momentum=0.1, coff_embedding=4):
        super().__init__(in_channels, out_channels, A, bn_momentum)
        self.inter_c = out_channels // coff_embedding
        self.a_conv = nn.ModuleList(nn.Conv2d(in_channels, self.inter_c, 1) for _ in range(self.num_subset))
        self.b_conv = nn.ModuleList(nn.Conv2d(in_channels, self.inter_c, 1) for _ in range(self.num_subset))
        for m in list(self.a_conv) + list(self.b_conv):
            init_weights(m)
        self.soft = nn.Softmax(-2)

    def _fold(self):
        sd = {k: v.detach().cpu() for k, v in self.state_dict().items()}
        f = fold.fold_graph_conv(sd)                      # weights / bias as for GraphConvolution ...
        v = f["V"]
        # ... but the adjacency is dense and per sample: index pattern 0..V-1 for every column
        f["ell_src"] = torch.arange(v, dtype=torch.int32).repeat(3, v, 1).contiguous()
        f["ell_cnt_host"] = torch.tensor([v, v, v], dtype=torch.int32)
        f["ell_w"] = v
        f["ell_val"] = None
        f["a_sum"] = (sd["A"].double() + sd["graph_attn"].double()).float().contiguous()      # a_gcn.py:50
        inter, ci = self.inter_c, self.in_channels
        we = torch.cat([sd[f"a_conv.{i}.weight"] for i in range(3)] + [sd[f"b_conv.{i}.weight"] for i in range(3)], 0)
        be = torch.cat([sd[f"a_conv.{i}.bias"] for i in range(3)] + [sd[f"b_conv.{i}.bias"] for i in range(3)], 0)
        f["w_embed"] = fold.pack_conv_weight(we.view(6 * inter, ci, 1, 1), torch.ones(6 * inter, dtype=torch.float64))
        f["b_embed"] = fold.pad_vec(be.double())
        # pair-major row order (a_i rows, then b_i rows, i = 0, 1, 2) for the fused step kernel
        order = [r for i in range(3) for r in list(range(i * inter, (i + 1) * inter)) + list(range((3 + i) * inter, (4 + i) * inter))]
        f["w_embed_pairs"] = fold.pack_conv_weight(we[order].view(6 * inter, ci, 1, 1), torch.ones(6 * inter, dtype=torch.float64))
        f["b_embed_pairs"] = fold.pad_vec(be[order].double())
        return f

    def _attention(self, E, ops, n_seg, T, V, e_seg_stride, e_chan_stride, seg_per_group=None, e_group_stride=0):
        adj = torch.empty((n_seg, 3, V, V), device=E.device, dtype=torch.float32)
        scratch = torch.empty((n_seg, 3, 4, V, V), device=E.device, dtype=torch.float32) if T > 1 else None
        rc = native.lib().csk_agcn_attention_f32(native.ptr(E), native.ptr(ops["a_sum"]), native.ptr(adj), native.ptr(scratch), n_seg,
                                                 self.inter_c, T, V, e_seg_stride, e_chan_stride,
                                                 seg_per_group or n_seg, e_group_stride, native.stream_of(E))
        native.check(rc, "csk_agcn_attention_f32")
        return adj

    def _adjacency(self, x, ops, n_seg, frames, x_strides, per_frame, fuse=True, row=None):
        """The dense adjacencies of ``n_seg`` segments of ``frames`` frames of ``x`` (segment and channel stride ``x_strides``):
        one (3, V, V) per segment over all its frames -- the clip form -- or with ``per_frame`` one per (segment, frame),
        segment-major.  THE place that picks the launches: csk_agcn_embed_attention_f32 (embedding convs + logits in one launch)
        where ``fuse``, the caller's own gate, and ``_fused_ok`` allow it, else the embeddings E through csk_conv1x1_f32 (the six
        1x1 convs as one) and csk_agcn_attention_f32.  ``row``: floats of a segment's embedding row in E (default frames * V;
        ``stage``: the padded row of its rings)."""
        v, c, e_ch = ops["V"], self.in_channels, 6 * self.inter_c
        n_adj = n_seg * frames if per_frame else n_seg
        if fuse and self._fused_ok(v, x.data_ptr(), *x_strides):
            adj = torch.empty((n_adj, 3, v, v), device=x.device, dtype=torch.float32)
            ft = 128 // v                              # frames per tile of the kernel: the clip form sums a partial logit of each
            scratch = None if per_frame else torch.empty((n_seg, 3, (frames + ft - 1) // ft, v, v), device=x.device, dtype=torch.float32)
            rc = native.lib().csk_agcn_embed_attention_f32(
                native.ptr(x), native.ptr(ops["w_embed_pairs"]), native.ptr(ops["b_embed_pairs"]), native.ptr(ops["a_sum"]),
                native.ptr(adj), native.ptr(scratch), n_seg, c, self.inter_c, frames, v, int(per_frame), x_strides[0], x_strides[1],
                native.stream_of(x))
            native.check(rc, "csk_agcn_embed_attention_f32")
            return adj
        row = frames * v if row is None else row
        if per_frame:
            E = torch.empty((n_seg, e_ch, row), device=x.device, dtype=torch.float32)
        else:       # (N, 6*inter, T, V), + 4 floats of slack behind it (the clip form of csk_agcn_attention_f32 reads whole 16-byte vectors)
            E = torch.empty((n_seg * e_ch * row + 4,), device=x.device, dtype=torch.float32)[: n_seg * e_ch * row].view(n_seg, e_ch, frames, v)
        rc = native.lib().csk_conv1x1_f32(native.ptr(x), native.ptr(E), native.ptr(ops["w_embed"]), native.ptr(ops["b_embed"]), n_seg, c,
                                          e_ch, frames, v, x_strides[0], x_strides[1], e_ch * row, row, native.stream_of(x))
        native.check(rc, "csk_conv1x1_f32")
        if per_frame:   # every (segment, frame) its own "sample" of T = 1: V floats apart in a row, a segment's rows e_ch * row apart
            return self._attention(E, ops, n_adj, 1, v, v, row, seg_per_group=frames, e_group_stride=e_ch * row)
        return self._attention(E, ops, n_seg, frames, v, e_ch * row, row)

    @staticmethod
    def _graph_conv(x, y, ops, adj, n_seg, frames, x_strides, y_strides, per_frame):
        """The general GCN stage kernel on ``x`` into ``y`` with the adjacencies ``adj`` of ``_adjacency`` as the ELL values."""
        blocks.gcn_stage(x, y, dict(ops, ell_val=adj), n_seg=n_seg, frames=frames, x_strides=x_strides, y_strides=y_strides,
                         adj_seg_stride=3 * ops["V"] * ops["V"], adj_per_frame=int(per_frame))

    def forward(self, x):
        self._require_eval()
        _check_input(x, self.in_channels, "AdaptiveGraphConvolution input")
        ops = self._packed_ops(x.device)
        n, c, t, v = x.shape
        xs, ys = (c * t * v, t * v), (self.out_channels * t * v, t * v)
        y = torch.empty((n, self.out_channels, t, v), device=x.device, dtype=torch.float32)
        # (V = 25: the fused clip form measured SLOWER than GEMM + logits kernels -- 28.0 vs 24.2 ms per NTU batch-64 forward: five
        # frames per tile, joints staged one by one -- so it is used at V = 18 only; the step form gains 4 % at V = 25 too)
        adj = self._adjacency(x, ops, n, t, xs, per_frame=False, fuse=v == 18)
        self._graph_conv(x, y, ops, adj, n, t, xs, ys, per_frame=False)
        return y

    fuse_embed_attention = True     # False: two launches (csk_conv1x1_f32 + csk_agcn_attention_f32) -- for A/B measurements
    fuse_framewise = True           # False: forward_framewise composes the per-frame launches -- for A/B measurements
    # False: the frame-wise kernel only at the shapes where it measured faster than the composed launches
    # (profiles/r23_agcn_framewise.md: V = 18 at inter 16; V = 25 at layer 1 and at inter 32 with the conv residual; the composed
    # launches are 2-30 % faster at the others); True: wherever it is built -- for tests and A/B measurements
    framewise_everywhere = False
    # Bytes of per-frame adjacencies (3 V V floats per skeleton frame; + the embeddings on the two-launch route) the composed form
    # of forward_framewise may hold at a time: the clip is taken in chunks of frames that stay below it (at least one frame)
    framewise_budget_bytes = 256 << 20

    def framewise_route(self, x):
        """The instantiation of csk_agcn_stage_framewise_f32 ``forward_framewise(x)`` launches (INTER * 1000 + V * 10 + CONVRES), or
        0 where it composes the per-frame launches.  Host arithmetic only."""
        if not self.fuse_framewise:
            return 0
        ops = self._packed_ops(x.device)
        n, c, t, v = x.shape
        rc = native.lib().csk_agcn_stage_framewise_f32_route(native.ptr(x), n, c, self.out_channels, self.inter_c, t, v, c * t * v, t * v,
                                                             ops["res_mode"])
        native.check(min(rc, 0), "csk_agcn_stage_framewise_f32_route")
        if rc and not self.framewise_everywhere:
            conv = ops["res_mode"] == 2
            faster = self.inter_c == 16 if v == 18 else ((self.inter_c == 16 and c <= 4) or (self.inter_c == 32 and conv))
            return rc if faster else 0
        return rc

    def forward_framewise(self, x):
        """(NM, C, T, V) -> (NM, C_out, T, V) with the attention formed per (skeleton, frame): for every frame what ``stage``
        computes for it on a step (models/coa_gcn/coa_gcn.py:11-14), on a whole clip.  One launch of csk_agcn_stage_framewise_f32
        where it is built (V in {18, 25}, inter in {16, 32, 64}) and measured faster (``framewise_everywhere``): the per-frame
        adjacencies never reach memory.  Elsewhere the
        per-frame launches of ``stage`` on chunks of frames whose adjacencies stay below ``framewise_budget_bytes``; a frame's
        result does not depend on the chunking (every kernel involved forms a frame from that frame alone)."""
        self._require_eval()
        _check_input(x, self.in_channels, "AdaptiveGraphConvolution input")
        x = x.contiguous()
        ops = self._packed_ops(x.device)
        n, c, t, v = x.shape
        y = torch.empty((n, self.out_channels, t, v), device=x.device, dtype=torch.float32)
        if self.framewise_route(x):
            rc = native.lib().csk_agcn_stage_framewise_f32(
                native.ptr(x), native.ptr(y), native.ptr(ops["w"]), native.ptr(ops["bias"]), native.ptr(ops["w_embed_pairs"]),
                native.ptr(ops["b_embed_pairs"]), native.ptr(ops["a_sum"]), n, c, self.out_channels, self.inter_c, t, v, c * t * v, t * v,
                self.out_channels * t * v, t * v, ops["res_mode"], native.stream_of(x))
            native.check(rc, "csk_agcn_stage_framewise_f32")
            return y
        xs, ys = (c * t * v, t * v), (self.out_channels * t * v, t * v)
        fused = self._fused_ok(v, x.data_ptr(), *xs)    # (a chunk starts t0 * V floats into a row: even for even V)
        chunk = max(1, int(self.framewise_budget_bytes // (4 * n * (3 * v * v + (0 if fused else 6 * self.inter_c * v)))))
        for t0 in range(0, t, chunk):
            f = min(chunk, t - t0)
            xc, yc = x[:, :, t0:], y[:, :, t0:]         # frames t0 .. of every channel: same strides, f frames taken
            adj = self._adjacency(xc, ops, n, f, xs, per_frame=True, fuse=fused)
            self._graph_conv(xc, yc, ops, adj, n, f, xs, ys, per_frame=True)
        return y

    def _fused_shape(self, v):
        """Shapes csk_agcn_embed_attention_f32 is built for (and the A/B switch)."""
        return self.fuse_embed_attention and v in (18, 25) and self.inter_c in (16, 32, 64)

    def _fused_ok(self, v, data_ptr, seg_stride, chan_stride):
        """``_fused_shape`` and what the entry asks of the operand (even V: 8-byte aligned activation rows)."""
        return self._fused_shape(v) and (v % 2 == 1 or (data_ptr % 8 == 0 and seg_stride % 2 == 0 and chan_stride % 2 == 0))

    def plan_operands(self, device):
        """Operands of the native step executor (csk_co_layer.agcn_*: the per-frame form of csk_agcn_embed_attention_f32), or
        None where that entry is not built (V not in {18, 25}, inter not in {16, 32, 64}): such stacks keep the Python engine."""
        ops = self._packed_ops(device)
        if not self._fused_shape(ops["V"]):
            return None
        return dict(inter=self.inter_c, w_pairs=ops["w_embed_pairs"], b_pairs=ops["b_embed_pairs"], a_sum=ops["a_sum"])

    def stage(self, x, y, n_seg, frames, x_strides, y_strides):
        """Continual use on channel-major frames (C, P): every skeleton is its own 'sample' with T = 1, so the
        attention is computed per skeleton and frame (coa_gcn.py: forward_stepping of the module) and the graph
        conv runs with a per-frame adjacency.  The n_seg consecutive ring slots of a launch cycle go through the launches of
        ``_adjacency`` together (segment = ring slot, frames = skeletons, one embedding row of P floats per slot), then the graph
        conv: adjacency per "frame" of a segment (= skeleton), index seg * frames + skeleton."""
        ops = self._packed_ops(x.device)
        adj = self._adjacency(x, ops, n_seg, frames, x_strides, per_frame=True, row=x_strides[1])
        self._graph_conv(x, y, ops, adj, n_seg, frames, x_strides, y_strides, per_frame=True)


class AdaptiveGraphConvolutionMod(GraphConvolution):
    """models/a_gcn_mod/a_gcn_mod.py:12-64, the graph conv of A-GCN*: same constructor, parameters and state_dict keys (``a_conv.*``,
    ``b_conv.*`` beside GraphConvolution's).  Its forward (a_gcn_mod.py:48-64) forms the attention per frame,
        A1 = softmax_w( a_i(x)[n, :, t, v] . b_i(x)[n, :, t, w] / inter_c ) + (A + graph_attn)_i[v, w],
    and applies it with ``einsum("nctv,nvwt->nctv", x, A1)`` -- an einsum that does not contract x over the joints: it multiplies
    x[n, c, t, v] by the row sum of A1 over w.  The softmax sums to 1 over w, so that factor is
        s_i[v] = 1 + sum_w (A + graph_attn)_i[v, w],
    a constant of the weights: the embedding convs never reach the output.  The published checkpoints were trained with exactly this
    arithmetic.  On the device it is therefore the plain sparse graph conv with a DIAGONAL adjacency -- one ELL entry per column
    (source v, value s_i[v], formed in float64 and rounded once) -- through csk_gcn_stage_f32 in the clip and the step form, the
    native plan included (``folds_to_plain``).  ``a_conv`` / ``b_conv`` are carried for the state_dict and never launched.
    One divergence: where a frame's attention logits hold a NaN or an infinity the reference's output is NaN; here it stays
    finite, because the softmax is never formed."""

    folds_to_plain = True

    def __init__(self, in_channels, out_channels, A, bn_momentum=0.1, coff_embedding=4):
        super().__init__(in_channels, out_channels, A, bn_momentum)
        self.inter_c = out_channels // coff_embedding
        self.a_conv = nn.ModuleList(nn.Conv2d(in_channels, self.inter_c, 1) for _ in range(self.num_subset))
        self.b_conv = nn.ModuleList(nn.Conv2d(in_channels, self.inter_c, 1) for _ in range(self.num_subset))
        for m in list(self.a_conv) + list(self.b_conv):
            init_weights(m)
        self.soft = nn.Softmax(-2)

    def _fold(self):
        sd = {k: v.detach().cpu() for k, v in self.state_dict().items() if not k.startswith(("a_conv.", "b_conv."))}
        f = fold.fold_graph_conv(sd)                      # weights / bias as for GraphConvolution ...
        v = f["V"]
        # ... and the diagonal adjacency: column v of subset i holds the one entry (v, s_i[v])
        s = 1.0 + (sd["A"].double() + sd["graph_attn"].double()).sum(-1)          # (3, V), a_gcn_mod.py:50, 56-60
        f["ell_src"] = torch.arange(v, dtype=torch.int32).repeat(3, 1).unsqueeze(-1).contiguous()
        f["ell_val"] = s.float().unsqueeze(-1).contiguous()
        f["ell_cnt_host"] = torch.tensor([1, 1, 1], dtype=torch.int32)
        f["ell_w"] = 1
        return f


def CoAdaptiveGraphConvolutionMod(in_channels, out_channels, A, bn_momentum=0.1):
    """models/coa_gcn_mod/coa_gcn_mod.py:11-14 -- per frame already, so the same module"""
    return AdaptiveGraphConvolutionMod(in_channels, out_channels, A, bn_momentum)


def CoAdaptiveGraphConvolution(in_channels, out_channels, A, bn_momentum=0.1):
    """models/coa_gcn/coa_gcn.py:11-14"""
    return AdaptiveGraphConvolution(in_channels, out_channels, A, bn_momentum)


class AGcn(StGcn):
    """models/a_gcn/a_gcn.py:72-145: the ST-GCN layer table with AdaptiveGraphConvolution."""

    def __init__(self, graph_A, input_shape=(3, 300, 25, 2), num_classes=60):
        super().__init__(graph_A, input_shape, num_classes, GraphConv=AdaptiveGraphConvolution)


class CoAGcn(CoStGcn):
    """models/coa_gcn/coa_gcn.py: CoST-GCN stack with the adaptive graph conv applied per frame."""

    def __init__(self, graph_A, input_shape=(3, 300, 25, 2), num_classes=60, pool_size=-1, pool_padding=-1):
        super().__init__(graph_A, input_shape, num_classes, pool_size, pool_padding, CoGraphConv=CoAdaptiveGraphConvolution)

    # ---- a stored clip at the steps' arithmetic ---------------------------------------------------
    def clip_as_steps_map(self, t, pad_end=False):
        """Host only.  ``(frames, entries)`` for a fresh model stepped through ``t`` frames: layer 10 has emitted ``frames``
        feature frames -- frame j of the clip pass -- (``prime_counts(t)[-1]``; with ``pad_end`` every block is flushed and all
        ``prime_clip_frames(t)[-1]`` frames of the clip come out), the pooling window has taken them in order, followed with
        ``pad_end`` by ``pool_padding`` zero entries; entry j (0-based) releases a prediction when j + 1 >= pool_size -
        pool_padding, the mean over pool_size of entries max(0, j + 1 - pool_size) .. j (entries >= ``frames`` and the ones
        before the first are zeros).  ``entries`` lists (first, last) of every prediction, inclusive, in order."""
        frames = self.prime_clip_frames(t)[-1] if (pad_end and t > 0) else self.prime_counts(t)[-1]
        total = frames + (self.pool_padding if (pad_end and t > 0) else 0)
        first = max(0, self.pool_size - self.pool_padding - 1)
        return frames, [(max(0, j + 1 - self.pool_size), j) for j in range(first, total)]

    def features_clip_as_steps(self, x):
        """(N, C, T, V, M) -> (N*M, 256, T', V): the layer-10 feature frames of ONE clip pass in which every adaptive graph conv
        forms its attention per frame (``AdaptiveGraphConvolution.forward_framewise``) -- frame j is what the steps emit as
        their j-th layer-10 frame, as long as they emit it (``clip_as_steps_map``); the frames behind it are the ones the end
        padding releases.  The input pre-passes as the steps apply them (a motion modality: the backward difference;
        ``_prepare_clip_as_stepped``).  Reads and writes no continual state."""
        self._require_eval()
        x = self._intake_clip(x)
        native.require_device_f32(x, "CoAGcn input")
        _, d = self._prepare_clip_as_stepped(x)
        return self._through_blocks(self.input_norm(d), lambda blk, h: self._framewise_parts(blk, h)[1])

    def forward_clip_as_steps(self, x, pad_end=False):
        """(N, C, T, V, M) -> (N, classes, n_predictions): what ``clean_state(); forward_steps(x, pad_end)`` returns (within the
        clip-versus-steps tolerance), by one clip pass (``features_clip_as_steps``) and the continual head applied to the
        feature frames in the steps' alignment (``clip_as_steps_map``): per-frame spatial pool, the zero-initialised pooling
        window -- the summation order of the step kernel, oldest entry first -- and the FC.  Neither reads nor writes the
        continual state; needs no bound slab."""
        h = self.features_clip_as_steps(x)
        n, t = x.shape[0], x.shape[self.time_axis]
        _, _, v, m = self.input_shape
        frames, entries = self.clip_as_steps_map(t, pad_end)
        if h.shape[2] < frames:
            raise RuntimeError(f"the clip pass gave {h.shape[2]} feature frames, the steps emit {frames}")
        if not entries:
            return torch.empty((n, self.num_classes, 0), device=x.device)
        lib, stream, w = native.lib(), native.stream_of(h), self.pool_size
        # entries of the pooling window, [entry][N][256]: the spatial pool of feature frame j, then zeros (end padding; slots
        # the kernel never reads fill the array up to one window behind the last entry)
        ring = torch.zeros((max(entries[-1][1] + 1, w) + w, n, 256), device=x.device, dtype=torch.float32)
        if frames:
            hf = h[:, :, :frames].permute(2, 0, 1, 3).contiguous()          # (frames, N*M, 256, V): a frame = N "samples" of M
            native.check(lib.csk_pool_scaled_f32(native.ptr(hf), native.ptr(ring), frames * n, m, 256, v, 1.0, stream),
                         "csk_pool_scaled_f32")
        pooled = torch.empty((len(entries), n, 256), device=x.device, dtype=torch.float32)
        for k, (first, last) in enumerate(entries):
            # window slots first .. first + w - 1 of the array; the `count` newest end at entry `last`
            native.check(lib.csk_co_window_mean_f32(native.ptr(ring[first]), native.ptr(pooled[k]), n * 256, w, last - first,
                                                    last - first + 1, stream), "csk_co_window_mean_f32")
        return self._fc(pooled).permute(1, 2, 0).contiguous()

    # ---- priming from buffered history at the steps' arithmetic (DESIGN.md sections 3e, 3h) ------------------------------
    @staticmethod
    def _framewise_parts(blk, h):
        """``(y, out)`` of a block with the attention formed per frame: the two stages of ``SpatioTemporalBlock.forward_parts``,
        the first one frame-wise.  What ``features_clip_as_steps`` walks the stack with and ``prime_state_as_steps`` keeps."""
        y = blk.gcn.forward_framewise(h)
        return y, blocks.SpatioTemporalBlock._tail(blk, h, y, None)

    def prime_state_as_steps(self, x_hist):
        """``prime_state`` for this family: the ``StreamState`` of ``n`` streams that have received the frames of ``x_hist``
        (n, C, T, V, M), by the clip pass of ``prime_state`` with every adaptive graph conv run frame-wise
        (``forward_framewise``: the post-GCN tensors are then the ones the steps' rings hold; the induction of 3e holds as it
        stands, the graph conv being per frame) and the same single pack launch per chunk of streams.  Every check of
        ``prime_state`` but the adaptive-graph-conv refusal, before anything launches; ``prime_state`` itself keeps refusing
        this class.  ``framewise_everywhere`` / ``fuse_framewise`` pick the fused kernel or the composed launches per block; a
        record's bits depend on neither, nor on the chunking.  Memory: ``prime_stream_bytes(T)`` of intermediates per stream,
        in chunks under ``prime_budget_bytes``, plus -- where a block composes the per-frame launches -- that block's chunk
        of per-frame adjacencies (and embeddings) under ``AdaptiveGraphConvolution.framewise_budget_bytes`` (256 MiB), one
        block's at a time."""
        return self._prime_records(x_hist, self._check_prime(x_hist, framewise=True), self._framewise_parts)

    def prime_streams_as_steps(self, x_hist, indices):
        """``import_streams(prime_state_as_steps(x_hist), indices)``; every host check of both halves runs before the first
        launch."""
        self._check_prime_streams(x_hist, indices, framewise=True)
        self.import_streams(self.prime_state_as_steps(x_hist), indices)


class AGcnMod(StGcnMod):
    """A-GCN*: models/a_gcn_mod/a_gcn_mod.py:67-124 -- StGcnMod's table, geometry (T >= 81, one feature frame per input frame from
    frame 80 on) and refusals with ``AdaptiveGraphConvolutionMod`` in every block, i.e. StGcnMod's launches with a diagonal
    adjacency: no embedding GEMM, no attention launch.  The conv-residual blocks (layers 5 and 8) run the valid Winograd form with
    the conv residual (csk_tcn_stage_wino_valid_res_f32)."""

    def __init__(self, graph_A, input_shape=(3, 300, 25, 2), num_classes=60):
        super().__init__(graph_A, input_shape, num_classes, GraphConv=AdaptiveGraphConvolutionMod)
        use_wino_valid_res(self)


class CoAGcnMod(CoStGcnMod):
    """CoA-GCN*: models/coa_gcn_mod/coa_gcn_mod.py -- CoStGcnMod with ``AdaptiveGraphConvolutionMod`` per frame.  The graph conv is
    per frame in the clip model too, so emission s is AGcnMod's clip feature frame s - 80 (which CoAGcn cannot offer against AGcn).
    A stack of plain graph convs for the native plan."""

    def __init__(self, graph_A, input_shape=(3, 300, 25, 2), num_classes=60, pool_size=-1, pool_padding=-1):
        super().__init__(graph_A, input_shape, num_classes, pool_size, pool_padding, CoGraphConv=CoAdaptiveGraphConvolutionMod)
        use_wino_valid_res(self)
