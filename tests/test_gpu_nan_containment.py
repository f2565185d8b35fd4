"""NaN containment on the device: ONE poisoned element inside an operand, through every kernel family.

Every case runs the same launch twice on the same operands -- clean, and with the one NaN -- both between NaN guards, and
asserts, all exact (set inclusion and bit equality, no tolerance anywhere in this file):

  * isnan(got) contains ``must``: nothing swallowed (an fmaxf epilogue, a softmax that skips the NaN);
  * isnan(got) lies in ``may``: nothing leaked (a zero-weight product with a neighbour's element: NaN x 0);
  * every element that is not NaN is bit for bit the clean run's -- every other sequence and stream entirely;
  * the clean run has no NaN.

The masks come from tests/nan_cone_fixture.py (fp64 reference only; proven on the host by tests/test_nan_cone_fixture_cpu.py).
The one documented exception is named, not silent: a launch that the route model gives to tcn_stage_wino_s2_kernel is held to
``may_wino_s2`` -- the dense cone plus the even output frame in front of it that the transform's zero-tap groups reach (the
fixture's finding); ``must`` and the other sequences are held as everywhere.

Which kernel a launch runs is asserted through the host queries and the route models the suite already pins
(csk_gcn_stage_f32_tile / csk_gcn_stage_f32_route, tcn_direct_fixture.select, tcn_wino_fixture.select) and appended to
nan_containment_routes.jsonl beside the suite's parity report (tests/helpers.py)."""
import os
import subprocess
import sys

import pytest
import torch

import _bootstrap
from oracle import stgcn_oracle as o
from tests import nan_cone_fixture as fx
from tests import tcn_direct_fixture as tdf
from tests import tcn_wino_fixture as twf
from tests import helpers
from tests.helpers import guarded_allocs, randomise_unit_

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native = pkg.native
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES_MODE = {"none": 0, "identity": 1, "conv": 2}


# ---- the four assertions ---------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def check(got, clean, must, may, info):
    assert tuple(got.shape) == tuple(clean.shape) == tuple(must.shape) == tuple(may.shape), info
    assert not bool(torch.isnan(clean).any()), ("the clean run holds a NaN", info)
    nan = torch.isnan(got)
    lost, leak = must & ~nan, nan & ~may
    assert not bool(lost.any()), (f"{int(lost.sum())} outputs swallowed the NaN, first {lost.nonzero()[0].tolist()}", info)
    assert not bool(leak.any()), (f"{int(leak.sum())} outputs outside the cone are NaN, first {leak.nonzero()[0].tolist()}", info)
    differ = ~nan & (_bits(got) != _bits(clean))
    assert not bool(differ.any()), (f"{int(differ.sum())} finite outputs differ from the clean run, first {differ.nonzero()[0].tolist()}", info)


def guarded(t, pad=1 << 14):
    """a device copy of ``t`` in the middle of a buffer whose ``pad`` floats either side are NaN"""
    buf = torch.full((t.numel() + 2 * pad,), float("nan"), device=DEV)
    v = buf[pad: pad + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def record(**kw):
    helpers.append_report("nan_containment_routes.jsonl", **kw)


# ---- routes (host arithmetic only) -------------------------------------------------------------------------------------------
ALIGNED = 1 << 20          # stand-in for x, y and the split scratch: the queries read their alignment only, and the launch's own x
                           # (a view 64 KiB into its guarded buffer) and y (a fresh allocation) are 256-byte aligned as well
SPARSE2, TILE16, DENSE2, DENSE128 = 1, 2, 3, 4      # families of csk_gcn_stage_f32_route
SPLIT_BIT = 1 << 30                                 # csk_gcn_stage_splitk_f32_route: a split launch


def gcn_route(g, n_seg, frames, adj_seg_stride=0, adj_per_frame=0, ell_val=None, row=0):
    """(tile, route, entry) of the clip launch ``GraphConvolution.forward`` makes for ``g`` at (n_seg, C, frames, V), asked with
    the module's own folded operands (its ELL counts and width, its res_mode, its ell_val) the way ``forward`` picks the entry:
    csk_gcn_stage_bf16x3 where the split image applies (no route query exists for it: the entry is the record),
    csk_gcn_stage_splitk_f32_route in latency mode, else csk_gcn_stage_f32_tile / csk_gcn_stage_f32_route.  tile = NB * 1000 +
    F * 100 + CONVRES * 10 of gcn16_kernel, or 0.  ``row``: floats of a channel row where it is longer than frames * V (a ring slot)."""
    ops = g._packed_ops(torch.device(DEV))
    ci, co, V = ops["c_in"], ops["c_out"], ops["V"]
    cnt, w, res = native.ptr(ops["ell_cnt_host"]), ops["ell_w"], ops["res_mode"]
    ell = native.ptr(ops["ell_val"] if ell_val is None else ell_val)
    tv, lib = (row or frames * V), native.lib()
    if type(g) is pkg.blocks.GraphConvolution and g._split_applies(ops):
        return 0, 0, "csk_gcn_stage_bf16x3"
    ks = g._clip_ksplit() if n_seg <= g.clip_split_max_seq else 1
    if ks > 1:
        route = lib.csk_gcn_stage_splitk_f32_route(ALIGNED, ALIGNED, ell, cnt, w, n_seg, ci, co, frames, V, ci * tv, tv, co * tv, tv, res, ks, ALIGNED)
        return 0, route, "csk_gcn_stage_splitk_f32"
    tile = lib.csk_gcn_stage_f32_tile(ALIGNED, ALIGNED, cnt, w, adj_seg_stride, adj_per_frame, n_seg, ci, co, frames, V, ci * tv, tv, co * tv, tv, res)
    route = lib.csk_gcn_stage_f32_route(ALIGNED, ALIGNED, ell, cnt, w, adj_seg_stride, adj_per_frame, n_seg, ci, co, frames, V, ci * tv, tv,
                                        co * tv, tv, res)
    return tile, route, "csk_gcn_stage_f32"


def tail_route(case, route, tcn16_mode=0):
    """the kernel of the block's temporal launch, from the suite's route models: (name, key)"""
    c, V, s, N = case.co, case.V, case.stride, case.N
    res = RES_MODE[case.res]
    c_res = case.ci if case.res == "conv" else c if case.res == "identity" else 0
    pad, off = (4, 0) if case.pad < 0 else (0, 4)
    if route in ("default", "wino_valid", "wino_valid_res", "forced"):
        entry = None
        if case.pad == 0:
            entry = "valid" if case.res == "identity" else "valid_res" if route == "wino_valid_res" else None
        elif case.res == "identity":
            entry = "id"
        elif not (case.res == "none" and s == 1):
            entry = "ext"
        if entry:
            sel = twf.select(entry, c, c, c_res, fx.T, V, 9, s, pad, res, off, n_seg=N)
            if not sel.reject:
                return sel.kernel, entry
    if route == "bf16x3":
        return "tcn_stage_bf16x3", ""
    ks = max(1, min(4, -(-c // 8))) if route == "latency" else 1
    sel = tdf.select(c, c, c_res, fx.T, V, 9, s, pad, res, off, ks, tcn16_mode, n_seg=N)
    return sel.key[0] + ("/split" if sel.split else ""), str(sel.key[1:])


# ---- clip blocks ---------------------------------------------------------------------------------------------------------------
def _configure(blk, route):
    if route == "few":
        blk.fuse_few_channels = True
    elif route == "bf16x3":
        pkg.set_precision(blk, "bf16x3")
    elif route == "latency":
        pkg.set_clip_latency_mode(blk, 4)
    elif route == "wino_valid_res":
        blk.wino_valid_res = True
    elif route == "direct":                       # the Winograd images withheld: the direct kernels at every row
        ops = blk._packed_ops(torch.device(DEV))
        ops["w_wino"] = ops["w_wino_ext"] = None


def _forward(module, x_h, fn=None):
    with guarded_allocs() as ga, torch.no_grad():
        out = (fn or module)(guarded(x_h))
        torch.cuda.synchronize()
    assert ga.count > 0
    return out.cpu()


_blocks, _clean = {}, {}


def _block(case, route):
    key = (case.geometry, route)
    if key not in _blocks:
        blk = fx.make_block(case.geometry).to(DEV)
        _configure(blk, route)
        _blocks[key] = blk
        _clean[key] = _forward(blk, fx.block_input(case, clean=True))
    return _blocks[key], _clean[key]


def _block_may(case, kernel):
    must, may = fx.block_masks(case)
    return must, (fx.may_wino_s2(case) if kernel == "tcn_stage_wino_s2_kernel" else may)


def run_block_case(case, route, tcn16_mode=0):
    blk, clean = _block(case, route)
    kernel, key = tail_route(case, route, tcn16_mode)
    if route == "few":
        assert blk._few_channels_fusable(fx.block_input(case).to(DEV))
        kernel, gcn = "block1_fused16_kernel", (0, 0, "csk_block_few_channels_f32")
    else:
        gcn = gcn_route(blk.gcn, case.N, fx.T)
        want_entry = {"bf16x3": "csk_gcn_stage_bf16x3" if case.co % 128 == 0 else "csk_gcn_stage_f32",
                      "latency": "csk_gcn_stage_splitk_f32" if case.ci >= 16 else "csk_gcn_stage_f32"}.get(route, "csk_gcn_stage_f32")
        assert gcn[2] == want_entry, (case.id, route, gcn)
        if route == "latency" and case.ci >= 16:
            assert gcn[1] & SPLIT_BIT, (case.id, gcn)                  # really split: gcn_stage_sparse2_kernel<.., true> + gcn_reduce_kernel
    if route == "wino_valid" or route == "wino_valid_res":
        assert kernel == "tcn_stage_wino_kernel", (case.id, route, kernel)
    got = _forward(blk, fx.block_input(case))
    must, may = _block_may(case, kernel)
    record(case=case.id, route=route, tail=kernel, tail_key=key, gcn_tile=gcn[0], gcn_route=gcn[1], gcn_entry=gcn[2])
    check(got, clean, must, may, (case.id, route, kernel, gcn))
    return kernel, gcn


CLIP_ROUTES = ("default", "direct", "bf16x3", "latency")


@pytest.mark.parametrize("route", CLIP_ROUTES)
@pytest.mark.parametrize("case", fx.BLOCK_CASES, ids=lambda c: c.id)
def test_clip_block(case, route):
    """SpatioTemporalBlock at the six layer-table rows, V = 25 (3 sequences) and 18 (4): the default route (Winograd where the
    entries take the row), the direct kernels, bf16x3 and the split-K latency mode"""
    run_block_case(case, route)


@pytest.mark.parametrize("case", [c for c in fx.BLOCK_CASES if c.ci == 3], ids=lambda c: c.id)
def test_clip_block_few_channels_fused(case):
    """csk_block_few_channels_f32 (block1_fused16_kernel): threads past the window redo its last column"""
    run_block_case(case, "few")


@pytest.mark.parametrize("case", fx.MOD_CASES, ids=lambda c: c.id)
def test_unpadded_block_on_the_valid_winograd_entries(case):
    """the "*" blocks: csk_tcn_stage_wino_valid_f32 (identity rows) and csk_tcn_stage_wino_valid_res_f32 (conv rows)"""
    run_block_case(case, "wino_valid" if case.res == "identity" else "wino_valid_res")


def test_the_clip_routes_reach_the_kernels_they_are_listed_for():
    """host arithmetic only: between them the in-process routes run both Winograd kernels, both strides of tcn_stage16_kernel,
    tcn_stage_kernel (whole and split) and the sparse graph conv -- unsplit, split-K in latency mode, and the bf16x3 entry"""
    tails = {tail_route(c, r)[0] for c in fx.BLOCK_CASES for r in CLIP_ROUTES}
    tails |= {tail_route(c, "wino_valid" if c.res == "identity" else "wino_valid_res")[0] for c in fx.MOD_CASES}
    assert {"tcn_stage_wino_kernel", "tcn_stage_wino_s2_kernel", "tcn_stage_kernel", "tcn_stage_kernel/split", "tcn_stage16_kernel",
            "tcn_stage_bf16x3"} <= tails, tails
    strides16 = {c.stride for c in fx.BLOCK_CASES if tail_route(c, "direct")[0] == "tcn_stage16_kernel"}
    assert strides16 == {1, 2}
    routes = {gcn_route(_block(c, "default")[0].gcn, c.N, fx.T) for c in fx.BLOCK_CASES}
    assert all(tile == 0 for tile, _, _ in routes), routes       # the policy keeps these sizes off the 16-wide tiles ...
    assert all(r > 0 and r // 1000000 == SPARSE2 for _, r, _ in routes), routes    # ... on gcn_stage_sparse2_kernel
    split = {gcn_route(_block(c, "latency")[0].gcn, c.N, fx.T) for c in fx.BLOCK_CASES if c.ci >= 16}
    assert split and all(e == "csk_gcn_stage_splitk_f32" and r & SPLIT_BIT for _, r, e in split), split
    pieces = {gcn_route(_block(c, "bf16x3")[0].gcn, c.N, fx.T)[2] for c in fx.BLOCK_CASES if c.co % 128 == 0}
    assert pieces == {"csk_gcn_stage_bf16x3"}, pieces


# ---- both 16-wide families, forced (one fresh child process for all cases) ---------------------------------------------------
CHILD_SECONDS = 300


def forced_child(path):
    """(child process, CSK_DIAG=1 CSK_GCN16=2 CSK_TCN16=2) every block case (and the 6-sequence ones) on the direct route and the default route: the
    assertions run here, the routes go back to the parent"""
    seen = []
    for route in ("direct", "default"):
        for case in fx.BLOCK_CASES + fx.SIX_CASES:
            kernel, gcn = run_block_case(case, route, tcn16_mode=2)
            seen.append((case.id, route, kernel, case.stride, gcn[0], gcn[1]))
    torch.save(seen, path)


@pytest.fixture(scope="module")
def forced(tmp_path_factory):
    code = "import sys; sys.path.insert(0, %r); from tests import test_gpu_nan_containment as t; t.forced_child(sys.argv[1])" % ROOT
    path = str(tmp_path_factory.mktemp("nan16") / "forced.pt")
    env = dict(os.environ, CSK_DIAG="1", CSK_GCN16="2", CSK_TCN16="2")
    env.pop("CSK_GCN_GENERAL", None)
    rc = subprocess.call(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, "-c", code, path], env=env)
    assert rc == 0, f"the child with the 16-wide families forced exited {rc} (its assertions are the containment checks)"
    return torch.load(path)


def test_forced_tile_families_contain_the_nan(forced):
    """every block case again with gcn16_kernel and tcn_stage16_kernel wherever they are built: the child asserted containment
    for each; here: that the list reached gcn16_kernel with F = 4, 2 and 1 and both strides of tcn_stage16_kernel"""
    assert len(forced) == 2 * len(fx.BLOCK_CASES + fx.SIX_CASES)
    tiles = {t for *_, t, _ in forced if t}
    assert {t // 100 % 10 for t in tiles} >= {4, 2, 1}, tiles
    assert {s for _, route, k, s, _, _ in forced if k == "tcn_stage16_kernel"} == {1, 2}
    assert {k for _, route, k, *_ in forced if route == "default"} >= {"tcn_stage_wino_kernel", "tcn_stage_wino_s2_kernel"}


# ---- adaptive graph conv -----------------------------------------------------------------------------------------------------
_agcn = {}


@pytest.mark.parametrize("case", fx.AGCN_CASES, ids=lambda c: c.id)
def test_adaptive_graph_conv(case):
    """clip: embeddings + logits over the sequence + softmax + dense graph conv (agcn_embed_attention_kernel at V = 18, conv1x1 +
    agcn attention kernels at V = 25, gcn_stage_dense2_kernel); frame: the steps' arithmetic on a whole clip, on the frame-wise
    kernel wherever it is built AND as the composed per-frame launches.  One NaN makes its whole frame NaN (clip: its whole
    sequence, as the reference's attention sums over the frames)."""
    forms = ("clip",) if case.form == "clip" else ("framewise", "composed")
    must, may = fx.agcn_masks(case)
    for form in forms:
        key = (case.geometry, form)
        if key not in _agcn:
            g = fx.make_agcn(case.geometry).to(DEV)
            g.framewise_everywhere, g.fuse_framewise = True, form != "composed"
            fn = None if form == "clip" else g.forward_framewise
            _agcn[key] = (g, fn, _forward(g, fx.agcn_input(case, clean=True), fn))
        g, fn, clean = _agcn[key]
        route = g.framewise_route(fx.agcn_input(case).to(DEV)) if form != "clip" else -1
        assert form != "framewise" or route > 0, (case.id, "the frame-wise kernel is not built for this shape")
        assert form != "composed" or route == 0
        # the attention launch: one fused kernel at V = 18, the embedding conv + the attention kernels at V = 25 (forward's rule);
        # the graph conv behind it, asked with the dense adjacency's stride: per sequence (clip) or per frame (composed)
        fused = case.V == 18 and g._fused_ok(case.V, ALIGNED, case.ci * fx.T * case.V, fx.T * case.V)
        assert fused == (case.V == 18), (case.id, "agcn_embed_attention_kernel is built for V = 18 clips")
        attention = "agcn_embed_attention_kernel" if fused else "conv1x1 + agcn attention + agcn_softmax"
        dense = -1
        if form != "framewise":
            _, dense, _ = gcn_route(g, case.N, fx.T, 3 * case.V * case.V, int(form == "composed"), ell_val=torch.empty(4, device=DEV))
            assert dense // 1000000 == DENSE2, (case.id, form, dense)          # gcn_stage_dense2_kernel
        got = _forward(g, fx.agcn_input(case), fn)
        record(case=case.id, route=form, framewise_route=route, attention=attention, gcn_route=dense)
        check(got, clean, must, may, (case.id, form, route, dense))


@pytest.mark.parametrize("case", fx.AGCN_STEP_CASES, ids=lambda c: c.id)
def test_adaptive_graph_conv_step_form(case):
    """AdaptiveGraphConvolution.stage on channel-major frames, as the continual engine calls it: 2 ring slots of 7 skeletons (a
    ragged tile that holds several streams).  The masks are the fixture's (the reference sees a slot as a sequence and a skeleton
    as a frame): the NaN's skeleton, every joint and channel, nothing else.  The graph conv runs gcn_stage_dense2_kernel on one
    adjacency per skeleton, formed by agcn_embed_attention_kernel's per-frame form."""
    ci, co, V, slots, skel = case.ci, case.co, case.V, case.N, case.frames
    g = fx.make_agcn(case.geometry).to(DEV)
    must, may = fx.agcn_masks(case)
    P = (skel * V + 3) // 4 * 4
    assert g._fused_ok(V, ALIGNED, ci * P, P), (case.id, "the per-frame attention kernel is not built for this shape")
    _, dense, _ = gcn_route(g, slots, skel, 3 * V * V, 1, ell_val=torch.empty(4, device=DEV), row=P)
    assert dense // 1000000 == DENSE2, (case.id, dense)
    outs = []
    for clean in (True, False):
        x = torch.zeros((slots, ci, P))
        x[:, :, : skel * V] = fx.agcn_input(case, clean=clean).reshape(slots, ci, skel * V)
        with guarded_allocs(), torch.no_grad():
            xd = guarded(x)
            y = torch.zeros((slots, co, P), device=DEV)
            g.stage(xd, y, n_seg=slots, frames=skel, x_strides=(ci * P, P), y_strides=(co * P, P))
            torch.cuda.synchronize()
        outs.append(y[:, :, : skel * V].cpu().reshape(slots, co, skel, V))
    record(case=case.id, route="step", attention="agcn_embed_attention_kernel", gcn_route=dense)
    check(outs[1], outs[0], must, may, case.id)


# ---- head ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fx.HEAD_CASES, ids=lambda c: c.id)
def test_pool_fc_head(case):
    """csk_pool_fc_f32: a NaN in one sequence's features -> exactly that sample's row of logits, every class"""
    h, w, b = fx.head_operands(case)
    must, may = fx.head_masks(case)
    outs = []
    for poison in (False, True):
        hh = h.clone()
        if poison:
            hh[case.poison] = float("nan")
        hd, wd, bd = guarded(hh), guarded(w), guarded(b)
        feat = guarded(torch.zeros((case.N, fx.HEAD_C)))
        logits = guarded(torch.zeros((case.N, case.classes)))
        rc = native.lib().csk_pool_fc_f32(native.ptr(hd), native.ptr(wd), native.ptr(bd), native.ptr(feat), native.ptr(logits), case.N,
                                          case.M, fx.HEAD_C, case.t * case.V, case.classes, native.stream_of(hd))
        native.check(rc, "csk_pool_fc_f32")
        torch.cuda.synchronize()
        outs.append(logits.cpu())
    check(outs[1], outs[0], must, may, case.id)


def _co_head_step_run(case, h, w, b):
    """csk_co_head_step_f32 stepped through the feature frames from a zero ring: (n_pred, N, classes) on the host"""
    n, c, mv = case.N, fx.HEAD_C, case.M * case.V
    P = (n * mv + 4) // 4 * 4
    wd, bd = guarded(w), guarded(b)
    ring = guarded(torch.zeros((case.window, n, c)))
    pooled, logits = guarded(torch.zeros((n, c))), guarded(torch.zeros((n, case.classes)))
    out = []
    for t in range(case.steps):
        frame = torch.zeros((c, P))                                   # channel-major: stream n at positions n MV .. (n + 1) MV - 1
        frame[:, : n * mv] = h[t].view(n, case.M, c, case.V).permute(2, 0, 1, 3).reshape(c, n * mv)
        hd = guarded(frame)
        emit = int(t >= case.first_entry)
        rc = native.lib().csk_co_head_step_f32(native.ptr(hd), native.ptr(ring), native.ptr(pooled), native.ptr(wd), native.ptr(bd),
                                               native.ptr(logits), n, c, mv, P, case.window, t % case.window, min(t + 1, case.window), emit,
                                               case.classes, native.stream_of(hd))
        native.check(rc, "csk_co_head_step_f32")
        torch.cuda.synchronize()
        if emit:
            out.append(logits.cpu())
    return torch.stack(out, 0)


def _co_head_clip_run(case, h, w, b):
    """csk_co_head_clip_f32 on the same frames as one clip tensor (N M, C, steps + 2, V): the two frames behind hold NaN and
    are never read"""
    n, c = case.N, fx.HEAD_C
    n_pred = case.steps - case.first_entry
    clip = torch.full((n * case.M, c, case.steps + 2, case.V), float("nan"))
    clip[:, :, : case.steps] = h.permute(1, 2, 0, 3)
    hd, wd, bd = guarded(clip), guarded(w), guarded(b)
    entries, pooled = guarded(torch.zeros((case.steps, n, c))), guarded(torch.zeros((n_pred, n, c)))
    logits = guarded(torch.zeros((n_pred, n, case.classes)))
    rc = native.lib().csk_co_head_clip_f32(native.ptr(hd), case.steps + 2, case.steps, native.ptr(entries), case.window, case.first_entry,
                                           n_pred, native.ptr(wd), native.ptr(bd), native.ptr(pooled), native.ptr(logits), n, case.M, c,
                                           case.V, case.classes, native.stream_of(hd))
    native.check(rc, "csk_co_head_clip_f32")
    torch.cuda.synchronize()
    return logits.cpu()


@pytest.mark.parametrize("run", [_co_head_step_run, _co_head_clip_run], ids=["csk_co_head_step_f32", "csk_co_head_clip_f32"])
@pytest.mark.parametrize("case", fx.CO_HEAD_CASES, ids=lambda c: c.id)
def test_continual_head(case, run):
    """the step head and the clip-as-steps head on the same feature frames, NaN in one sequence's features: exactly that stream's
    row of logits is NaN, in all classes, for exactly the predictions whose zero-initialised pooling window holds the frame (the
    reference head's masks); the other streams and the recovered predictions are the clean run's bits"""
    h, w, b = fx.co_head_operands(case)
    must, may = fx.co_head_masks(case)
    with guarded_allocs():
        clean = run(case, h, w, b)
        got = run(case, fx.co_head_poisoned(case, h), w, b)
    check(got, clean, must, may, (case.id, run.__name__))


# ---- the continual models ------------------------------------------------------------------------------------------------------
def _co_net(model, V, fuse=True, seed=7, weights=None):
    A = fx.graph_A(V)
    cls = pkg.CoAGcn if model == "agcn" else pkg.CoStGcn
    net = cls(A, (3, 300, V, fx.CO_M), 60, pool_size=fx.CO_POOL[0], pool_padding=fx.CO_POOL[1]).eval()
    if weights is None:
        randomise_unit_(net, seed, attn_scale=1.0 / V if model == "agcn" else 1.0)
    else:
        net.load_state_dict(weights)
    for blk in net.layers.values():
        blk.fuse_step = fuse
    return net.to(DEV)


def _plain_sd(net):
    """the model's weights under the plain StGcn keys the oracle reads"""
    return {k.replace("0.1.", "").replace("0.0.residual", "residual"): v.detach().cpu() for k, v in net.state_dict().items()}


def _step_all(net, frames, r=4, lo=0, hi=None):
    """frames (T, N, C, V, M) on the host, in cycles of ``r`` -> the list of logits (host) in emission order"""
    out = []
    hi = frames.shape[0] if hi is None else hi
    with guarded_allocs(), torch.no_grad():
        fd = guarded(frames)
        for t in range(lo, hi, r):
            out += [y.cpu() for y in net.forward_cycle([fd[s] for s in range(t, min(t + r, hi))])]
        torch.cuda.synchronize()
    return out


def _derive(frames_stream, modality, prenorm, V):
    """what the oracle is fed for one stream (T, 3, V, M): the public host restatements of the input pre-passes, in chain order"""
    import numpy as np
    from tests import modality_oracle, prenorm_oracle
    x = frames_stream.permute(1, 0, 2, 3)[None].numpy()                      # (1, C, T, V, M)
    with np.errstate(all="ignore"):
        if prenorm:
            x = prenorm_oracle.pre_normalize_steps(x)
        x = modality_oracle.derive_steps(x, modality, pkg.modality.bone_parents(V))
    return torch.from_numpy(np.ascontiguousarray(x[0])).permute(1, 0, 2, 3)   # (T, C, V, M)


def check_streams(got, clean, oracle_nan, info):
    """containment and recovery: every emission, every stream"""
    want = [m for m in oracle_nan if m is not None]
    assert len(got) == len(clean) == len(want) > 0, (len(got), len(clean), len(want), info)
    others = [n for n in range(fx.CO_STREAMS) if n != fx.CO_POISONED]
    for i, (g, c, m) in enumerate(zip(got, clean, want)):
        assert not bool(torch.isnan(c).any()), (i, info)
        assert torch.equal(_bits(g[others]), _bits(c[others])), (i, "another stream changed", info)
        nan = torch.isnan(g[fx.CO_POISONED])
        assert torch.equal(nan, m), (i, "stream NaN where the oracle is not, or the reverse", int(nan.sum()), int(m.sum()), info)
        if not bool(m.any()):
            assert torch.equal(_bits(g[fx.CO_POISONED]), _bits(c[fx.CO_POISONED])), (i, "not recovered bit for bit", info)
    return want


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("model,V", [("stgcn", 25), ("stgcn", 18), ("agcn", 18)])
def test_continual_model_contains_and_recovers(model, V, fuse):
    """5 streams (M = 2: tiles span streams), one NaN in stream 2 at step 6: the other streams are the clean run's bits at every
    emission; stream 2 is NaN exactly where the fp64 oracle is, and the clean run's bits from the oracle's first clean step on"""
    net = _co_net(model, V, fuse)
    clean = _step_all(net, fx.co_frames(V, clean=True))
    net.clean_state()
    got = _step_all(net, fx.co_frames(V))
    gcn = o.adaptive_graph_conv if model == "agcn" else o.graph_conv
    want = check_streams(got, clean, fx.co_oracle_nan(_plain_sd(net), fx.co_frames(V)[:, fx.CO_POISONED], gcn), (model, V, fuse))
    assert bool(want[0].all()) and not bool(want[-1].any())          # the oracle: poisoned at first, recovered in the end


@pytest.mark.parametrize("modality,prenorm", [("bone", False), ("joint_motion", False), ("joint", True), ("bone_motion", True)])
def test_continual_model_input_chain(modality, prenorm):
    """the same with the input pre-passes on: the oracle, fed what the host restatements of the pre-passes make of the poisoned
    stream's frames, decides where the stream is NaN and whether it recovers"""
    V = 25
    net = _co_net("stgcn", V)
    if prenorm:
        pkg.set_pre_normalization(net)
    pkg.set_input_modality(net, modality)
    clean = _step_all(net, fx.co_frames(V, clean=True))
    net.clean_state()
    got = _step_all(net, fx.co_frames(V))
    fed = _derive(fx.co_frames(V)[:, fx.CO_POISONED], modality, prenorm, V)
    check_streams(got, clean, fx.co_oracle_nan(_plain_sd(net), fed), (modality, prenorm))


def test_stream_shards_contain_the_nan():
    """2 shards (streams 0-2 and 3-4, or 0-1 and 2-4): the poisoned stream's shard holds it, the other shard never sees it"""
    V = 25
    first = _co_net("stgcn", V)
    weights = first.state_dict()
    shards = pkg.parallel.StreamShards(lambda: _co_net("stgcn", V, weights=weights), fx.CO_STREAMS, 2, torch.device(DEV))
    runs = []
    for clean in (True, False):
        for m in shards.models:
            m.clean_state()
        frames, out = fx.co_frames(V, clean=clean), []
        with guarded_allocs(), torch.no_grad():
            fd = guarded(frames)
            for t in range(0, frames.shape[0], 4):
                y = shards.forward_cycle([fd[s] for s in range(t, t + 4)])
                if y is not None:
                    out.append(y.cpu())
            torch.cuda.synchronize()
        runs.append(out)
    single = _step_all(first, fx.co_frames(V))
    assert len(runs[1]) == len(single)
    check_streams(runs[1], runs[0], fx.co_oracle_nan(_plain_sd(first), fx.co_frames(V)[:, fx.CO_POISONED]), "shards")
    for a, b in zip(runs[1], single):                                   # and a shard's bits are the single slab's, NaN included
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(_bits(a)[~torch.isnan(a)], _bits(b)[~torch.isnan(b)])


@pytest.mark.parametrize("model,V", [("stgcn", 25), ("agcn", 18)])
def test_clip_as_steps_contains_and_recovers(model, V):
    """forward_clip_as_steps (one clip pass + csk_co_head_clip_f32) on the same 5 streams: the predictions of the other streams
    are the clean clip's bits, stream 2 is NaN exactly in the predictions where the fp64 step oracle is and the clean clip's
    bits from there on"""
    net = _co_net(model, V)
    runs = []
    for clean in (True, False):
        x = fx.co_frames(V, clean=clean).permute(1, 2, 0, 3, 4).contiguous()           # (N, C, T, V, M)
        y = _forward(net, x, net.forward_clip_as_steps)                                 # (N, classes, n_pred)
        runs.append([y[:, :, k] for k in range(y.shape[2])])
    gcn = o.adaptive_graph_conv if model == "agcn" else o.graph_conv
    check_streams(runs[1], runs[0], fx.co_oracle_nan(_plain_sd(net), fx.co_frames(V)[:, fx.CO_POISONED], gcn), (model, V, "clip as steps"))


# ---- stream operations ---------------------------------------------------------------------------------------------------------
def _slabs(net):
    """both slabs of every block -- the post-GCN ring and the output ring -- and the pooling window, on the host, the streams on
    an axis of their own: [(slots, C, N, M V)] + [(window, N, C) -> (window, C, N, 1)]"""
    _, _, v, m = net.input_shape
    n, out = fx.CO_STREAMS, []
    for blk in net.layers.values():
        for ring in (blk._state.y, blk._state.out):
            out.append(ring[:, :, : n * m * v].cpu().reshape(ring.shape[0], ring.shape[1], n, m * v))
    return out


def _same_slabs(a, b, streams, info):
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(_bits(x[:, :, streams]), _bits(y[:, :, streams])), (info, "slab", i // 2, "y" if i % 2 == 0 else "out")


def test_prime_streams_with_a_poisoned_history():
    """prime_streams([2]) from a history of 88 frames that holds the NaN (one clip pass + csk_co_prime_pack_f32 + the import), in
    a slab whose other streams are live: right after it both slabs of streams 0, 1, 3, 4 are bit for bit those of a twin primed
    with the clean history, and so are their logits at every later step; stream 2 is NaN exactly where the fp64 oracle, stepped
    through the same frames, is NaN, and the clean-primed twin's bits once the oracle is clean again"""
    V, t_prime = 25, 88
    net = _co_net("stgcn", V)
    twin = _co_net("stgcn", V, weights=net.state_dict())
    clean_frames, frames = fx.co_frames(V, clean=True), fx.co_frames(V)
    assert fx.CO_POISON_FRAME < t_prime and t_prime % 8 == 0
    runs = []
    for model, src in ((twin, clean_frames), (net, frames)):
        before = _step_all(model, clean_frames, hi=t_prime)                  # every stream live; stream 2's own past is clean
        hist = src[:t_prime, fx.CO_POISONED: fx.CO_POISONED + 1].permute(1, 2, 0, 3, 4).contiguous()    # (1, C, T, V, M)
        with guarded_allocs(), torch.no_grad():
            model.prime_streams(guarded(hist), [fx.CO_POISONED])
            torch.cuda.synchronize()
        runs.append((before, _slabs(model), _step_all(model, clean_frames, lo=t_prime)))
    others = [n for n in range(fx.CO_STREAMS) if n != fx.CO_POISONED]
    (before_c, slabs_c, clean), (before_p, slabs_p, got) = runs
    _same_slabs(slabs_p, slabs_c, others, "right after prime_streams")
    assert any(bool(torch.isnan(s[:, :, fx.CO_POISONED]).any()) for s in slabs_p), "the poisoned history left no NaN in the slab"
    assert not any(bool(torch.isnan(s).any()) for s in slabs_c)
    oracle = fx.co_oracle_nan(_plain_sd(net), frames[:, fx.CO_POISONED])     # the stream as the history + the frames that follow
    want = [m for m in oracle[t_prime:] if m is not None]
    assert len(want) == len(got) == len(clean) and bool(want[0].all()) and not bool(want[-1].any())
    check_streams(got, clean, want, "prime_streams")
    for a, b in zip(before_p, before_c):                                      # (the two models were the same up to the prime)
        assert torch.equal(_bits(a), _bits(b))


def test_reset_right_after_the_poison_gives_a_fresh_stream():
    """reset_streams([2]) at the first stride boundary after the NaN: from the twin's first emission on, stream 2 is bit for bit
    a twin model's fresh stream fed the same frames; the untouched streams are the clean run's bits throughout"""
    V = 25
    net = _co_net("stgcn", V)
    twin = _co_net("stgcn", V, weights=net.state_dict())
    clean_frames, frames = fx.co_frames(V, clean=True), fx.co_frames(V)
    t_reset = 8                                                        # the NaN came at step 6; 8 is a multiple of the stride
    clean = _step_all(net, clean_frames, hi=t_reset)
    slabs_clean = _slabs(net)
    clean += _step_all(net, clean_frames, lo=t_reset)
    end_clean = _slabs(net)
    net.clean_state()
    got = _step_all(net, frames, hi=t_reset)
    assert any(bool(torch.isnan(s[:, :, fx.CO_POISONED]).any()) for s in _slabs(net)), "the NaN never reached the slab"
    net.reset_streams([fx.CO_POISONED])
    slabs_reset = _slabs(net)
    got += _step_all(net, frames, lo=t_reset)
    fresh = _step_all(twin, frames[t_reset:, fx.CO_POISONED: fx.CO_POISONED + 1].contiguous())
    assert len(got) == len(clean) and 0 < len(fresh) <= len(got)
    others = [n for n in range(fx.CO_STREAMS) if n != fx.CO_POISONED]
    for g, c in zip(got, clean):
        assert torch.equal(_bits(g[others]), _bits(c[others]))
    for j in range(1, len(fresh) + 1):                                 # aligned at the end: both have seen the same last frame
        g, f = got[-j][fx.CO_POISONED], fresh[-j][0]
        assert not bool(torch.isnan(f).any()) and torch.equal(_bits(g), _bits(f)), j
    _same_slabs(slabs_reset, slabs_clean, others, "right after reset_streams")      # both slabs of the untouched streams
    _same_slabs(_slabs(net), end_clean, others, "at the end")
    for s in slabs_reset:                                              # no NaN left in any slot of the reset stream
        assert not bool(torch.isnan(s).any())
    for blk in net.layers.values():
        assert not bool(torch.isnan(blk._state.y).any()) and not bool(torch.isnan(blk._state.out).any())


def test_export_import_moves_the_nan_with_its_stream_only():
    """a poisoned, ready stream exported and imported into stream 1 of another slab: there NaN appears in stream 1 alone and the
    other streams keep the clean run's bits; the source slab is unchanged by the export"""
    V = 25
    src = _co_net("stgcn", V)
    dst = _co_net("stgcn", V, weights=src.state_dict())
    ref = _co_net("stgcn", V, weights=src.state_dict())
    clean_frames = fx.co_frames(V, clean=True)
    late = clean_frames.clone()
    t_nan, t_move = 158, 160                                           # the stream is ready (past the stack's delay) when it moves
    late[t_nan, fx.CO_POISONED, 0, 0, 0] = float("nan")
    _step_all(src, late, hi=t_move)
    _step_all(dst, clean_frames, hi=t_move)
    _step_all(ref, clean_frames, hi=t_move)
    assert bool(src.streams_ready().all())
    src_before = _slabs(src)
    state = src.export_streams([fx.CO_POISONED])
    dst.import_streams(state, [1])
    torch.cuda.synchronize()
    every = list(range(fx.CO_STREAMS))
    _same_slabs(_slabs(src), src_before, every, "the source slab after export_streams")        # NaN bits included
    _same_slabs(_slabs(dst), _slabs(ref), [n for n in every if n != 1], "the target slab after import_streams")
    assert any(bool(torch.isnan(s[:, :, 1]).any()) for s in _slabs(dst)) and not any(bool(torch.isnan(s).any()) for s in _slabs(ref))
    tail = clean_frames.clone()
    tail[:, 1] = clean_frames[:, fx.CO_POISONED]                       # stream 1 goes on with the moved stream's frames
    got = _step_all(dst, tail, lo=t_move)
    want = _step_all(ref, clean_frames, lo=t_move)
    after_src = _step_all(src, late, lo=t_move)
    assert len(got) == len(want) == len(after_src) > 0
    others = [n for n in range(fx.CO_STREAMS) if n != 1]
    for i, (g, w, s) in enumerate(zip(got, want, after_src)):
        assert torch.equal(_bits(g[others]), _bits(w[others])), i
        assert torch.equal(torch.isnan(g[1]), torch.isnan(s[fx.CO_POISONED])), i        # the moved stream: NaN as at its source
        keep = ~torch.isnan(g[1])
        assert torch.equal(_bits(g[1])[keep], _bits(s[fx.CO_POISONED])[keep]), i
    assert bool(torch.isnan(got[0][1]).all())
