"""GPU parity, continual path.  The identities are the ones the reference's own tests assert
(tests/test_cost_gcn.py, tests/test_st_gcn_mod.py): continual output == clip output at a shifted index; the
clip side comes from the golden vectors produced by the reference's classes.  Tolerance 1e-4 absolute."""
import pytest
import torch

import _bootstrap
from oracle import stgcn_oracle as o
from tests.helpers import check_parity, g6_state_dict, load_golden, max_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
pkg = _bootstrap.load()
DEV = "cuda:0"
A = pkg.ntu_graph().A


def test_co_temporal_convolution_pad_end():
    """tests/test_cost_gcn.py:37-68"""
    a, sd = load_golden("g2_tcn_k9s1p4")
    co = pkg.CoTemporalConvolution(4, 4, 9, 4, 1).eval()
    co.load_state_dict(sd, strict=True)
    co = co.to(DEV)
    x = torch.from_numpy(a["x"]).to(DEV)
    check_parity(co.forward(x).cpu(), a["y"])
    check_parity(co.forward_steps(x, pad_end=True).cpu(), a["y"])


def _co_block(tag, padding=4):
    a, sd = load_golden(f"g3_block_{tag}")
    ci, co_, s, res, tp = (int(v) for v in a["meta"])
    blk = pkg.CoSpatioTemporalBlock(ci, co_, A, s, bool(res), padding=padding).eval()
    blk.load_state_dict(sd, strict=True)          # plain layout from the reference's regular block
    return blk.to(DEV), torch.from_numpy(a["x"]).to(DEV), torch.from_numpy(a["y"]), s


@pytest.mark.parametrize("tag", ["nores", "ident"])
def test_block_step_lags_clip_by_4(tag):
    """tests/test_cost_gcn.py:71-176: output[t + 4] == target[:, :, t]"""
    blk, x, target, _ = _co_block(tag)
    outs = [blk.forward_step(x[:, :, i].contiguous()) for i in range(x.shape[2])]
    assert all(v is None for v in outs[:4])
    for t in range(x.shape[2] - 4):
        check_parity(outs[t + 4].cpu(), target[:, :, t], note=t)


@pytest.mark.parametrize("tag", ["convres", "strided", "ident", "nores"])
def test_block_forward_and_forward_steps(tag):
    """tests/test_cost_gcn.py:179-271"""
    blk, x, target, s = _co_block(tag)
    check_parity(blk.forward(x).cpu(), target)
    o1 = blk.forward_steps(x, pad_end=False).cpu()
    cut = blk.delay // s
    assert o1.shape[2] == target.shape[2] - cut
    check_parity(o1, target[:, :, : target.shape[2] - cut])
    blk.clean_state()
    o2 = blk.forward_steps(x, pad_end=True).cpu()
    assert o2.shape == target.shape
    check_parity(o2, target)


@pytest.mark.parametrize("tag", ["nopad", "nopad_strided"])
def test_block_nopad(tag):
    """tests/test_st_gcn_mod.py:11-54 (padding=0: forward and stepping both give the un-padded clip output)"""
    blk, x, target, _ = _co_block(tag, padding=0)
    check_parity(blk.forward(x).cpu(), target)
    out = blk.forward_steps(x).cpu()
    assert out.shape == target.shape
    check_parity(out, target)


def test_stack_of_three_blocks():
    """tests/test_cost_gcn.py:274-326"""
    a, sd = load_golden("g4_stack")
    blocks = [pkg.CoSpatioTemporalBlock(3, 3, A, residual=False, padding=4), pkg.CoSpatioTemporalBlock(3, 3, A, padding=4),
              pkg.CoSpatioTemporalBlock(3, 4, A, stride=2, padding=4)]
    h1 = h2 = torch.from_numpy(a["x"]).to(DEV)
    for i, b in enumerate(blocks):
        b.load_state_dict({k[2:]: v for k, v in sd.items() if k.startswith(f"{i}.")}, strict=True)
        b = b.eval().to(DEV)
        h1 = b.forward(h1)
        h2 = b.forward_steps(h2, pad_end=True)
    check_parity(h1.cpu(), a["y"], note="forward")
    check_parity(h2.cpu(), a["y"], note="forward_steps pad_end")


def test_clean_state_and_restart():
    blk, x, target, _ = _co_block("ident")
    first = blk.forward_steps(x).cpu()
    blk.clean_state()
    again = blk.forward_steps(x).cpu()
    assert torch.equal(first, again)
    blk.forward_steps(x[:, :, :7].contiguous())        # leave dirty state, different history
    blk.clean_state()
    assert torch.equal(blk.forward_steps(x).cpu(), first)


def test_costgcn_features_equal_clip_features_at_shifted_index():
    """Layer-10 emission j (input frame 76 + 4j) == clip layer-10 frame j (the whole-stack form of the block
    identity; the clip side is pinned by fixture G6)."""
    a, sd, x = g6_state_dict("ntu")
    reg = pkg.StGcn(A).eval()
    reg.load_state_dict(sd, strict=True)
    co = pkg.CoStGcn(A).eval()
    co.load_state_dict(sd, strict=True)
    reg, co, x = reg.to(DEV), co.to(DEV), x[:1].to(DEV)
    clip_feat = reg.features(x)                                          # (M, 256, 75, 25)
    T = 76 + 4 * 6 + 1
    got = []
    for t in range(T):
        slot = co.features_step(x[:, :, t].contiguous())
        assert (slot is not None) == (t >= 76 and (t - 76) % 4 == 0)
        if slot is not None:
            st = co.layers["layer10"]._state
            got.append(st.out[slot, :, : 2 * 25].view(256, 2, 25).permute(1, 0, 2).clone())
    assert len(got) == 7
    for j, g in enumerate(got):
        check_parity(g.cpu(), clip_feat[:, :, j].cpu(), note=j)


def test_costgcn_logits_vs_oracle_and_forward_modes():
    """Whole CoST-GCN stepping (data_bn, 10 blocks, spatial pool, temporal average pool, fc) vs the CPU oracle,
    with a small pool so that predictions appear early; and forward('clip') == forward('frame') like
    tests/test_cost_gcn.py:359-362."""
    a, sd, x = g6_state_dict("ntu")
    x = x[:1, :, :120].contiguous()
    co = pkg.CoStGcn(A, pool_size=6, pool_padding=2).eval()
    co.load_state_dict(sd, strict=True)
    co = co.to(DEV)
    got = co.forward_steps(x.to(DEV)).cpu()                              # (1, 60, n_pred)
    orc = o.CoStGcnOracle(sd, pool_size=6, pool_padding=2)
    want = []
    with torch.no_grad():
        for t in range(x.shape[2]):
            r = orc.forward_step(x[:, :, t])
            if r is not None:
                want.append(r)
    want = torch.stack(want, dim=2)
    assert got.shape == want.shape and got.shape[2] >= 5
    check_parity(got, want)
    # default pool (75 / 19): after exactly T=300 frames one prediction exists and equals the clip-mode forward
    a, sd, x = g6_state_dict("ntu")
    co = pkg.CoStGcn(A).eval()
    co.load_state_dict(sd, strict=True)
    co = co.to(DEV)
    xd = x[:1].to(DEV)
    frame = co.forward(xd, forward_mode="frame").cpu()
    clip = co.forward(xd, forward_mode="clip").cpu()
    assert frame.shape == (1, 60)
    check_parity(frame, clip)


def test_costgcn_top3_equals_stgcn_default_init_default_pool():
    """Mirror of the reference's one model-level pin, its tests/test_cost_gcn.py:329-362: StGcn and CoStGcn
    with the constructors' DEFAULT initialisation (gcn.bn.weight = 1e-6, base.py:257) and the DEFAULT pool (75 / 19),
    weights transferred with ``co.load_state_dict(co.map_state_dict(reg.state_dict()))``; on a dummy_ntu sample
    (torch.rand, datasets/datasets.py:301) the top-3 classes of ``reg(sample)``, ``co.forward(sample)`` and
    ``co.forward_steps(sample)`` agree, and forward ~ forward_steps (rtol 1e-4)."""
    torch.manual_seed(42)
    reg = pkg.StGcn(A).eval()
    co = pkg.CoStGcn(A).eval()
    co.load_state_dict(co.map_state_dict(reg.state_dict()), strict=False)
    assert (co.pool_size, co.pool_padding) == (75, 19)
    reg, co = reg.to(DEV), co.to(DEV)
    sample = torch.rand((1, 3, 300, 25, 2), generator=torch.Generator().manual_seed(0)).to(DEV)
    target = reg(sample)
    ks = 3
    target_inds = torch.topk(target, ks).indices
    o_co1 = co.forward(sample)
    assert torch.equal(target_inds, torch.topk(o_co1, ks).indices)
    o_co2 = co.forward_steps(sample)
    assert o_co2.shape == (1, 60, 1)               # T = 300 frames -> exactly one prediction with the default pool
    o_co2 = o_co2.squeeze(-1)                      # the reference's trailing ``squeeze`` module (base.py:99-101)
    assert torch.equal(target_inds, torch.topk(o_co2, ks).indices)
    # the reference asserts allclose(rtol=1e-4) with torch's default atol = 1e-8; the logits are sums of O(10) terms, so an
    # entry that cancels to ~ 4e-3 carries the ~ 3e-6 absolute rounding difference of two fp32 evaluation orders (clip-form
    # pooling vs the continual window mean) as a 3e-4 RELATIVE one.  atol = 1e-5 here; the absolute 1e-4 bound of the
    # north star is asserted (and its margin recorded) by check_parity right below.
    assert torch.allclose(o_co1, o_co2, rtol=1e-4, atol=1e-5)
    check_parity(o_co2.cpu(), o_co1.cpu(), ref_cap=32.0, note="forward_steps vs forward, default init / pool")
    # and the oracle agrees with all three on the same weights
    sd = {k: v.cpu() for k, v in reg.state_dict().items()}
    with torch.no_grad():
        check_parity(target.cpu(), o.stgcn_forward(sample.cpu(), sd), ref_cap=32.0, note="StGcn default init vs oracle")


@pytest.mark.parametrize("native_plan", [True, False])
def test_model_forward_steps_pad_end(native_plan):
    """CoModelBase.forward_steps(x, pad_end=True) (models/base.py:187-190): flushing every block turns the stack into
    the 'same'-padded clip stack and the pooling window gets its end padding -- the predictions must equal the
    clip-form evaluation (oracle.co_stgcn_steps_pad_end: clip features, AvgPool1d with symmetric zero padding, fc);
    update_state=False leaves the state where it was."""
    a, sd, x = g6_state_dict("ntu")
    x = x[:1, :, :64].contiguous()
    co = pkg.CoStGcn(A, pool_size=6, pool_padding=2).eval()
    co.use_native_plan = native_plan
    co.load_state_dict(sd, strict=True)
    co = co.to(DEV)
    with torch.no_grad():
        want = o.co_stgcn_steps_pad_end(x, sd, 6, 2)                     # (1, 60, 16 + 4 - 6 + 1)
    peek = co.forward_steps(x.to(DEV), pad_end=True, update_state=False).cpu()
    got = co.forward_steps(x.to(DEV), pad_end=True).cpu()
    assert got.shape == want.shape == (1, 60, 15)
    check_parity(got, want)
    assert torch.equal(peek, got)                                        # the peek ran from the same (clean) state


def test_forward_cycle_equals_per_frame_stepping():
    """Batching the frames of a stride cycle into one launch per block must not change a single bit, for
    aligned cycles of 4 and 8 (the longest a launch takes), ragged cycle lengths and cycles that wrap the ring
    buffers."""
    a, sd, x = g6_state_dict("ntu")
    x = x[:1, :, :130].to(DEV)
    ref = pkg.CoStGcn(A, pool_size=5, pool_padding=1).eval()
    ref.load_state_dict(sd, strict=True)
    ref = ref.to(DEV)
    want = [o for o in (ref.forward_step(x[:, :, t].contiguous()) for t in range(x.shape[2])) if o is not None]
    for pattern in ([4], [3, 4, 1, 2], [1, 4, 4, 3], [8], [7, 8, 5, 8, 6, 2]):
        co = pkg.CoStGcn(A, pool_size=5, pool_padding=1).eval()
        co.load_state_dict(sd, strict=True)
        co = co.to(DEV)
        got, t, i = [], 0, 0
        while t < x.shape[2]:
            r = min(pattern[i % len(pattern)], x.shape[2] - t)
            got += co.forward_cycle([x[:, :, t + f].contiguous() for f in range(r)])
            t, i = t + r, i + 1
        assert len(got) == len(want) and len(want) >= 8
        assert all(torch.equal(g, w) for g, w in zip(got, want)), pattern


def test_native_plan_equals_python_engine_and_survives_weight_reload():
    """The C++ step executor (csk_co_plan_*) and the Python-driven engine issue the same launches: bitwise equal
    predictions; reloading weights mid-stream keeps the continual state (as in the reference, where weights and
    state buffers are independent) on both paths."""
    a, sd, x = g6_state_dict("ntu")
    x = x[:2, :, :140].to(DEV)
    sd2 = {k: (v * 1.01 if v.dtype.is_floating_point and "running_var" not in k and k.split(".")[-1] != "A" else v)
           for k, v in sd.items()}
    outs = {}
    for native_plan in (True, False):
        co = pkg.CoStGcn(A, pool_size=4, pool_padding=1).eval()
        co.use_native_plan = native_plan
        co.load_state_dict(sd, strict=True)
        co = co.to(DEV)
        got = []
        for t in range(0, 140, 4):
            if t == 100:
                co.load_state_dict(sd2, strict=True)
            got += co.forward_cycle([x[:, :, t + f].contiguous() for f in range(4)])
        assert (co.__dict__.get("_plan") is not None) == native_plan
        outs[native_plan] = got
    assert len(outs[True]) == len(outs[False]) >= 10
    assert all(torch.equal(p, q) for p, q in zip(outs[True], outs[False]))


@pytest.mark.parametrize("edit", ["replace_parameter", "swap_submodule", "in_place", "data_assign"])
def test_native_plan_sees_every_kind_of_weight_edit_at_once(edit):
    """The native plan's operands are refolded on the FIRST cycle after a weight edit that no hook can see: a replaced
    Parameter object, a swapped sub-module, an in-place edit, ``p.data = ...``.  After the edit the native plan and the
    Python engine (which refolds from the live modules on every launch) must agree bitwise on every later prediction,
    and the predictions must differ from those of the unedited weights."""
    a, sd, x = g6_state_dict("ntu")
    x = x[:2, :, :120].to(DEV)
    outs = {}
    for native_plan, edited in ((True, True), (False, True), (True, False)):
        co = pkg.CoStGcn(A, pool_size=4, pool_padding=1).eval()
        co.use_native_plan = native_plan
        co.load_state_dict(sd, strict=True)
        co = co.to(DEV)
        got = []
        for t in range(0, 120, 4):
            if t == 96 and edited:
                with torch.no_grad():
                    if edit == "replace_parameter":
                        co.fc.weight = torch.nn.Parameter(co.fc.weight.detach() * 1.5)
                    elif edit == "swap_submodule":
                        old = co.layers["layer3"].tcn.bn
                        new = torch.nn.BatchNorm2d(old.num_features).to(DEV).eval()
                        new.load_state_dict({k: (v * 1.25 if k == "weight" else v) for k, v in old.state_dict().items()})
                        co.layers["layer3"].tcn.bn = new
                    elif edit == "in_place":
                        co.fc.bias.add_(0.5)
                    else:
                        co.layers["layer10"].tcn.t_conv.weight.data = co.layers["layer10"].tcn.t_conv.weight.data * 1.25
            got += co.forward_cycle([x[:, :, t + f].contiguous() for f in range(4)])
        outs[(native_plan, edited)] = got
    nat, py, plain = outs[(True, True)], outs[(False, True)], outs[(True, False)]
    assert len(nat) == len(py) == len(plain) >= 8
    assert all(torch.equal(p, q) for p, q in zip(nat, py))
    assert torch.equal(nat[0], plain[0]) and not torch.equal(nat[-1], plain[-1])      # the edit took effect


class _ForeignGraphConv(torch.nn.Module):
    """A graph conv the package knows nothing about (stands for the spatial-attention module S-TR passes as
    ``GraphConv`` / ``CoGraphConv``, models/base.py:338-349,390-400): plain PyTorch ops, no ``stage`` method."""

    def __init__(self, in_channels, out_channels, A, bn_momentum=0.1):
        super().__init__()
        self.mix = torch.nn.Conv2d(in_channels, out_channels, 1)
        self.register_buffer("A", torch.as_tensor(A, dtype=torch.float32).sum(0))

    def forward(self, x):                                            # (N, C, T, V) -> (N, C_out, T, V)
        return torch.relu(torch.matmul(self.mix(x), self.A))


def _foreign_gcn_oracle(x, sd, p=""):                                # p = "<block prefix>gcn." as the oracle's block passes it
    y = torch.nn.functional.conv2d(x, sd[p + "mix.weight"], sd[p + "mix.bias"])
    return torch.relu(torch.matmul(y, sd[p + "A"]))


@pytest.mark.parametrize("ci,co,stride", [(6, 6, 1), (4, 8, 2)])
def test_blocks_accept_a_foreign_graph_conv_module(ci, co, stride):
    """the blocks take arbitrary graph-conv factories.  Clip: module output feeds the fused TCN stage;
    continual: the module is applied per frame on tensors converted from / to the ring slots; both vs the oracle."""
    torch.manual_seed(5)
    blk = pkg.SpatioTemporalBlock(ci, co, A, stride=stride, GraphConv=_ForeignGraphConv).eval()
    for name, buf in blk.named_buffers():
        if name.endswith("running_var"):
            buf.uniform_(0.5, 1.5)
        elif name.endswith("running_mean"):
            buf.uniform_(-0.5, 0.5)
    sd = {k: v.clone() for k, v in blk.state_dict().items()}
    x = torch.rand(3, ci, 21, 25)
    with torch.no_grad():
        want = o.st_block(x, sd, "", stride, True, gcn=_foreign_gcn_oracle)
    got = blk.to(DEV)(x.to(DEV)).cpu()
    assert got.shape == want.shape
    check_parity(got, want)
    co_blk = pkg.CoSpatioTemporalBlock(ci, co, A, stride=stride, padding=4, CoGraphConv=_ForeignGraphConv).eval()
    co_blk.load_state_dict(sd, strict=True)
    steps = co_blk.to(DEV).forward_steps(x.to(DEV), pad_end=True).cpu()
    assert steps.shape == want.shape
    check_parity(steps, want)


def test_update_state_false_peeks_without_advancing():
    """forward_step / forward_steps(update_state=False) (models/base.py:183-190 pass the flag through): the output
    equals what the real step produces, and a stream that was peeked at continues exactly -- bit for bit -- like a
    twin that never was.  Block level, model level on the native executor and on the Python engine."""
    a, sd, x = g6_state_dict("ntu")
    x = x[:2, :, :120].to(DEV)
    for native_plan in (True, False):
        twins = []
        for _ in range(2):
            co = pkg.CoStGcn(A, pool_size=4, pool_padding=1).eval()
            co.use_native_plan = native_plan
            co.load_state_dict(sd, strict=True)
            twins.append(co.to(DEV))
        peeker, plain = twins
        for t in range(120):
            f = x[:, :, t].contiguous()
            if t in (0, 3, 50, 83, 84, 100):
                p1 = peeker.forward_step(f, update_state=False)
                p2 = peeker.forward_step(f, update_state=False)            # peeking twice changes nothing either
                assert (p1 is None) == (p2 is None) and (p1 is None or torch.equal(p1, p2))
            if t == 90:                                                      # a multi-frame peek (copies the slab)
                ahead = peeker.forward_steps(x[:, :, 90:110].contiguous(), update_state=False)
                assert ahead.shape[2] == 5                                   # predictions at frames 92, 96, ..., 108
            got, want = peeker.forward_step(f), plain.forward_step(f)
            assert (got is None) == (want is None)
            if want is not None:
                assert torch.equal(got, want), (native_plan, t)
                if t in (83, 84, 100) and p1 is not None:
                    assert torch.equal(p1, want)
            if t == 108:
                assert torch.equal(ahead[:, :, -1], want)                   # the look-ahead saw the same prediction
    # block level (identity residual, stride 1) and the bare continual temporal conv
    blk = pkg.CoSpatioTemporalBlock(6, 6, A, padding=4).eval().to(DEV)
    twin = pkg.CoSpatioTemporalBlock(6, 6, A, padding=4).eval()
    twin.load_state_dict(blk.state_dict(), strict=True)
    twin = twin.to(DEV)
    tc = pkg.CoTemporalConvolution(6, 6, padding="equal").eval().to(DEV)
    tc_twin = pkg.CoTemporalConvolution(6, 6, padding="equal").eval()
    tc_twin.load_state_dict(tc.state_dict(), strict=True)
    tc_twin = tc_twin.to(DEV)
    xb = torch.rand(3, 6, 30, 25, device=DEV)
    for m, tw in ((blk, twin), (tc, tc_twin)):
        for t in range(30):
            f = xb[:, :, t].contiguous()
            peek = m.forward_step(f, update_state=False)
            if t == 12:
                m.forward_steps(xb[:, :, 12:26].contiguous(), update_state=False)
            got, want = m.forward_step(f), tw.forward_step(f)
            assert (got is None) == (want is None) == (peek is None)
            if want is not None:
                assert torch.equal(got, want) and torch.equal(peek, want), t


@pytest.mark.parametrize("pad_end", [False, True])
@pytest.mark.parametrize("kind", ["conv", "block"])
def test_multi_frame_peek_restores_rings_and_counters_bitwise(kind, pad_end):
    """forward_steps(update_state=False) of the bare continual temporal conv and of a stand-alone block (4 -> 8 channels,
    stride 2, conv residual), from a state 5 frames in: every ring and counter is afterwards bit for bit what it was, and the
    output is what the same call with update_state=True returns from that state."""
    if kind == "conv":
        m = pkg.CoTemporalConvolution(4, 8, padding="equal", stride=2).eval().to(DEV)
    else:
        m = pkg.CoSpatioTemporalBlock(4, 8, A, stride=2, padding="equal").eval().to(DEV)

    def state():
        if kind == "conv":
            return [m._ring.clone()], m._s
        st = m._state
        return [st.y.clone(), st.out.clone(), st.xin.clone()], (st.s, st.e)

    x = torch.rand(1, 4, 17, 25, device=DEV)
    m.forward_steps(x[:, :, :5].contiguous())
    rings, counters = state()
    assert counters in (5, (5, 1))
    peek = m.forward_steps(x[:, :, 5:].contiguous(), pad_end=pad_end, update_state=False)
    rings_after, counters_after = state()
    assert counters_after == counters and all(torch.equal(a, b) for a, b in zip(rings, rings_after))
    real = m.forward_steps(x[:, :, 5:].contiguous(), pad_end=pad_end)
    assert peek.shape[2] == (8 if pad_end else 6) and torch.equal(peek, real)
    assert state()[1] != counters and not all(torch.equal(a, b) for a, b in zip(rings, state()[0]))     # the real run moved both


@pytest.mark.parametrize("native_plan", [True, False])
def test_latency_mode_split_k_matches_oracle_and_default(native_plan):
    """set_latency_mode (split-K in the TCN steps for a handful of streams): same predictions as the oracle and as
    the default path up to fp32 summation order; per-frame stepping and 4-frame cycles stay bitwise equal to each
    other; the split factor does not depend on the slab size (a stream alone == the same stream in a larger slab, bitwise)."""
    a, sd, x = g6_state_dict("ntu")
    T = 160
    x = x[:2, :, :T].to(DEV)
    nets = {}
    for mode in ("default", "latency", "latency_cycles"):
        co = pkg.CoStGcn(A, pool_size=4, pool_padding=1).eval()
        co.use_native_plan = native_plan
        co.load_state_dict(sd, strict=True)
        co = co.to(DEV)
        if mode != "default":
            co.set_latency_mode(8)
        nets[mode] = co
    outs = {m: [] for m in nets}
    for t in range(T):
        f = x[:, :, t].contiguous()
        for m in ("default", "latency"):
            r = nets[m].forward_step(f)
            if r is not None:
                outs[m].append(r)
    for t in range(0, T, 4):
        outs["latency_cycles"] += nets["latency_cycles"].forward_cycle([x[:, :, t + f].contiguous() for f in range(4)])
    assert len(outs["default"]) == len(outs["latency"]) == len(outs["latency_cycles"]) >= 18
    # default: nothing is split (the slot-balanced tiles of csrc/step16.hip pack the 256-channel launches without it;
    # rounds 2-5 cut their K loop in 3)
    assert [nets["default"].layers[f"layer{i + 1}"]._state.ksplit for i in range(10)] == [1] * 10
    assert nets["latency"].layers["layer9"]._state.ksplit > 3 and nets["latency"].layers["layer2"]._state.ksplit > 1
    # ... and the graph convs split theirs too (csk_gcn_stage_splitk_f32); layer 1 (3 input channels) has nothing to split
    assert [nets["default"].layers[f"layer{i + 1}"]._state.gcn_ksplit for i in range(10)] == [1] * 10
    assert nets["latency"].layers["layer1"]._state.gcn_ksplit == 1 and nets["latency"].layers["layer9"]._state.gcn_ksplit >= 8
    for d, l, c in zip(outs["default"], outs["latency"], outs["latency_cycles"]):
        check_parity(l.cpu(), d.cpu(), note="latency mode vs default (summation order)")
        assert torch.equal(l, c)                                # 4-frame cycles: bit-identical to per-frame stepping
    orc = o.CoStGcnOracle(sd, pool_size=4, pool_padding=1)
    want = [r for r in (orc.forward_step(x[:, :, t].cpu()) for t in range(120)) if r is not None]
    for l, w in zip(outs["latency"], want):
        check_parity(l.cpu(), w, note="latency mode vs oracle")
    # the split factor is a function of the layer only, never of the slab: a stream's predictions in latency mode are BITWISE
    # the same alone and among 46 other streams (until round 4 the factor shrank with the slab and they differed)
    small, big = [pkg.CoStGcn(A, pool_size=2, pool_padding=0).eval() for _ in range(2)]
    for b in (small, big):
        b.use_native_plan = native_plan
        b.load_state_dict(sd, strict=True)
    small, big = small.to(DEV), big.to(DEV)
    small.set_latency_mode(8)
    big.set_latency_mode(8)
    frames = torch.rand((88, 48, 3, 25, 2), device=DEV)
    seen = 0
    for t in range(88):
        r0, r1 = small.forward_step(frames[t, :2].contiguous()), big.forward_step(frames[t])
        assert (r0 is None) == (r1 is None)
        if r0 is not None:
            assert torch.equal(r0, r1[:2])
            seen += 1
    assert seen > 0
    assert all(big.layers[f"layer{i + 1}"]._state.ksplit == small.layers[f"layer{i + 1}"]._state.ksplit for i in range(10))
    assert all(big.layers[f"layer{i + 1}"]._state.gcn_ksplit == small.layers[f"layer{i + 1}"]._state.gcn_ksplit for i in range(10))
    assert big.layers["layer9"]._state.ksplit == 32 and big.layers["layer6"]._state.ksplit == 16 and big.layers["layer2"]._state.ksplit == 8


def _set_fusion(model, on):
    for i in range(10):
        model.layers[f"layer{i + 1}"].fuse_step = on
    model._n = None                                  # re-bind (the native plan reads the flag when it is built)


@pytest.mark.parametrize("graph,n", [("ntu", 5), ("kinetics", 3)])
@pytest.mark.parametrize("native_plan", [True, False])
def test_fused_block_step_equals_two_launch_form(graph, n, native_plan):
    """csk_co_block_step_f32 (GCN stage + TCN step of a block in one launch; layers 1-4 of the stack) against the
    two-launch form: logits AND every state ring bit-identical over many 4-frame cycles; ragged position counts
    (5 streams x 2 x 25 = 250, 3 x 2 x 18 = 108)."""
    A_ = (pkg.ntu_graph() if graph == "ntu" else pkg.kinetics_graph()).A
    v = A_.shape[-1]
    torch.manual_seed(3)
    fused = pkg.CoStGcn(A_, input_shape=(3, 300, v, 2), pool_size=3, pool_padding=1).eval()
    plain = pkg.CoStGcn(A_, input_shape=(3, 300, v, 2), pool_size=3, pool_padding=1).eval()
    import bench
    bench.randomise_(fused, 5)
    plain.load_state_dict(fused.state_dict())
    fused.use_native_plan = plain.use_native_plan = native_plan
    _set_fusion(fused, True)
    _set_fusion(plain, False)
    fused, plain = fused.to(DEV), plain.to(DEV)
    frames = torch.rand((4 * 26, n, 3, v, 2), generator=torch.Generator().manual_seed(9)).to(DEV)
    n_pred = 0
    for c in range(26):
        fr = [frames[4 * c + f] for f in range(4)]
        a, b = fused.forward_cycle(fr), plain.forward_cycle(fr)
        assert len(a) == len(b)
        for la, lb in zip(a, b):
            assert torch.equal(la, lb)
            n_pred += 1
        for i in (1, 2, 3, 4):
            sa, sb = fused.layers[f"layer{i}"]._state, plain.layers[f"layer{i}"]._state
            assert torch.equal(sa.y, sb.y) and torch.equal(sa.out, sb.out), (c, i)
    assert n_pred >= 3


@pytest.mark.parametrize("ci,co,res", [(4, 4, True), (6, 6, False), (3, 8, False), (64, 64, True)])
def test_fused_block_step_small_and_ragged_channels(ci, co, res):
    """Block level, channel counts below the 64-row tile (general epilogue path) and a conv gcn_residual: engine_advance
    of a whole cycle, fused against unfused, rings bit-identical; 7 skeletons (P = 176 of 175 positions)."""
    torch.manual_seed(1)
    a = pkg.CoSpatioTemporalBlock(ci, co, A, residual=res, padding="equal").eval()
    import bench
    bench.randomise_(a, 2)
    b = pkg.CoSpatioTemporalBlock(ci, co, A, residual=res, padding="equal").eval()
    b.load_state_dict(a.state_dict())
    a, b = a.to(DEV), b.to(DEV)
    a.fuse_step, b.fuse_step = True, False
    n_skel, p = 7, 176
    sa, sb = a.bind_state(p, torch.device(DEV)), b.bind_state(p, torch.device(DEV))
    g = torch.Generator().manual_seed(4)
    for cyc in range(9):
        x = torch.rand((4, ci, p), generator=g).to(DEV)
        for st in (sa, sb):
            for f in range(4):
                st.xin[(st.s + f) % st.xin.shape[0]] = x[f]
        ra, rb = a.engine_advance(4, n_skel, 25), b.engine_advance(4, n_skel, 25)
        assert ra == rb
        assert torch.equal(sa.y, sb.y) and torch.equal(sa.out, sb.out), cyc
    assert ra is not None and ra[1] == 4


@pytest.mark.parametrize("n,c,mv,classes,window", [(5, 256, 50, 60, 7), (3, 256, 36, 400, 4), (2, 70, 50, 11, 3)])
def test_fused_head_equals_the_three_launches_bitwise(n, c, mv, classes, window):
    """csk_co_head_step_f32 (spatial pool + pooling-window mean + FC in one launch) against csk_co_spatial_pool_f32 ->
    csk_co_window_mean_f32 -> csk_fc_f32, the launches it replaces (models/base.py:84-101): identical bits for the ring
    entry, the pooled features and the logits, on filling (count < window), full and wrapped windows, and on a zero
    feature (end padding)."""
    from continual_skeletons_amd import native
    lib = native.lib()
    g = torch.Generator().manual_seed(n * 100 + c)
    P = (n * mv + 3) // 4 * 4
    w = (torch.rand((classes, c), generator=g) - 0.5).to(DEV)
    b = (torch.rand((classes,), generator=g) - 0.5).to(DEV)
    ring_a = torch.zeros((window, n, c), device=DEV)
    ring_b = torch.zeros((window, n, c), device=DEV)
    stream = native.stream_of(w)
    for step in range(2 * window + 3):
        h = torch.rand((c, P), generator=g).to(DEV) if step != window + 1 else None          # one zero feature on the way
        head, count = step % window, min(step + 1, window)
        if h is None:
            ring_a[head].zero_()
        else:
            native.check(lib.csk_co_spatial_pool_f32(native.ptr(h), native.ptr(ring_a[head]), n, c, mv, P, stream), "pool")
        pooled_a = torch.empty((n, c), device=DEV)
        native.check(lib.csk_co_window_mean_f32(native.ptr(ring_a), native.ptr(pooled_a), n * c, window, head, count, stream), "mean")
        logits_a = torch.empty((n, classes), device=DEV)
        if c % 4 == 0:
            native.check(lib.csk_fc_f32(native.ptr(pooled_a), native.ptr(w), native.ptr(b), native.ptr(logits_a), n, c, classes, stream), "fc")
        else:                                   # csk_fc_f32's scalar path has no alignment demands either
            native.check(lib.csk_fc_f32(native.ptr(pooled_a), native.ptr(w), native.ptr(b), native.ptr(logits_a), n, c, classes, stream), "fc")
        pooled_b, logits_b = torch.empty((n, c), device=DEV), torch.empty((n, classes), device=DEV)
        native.check(lib.csk_co_head_step_f32(native.ptr(h), native.ptr(ring_b), native.ptr(pooled_b), native.ptr(w), native.ptr(b),
                                              native.ptr(logits_b), n, c, mv, P, window, head, count, 1, classes, stream), "head")
        assert torch.equal(ring_a, ring_b) and torch.equal(pooled_a, pooled_b) and torch.equal(logits_a, logits_b), step


def test_max_cycle_4_slab_is_smaller_and_bitwise_the_same():
    """CoStGcn.set_max_cycle(4): rings sized for 4-frame cycles (what bench.py's online leg issues) instead of 8 -- the same
    predictions bit for bit, a smaller slab, cycles of 5 frames refused (Python and plan)."""
    a, sd, x = g6_state_dict("ntu")
    x = x[:2, :, :160].to(DEV)
    big = pkg.CoStGcn(A, pool_size=4, pool_padding=1).eval()
    small = pkg.CoStGcn(A, pool_size=4, pool_padding=1).eval()
    for m in (big, small):
        m.load_state_dict(sd, strict=True)
    small.set_max_cycle(4)
    big, small = big.to(DEV), small.to(DEV)
    got, want = [], []
    for t in range(0, 160, 4):
        fr = [x[:, :, t + f].contiguous() for f in range(4)]
        want += big.forward_cycle(fr)
        got += small.forward_cycle(fr)
    assert len(got) == len(want) >= 18 and all(torch.equal(g, w) for g, w in zip(got, want))
    assert small.state_bytes() < 0.85 * big.state_bytes()           # 19 % smaller
    assert small.layers["layer1"]._state.y.shape[0] == 12 and big.layers["layer1"]._state.y.shape[0] == 16
    with pytest.raises(ValueError, match="1..4 frames"):
        small.forward_cycle([x[:, :, f].contiguous() for f in range(5)])
    with pytest.raises(ValueError):
        small.set_max_cycle(9)


def _twins(count, native_plan, latency=False, pool=(4, 1)):
    """``count`` CoST-GCNs with the G6 weights; element i steps on the native plan where native_plan[i]."""
    a, sd, x = g6_state_dict("ntu")
    nets = []
    for i in range(count):
        co = pkg.CoStGcn(A, pool_size=pool[0], pool_padding=pool[1]).eval()
        co.use_native_plan = native_plan[i]
        co.load_state_dict(sd, strict=True)
        co = co.to(DEV)
        if latency:
            co.set_latency_mode(8)
        nets.append(co)
    return nets, x


def _block_counters(net):
    return [(net.layers[f"layer{i + 1}"]._state.s, net.layers[f"layer{i + 1}"]._state.e) for i in range(10)]


@pytest.mark.parametrize("latency", [False, True])
def test_plan_and_python_engine_interleave_on_one_counter_store(latency):
    """The stepping position has ONE store (CoStGcn._ctr; the blocks' s / e and the plan's ``counters`` argument are that
    buffer), so the native plan and the Python engine may take turns: a model whose ``use_native_plan`` flips on every
    4-frame cycle equals -- logits, every state tensor and the counters, bit for bit after every cycle -- a twin that runs
    the plan only and one that runs the Python engine only.  120 frames: the first prediction falls at frame 84 and the
    16-slot y ring of layer 1 wraps seven times."""
    (mixed, plan, py), x = _twins(3, (True, True, False), latency)
    x = x[:2, :, :120].to(DEV)
    n_pred = 0
    for c in range(30):
        fr = [x[:, :, 4 * c + f].contiguous() for f in range(4)]
        mixed.use_native_plan = c % 2 == 0
        outs = [net.forward_cycle(fr) for net in (mixed, plan, py)]
        assert len(outs[0]) == len(outs[1]) == len(outs[2])
        for lm, lp, ly in zip(*outs):
            assert torch.equal(lm, lp) and torch.equal(lm, ly), c
            n_pred += 1
        assert mixed._counters() == plan._counters() == py._counters(), c
        assert _block_counters(mixed) == _block_counters(plan) == _block_counters(py), c
        for i, (tm, tp, ty) in enumerate(zip(mixed._state_tensors(), plan._state_tensors(), py._state_tensors())):
            if n_pred or tm is not mixed._pooled:          # _pooled is torch.empty until the first prediction writes it
                assert torch.equal(tm, tp) and torch.equal(tm, ty), (c, i)
    assert n_pred == 9 and mixed._counters()[:4] == [120, 11, 120, 116]
    assert mixed.__dict__.get("_plan") and plan.__dict__.get("_plan") and not py.__dict__.get("_plan")
    assert plan.layers["layer9"]._state.ksplit == (32 if latency else 1)


def test_failed_plan_cycle_leaves_no_trace():
    """csk_co_plan_cycle works on a copy of the caller's counters and stores it back only when every launch of the cycle was
    issued.  A second plan over the SAME rings whose layer 2 claims a split-K scratch for one graph-conv frame refuses a
    2-frame cycle on the host, after the input norm and layer 1 were launched: non-zero return, the counters it was given
    unchanged.  The model then takes the same two frames (rewriting the slots the failed call touched) and goes on bitwise
    like a twin that never saw the failed call."""
    import ctypes
    native = pkg.native
    lib = native.lib()
    (net, twin), x = _twins(2, (True, True), latency=True)
    x = x[:2, :, :120].to(DEV)
    cycles = [[x[:, :, 2 * c + f].contiguous() for f in range(2)] for c in range(60)]
    for fr in cycles[:20]:
        assert net.forward_cycle(fr) == twin.forward_cycle(fr) == []
    assert net.layers["layer2"]._state.gcn_ksplit > 1
    arr, keep, ops, fcw, fcb = net._layer_structs(torch.device(DEV))
    arr[1].gcn_partial_frames = 1
    plan2 = lib.csk_co_plan_create(10, ctypes.byref(arr), native.ptr(net._xin0), net._xin0.shape[0], net._n, 3, 25, 2, net._p,
                                   native.ptr(ops["scale"]), native.ptr(ops["shift"]), 60, native.ptr(fcw), native.ptr(fcb),
                                   net.pool_size, net.pool_padding, native.ptr(net._pool_ring), native.ptr(net._pooled))
    assert plan2, lib.csk_last_error()
    before = net._counters()
    assert before[:6] == [40, 0, 40, 36, 36, 32]
    buf = (ctypes.c_int64 * 22)(*before)
    ptrs = (ctypes.c_void_p * 2)(*[f.data_ptr() for f in cycles[20]])
    logits = torch.empty((8, 2, 60), device=DEV)
    slot, nf, nl = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = lib.csk_co_plan_cycle(ctypes.c_void_p(plan2), buf, 22, ptrs, 2, native.ptr(logits), ctypes.byref(slot), ctypes.byref(nf),
                               ctypes.byref(nl), native.stream_of(logits))
    msg = lib.csk_last_error()
    lib.csk_co_plan_destroy(ctypes.c_void_p(plan2))
    assert rc != 0 and b"exceed the split-K scratch" in msg, (rc, msg)
    assert all(buf[i] == before[i] for i in range(22)) and net._counters() == before
    n_pred = 0
    for c, fr in enumerate(cycles[20:]):
        got, want = net.forward_cycle(fr), twin.forward_cycle(fr)
        assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want)), c
        n_pred += len(got)
        assert net._counters() == twin._counters(), c
    assert n_pred == 9
    for tn, tt in zip(net._state_tensors(), twin._state_tensors()):
        assert torch.equal(tn, tt)


def test_peeking_at_a_plan_driven_model_leaves_every_counter_where_it_was():
    """update_state=False on a model the native plan drives: after ``forward_step`` and after ``forward_steps(pad_end=True)``
    -- whose flush runs on the Python engine -- the counter buffer equals its value before the call, and every block's
    s / e is what a Python-engine twin holds at the same point (with a copy of the counters inside the plan, the blocks of
    a plan-driven model read 0 here)."""
    (net, py), x = _twins(2, (True, False))
    x = x[:2, :, :130].to(DEV)
    for t in range(110):
        f = x[:, :, t].contiguous()
        if t in (3, 50, 90):
            before = net._counters()
            net.forward_step(f, update_state=False)
            assert net._counters() == before and _block_counters(net) == _block_counters(py), t
            ahead = net.forward_steps(x[:, :, t:t + 20].contiguous(), pad_end=True, update_state=False)
            assert ahead.shape[:2] == (2, 60) and not net._flushed
            assert net._counters() == before and _block_counters(net) == _block_counters(py), t
            assert before[0] == t and before[2:4] == [t, max(0, t - 4)]
        got, want = net.forward_step(f), py.forward_step(f)
        assert (got is None) == (want is None) and (want is None or torch.equal(got, want)), t
    assert net.__dict__.get("_plan") and not py.__dict__.get("_plan")
