"""S-TR / CoS-TR hardening: csk_str_unit_f32 (through GcnUnitAttention.stage, explicit strides) against the fp64 recomputation
from its own folded operands (tests/str_oracle.folded_unit) over a seeded sweep of channel pairs, tile shapes and layouts;
bitwise position invariance of a segment and of a frame; softmax beyond the fp32 expf range, uniform attention, NaN
containment; and the continual behaviour of CoSTr (stream counts, cycles, peeking, restart, a stride-2 block, hipGraph capture
of the default clip mode).  Tolerance 1e-4 absolute (tests/helpers.check_parity) on O(1) fixtures throughout."""
import pytest
import torch

import _bootstrap
from oracle import stgcn_oracle as o
from tests import str_oracle as so
from tests.helpers import TOL, check_parity, max_err, model_fixture, randomise_unit_

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
DEV = "cuda:0"
NAN = float("nan")
PAD = 1 << 14


def _graph(v):
    return pkg.ntu_graph().A if v == 25 else pkg.kinetics_graph().A


def _unit(ci, co, v, seed, qk_scale=3.0):
    """A unit with O(1) activations (randomise_unit_) and a peaked, non-uniform attention: the q and k rows of qkv_conv
    (its first 2 dk output channels) scaled by ``qk_scale``."""
    m = pkg.GcnUnitAttention(ci, co, _graph(v), num_point=v).eval()
    randomise_unit_(m, seed)
    with torch.no_grad():
        m.attention_conv.qkv_conv.weight[: 2 * m.attention_conv.dk].mul_(qk_scale)
    return m


def _rand_x(n, ci, t, v, seed):
    return torch.rand((n, ci, t, v), generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _logits64(x, ops):
    """The attention logits q_i . k_j of tests/str_oracle.folded_unit (fp64, from the folded operands)."""
    n, c, t, v = x.shape
    dk = ops["dk"]
    xh = x.double() * ops["s_in"].double().view(1, c, 1, v) + ops["t_in"].double().view(1, c, 1, v)
    qk = torch.einsum("km,nktv->nmtv", ops["w_qkv"].double()[:, : 2 * dk], xh) + ops["b_qkv"].double()[: 2 * dk].view(1, -1, 1, 1)
    q = qk[:, :dk].reshape(n, so.NH, dk // so.NH, t, v)
    k = qk[:, dk:].reshape(n, so.NH, dk // so.NH, t, v)
    return torch.einsum("nhdti,nhdtj->nhtij", q, k)


def _guarded(t, fill, pad=PAD):
    """A device copy of ``t`` inside a larger buffer whose ``pad`` elements in front of it and behind it hold ``fill``."""
    buf = torch.full((t.numel() + 2 * pad,), fill, device=DEV)
    v = buf[pad: pad + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _strides(c, ncols, layout, extra):
    """(segment stride, channel stride).  "dense" is the clip layout; "ring" has the shape of the continual ring slots: a
    channel stride beyond frames * V (a multiple of 4, like P) and a segment stride beyond C * channel stride."""
    if layout == "dense":
        return c * ncols, ncols
    chan = (ncols + 3) // 4 * 4 + extra
    return c * chan + 2 * extra, chan


def _place(x3, strides, fill, pad=PAD):
    """(n, C, ncols) values laid out with ``strides`` in a flat device buffer; everything between the rows and ``pad``
    elements on either side hold ``fill``.  Returns (buffer, the tensor to hand to stage, the strided view of the values)."""
    n, c, ncols = x3.shape
    seg, chan = strides
    body = (n - 1) * seg + (c - 1) * chan + ncols
    buf = torch.full((body + 2 * pad,), fill, device=DEV)
    start = buf[pad:]
    view = start.as_strided((n, c, ncols), (seg, chan, 1))
    view.copy_(x3)
    return buf, start, view


def _stage(m, x, layout="dense", x_fill=NAN):
    """Run ``m.stage`` on x (n, C_in, T, V; CPU) in the given layout.  x sits in a buffer whose unused parts are ``x_fill``;
    y is pre-filled with NaN and x's channel stride is larger than y's.  Returns the output (n, C_out, T, V) on the CPU after
    checking that exactly the elements (seg, c < C_out, col < frames * V) of the y buffer were written."""
    n, ci, t, v = x.shape
    co, ncols = m.out_channels, t * v
    xs, ys = _strides(ci, ncols, layout, 12), _strides(co, ncols, layout, 4)
    _, x_dev, _ = _place(x.reshape(n, ci, ncols).to(DEV), xs, x_fill)
    ybuf, y_dev, y_view = _place(torch.full((n, co, ncols), NAN, device=DEV), ys, NAN)
    m.stage(x_dev, y_dev, n_seg=n, frames=t, x_strides=xs, y_strides=ys)
    torch.cuda.synchronize()
    written = torch.isfinite(ybuf)
    expect = torch.zeros_like(written)
    expect[PAD:].as_strided((n, co, ncols), (ys[0], ys[1], 1)).fill_(True)
    assert torch.equal(written, expect), "stage wrote outside (seg, c < C_out, col < frames * V) or left a hole"
    return y_view.reshape(n, co, t, v).cpu()


# ---- 1. the unit against fp64 over a seeded sweep ------------------------------------------------------------------------
# (C_in, C_out, V, n_seg, frames, layout).  C_out = 64 and 256 take the 128-row QKV tile, 32 and 128 the 64-row one.  Every C_out
# has C_in == C_out (skip) and C_in != C_out (no skip) for V = 18 and V = 25; C_in covers {16, 32, 48, 80, 144, 256}.
SWEEP = [
    (32, 32, 18, 1, 1, "dense"),          # n_seg = 1, frames = 1: one column tile of 18 columns
    (32, 32, 25, 3, 41, "ring"),          # 1025 columns = 4 * 256 + 1, odd n_seg, skip on a non-dense layout
    (16, 32, 18, 3, 128, "dense"),        # 2304 columns = 9 * 256 exactly
    (48, 32, 25, 1, 1, "ring"),           # one column tile of 25 columns
    (64, 64, 18, 2, 128, "dense"),        # 128-row tile on exactly full column tiles
    (64, 64, 25, 3, 41, "ring"),          # 128-row tile, last column tile holds a single column, skip with x stride != y stride
    (64, 64, 25, 1, 1, "ring"),
    (80, 64, 18, 1, 1, "dense"),          # 128-row tile, ncols < 256 with one frame
    (144, 64, 25, 1, 256, "dense"),       # 6400 columns = 25 * 256 exactly
    (128, 128, 18, 5, 7, "ring"),         # odd n_seg, 126 columns
    (128, 128, 25, 1, 1, "dense"),
    (256, 128, 18, 1, 128, "dense"),
    (48, 128, 25, 3, 41, "dense"),
    (80, 128, 25, 5, 3, "ring"),
    (256, 256, 18, 1, 1, "dense"),
    (256, 256, 25, 1, 256, "dense"),      # 128-row tile, 6400 columns exactly
    (256, 256, 25, 3, 41, "ring"),
    (144, 256, 18, 3, 9, "ring"),
    (16, 256, 25, 5, 11, "ring"),
    (32, 256, 18, 2, 15, "dense"),
]
_SWEEP_IDS = [f"{ci}to{co}-V{v}-seg{n}-f{t}-{lay}" for ci, co, v, n, t, lay in SWEEP]


def test_sweep_covers_the_matrix():
    """The parametrisation holds every case the sweep is meant to hold (checked, not trusted)."""
    for co in (32, 64, 128, 256):
        for v in (18, 25):
            assert any(c[1] == co and c[2] == v and c[0] == co for c in SWEEP), ("skip", co, v)
            assert any(c[1] == co and c[2] == v and c[0] != co for c in SWEEP), ("no skip", co, v)
    assert {c[0] for c in SWEEP} >= {16, 32, 48, 80, 144, 256}
    assert any(c[3] == 1 and c[4] == 1 and c[2] == 18 for c in SWEEP) and any(c[3] == 1 and c[4] == 1 and c[2] == 25 for c in SWEEP)
    assert (16, 32, 18, 3, 128, "dense") in SWEEP and any(c[2] == 25 and c[4] == 256 for c in SWEEP)
    assert any((c[2] * c[4]) % 256 == 1 for c in SWEEP)
    assert any(c[3] >= 3 and c[3] % 2 == 1 for c in SWEEP)
    for co in (64, 128):                                                            # both tile heights, skip, non-dense
        assert any(c[0] == c[1] == co and c[5] == "ring" for c in SWEEP)


@pytest.mark.parametrize("ci,co,v,n,t,layout", SWEEP, ids=_SWEEP_IDS)
def test_unit_sweep_vs_fp64(ci, co, v, n, t, layout):
    """stage() with explicit strides against folded_unit (fp64, same folded operands) and against str_unit (the op-for-op
    fp32 restatement from the state dict).  The restatement's own error against fp64 is recorded with each line of the parity
    report, so the kernel's margin over plain fp32 is on record."""
    seed = 1000 * ci + co + v + n + t
    m = _unit(ci, co, v, seed)
    x = _rand_x(n, ci, t, v, seed + 1)
    sd = {k: p.clone() for k, p in m.state_dict().items()}
    ops = m._fold()
    assert (ops["res_scale"] is not None) == (ci == co)
    with torch.no_grad():
        want64 = so.folded_unit(x, ops)
        want32 = so.str_unit(x, sd, "")
    e32 = max_err(want32, want64)
    got = _stage(m.to(DEV), x, layout)
    case = f"{ci}->{co} V={v} n_seg={n} frames={t} {layout}"
    check_parity(got, want64, note=f"unit vs fp64: {case}", fp32_restatement_err_vs_fp64=e32)
    check_parity(got, want32, note=f"unit vs fp32 restatement: {case}", fp32_restatement_err_vs_fp64=e32)


@pytest.mark.parametrize("ci,co,v,n,t,layout", [(64, 64, 25, 3, 41, "ring"), (48, 128, 18, 2, 15, "dense"), (128, 128, 18, 3, 7, "ring"),
                                                (144, 256, 25, 1, 1, "dense"), (32, 32, 25, 2, 11, "dense")])
def test_unit_operands_between_nan_guards(ci, co, v, n, t, layout):
    """Weights, biases, s_in / t_in, res_scale and x each in a buffer of their own with NaN on both sides: a read past M / Mpad,
    past C_in * V or outside x (staging, or the residual of the epilogue) puts a NaN into a sum.  The output must be finite and
    bit for bit that of the run with zero guards."""
    x = _rand_x(n, ci, t, v, 17)
    outs = []
    for fill in (0.0, NAN):
        m = _unit(ci, co, v, 23).to(DEV)
        ops = m._packed_ops(torch.device(DEV))                      # the cached operand dict stage() reads
        for key in ("w_qkv", "b_qkv", "s_in", "t_in", "w_out", "b_out", "res_scale"):
            if ops[key] is not None:
                ops[key] = _guarded(ops[key], fill)
        assert (ops["res_scale"] is not None) == (ci == co)
        outs.append(_stage(m, x, layout, x_fill=fill))
        assert m._packed_ops(torch.device(DEV)) is ops              # the launch used the guarded operands
    assert bool(torch.isfinite(outs[1]).all()), "the unit read outside an operand"
    assert torch.equal(outs[0], outs[1])
    with torch.no_grad():
        check_parity(outs[1], so.folded_unit(x, _unit(ci, co, v, 23)._fold()), note=f"guarded operands {ci}->{co} V={v}")


# ---- 2. position invariance, bitwise ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci,co,v", [(64, 64, 25), (128, 128, 18), (64, 128, 25), (128, 256, 18)])
def test_segment_equals_the_segment_launched_alone(ci, co, v):
    m = _unit(ci, co, v, 31).to(DEV)
    x = _rand_x(5, ci, 23, v, 32).to(DEV)
    full = m(x)
    for i in range(5):
        assert torch.equal(m(x[i:i + 1].contiguous()), full[i:i + 1]), i


@pytest.mark.parametrize("ci,co,v", [(64, 64, 25), (128, 128, 18), (64, 64, 18), (128, 128, 25), (16, 32, 25), (80, 256, 18)])
def test_frame_equals_the_frame_alone_and_at_another_index(ci, co, v):
    """Frame 3 of a 40-frame segment (column tile 0) against the same frame launched alone (columns 0 .. V - 1) and placed at
    frame 17 (V = 25: columns 425 .., V = 18: columns 306 ..: column tile 1, another lane) or 39 (the ragged last tile) of a
    segment whose other frames differ."""
    m = _unit(ci, co, v, 41).to(DEV)
    x = _rand_x(1, ci, 40, v, 42).to(DEV)
    y = m(x)
    alone = m(x[:, :, 3:4].contiguous())
    assert torch.equal(alone[:, :, 0], y[:, :, 3])
    for f in (17, 39):
        assert (f * v) // 256 != (3 * v) // 256 and (f * v) % 64 != (3 * v) % 64
        x2 = _rand_x(1, ci, 40, v, 43 + f).to(DEV)
        x2[:, :, f] = x[:, :, 3]
        assert torch.equal(m(x2)[:, :, f], y[:, :, 3]), f


# ---- 3. softmax and NaN edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci,co,v", [(64, 64, 25), (128, 128, 18), (16, 64, 25), (256, 256, 25), (32, 32, 18)])
def test_softmax_with_logits_beyond_expf_overflow(ci, co, v):
    """q and k rows of qkv_conv.weight scaled by 16 (v rows untouched): the fp64 logits reach 160 .. 250 in magnitude, far
    beyond where expf overflows (88.7), so a softmax without the row-maximum subtraction yields inf / NaN.  A peaked softmax
    amplifies the fp32 rounding of the logits; at this scale the fp32 restatement stays within TOL / 4 of fp64 (measured on
    the CPU: 1.9e-6 .. 4.8e-6; both conditions are asserted here from the references alone), so the plain 1e-4 holds."""
    m = _unit(ci, co, v, 5, qk_scale=16.0)
    x = _rand_x(3, ci, 21, v, 1)
    sd = {k: p.clone() for k, p in m.state_dict().items()}
    ops = m._fold()
    with torch.no_grad():
        want64, want32 = so.folded_unit(x, ops), so.str_unit(x, sd, "")
    peak = float(_logits64(x, ops).abs().max())
    e32 = max_err(want32, want64)
    assert peak >= 100.0, peak
    assert e32 <= TOL / 4, e32
    got = _stage(m.to(DEV), x, "dense")
    check_parity(got, want64, note=f"softmax overflow range {ci}->{co} V={v}", max_abs_logit=peak, fp32_restatement_err_vs_fp64=e32)


@pytest.mark.parametrize("ci,co,v", [(64, 64, 25), (48, 128, 18), (144, 256, 25)])
def test_uniform_attention_is_the_mean_of_v_over_the_joints(ci, co, v):
    """q = k = 0 (weight rows and bias): every logit is 0, every attention output the mean of v over the joints."""
    m = _unit(ci, co, v, 51)
    dk = m.attention_conv.dk
    with torch.no_grad():
        m.attention_conv.qkv_conv.weight[: 2 * dk].zero_()
        m.attention_conv.qkv_conv.bias[: 2 * dk].zero_()
    x = _rand_x(2, ci, 13, v, 52)
    ops = m._fold()
    rows, dv = 2 * dk + co, co
    xh = x.double() * ops["s_in"].double().view(1, ci, 1, v) + ops["t_in"].double().view(1, ci, 1, v)
    vv = torch.einsum("km,nktv->nmtv", ops["w_qkv"].double()[:, 2 * dk:rows], xh) + ops["b_qkv"].double()[2 * dk:rows].view(1, dv, 1, 1)
    att = vv.mean(dim=3, keepdim=True).expand(-1, -1, -1, v)
    want = torch.einsum("km,nktv->nmtv", ops["w_out"].double()[:, :dv], att) + ops["b_out"].double()[:dv].view(1, dv, 1, 1)
    if ops["res_scale"] is not None:
        want = want + ops["res_scale"].double().view(1, dv, 1, 1) * x.double()
    want = torch.relu(want).float()
    got = _stage(m.to(DEV), x, "ring")
    check_parity(got, want, note=f"uniform attention {ci}->{co} V={v}")
    if ci != co:                                  # no skip: all joints of a frame carry the same value, bit for bit
        assert torch.equal(got, got[..., :1].expand_as(got))


@pytest.mark.parametrize("layout", ["dense", "ring"])
@pytest.mark.parametrize("ci,co,v", [(64, 64, 25), (48, 128, 18)])
def test_one_nan_poisons_its_frame_and_nothing_else(ci, co, v, layout):
    """One NaN at (seg, c, f, v) of x: the joint's q, k and v columns are NaN, so every softmax row of that frame holds a NaN
    logit (fmaxf skips it in the max pass, expf(NaN - mx) does not) and every output element of the frame is NaN; every other
    frame and segment stays finite.  tests/str_oracle.str_unit does the same on the CPU (asserted first).  Clip layout and ring
    layout (frames = skeletons, segments = slots)."""
    m = _unit(ci, co, v, 61)
    n, t = 3, 12
    seg, c, f, j = 1, ci - 3, 10, v - 2                 # V = 25: column 273, in the ragged second column tile
    x = _rand_x(n, ci, t, v, 62)
    x[seg, c, f, j] = NAN
    want_nan = torch.zeros((n, co, t, v), dtype=torch.bool)
    want_nan[seg, :, f, :] = True
    with torch.no_grad():
        ref = so.str_unit(x, {k: p.clone() for k, p in m.state_dict().items()}, "")
    assert torch.equal(torch.isnan(ref), want_nan) and bool(torch.isfinite(ref[~want_nan]).all())
    ncols = t * v
    xs, ys = _strides(ci, ncols, layout, 12), _strides(co, ncols, layout, 4)
    m = m.to(DEV)
    _, x_dev, _ = _place(x.reshape(n, ci, ncols).to(DEV), xs, 0.0)
    _, y_dev, y_view = _place(torch.zeros((n, co, ncols), device=DEV), ys, 0.0)
    m.stage(x_dev, y_dev, n_seg=n, frames=t, x_strides=xs, y_strides=ys)
    got = y_view.reshape(n, co, t, v).cpu()
    assert torch.equal(torch.isnan(got), want_nan)
    assert bool(torch.isfinite(got[~want_nan]).all())
    check_parity(got[~want_nan], ref[~want_nan], note=f"NaN containment {ci}->{co} V={v} {layout}")


# ---- 6. continual behaviour of CoSTr ----------------------------------------------------------------------------------------
def _costr(v, pool_size, pool_padding):
    tag = "ntu" if v == 25 else "kin"
    arrays, sd, x = model_fixture(f"g12_str_{tag}", v)
    co = pkg.CoSTr(_graph(v), (3, 300, v, 2), 60 if v == 25 else 400, pool_size=pool_size, pool_padding=pool_padding).eval()
    co.load_state_dict(co.map_state_dict(sd), strict=True)
    return co.to(DEV), sd


def _frames(n, t, v, seed):
    return torch.rand((n, 3, t, v, 2), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("v", [25, 18])
@pytest.mark.parametrize("n", [1, 3, 7])
def test_costr_stream_counts_vs_oracle(n, v):
    """1, 3 and 7 streams (ragged position counts in the shared rings), both skeleton graphs: forward_steps(pad_end=True)
    against the clip-form oracle with the attention unit as the graph conv."""
    co, sd = _costr(v, 6, 2)
    x = _frames(n, 48, v, 70 + n)
    with torch.no_grad():
        want = o.co_stgcn_steps_pad_end(x, sd, 6, 2, gcn=so.gcn)
    got = co.forward_steps(x.to(DEV), pad_end=True).cpu()
    assert got.shape == want.shape and got.shape[2] >= 5
    check_parity(got, want, note=f"CoSTr {n} streams V={v}")


def test_costr_forward_cycle_equals_per_frame_stepping():
    """Cycles of 1 .. 4 frames in mixed order: bit for bit the predictions of per-frame stepping."""
    x = _frames(2, 110, 25, 81).to(DEV)
    ref, _ = _costr(25, 5, 1)
    want = [r for r in (ref.forward_step(x[:, :, t].contiguous()) for t in range(x.shape[2])) if r is not None]
    for pattern in ([4], [3, 4, 1, 2], [1, 4, 4, 3], [2, 1, 3]):
        co, _ = _costr(25, 5, 1)
        got, t, i = [], 0, 0
        while t < x.shape[2]:
            r = min(pattern[i % len(pattern)], x.shape[2] - t)
            got += co.forward_cycle([x[:, :, t + f].contiguous() for f in range(r)])
            t, i = t + r, i + 1
        assert len(got) == len(want) and len(want) >= 5
        assert all(torch.equal(g, w) for g, w in zip(got, want)), pattern


def test_costr_update_state_false_peeks_without_advancing():
    x = _frames(3, 100, 25, 82).to(DEV)
    peeker, _ = _costr(25, 4, 1)
    plain, _ = _costr(25, 4, 1)
    seen = 0
    for t in range(100):
        f = x[:, :, t].contiguous()
        p1 = None
        if t in (0, 3, 50, 83, 84, 88, 96):
            p1 = peeker.forward_step(f, update_state=False)
            p2 = peeker.forward_step(f, update_state=False)
            assert (p1 is None) == (p2 is None) and (p1 is None or torch.equal(p1, p2))
        got, want = peeker.forward_step(f), plain.forward_step(f)
        assert (got is None) == (want is None)
        if want is not None:
            assert torch.equal(got, want), t
            if p1 is not None:
                assert torch.equal(p1, want), t
                seen += 1
    assert seen >= 2                                                   # peeks that did predict (frames 84, 88, 96)


def test_costr_clean_state_and_replay():
    x = _frames(2, 100, 25, 83).to(DEV)
    co, _ = _costr(25, 4, 1)
    first = co.forward_steps(x)
    assert first.shape[2] >= 3
    co.clean_state()
    assert torch.equal(co.forward_steps(x), first)
    co.forward_steps(x[:, :, :37].contiguous())                       # leave dirty state, another history
    co.clean_state()
    assert torch.equal(co.forward_steps(x), first)


def test_continual_stride2_block_with_unit_vs_block_oracle():
    """CoSpatioTemporalBlock 64 -> 128, temporal stride 2, conv residual, the unit as CoGraphConv, stepped frame by frame
    against CoBlockOracle(gcn=so.gcn)."""
    blk = pkg.CoSpatioTemporalBlock(64, 128, _graph(25), stride=2, padding="equal",
                                    CoGraphConv=lambda ci, co, A, bn_momentum=0.1: pkg.GcnUnitAttention(ci, co, A, bn_momentum)).eval()
    randomise_unit_(blk, 12)
    sd = {k.replace("0.1.", "").replace("0.0.residual", "residual"): t.clone() for k, t in blk.state_dict().items()}
    assert "residual.t_conv.weight" in sd and "gcn.attention_conv.qkv_conv.weight" in sd, sorted(sd)
    x = torch.rand((3, 64, 15, 25), generator=torch.Generator().manual_seed(6)) * 2 - 1
    with torch.no_grad():
        want = o.CoBlockOracle(sd, "", 2, True, padding=4, gcn=so.gcn).forward_steps(x, pad_end=True)
    got = blk.to(DEV).forward_steps(x.to(DEV), pad_end=True).cpu()
    assert got.shape == want.shape == (3, 128, 8, 25)
    check_parity(got, want, note="stride-2 CoSpatioTemporalBlock + unit")


def test_str_default_mode_clip_forward_is_graph_capturable():
    """The default (throughput) mode of STr: a whole forward captured into a hipGraph replays bit-identically and computes
    the new result for new input in the captured buffer."""
    arrays, sd, x = model_fixture("g12_str_ntu", 25)
    net = pkg.STr(_graph(25)).eval()
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV)
    xd = x[:1].to(DEV)
    fresh = torch.rand(xd.shape, generator=torch.Generator().manual_seed(91)).to(DEV)
    for _ in range(2):
        ref = net(xd)                     # warm-up: folds weights, fills the caching allocator
    eager2 = net(fresh).clone()
    check_parity(ref.cpu(), arrays["logits"], note="STr eager, fixture input")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = net(xd)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    xd.copy_(fresh)                       # fresh input in the captured buffer
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager2) and not torch.equal(out, ref)
