"""The opt-in step precision "bf16x3" (csrc/step_split.hip; continual.set_step_precision): the continual temporal step of the
128- / 256-channel blocks on the bf16 matrix pipe.  fp32-GRADE, so it has tests of its own: the kernel against fp64 on the
fixtures of tests/step_split_fixture.py (a lost piece product misses their tolerance: tests/test_step_split_fixture_cpu.py),
blocks and the whole CoStGcn against the oracle and the exact engine at the suite's 1e-4, and the invariances the exact
engine has (alone / in a batch, peeking, run to run), bitwise."""
import pytest
import torch

import _bootstrap
from oracle import stgcn_oracle as o
from tests import split_fixture as sf
from tests import step_split_fixture as ssf
from tests.helpers import BLOCK_OUT_KEYS, check_parity, g6_state_dict, guarded_allocs, load_golden, unit_scale_

gpu = pytest.mark.gpu
pkg = _bootstrap.load()
from continual_skeletons_amd import fold  # noqa: E402

native = pkg.native
DEV = "cuda:0"
MODE = "bf16x3"
A = pkg.ntu_graph().A


# ---- 1. the kernel against fp64 through the C ABI ---------------------------------------------------------------------
def _launch(sc, fx, reps=1):
    """csk_tcn_step_bf16x3 on the step case, its positions repeated ``reps`` times along P -> the emissions (reps, N, C_out,
    n_emit, V); asserts that the spare slot of the output ring is untouched"""
    case, P = sc.case, sc.P
    g = ssf.launch_geometry(sc)
    wide = (lambda t: t) if reps == 1 else (lambda t: t.repeat(1, 1, reps))
    assert reps == 1 or P == case.N * case.V
    ring = wide(ssf.ring_of(ssf.channel_major(fx.x, P), g["slots"], g["rot"])).to(DEV)
    w_img, r_img = (None if t is None else t.to(DEV) for t in sf.pack_images(fx, fold))
    xres = None if fx.x_res is None else wide(ssf.ring_of(ssf.channel_major(fx.x_res, P), g["x_slots"], g["x_rot"])).to(DEV)
    out = torch.full((g["out_slots"], case.co, P * reps), float("nan"), device=DEV)
    bias = torch.zeros(128, device=DEV)
    mode = {"none": 0, "ident": 1, "conv": 2}[case.res]
    rc = native.lib().csk_tcn_step_bf16x3(
        native.ptr(ring), g["slots"], g["head"], case.stride, sc.n_emit, native.ptr(w_img), native.ptr(xres), g["x_slots"],
        g["x_slot0"], case.stride, native.ptr(r_img), native.ptr(bias), native.ptr(out), g["out_slots"], g["out_slot0"],
        case.ci, case.co, P * reps, 9, mode, case.c_res, 0, native.stream_of(out))
    native.check(rc, "csk_tcn_step_bf16x3")
    out = out.cpu()
    spare = (g["out_slot0"] + sc.n_emit) % g["out_slots"]
    assert bool(torch.isnan(out[spare]).all()), "a slot of the output ring that holds no emission was written"
    nv = case.N * case.V
    em = torch.stack([out[(g["out_slot0"] + j) % g["out_slots"]] for j in range(sc.n_emit)], dim=0)      # (n_emit, C_out, P reps)
    em = em.reshape(sc.n_emit, case.co, reps, P)[..., :nv].reshape(sc.n_emit, case.co, reps, case.N, case.V)
    return em.permute(2, 3, 1, 0, 4).contiguous()


@gpu
@pytest.mark.parametrize("sc", ssf.CASES + ssf.MIXED, ids=lambda c: c.id)
def test_step_kernel_vs_fp64(sc):
    fx = sf.build(sc.case)
    sf.check_case(_launch(sc, fx)[0], ssf.analyse(sc, fx), case=sc.id)


@gpu
@pytest.mark.parametrize("wc", ssf.WIDE, ids=lambda c: c.id)
def test_wide_tiles_vs_fp64_and_bitwise_the_narrow_tile(wc):
    """the wide instantiations (25 x 1 and 13 x 2 column blocks x emissions; the 25-block tile is the one whose LDS exceeds
    64 KB), which only a launch of > 256 narrow tiles picks: against fp64 like every case, and bit for bit what a narrow tile
    computes for the same positions -- an output's summation order does not depend on the tile"""
    sc = wc.sc
    tile = native.lib().csk_tcn_step_bf16x3_tile
    assert tile(sc.n_emit, sc.case.co, wc.P) == wc.blocks != tile(sc.n_emit, sc.case.co, sc.P)
    fx = sf.build(sc.case)
    an = ssf.analyse(sc, fx)
    small, big = _launch(sc, fx), _launch(sc, fx, wc.reps)
    sf.check_case(small[0], an, case=sc.id)
    sf.check_case(big[-1], an, case=wc.id)                                 # the repetition that ends in the partial tile
    assert torch.equal(big, small.expand_as(big))


# ---- 2. block level -----------------------------------------------------------------------------------------------------
def _plain(sd):
    return {k.replace("0.1.", "").replace("0.0.residual", "residual"): v for k, v in sd.items()}


def _seeded_block(ci, co, stride, T, N, v=25):
    g = torch.Generator().manual_seed(4321 + ci + co + T)
    m = pkg.CoSpatioTemporalBlock(ci, co, A, stride=stride, residual=True, padding="equal").eval()
    with torch.no_grad():
        for name, prm in m.named_parameters():
            if name.endswith("graph_attn") or name.endswith("bn.weight") or name.endswith("residual.1.weight"):
                prm.copy_(torch.rand(prm.shape, generator=g) + 0.5)
            elif name.endswith("bias"):
                prm.copy_(torch.rand(prm.shape, generator=g) - 0.5)
        for name, buf in m.named_buffers():
            if name.endswith("running_var"):
                buf.copy_(torch.rand(buf.shape, generator=g) + 0.5)
            elif name.endswith("running_mean"):
                buf.copy_(torch.rand(buf.shape, generator=g) - 0.5)
    sd = _plain({k: t.clone() for k, t in m.state_dict().items()})
    x = torch.rand(N, ci, T, v, generator=g)
    want = unit_scale_(m, sd, lambda s: o.st_block(x, s, "", stride, True), BLOCK_OUT_KEYS)
    return m, x, want


def _count_launches(monkeypatch):
    n = [0]
    real = pkg.blocks.tcn_step_split_launch

    def counting(*args):
        n[0] += 1
        return real(*args)
    monkeypatch.setattr(pkg.blocks, "tcn_step_split_launch", counting)
    return n


@gpu
@pytest.mark.parametrize("ci,co,stride", [(64, 128, 2), (128, 128, 1), (128, 256, 2)])
def test_block_steps_to_the_lagged_clip_output(ci, co, stride, monkeypatch):
    """seeded blocks inside the predicate (the golden block fixtures have a handful of channels: next test) against the oracle"""
    m, x, want = _seeded_block(ci, co, stride, T=24, N=2)
    pkg.set_step_precision(m, MODE)
    assert m._use_split_step()
    n = _count_launches(monkeypatch)
    m, xd = m.to(DEV), x.to(DEV)
    o1 = m.forward_steps(xd, pad_end=False).cpu()
    cut = m.delay // stride
    assert o1.shape[2] == want.shape[2] - cut and n[0] > 0
    check_parity(o1, want[:, :, : want.shape[2] - cut], mode=MODE, shape=(ci, co, stride), note="steps lag the clip output by 4")
    m.clean_state()
    o2 = m.forward_steps(xd, pad_end=True).cpu()
    check_parity(o2, want, mode=MODE, shape=(ci, co, stride), note="pad_end")
    m.clean_state()
    peek = m.forward_steps(xd, pad_end=True, update_state=False).cpu()     # peeking leaves no trace
    assert torch.equal(peek, o2) and torch.equal(m.forward_steps(xd, pad_end=True).cpu(), o2)


@gpu
@pytest.mark.parametrize("tag", ["ident", "convres", "strided"])
def test_golden_blocks_in_the_mode(tag, monkeypatch):
    """the golden block fixtures in the mode: their channel counts lie outside the predicate, so they keep the exact kernels
    without complaint and step to the reference's clip output"""
    a, sd = load_golden(f"g3_block_{tag}")
    ci, co_, s, res, tp = (int(v) for v in a["meta"])
    blk = pkg.CoSpatioTemporalBlock(ci, co_, A, s, bool(res), padding=4).eval()
    blk.load_state_dict(sd, strict=True)
    pkg.set_step_precision(blk, MODE)
    n = _count_launches(monkeypatch)
    blk, x, target = blk.to(DEV), torch.from_numpy(a["x"]).to(DEV), torch.from_numpy(a["y"])
    o1 = blk.forward_steps(x, pad_end=False).cpu()
    cut = blk.delay // s
    check_parity(o1, target[:, :, : target.shape[2] - cut], mode=MODE)
    blk.clean_state()
    check_parity(blk.forward_steps(x, pad_end=True).cpu(), target, mode=MODE)
    assert blk._use_split_step() or n[0] == 0


# ---- 3. model level -----------------------------------------------------------------------------------------------------
def _model(sd, step_precision=None, native_plan=True):
    co = pkg.CoStGcn(A, pool_size=4, pool_padding=1).eval()
    co.use_native_plan = native_plan
    co.load_state_dict(sd, strict=True)
    if step_precision is not None:
        pkg.set_step_precision(co, step_precision)
    return co.to(DEV)


@pytest.fixture(scope="module")
def g6():
    a, sd, x = g6_state_dict("ntu")
    x = x[:1, :, :64].contiguous()
    with torch.no_grad():
        want = o.co_stgcn_steps_pad_end(x, sd, 4, 1)
    ref = _model(sd).forward_steps(x.to(DEV), pad_end=True).cpu()          # the default engine (native plan)
    return sd, x, want, ref


@gpu
def test_model_logits_vs_exact_engine_and_oracle(g6):
    sd, x, want, ref = g6
    co = _model(sd, MODE)
    got = co.forward_steps(x.to(DEV), pad_end=True).cpu()
    assert got.shape == want.shape and got.shape[2] >= 1
    check_parity(got, ref, mode=MODE, note="vs the exact engine")
    check_parity(got, want, mode=MODE, note="vs the oracle")
    check_parity(ref, want, note="the exact engine vs the oracle")
    assert co.__dict__.get("_plan") is None                                # the mode runs on the Python engine
    co.clean_state()
    assert co.forward_steps(x.to(DEV)).shape == (1, 60, 0)                 # 64 frames: nothing is emitted without the flush
    # run to run, and peeking: update_state=False leaves no trace
    co.clean_state()
    xd = x.to(DEV)
    co.forward_steps(xd[:, :, :40].contiguous())
    assert co.forward_step(xd[:, :, 40].contiguous(), update_state=False) is None
    co.forward_steps(xd[:, :, 40:52].contiguous())
    peek = co.forward_steps(xd[:, :, 52:].contiguous(), pad_end=True, update_state=False).cpu()
    again = co.forward_steps(xd[:, :, 52:].contiguous(), pad_end=True).cpu()
    assert torch.equal(peek, got) and torch.equal(again, got)


@gpu
def test_model_forward_step_peek_then_real_step_bitwise(g6):
    """forward_step(update_state=False) followed by the real step is the real step, bit for bit, at frames that emit a
    prediction and at frames that do not (100 frames: the stack's delay is 76, a prediction every 4th frame after it)"""
    sd, x, want, ref = g6
    co = _model(sd, MODE)
    frames = [x[:, :, t % 64].contiguous().to(DEV) for t in range(100)]
    plain = [co.forward_step(f) for f in frames]
    assert sum(p is not None for p in plain) >= 3 and plain[0] is None
    co.clean_state()
    for f, p in zip(frames, plain):
        looked, real = co.forward_step(f, update_state=False), co.forward_step(f)
        assert (looked is None) == (real is None) == (p is None)
        if p is not None:
            assert torch.equal(looked, real) and torch.equal(real, p)


@gpu
def test_model_stream_alone_and_in_a_batch_bitwise(g6):
    sd, x, want, ref = g6
    g = torch.Generator().manual_seed(3)
    x3 = torch.cat([torch.rand(x.shape, generator=g), x, torch.rand(x.shape, generator=g)], 0)
    one = _model(sd, MODE).forward_steps(x.to(DEV), pad_end=True)
    three = _model(sd, MODE).forward_steps(x3.to(DEV), pad_end=True)
    assert torch.equal(three[1], one[0])


# ---- 4. what the parent commit does not have ---------------------------------------------------------------------------------
@gpu
def test_mode_exists_steps_and_launches_the_split_kernel_for_layers_5_to_10(g6, monkeypatch):
    sd, x, want, ref = g6
    assert callable(pkg.set_step_precision)
    co = _model(sd, MODE)
    cur, per_layer = [0], {}
    real = pkg.blocks.tcn_step_split_launch

    def counting(*args):
        per_layer[cur[0]] = per_layer.get(cur[0], 0) + 1
        return real(*args)
    monkeypatch.setattr(pkg.blocks, "tcn_step_split_launch", counting)
    for i in range(10):
        blk = co.layers[f"layer{i + 1}"]
        assert blk._use_split_step() == (i >= 4)

        def advance(*args, _i=i, _f=blk.engine_advance, **kw):
            cur[0] = _i + 1
            return _f(*args, **kw)
        blk.engine_advance = advance
    xd = x.to(DEV)
    frames = [xd[:, :, t].contiguous() for t in range(64)]
    for t in range(0, 96, 4):                                              # 24 cycles = 96 frames: past the stack's delay of 76, every layer emits
        co.forward_cycle(frames[t % 64: t % 64 + 4])
    per_layer.clear()
    assert len(co.forward_cycle(frames[0:4])) == 1                         # a steady-state cycle: one prediction
    assert all(per_layer.get(i, 0) >= 1 for i in range(5, 11)), per_layer
    assert all(per_layer.get(i, 0) == 0 for i in range(1, 5)), per_layer


@gpu
def test_block_outside_the_predicate_steps_bitwise_as_in_f32():
    g = torch.Generator().manual_seed(8)
    x = torch.rand(2, 2, 14, 25, generator=g).to(DEV)
    blk = pkg.CoSpatioTemporalBlock(2, 4, A, stride=2, padding="equal").eval().to(DEV)
    exact = blk.forward_steps(x, pad_end=True)
    pkg.set_step_precision(blk, MODE)
    assert not blk._use_split_step()
    assert torch.equal(blk.forward_steps(x, pad_end=True), exact)


# ---- 5. unchanged defaults ------------------------------------------------------------------------------------------------
@gpu
def test_defaults_are_unchanged(g6):
    sd, x, want, ref = g6
    co = _model(sd)
    pkg.set_precision(co, MODE)                                            # clip precision alone: stepping is refused as before
    with pytest.raises(NotImplementedError, match="clip kernels only"):
        co.forward_step(x[:, :, 0].contiguous().to(DEV))
    pkg.set_step_precision(co, MODE)                                       # with the step precision set, stepping is allowed
    assert co.forward_step(x[:, :, 0].contiguous().to(DEV)) is None
    pkg.set_precision(co, "f32")
    pkg.set_step_precision(co, "f32")                                      # and back: bitwise the default engine, native plan included
    got = co.forward_steps(x.to(DEV), pad_end=True).cpu()
    assert co.__dict__.get("_plan") is not None
    assert torch.equal(got, ref)


# ---- 6. guards ------------------------------------------------------------------------------------------------------------
@gpu
def test_strided_block_under_guarded_allocations():
    m, x, want = _seeded_block(128, 256, 2, T=24, N=2)
    pkg.set_step_precision(m, MODE)
    m, xd = m.to(DEV), x.to(DEV)
    plain = m.forward_steps(xd, pad_end=True).cpu()
    m._state = None
    with guarded_allocs() as ga:
        guarded = m.forward_steps(xd, pad_end=True).cpu()
    assert ga.count > 0 and torch.equal(guarded, plain)
    check_parity(plain, want, mode=MODE)


# ---- 7. argument errors (no GPU) ----------------------------------------------------------------------------------------------
def test_argument_errors():
    lib = native.lib()
    rc = lib.csk_tcn_step_bf16x3(None, 9, 0, 1, 1, None, None, 0, 0, 0, None, None, None, 1, 0, 16, 128, 100, 9, 0, 0, 1, None)
    assert rc == -1 and b"null pointer" in lib.csk_last_error()
    buf = torch.zeros(64)                                                  # never dereferenced: every call below fails its checks
    p = native.ptr(buf)

    def call(slots=9, head=0, head_step=1, n_emit=1, c=16, c_out=128, P=100, k=9, res_mode=0, c_res=0, out_slots=1):
        return lib.csk_tcn_step_bf16x3(p, slots, head, head_step, n_emit, p, None, 0, 0, 0, None, p, p, out_slots, 0, c, c_out, P, k,
                                       res_mode, c_res, 1, None)
    for kw, text in ((dict(P=102), b"multiple of 4"), (dict(c=0), b"bad dims"), (dict(k=3), b"9 x 1"), (dict(head_step=3), b"head_step"),
                     (dict(head=9), b"slots/head"), (dict(n_emit=2), b"emission geometry"), (dict(n_emit=2, out_slots=2), b"too shallow"),
                     (dict(res_mode=1), b"without x_res"), (dict(res_mode=7), b"res_mode")):
        assert call(**kw) == -1 and text in lib.csk_last_error(), (kw, lib.csk_last_error())
    m = pkg.CoSpatioTemporalBlock(4, 4, A, padding="equal").eval()
    with pytest.raises(ValueError, match="step precision must be"):
        pkg.set_step_precision(m, "fp16")
    with pytest.raises(ValueError, match="no CoSpatioTemporalBlock"):
        pkg.set_step_precision(pkg.GraphConvolution(4, 4, A), MODE)
    assert m.step_precision == "f32"
    agcn = pkg.CoAGcn(pkg.kinetics_graph().A, (3, 300, 18, 2), 400).eval()
    with pytest.raises(NotImplementedError, match="plain GraphConvolution"):
        pkg.set_step_precision(agcn, MODE)
    assert all(b.step_precision == "f32" for b in agcn.layers.values())
    assert pkg.set_step_precision(agcn, "f32") is agcn
