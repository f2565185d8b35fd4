"""GPU tests of the Winograd F(2, 3) temporal conv (csrc/tcn_wino.hip, csk_tcn_stage_wino_f32): the identity-residual blocks
against the oracle (1e-4) and against the direct kernels (1e-5), bitwise batch invariance, reads confined to y / x_res (NaN
guards), hipGraph capture, and the gate (which launches take the kernel)."""
import os
import subprocess
import sys

import pytest
import torch

import _bootstrap
from oracle import stgcn_oracle as o
from tests.helpers import BLOCK_OUT_KEYS, check_parity, unit_scale_

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native = pkg.native
from continual_skeletons_amd import fold  # noqa: E402
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _A(v):
    return (pkg.ntu_graph() if v == 25 else pkg.kinetics_graph()).A


def _block(c, v, seed):
    torch.manual_seed(seed)
    m = pkg.SpatioTemporalBlock(c, c, _A(v), 1, True).eval()
    with torch.no_grad():
        for name, prm in m.named_parameters():
            if name.endswith("graph_attn") or name.endswith("bn.weight"):
                prm.copy_(torch.rand_like(prm) + 0.5)
            elif name.endswith("bias"):
                prm.copy_(torch.rand_like(prm) - 0.5)
        for name, buf in m.named_buffers():
            if name.endswith("running_var"):
                buf.copy_(torch.rand_like(buf) + 0.5)
            elif name.endswith("running_mean"):
                buf.copy_(torch.rand_like(buf) - 0.5)
    return m


@pytest.mark.parametrize("v", [25, 18])
@pytest.mark.parametrize("t", [300, 150, 75, 9, 17])
@pytest.mark.parametrize("c", [64, 128, 256])
def test_wino_block_vs_oracle(c, t, v):
    m = _block(c, v, 77 + c + t + v)
    sd = {k: val.clone() for k, val in m.state_dict().items()}
    x = torch.rand(1, c, t, v)
    want = unit_scale_(m, sd, lambda s: o.st_block(x, s, "", 1, True), BLOCK_OUT_KEYS)
    got = m.to(DEV)(x.to(DEV)).cpu()
    check_parity(got, want, shape=(c, t, v))


def test_wino_vs_forced_direct_path(tmp_path):
    """CSK_TCN_WINO=1 (diagnostic, under CSK_DIAG=1) runs the direct kernels: the two differ by the rounding of the transformed
    operands only (<= 1e-5 on O(1) outputs), and not bit for bit (the Winograd kernel did run)."""
    code = (
        "import sys, torch; sys.path.insert(0, %r); import _bootstrap, bench; pkg = _bootstrap.load(); outs = [];\n"
        "for (c, t, v) in [(64, 300, 25), (128, 150, 25), (256, 75, 25), (64, 75, 18), (128, 17, 18)]:\n"
        "    A = (pkg.ntu_graph() if v == 25 else pkg.kinetics_graph()).A\n"
        "    b = pkg.SpatioTemporalBlock(c, c, A, stride=1).eval(); bench.randomise_(b, 3); b = b.to('cuda:0')\n"
        "    x = torch.rand((2, c, t, v), generator=torch.Generator().manual_seed(5)).to('cuda:0'); outs.append(b(x).cpu())\n"
        "torch.save(outs, sys.argv[1])\n"
    ) % ROOT
    res = []
    for forced in (False, True):
        path = str(tmp_path / f"wino_{int(forced)}.pt")
        env = dict(os.environ)
        env.pop("CSK_TCN_WINO", None)
        if forced:
            env.update(CSK_DIAG="1", CSK_TCN_WINO="1")
        subprocess.check_call([sys.executable, "-c", code, path], env=env)
        res.append(torch.load(path))
    for a_, b_ in zip(res[0], res[1]):
        assert bool(torch.isfinite(a_).all())
        check_parity(a_, b_, tol=1e-5, note="Winograd vs direct temporal conv")
    assert any(not torch.equal(a_, b_) for a_, b_ in zip(res[0], res[1]))


@pytest.mark.parametrize("c,t,v", [(64, 300, 25), (256, 75, 25), (128, 17, 18)])
def test_wino_batch_invariance_bitwise(c, t, v):
    m = _block(c, v, 5).to(DEV)
    x = torch.rand(6, c, t, v, device=DEV)
    full = m(x)
    for lo in range(0, 6, 2):
        assert torch.equal(m(x[lo:lo + 2].contiguous()), full[lo:lo + 2])
    assert torch.equal(m(x[5:6].contiguous()), full[5:6])


def _guarded(t, fill, pad=1 << 16):
    buf = torch.full((t.numel() + 2 * pad,), fill, device=DEV)
    v = buf[pad: pad + t.numel()].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("c,t,v", [(64, 300, 25), (128, 75, 25), (256, 9, 18), (64, 17, 18)])
def test_wino_reads_only_y_and_x_res(c, t, v):
    """y, x_res and the DIRECT weight between NaN guards / NaN-filled: the Winograd launch reads neither anything outside y and
    x_res nor the direct weight (so the gate took the kernel), and its output equals the zero-guarded run."""
    m = _block(c, v, 9).to(DEV)
    ops = m._packed_ops(torch.device(DEV))
    assert ops["w_wino"] is not None
    y_h, x_h = torch.rand(3, c, t, v), torch.rand(3, c, t, v)
    outs = []
    for fill in (float("nan"), 0.0):
        y, x = _guarded(y_h.to(DEV), fill), _guarded(x_h.to(DEV), fill)
        w_direct = torch.full_like(ops["w"], fill)
        out = pkg.blocks.tcn_stage(y, w_direct, ops["bias"], c, 9, 1, 4, relu=True, res_mode=1, x_res=x, w_wino=ops["w_wino"])
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert bool(torch.isfinite(outs[0]).all()), "the Winograd launch read outside y / x_res or read the direct weight"
    assert torch.equal(outs[0], outs[1])


def test_wino_gate_falls_back_to_the_direct_kernels():
    """Shapes outside the gate (conv residual / stride 2, no residual, c_out not a multiple of 64, V = 20) run csk_tcn_stage_f32
    from the same entry: the same bits as the direct call."""
    for (ci, co, s, res, v) in [(64, 128, 2, True, 25), (64, 64, 1, False, 25), (40, 40, 1, True, 25), (64, 64, 1, True, 20)]:
        a = torch.zeros(3, v, v)
        a[:, range(v), range(v)] = 1.0
        m = pkg.SpatioTemporalBlock(ci, co, a, stride=s, residual=res).eval().to(DEV)
        x = torch.rand(2, ci, 20, v, device=DEV)
        y = m.gcn(x)
        ops = m._packed_ops(x.device)
        conv = ci != co or s != 1
        mode = 2 if (res and conv) else 1 if res else 0
        wino = fold.pack_conv_weight_wino(m.tcn.t_conv.weight.detach().cpu(), torch.ones(co, dtype=torch.float64)).to(DEV)
        kw = dict(relu=True, res_mode=mode, x_res=x if res else None, w_res=ops["w_res"] if mode == 2 else None)
        want = pkg.blocks.tcn_stage(y, ops["w"], ops["bias"], co, 9, s, 4, **kw)
        got = pkg.blocks.tcn_stage(y, ops["w"], ops["bias"], co, 9, s, 4, w_wino=wino, **kw)
        assert torch.equal(got, want), (ci, co, s, res, v)


def test_wino_block_is_graph_capturable():
    m = _block(128, 25, 11).to(DEV)
    x = torch.rand(2, 128, 40, 25, device=DEV)
    for _ in range(2):
        ref = m(x)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m(x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    x2 = torch.rand(2, 128, 40, 25, device=DEV)
    x.copy_(x2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, m(x2))


def test_tile_families_bitwise_with_wino_off(tmp_path):
    """With the Winograd kernel switched off (CSK_TCN_WINO=1) the identity blocks run the direct kernels again, and the 16x16x4
    and 32x32x2 tile families stay bit for bit interchangeable there (CSK_TCN16=2 / 1)."""
    code = (
        "import sys, torch; sys.path.insert(0, %r); import _bootstrap, bench; pkg = _bootstrap.load(); A = pkg.ntu_graph().A; outs = [];\n"
        "for (ci, co) in [(64, 64), (128, 128)]:\n"
        "    b = pkg.SpatioTemporalBlock(ci, co, A, stride=1).eval(); bench.randomise_(b, 3); b = b.to('cuda:0')\n"
        "    x = torch.rand((3, ci, 45, 25), generator=torch.Generator().manual_seed(5)).to('cuda:0'); outs.append(b(x).cpu())\n"
        "torch.save(outs, sys.argv[1])\n"
    ) % ROOT
    res = []
    for mode in ("2", "1"):
        path = str(tmp_path / f"tile16_{mode}.pt")
        env = dict(os.environ, CSK_DIAG="1", CSK_TCN16=mode, CSK_TCN_WINO="1")
        subprocess.check_call([sys.executable, "-c", code, path], env=env)
        res.append(torch.load(path))
    for a_, b_ in zip(res[0], res[1]):
        assert torch.equal(a_, b_) and bool(torch.isfinite(a_).all())
