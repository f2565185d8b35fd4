"""GPU tests of the Winograd forms behind csk_tcn_stage_wino_ext_f32 (csrc/tcn_wino.hip): the stride-2 polyphase kernel (conv
residual or none), which the stride-2 blocks run, and the stride-1 kernel without residual, which is reached through
blocks.tcn_stage(w_wino_ext=) only (SpatioTemporalBlock keeps the direct kernels for that block) -- against the oracle
(check_parity's default tolerance), against the direct kernels (1e-5, not bitwise), bitwise batch invariance, reads confined to
y / x_res / the images (NaN guards), hipGraph capture, and the gate (which launches take the kernels)."""
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
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _A(v):
    return (pkg.ntu_graph() if v == 25 else pkg.kinetics_graph()).A


def _block(ci, co, s, res, v, seed):
    torch.manual_seed(seed)
    m = pkg.SpatioTemporalBlock(ci, co, _A(v), s, res).eval()
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


SHAPES = [(64, 128, 2, True), (128, 256, 2, True), (64, 64, 1, False)]


class _ExtTail(torch.nn.Module):
    """gcn + tcn_stage(w_wino_ext=): the block's own composition with the Winograd image passed for every shape (a block keeps the
    direct kernels for stride 1 without residual)."""

    def __init__(self, m, s, res):
        super().__init__()
        self.m, self.s, self.res = m, s, res

    def forward(self, x):
        ops = self.m._packed_ops(x.device)
        return pkg.blocks.tcn_stage(self.m.gcn(x), ops["w"], ops["bias"], ops["c_out"], 9, self.s, 4, relu=True,
                                    res_mode=2 if self.res else 0, x_res=x if self.res else None, w_res=ops["w_res"],
                                    w_wino_ext=ops["w_wino_ext"])


def _vs_oracle(ci, co, s, res, t, v):
    m = _block(ci, co, s, res, v, 77 + ci + co + t + v)
    assert m._fold()["w_wino_ext"] is not None
    sd = {k: val.clone() for k, val in m.state_dict().items()}
    x = torch.rand(1, ci, t, v)
    want = unit_scale_(m, sd, lambda d: o.st_block(x, d, "", s, res), BLOCK_OUT_KEYS)
    m = m.to(DEV)
    got = (m if s == 2 else _ExtTail(m, s, res))(x.to(DEV)).cpu()
    check_parity(got, want, shape=(ci, co, s, res, t, v))


@pytest.mark.parametrize("v", [25, 18])
@pytest.mark.parametrize("t", [9, 10, 17, 20, 75, 150])
@pytest.mark.parametrize("ci,co,s,res", SHAPES)
def test_ext_block_vs_oracle(ci, co, s, res, t, v):
    _vs_oracle(ci, co, s, res, t, v)


@pytest.mark.parametrize("t,v", [(9, 25), (20, 25), (17, 18)])
def test_s2_block_vs_oracle_padded_residual_channels(t, v):
    """3 -> 64, stride 2, conv residual: the residual's 3 channels are padded to one 8-channel chunk (clamped reads, zero weights)."""
    _vs_oracle(3, 64, 2, True, t, v)


def test_s2_vs_forced_direct_path(tmp_path):
    """CSK_TCN_WINO=1 (diagnostic, under CSK_DIAG=1) runs the direct kernels for these blocks too: the two differ by the rounding
    of the transformed operands only (<= 1e-5 on O(1) outputs; the float32 host model of the kernel's arithmetic,
    tests/test_wino_s2_fold_cpu.py::test_float32_model_rounding_error, gives about 1e-6), and not bit for bit (the new kernels
    did run)."""
    code = (
        "import sys, torch; sys.path.insert(0, %r); import _bootstrap, bench; pkg = _bootstrap.load(); outs = [];\n"
        "for (ci, co, s, res, t, v) in [(64, 128, 2, True, 150, 25), (128, 256, 2, True, 75, 25), (64, 128, 2, True, 20, 18),\n"
        "                               (64, 64, 2, False, 17, 25)]:\n"
        "    A = (pkg.ntu_graph() if v == 25 else pkg.kinetics_graph()).A\n"
        "    b = pkg.SpatioTemporalBlock(ci, co, A, stride=s, residual=res).eval(); bench.randomise_(b, 3); b = b.to('cuda:0')\n"
        "    x = torch.rand((2, ci, t, v), generator=torch.Generator().manual_seed(5)).to('cuda:0'); outs.append(b(x).cpu())\n"
        "torch.save(outs, sys.argv[1])\n"
    ) % ROOT
    res = []
    for forced in (False, True):
        path = str(tmp_path / f"wino_s2_{int(forced)}.pt")
        env = dict(os.environ)
        env.pop("CSK_TCN_WINO", None)
        if forced:
            env.update(CSK_DIAG="1", CSK_TCN_WINO="1")
        subprocess.check_call([sys.executable, "-c", code, path], env=env)
        res.append(torch.load(path))
    for a_, b_ in zip(res[0], res[1]):
        assert bool(torch.isfinite(a_).all())
        print(f"new vs direct {tuple(a_.shape)}: max |diff| {float((a_ - b_).abs().max()):.3e}, max |direct| {float(b_.abs().max()):.3f}")
        check_parity(a_, b_, tol=1e-5, note="Winograd ext forms vs direct temporal conv")
    assert all(not torch.equal(a_, b_) for a_, b_ in zip(res[0], res[1]))


@pytest.mark.parametrize("t,v", [(75, 25), (17, 18), (300, 25)])
def test_no_residual_form_vs_direct_call(t, v):
    """Stride 1 without residual (a block keeps the direct kernels for this shape, so the form is reached through tcn_stage): the
    Winograd launch against the direct call on a bench.randomise_ block with O(1) inputs, 1e-5 and not bit for bit."""
    import bench
    m = pkg.SpatioTemporalBlock(64, 64, _A(v), stride=1, residual=False).eval()
    bench.randomise_(m, 3)
    m = m.to(DEV)
    ops = m._packed_ops(torch.device(DEV))
    x = torch.rand(2, 64, t, v, device=DEV)
    y = m.gcn(x)
    want = pkg.blocks.tcn_stage(y, ops["w"], ops["bias"], 64, 9, 1, 4, relu=True)
    got = pkg.blocks.tcn_stage(y, ops["w"], ops["bias"], 64, 9, 1, 4, relu=True, w_wino_ext=ops["w_wino_ext"])
    assert torch.equal(m(x), want)                                        # the block itself: direct bits
    print(f"no-residual form T={t} V={v}: max |diff| {float((got - want).abs().max()):.3e}, max |direct| {float(want.abs().max()):.3f}")
    check_parity(got.cpu(), want.cpu(), tol=1e-5, note="Winograd no-residual form vs direct temporal conv")
    assert not torch.equal(got, want)


@pytest.mark.parametrize("ci,co,t,v", [(64, 128, 150, 25), (128, 256, 75, 25), (64, 128, 17, 18)])
def test_s2_batch_invariance_bitwise(ci, co, t, v):
    m = _block(ci, co, 2, True, v, 5).to(DEV)
    x = torch.rand(6, ci, t, v, device=DEV)
    full = m(x)
    for lo in range(0, 6, 2):
        assert torch.equal(m(x[lo:lo + 2].contiguous()), full[lo:lo + 2])
    assert torch.equal(m(x[5:6].contiguous()), full[5:6])


def _guarded(t, fill, pad=1 << 16):
    buf = torch.full((t.numel() + 2 * pad,), fill, device=DEV)
    v = buf[pad: pad + t.numel()].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("ci,co,s,res,t,v", [(64, 128, 2, True, 150, 25), (128, 256, 2, True, 75, 25), (3, 64, 2, True, 9, 18),
                                             (64, 128, 2, True, 10, 18), (64, 64, 2, False, 17, 25), (64, 64, 1, False, 75, 25),
                                             (64, 64, 1, False, 9, 18)])
def test_ext_reads_only_its_operands(ci, co, s, res, t, v):
    """y, x_res between NaN guards and the DIRECT weights w / w_res NaN-filled (the residual streams a guarded copy of w_res as its
    image): the launch reads nothing outside y / x_res, nor the direct conv weight (so the gate took the kernel), and its output
    equals the zero-guarded run."""
    m = _block(ci, co, s, res, v, 9).to(DEV)
    ops = m._packed_ops(torch.device(DEV))
    assert ops["w_wino_ext"] is not None
    y_h, x_h = torch.rand(3, co, t, v), torch.rand(3, ci, t, v)
    outs = []
    for fill in (float("nan"), 0.0):
        y = _guarded(y_h.to(DEV), fill)
        x = _guarded(x_h.to(DEV), fill) if res else None
        w_direct = torch.full_like(ops["w"], fill)
        w_res = _guarded(ops["w_res"], fill) if res else None
        img = _guarded(ops["w_wino_ext"], fill)
        out = pkg.blocks.tcn_stage(y, w_direct, ops["bias"], co, 9, s, 4, relu=True, res_mode=2 if res else 0, x_res=x, w_res=w_res,
                                   w_wino_ext=img)
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert bool(torch.isfinite(outs[0]).all()), "the launch read outside its operands or read the direct weight"
    assert torch.equal(outs[0], outs[1])


def test_s2_block_is_graph_capturable():
    m = _block(64, 128, 2, True, 25, 11).to(DEV)
    x = torch.rand(2, 64, 40, 25, device=DEV)
    for _ in range(2):
        ref = m(x)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m(x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    x2 = torch.rand(2, 64, 40, 25, device=DEV)
    x.copy_(x2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, m(x2))


def test_ext_gate_falls_back_to_the_direct_kernels():
    """Shapes outside the gate (c_out not a multiple of 64, V = 20, stride 2 with an identity residual) run csk_tcn_stage_f32 from
    the new entry: the same bits as the direct call."""
    for (ci, co, s, mode, v) in [(64, 40, 2, 2, 25), (64, 128, 2, 2, 20), (64, 64, 2, 1, 25)]:
        a = torch.zeros(3, v, v)
        a[:, range(v), range(v)] = 1.0
        m = pkg.SpatioTemporalBlock(ci, co, a, stride=s, residual=True).eval().to(DEV)
        x = torch.rand(2, ci, 20, v, device=DEV)
        y = m.gcn(x)
        ops = m._packed_ops(x.device)
        # identity residual at stride 2: out[t'] pairs with x_res[2 t'] (c_res == c_out, t_res == t_in)
        kw = dict(relu=True, res_mode=mode, x_res=x, w_res=ops["w_res"] if mode == 2 else None)
        want = pkg.blocks.tcn_stage(y, ops["w"], ops["bias"], co, 9, s, 4, **kw)
        got = pkg.blocks.tcn_stage(y, ops["w"], ops["bias"], co, 9, s, 4, w_wino_ext=ops["w_wino_ext"], **kw)
        assert ops["w_wino_ext"] is not None and torch.equal(got, want), (ci, co, s, mode, v)
