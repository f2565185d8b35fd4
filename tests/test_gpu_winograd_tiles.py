"""GPU tests of the two workgroup shapes of the Winograd temporal convs (csrc/tcn_wino.hip): wide, 64 channels x 128 pair columns,
and tall, 128 channels x 64 pair columns.  A wave's tile and MFMA order are the same in both, so the two give the same bits; the
host takes per layer the one that issues fewer columns.  On the smallest shapes that reach both shapes, a partial last tile, the
zero-padding tiles at both ends of a sequence and, for the stride-2 conv residual, more than one residual chunk:
(a) wide, tall and the host's own choice agree bit for bit, (b) they stay within 1e-5 of the direct kernels on O(1) outputs,
(c) they read nothing outside their operands (NaN guards; w_res stays finite), (d) two sequences give the same bits alone and
inside a batch of five.

The shapes are selected with the diagnostic switch (CSK_DIAG=1, CSK_TCN_WINO=2 wide / =3 tall / =1 direct), which the library
honours only if CSK_DIAG was set when it was loaded: one child process computes every output once, the tests compare them."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

# (form, c_in, c_out, stride, residual, T, V)
CASES = [(name, ci, co, s, res, t, v) for v in (25, 18) for (name, ci, co, s, res, t) in (
    ("s1_identity", 128, 128, 1, True, 11), ("s1_identity", 256, 256, 1, True, 6), ("s1_none", 128, 128, 1, False, 11),
    ("s2_conv", 64, 128, 2, True, 21), ("s2_none", 128, 128, 2, False, 21))]
IDS = ["%s-%dto%d-T%d-V%d" % (c[0], c[1], c[2], c[5], c[6]) for c in CASES]
ARMS = {"default": None, "wide": "2", "tall": "3", "direct": "1"}


def _guarded(t, fill, pad=1 << 14):
    buf = torch.full((t.numel() + 2 * pad,), fill, device=DEV)
    v = buf[pad: pad + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _child(path):
    """Every output the tests compare, keyed by (case index, name)."""
    os.environ["CSK_DIAG"] = "1"
    sys.path.insert(0, ROOT)
    import _bootstrap
    import bench
    pkg = _bootstrap.load()

    def arm(value):
        if value is None:
            os.environ.pop("CSK_TCN_WINO", None)
        else:
            os.environ["CSK_TCN_WINO"] = value

    out = {}
    for i, (name, ci, co, s, res, t, v) in enumerate(CASES):
        A = (pkg.ntu_graph() if v == 25 else pkg.kinetics_graph()).A
        blk = pkg.SpatioTemporalBlock(ci, co, A, stride=s, residual=res).eval()
        bench.randomise_(blk, 3)
        blk = blk.to(DEV)
        ops = blk._packed_ops(torch.device(DEV))
        mode = 0 if not res else 1 if name == "s1_identity" else 2
        img = "w_wino" if mode == 1 else "w_wino_ext"
        assert ops[img] is not None
        x5 = torch.rand((5, ci, t, v), generator=torch.Generator().manual_seed(7 + i)).to(DEV)
        y5 = blk.gcn(x5)
        x2, y2 = x5[[1, 3]].contiguous(), y5[[1, 3]].contiguous()

        def run(y, x, w=None, w_res=None, image=None):
            kw = {img: ops[img] if image is None else image}
            return pkg.blocks.tcn_stage(y, ops["w"] if w is None else w, ops["bias"], co, 9, s, 4, relu=True, res_mode=mode,
                                        x_res=x if mode else None, w_res=(ops["w_res"] if w_res is None else w_res) if mode == 2 else None,
                                        **kw)

        for a, value in ARMS.items():
            arm(value)
            out[(i, a)] = run(y2, x2).cpu()
            if a in ("wide", "tall"):
                out[(i, a + "_of5")] = run(y5, x5)[[1, 3]].cpu()
                for fill in (float("nan"), 0.0):
                    g = run(_guarded(y2, fill), _guarded(x2, fill), w=torch.full_like(ops["w"], fill),
                            w_res=_guarded(ops["w_res"], fill) if mode == 2 else None, image=_guarded(ops[img], fill))
                    torch.cuda.synchronize()
                    out[(i, a + ("_nan" if fill != 0.0 else "_zero"))] = g.cpu()
        arm(None)
    torch.save(out, path)


@pytest.fixture(scope="module")
def outs(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("wino_tiles") / "outs.pt")
    env = {k: val for k, val in os.environ.items() if k != "CSK_TCN_WINO"}
    subprocess.check_call([sys.executable, os.path.abspath(__file__), path], env=env)
    return torch.load(path)


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_tile_shapes_agree_bitwise(outs, i):
    """(a) wide == tall == the host's own choice, bit for bit."""
    assert bool(torch.isfinite(outs[(i, "wide")]).all())
    assert torch.equal(outs[(i, "wide")], outs[(i, "tall")])
    assert torch.equal(outs[(i, "default")], outs[(i, "tall")])


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_tile_shapes_vs_forced_direct_path(outs, i):
    """(b) within 1e-5 of the direct kernels on O(1) outputs (check_parity caps |direct|), and not bit for bit: the Winograd
    kernels did run."""
    from tests.helpers import check_parity
    want = outs[(i, "direct")]
    for a in ("wide", "tall"):
        got = outs[(i, a)]
        print(f"{IDS[i]} {a} vs direct: max |diff| {float((got - want).abs().max()):.3e}, max |direct| {float(want.abs().max()):.3f}")
        check_parity(got, want, tol=1e-5, note="Winograd %s tile vs direct temporal conv" % a)
        assert not torch.equal(got, want)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_tile_shapes_read_only_their_operands(outs, i):
    """(c) y, x_res, the Winograd image and w_res between NaN guards, the direct conv weight NaN-filled: finite output, equal to
    the zero-guarded run and to the unguarded one."""
    for a in ("wide", "tall"):
        assert bool(torch.isfinite(outs[(i, a + "_nan")]).all()), "the launch read outside its operands or read the direct weight"
        assert torch.equal(outs[(i, a + "_nan")], outs[(i, a + "_zero")])
        assert torch.equal(outs[(i, a + "_nan")], outs[(i, a)])


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_tile_shapes_batch_invariance_bitwise(outs, i):
    """(d) two sequences alone == the same two inside a batch of five."""
    for a in ("wide", "tall"):
        assert torch.equal(outs[(i, a)], outs[(i, a + "_of5")])


if __name__ == "__main__":
    _child(sys.argv[1])
