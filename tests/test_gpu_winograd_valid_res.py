"""csk_tcn_stage_wino_valid_res_f32: the valid (pad 0) Winograd temporal conv with the 1 x 1 conv + BN residual on the centred
shrink, out[u] = ReLU(conv9(y)[u] + w_res . x[u + 4] + bias), in both workgroup shapes (wide 64 x 128 pair columns; tall 128 x 64
where c_out % 128 == 0).

Shapes: three sequences; (c_res -> c_out) 16 -> 64, 64 -> 128, 128 -> 256; t_in 24, 25, 41 (t_out 16 even, 17 odd, 33 odd and ending
inside a tile); V 25 and 18.  The workgroup shape is forced with the diagnostic switch (CSK_DIAG=1, CSK_TCN_WINO=2 wide / =3 tall),
which the library honours only if CSK_DIAG was set when it was loaded: one child process computes every output once (as
tests/test_gpu_winograd_tiles.py), the tests compare them with the fp64 conv computed here.

(1) within 1e-4 of the fp64 direct computation; (2) with w_res = 0 bit for bit csk_tcn_stage_wino_valid_f32 without residual;
(3) an exact fixture -- integer activations, conv weights that are multiples of 4 (integer transformed weights), integer w_res,
every partial sum below 2^24 -- equals fp64 bit for bit: a wrong sign on M3 or a wrong frame offset cannot hide in rounding;
(4) operands between NaN guards: finite, bit for bit the unguarded run, guards behind the output intact; (5) unsupported shapes
answer -2 and write nothing.  The entry does not exist before this form was added: the file fails there."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N_SEG = 3
CASES = [(cr, co, t, v) for v in (25, 18) for (cr, co) in ((16, 64), (64, 128), (128, 256)) for t in (24, 25, 41)]
IDS = ["%dto%d-T%d-V%d" % c for c in CASES]
ARMS = {"default": None, "wide": "2", "tall": "3"}
GUARD, PAD = 7.25, 4096


def _arms(co):
    return [a for a in ARMS if a != "tall" or co % 128 == 0]


def _operands(i, exact=False):
    """y (n, c_out, t, V), x (n, c_res, t, V), conv weight (c_out, c_out, 9), w_res (c_out, c_res), bias (c_out,) -- fp32 on the CPU.
    exact: integers, the conv weight in multiples of 4; |sum| <= 9 * 256 * 3 * 8 + 128 * 3 * 3 + 8 < 2^24 whatever the order."""
    cr, co, t, v = CASES[i]
    g = torch.Generator().manual_seed(1000 + i)
    if exact:
        y = torch.randint(-3, 4, (N_SEG, co, t, v), generator=g).float()
        x = torch.randint(-3, 4, (N_SEG, cr, t, v), generator=g).float()
        w = 4.0 * torch.randint(-2, 3, (co, co, 9), generator=g).float()
        wr = torch.randint(-3, 4, (co, cr), generator=g).float()
        b = torch.randint(-8, 9, (co,), generator=g).float()
    else:
        y = torch.rand((N_SEG, co, t, v), generator=g) - 0.5
        x = torch.rand((N_SEG, cr, t, v), generator=g) - 0.5
        w = (torch.rand((co, co, 9), generator=g) - 0.5) * (12.0 / (9 * co)) ** 0.5 * 2
        wr = (torch.rand((co, cr), generator=g) - 0.5) * (12.0 / cr) ** 0.5
        b = torch.rand((co,), generator=g) - 0.5
    return y, x, w, wr, b


def _reference(y, x, w, wr, b):
    """fp64: ReLU(conv9 valid + w_res . x[u + 4] + bias)."""
    t = y.shape[2]
    z = torch.nn.functional.conv2d(y.double(), w.double().unsqueeze(-1))
    r = torch.einsum("oc,nctv->notv", wr.double(), x.double()[:, :, 4: t - 4])
    return torch.relu(z + r + b.double().view(1, -1, 1, 1))


def _guarded(t, fill, pad=PAD):
    buf = torch.full((t.numel() + 2 * pad,), fill, device=DEV)
    v = buf[pad: pad + t.numel()].view(t.shape)
    v.copy_(t)
    return v, buf


def _child(path):
    os.environ["CSK_DIAG"] = "1"
    sys.path.insert(0, ROOT)
    import _bootstrap
    pkg = _bootstrap.load()
    fold, native = pkg.fold, pkg.native
    lib = native.lib()

    def entry(y, x, w_res, bias, out, w_wino, t_in=None, k=9, stride=1, pad=0, mode=2, res_off=4, c_res=None, t_res=None):
        n, co, t, v = y.shape
        return lib.csk_tcn_stage_wino_valid_res_f32(
            native.ptr(y), native.ptr(x), native.ptr(w_res), native.ptr(bias), native.ptr(out), n, co, out.shape[1], t if t_in is None else t_in,
            v, k, stride, pad, mode, x.shape[1] if c_res is None else c_res, x.shape[2] if t_res is None else t_res, res_off, 1,
            native.ptr(w_wino), native.stream_of(y))

    res = {}
    for i, (cr, co, t, v) in enumerate(CASES):
        for exact in (False, True):
            y, x, w, wr, b = (a.to(DEV) for a in _operands(i, exact))
            one = torch.ones(co, dtype=torch.float64)
            w_wino = fold.pack_conv_weight_wino(w.cpu(), one).to(DEV)
            w_dir = fold.pack_conv_weight(w.cpu().unsqueeze(-1), one).to(DEV)
            w_res = fold.pack_conv_weight(wr.cpu().view(co, cr, 1, 1), one).to(DEV)
            bias = fold.pad_vec(b.cpu().double()).to(DEV)
            for arm in _arms(co):
                if ARMS[arm] is None:
                    os.environ.pop("CSK_TCN_WINO", None)
                else:
                    os.environ["CSK_TCN_WINO"] = ARMS[arm]
                out, buf = _guarded(torch.zeros((N_SEG, co, t - 8, v)), GUARD)
                rc = entry(y, x, w_res, bias, out, w_wino)
                torch.cuda.synchronize()
                key = (i, arm, "exact" if exact else "rand")
                res[key] = (rc, out.cpu().clone(), bool((buf[:PAD] == GUARD).all()) and bool((buf[PAD + out.numel():] == GUARD).all()))
                if exact:
                    continue
                # (2) w_res = 0 against the valid entry without residual, the same operands
                out0 = torch.empty_like(out)
                rc0 = entry(y, x, torch.zeros_like(w_res), bias, out0, w_wino)
                none = pkg.blocks.tcn_stage(y, w_dir, bias, co, 9, 1, 0, relu=True, w_wino_valid=w_wino)
                res[(i, arm, "zero")] = (rc0, out0.cpu(), none.cpu())
                # (4) every operand between NaN guards
                gy, gx, gwr, gb, gww = (_guarded(a, float("nan"))[0] for a in (y, x, w_res, bias, w_wino))
                gout, gbuf = _guarded(torch.zeros((N_SEG, co, t - 8, v)), float("nan"))
                rcg = entry(gy, gx, gwr, gb, gout, gww)
                torch.cuda.synchronize()
                n_nan = int(torch.isnan(gbuf).sum())
                res[(i, arm, "nan")] = (rcg, gout.cpu().clone(), n_nan == 2 * PAD)
            os.environ.pop("CSK_TCN_WINO", None)
            if exact or i % 9:
                continue
            # (5) not shapes of the kernel: -2, nothing written
            out, buf = _guarded(torch.zeros((N_SEG, co, t - 8, v)), GUARD)
            out.fill_(GUARD)
            odd_x = x[:, : cr - 8].contiguous()
            refused = dict(stride2=entry(y, x, w_res, bias, out, w_wino, stride=2), pad4=entry(y, x, w_res, bias, out, w_wino, pad=4),
                           k3=entry(y, x, w_res, bias, out, w_wino, k=3), identity=entry(y, x, w_res, bias, out, w_wino, mode=1),
                           none=entry(y, x, w_res, bias, out, w_wino, mode=0), res_off0=entry(y, x, w_res, bias, out, w_wino, res_off=0),
                           c_res8=entry(y, odd_x, w_res, bias, out, w_wino), t_res=entry(y, x, w_res, bias, out, w_wino, t_res=t - 1),
                           short=entry(y, x, w_res, bias, out, w_wino, t_in=8, t_res=8), no_w_res=entry(y, x, None, bias, out, w_wino),
                           no_image=entry(y, x, w_res, bias, out, None))
            yv = torch.zeros((1, 64, 24, 20), device=DEV)
            refused["V20"] = entry(yv, torch.zeros((1, 16, 24, 20), device=DEV), w_res, bias, out, w_wino)
            y72 = torch.zeros((1, 72, 24, v), device=DEV)
            refused["c_out72"] = lib.csk_tcn_stage_wino_valid_res_f32(
                native.ptr(y72), native.ptr(x), native.ptr(w_res), native.ptr(bias), native.ptr(out), 1, 72, 72, 24, v, 9, 1, 0, 2, cr, 24, 4, 1,
                native.ptr(w_wino), native.stream_of(y))
            torch.cuda.synchronize()
            res[(i, "refused")] = (refused, bool((buf == GUARD).all()))
    torch.save(res, path)


@pytest.fixture(scope="module")
def outs(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("wino_valid_res") / "outs.pt")
    env = {k: val for k, val in os.environ.items() if k != "CSK_TCN_WINO"}
    subprocess.check_call([sys.executable, os.path.abspath(__file__), path], env=env)
    return torch.load(path)


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_fp64(outs, i):
    """(1) every shape took the kernel (rc 0), within 1e-4 of fp64 (check_parity), guards intact; wide, tall and the host's own
    choice agree bit for bit."""
    from tests.helpers import check_parity
    want = _reference(*_operands(i)).float()
    assert float(want.max()) > 0.5                                # not all clipped by the ReLU
    for arm in _arms(CASES[i][1]):
        rc, got, guards = outs[(i, arm, "rand")]
        assert rc == 0 and guards
        print(f"{IDS[i]} {arm}: max |err| {float((got.double() - _reference(*_operands(i))).abs().max()):.3e}")
        check_parity(got, want, case=IDS[i], arm=arm, what="wino_valid_res vs fp64")
        assert torch.equal(got, outs[(i, "default", "rand")][1])


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_zero_residual_weight_is_the_valid_form_without_residual(outs, i):
    for arm in _arms(CASES[i][1]):
        rc, got, none = outs[(i, arm, "zero")]
        assert rc == 0 and torch.equal(got, none)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_exact_fixture_equals_fp64_bit_for_bit(outs, i):
    y, x, w, wr, b = _operands(i, exact=True)
    want = _reference(y, x, w, wr, b)
    assert float(want.max()) < 2 ** 24 and torch.equal(want, want.float().double())
    no_res = _reference(y, torch.zeros_like(x), w, wr, b)
    assert not torch.equal(no_res, want)
    for arm in _arms(CASES[i][1]):
        rc, got, guards = outs[(i, arm, "exact")]
        assert rc == 0 and guards and torch.equal(got.double(), want)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_reads_only_its_operands(outs, i):
    for arm in _arms(CASES[i][1]):
        rc, got, guards = outs[(i, arm, "nan")]
        assert rc == 0 and bool(torch.isfinite(got).all()), "the launch read outside its operands"
        assert guards, "a guard value next to the output was overwritten"
        assert torch.equal(got, outs[(i, arm, "rand")][1])


@pytest.mark.parametrize("i", [i for i in range(len(CASES)) if i % 9 == 0], ids=[IDS[i] for i in range(len(CASES)) if i % 9 == 0])
def test_unsupported_shapes_answer_minus_2_and_write_nothing(outs, i):
    refused, untouched = outs[(i, "refused")]
    assert refused and all(rc == -2 for rc in refused.values()), refused
    assert untouched


def test_block_falls_back_to_the_direct_kernel_where_the_entry_refuses():
    """blocks.tcn_stage(w_wino_valid_res=) on a shape the entry refuses (c_res = 8) gives the direct kernel's bits."""
    sys.path.insert(0, ROOT)
    import _bootstrap
    pkg = _bootstrap.load()
    m = pkg.SpatioTemporalBlock(8, 64, pkg.ntu_graph().A, temporal_padding=0).eval().to(DEV)
    x = torch.rand((2, 8, 20, 25), generator=torch.Generator().manual_seed(4)).to(DEV)
    want = m(x)
    m.wino_valid_res = True
    assert torch.equal(m(x), want) and tuple(want.shape) == (2, 64, 12, 25)
    m2 = pkg.SpatioTemporalBlock(16, 64, pkg.ntu_graph().A, temporal_padding=0).eval().to(DEV)
    x2 = torch.rand((2, 16, 20, 25), generator=torch.Generator().manual_seed(5)).to(DEV)
    direct = m2(x2)
    m2.wino_valid_res = True
    got = m2(x2)
    assert not torch.equal(got, direct) and float((got - direct).abs().max()) <= 1e-5 * max(1.0, float(direct.abs().max()))


if __name__ == "__main__":
    _child(sys.argv[1])
