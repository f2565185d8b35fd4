"""Border tiles and the conv-residual phases of the Winograd clip temporal convs (csrc/tcn_wino.hip), pinned on the device.

1. Exact arithmetic: the integer operands of tests/tcn_border_fixture.py make every product and partial sum exact in fp32 in any
   order (bound asserted below and in tests/test_tcn_border_fixture_cpu.py), so each launch must equal an fp64 conv BIT FOR BIT --
   sequences that are all border, odd T, the first interior tiles, every chunk pattern of the stride-2 residual phase, and the valid
   form with its conv residual.  y, x_res and the output lie between NaN guards; the direct conv weight is NaN (a launch the
   Winograd gate left to the direct kernels would show).
2. A tile that is a border tile of a short launch and an interior tile of a launch on the same data embedded in zeros: bitwise equal.
3. Batch invariance, bitwise."""
import pytest
import torch
import torch.nn.functional as F

import _bootstrap
from tests import tcn_border_fixture as fx

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
fold = pkg.fold
DEV = "cuda:0"
GUARD = 1 << 14
NAN = float("nan")

assert max(fx.partial_sum_bound(c, r) for c in fx.C_IN for r in (0,) + fx.S2_CRES + fx.VALID_CRES) < 2 ** 24


class _Guarded:
    """a device tensor between two NaN guards"""

    def __init__(self, shape, src=None):
        n = 1
        for d in shape:
            n *= d
        self.buf = torch.full((n + 2 * GUARD,), NAN, device=DEV)
        self.t = self.buf[GUARD: GUARD + n].view(shape)
        if src is not None:
            self.t.copy_(src)

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[-GUARD:]).all())


def _ints(gen, shape, lo, hi, step=1):
    return (torch.randint(0, (hi - lo) // step + 1, shape, generator=gen) * step + lo).float()


def _case(form, v, c, co, t, res, c_res, seed, n=fx.N_SEG, floats=False):
    """operands of one launch (host): form 's1' | 's2' | 'valid'; res 'none' | 'identity' | 'conv'"""
    g = torch.Generator().manual_seed(seed)
    if floats:
        rnd = lambda shape, *_: torch.rand(shape, generator=g) - 0.5
    else:
        rnd = lambda shape, lo, hi, step=1: _ints(g, shape, lo, hi, step)
    d = dict(form=form, v=v, c=c, co=co, t=t, res=res)
    d["y"] = rnd((n, c, t, v), -fx.ACT, fx.ACT)
    d["w"] = rnd((co, c, 9, 1), -fx.W_EVEN, fx.W_EVEN, 2)
    d["bias"] = rnd((co,), -fx.BIAS, fx.BIAS)
    if res == "identity":
        d["x"] = rnd((n, co, t, v), -fx.ACT, fx.ACT)
    elif res == "conv":
        d["x"] = rnd((n, c_res, t, v), -fx.ACT, fx.ACT)
        d["wres"] = rnd((co, c_res, 1, 1), -fx.W_RES, fx.W_RES)
    return d


def _reference(d):
    """the fp64 conv on the host, cast to fp32"""
    stride, pad = (2, 4) if d["form"] == "s2" else (1, 0) if d["form"] == "valid" else (1, 4)
    out = F.conv2d(d["y"].double(), d["w"].double(), d["bias"].double(), stride=(stride, 1), padding=(pad, 0))
    if d["res"] == "identity":
        out = out + d["x"].double()
    elif d["res"] == "conv":
        x = d["x"].double()
        out = out + F.conv2d(x[:, :, 4: d["t"] - 4] if d["form"] == "valid" else x, d["wres"].double(), stride=(stride, 1))
    return torch.relu(out).float()


def _launch(d, exact=True):
    """the Winograd entry of the form on guarded operands -> (output on the host, guards intact)"""
    ones = torch.ones(d["co"], dtype=torch.float64)
    s2 = d["form"] == "s2"
    img = (fold.pack_conv_weight_wino_s2 if s2 else fold.pack_conv_weight_wino)(d["w"], ones)
    if exact:
        assert torch.equal(img, img.round())                              # the transformed weights are integers
    direct = torch.full((9,) + tuple(img.shape[1:]), NAN, device=DEV)       # never read: the Winograd kernels take these shapes
    y = _Guarded(d["y"].shape, d["y"])
    x = _Guarded(d["x"].shape, d["x"]) if "x" in d else None
    wres = fold.pack_conv_weight(d["wres"], ones).to(DEV) if "wres" in d else None
    t_out = {"s1": d["t"], "valid": d["t"] - 8, "s2": (d["t"] - 1) // 2 + 1}[d["form"]]
    out = _Guarded((d["y"].shape[0], d["co"], t_out, d["v"]))
    kw = dict(relu=True, res_mode={"none": 0, "identity": 1, "conv": 2}[d["res"]], x_res=x.t if x else None, w_res=wres, out=out.t)
    bias = fold.pad_vec(d["bias"]).to(DEV)
    img = img.to(DEV)
    if d["form"] == "valid":
        pkg.blocks.tcn_stage(y.t, direct, bias, d["co"], 9, 1, 0, res_off=4, w_wino_valid_res=img, **kw)
    elif s2 or d["res"] == "none":
        pkg.blocks.tcn_stage(y.t, direct, bias, d["co"], 9, 2 if s2 else 1, 4, w_wino_ext=img, **kw)
    else:
        pkg.blocks.tcn_stage(y.t, direct, bias, d["co"], 9, 1, 4, w_wino=img, **kw)
    torch.cuda.synchronize()
    return out.t.cpu(), all(b.guards_intact() for b in (y, out) + ((x,) if x else ()))


def _check_exact(d):
    got, intact = _launch(d)
    want = _reference(d)
    tag = {k: d[k] for k in ("form", "v", "c", "co", "t", "res")} | ({"c_res": d["x"].shape[1]} if "x" in d else {})
    assert intact, f"a guard was overwritten: {tag}"
    assert bool(torch.isfinite(got).all()), f"read outside the operands, or the direct kernels ran: {tag}"
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} outputs differ from fp64: {tag}"


@pytest.mark.parametrize("co", fx.C_OUT)
@pytest.mark.parametrize("v", fx.JOINTS)
def test_stride1_equals_fp64(v, co):
    for i, (c, t, res) in enumerate((c, t, res) for c in fx.C_IN for t in fx.S1_T for res in ("identity", "none")):
        _check_exact(_case("s1", v, c, co, t, res, 0, 1000 + i))


@pytest.mark.parametrize("co", fx.C_OUT)
@pytest.mark.parametrize("v", fx.JOINTS)
def test_stride2_equals_fp64(v, co):
    for i, (c, t, c_res) in enumerate((c, t, r) for c in fx.C_IN for t in fx.S2_T for r in (0,) + fx.S2_CRES):
        _check_exact(_case("s2", v, c, co, t, "conv" if c_res else "none", c_res, 2000 + i))


@pytest.mark.parametrize("co", fx.C_OUT)
@pytest.mark.parametrize("v", fx.JOINTS)
def test_valid_form_with_conv_residual_equals_fp64(v, co):
    for i, (c, t, c_res) in enumerate((c, t, r) for c in fx.C_IN for t in fx.VALID_T for r in fx.VALID_CRES):
        _check_exact(_case("valid", v, c, co, t, "conv", c_res, 3000 + i))


def _embed(d, front, back):
    """the same launch on rows with `front` / `back` zero frames around the data"""
    e = dict(d, t=front + d["t"] + back)
    for k in ("y", "x"):
        if k in d:
            e[k] = F.pad(d[k], (0, 0, front, back))
    return e


@pytest.mark.parametrize("co", fx.C_OUT)
@pytest.mark.parametrize("v", fx.JOINTS)
@pytest.mark.parametrize("form", ["s1", "s2"])
def test_interior_and_border_tiles_agree_bitwise(form, v, co):
    """zero frames around the data are what the conv's padding supplies, so the launch on the embedded row computes the short
    launch's outputs from the same values -- in interior tiles where the short launch has border tiles (asserted on the CPU:
    test_embedding_turns_border_tiles_into_interior_tiles).  Random float data: same bits, not merely close."""
    t, front, back = fx.LONG_S1 if form == "s1" else fx.LONG_S2
    stride = 2 if form == "s2" else 1
    d = _case(form, v, 24, co, t, "conv" if form == "s2" else "identity", 24, 7, floats=True)
    d["bias"] = torch.zeros(co)                        # the embedded row's residual and conv are zero outside the data
    short, ok_s = _launch(d, exact=False)
    long_, ok_l = _launch(_embed(d, front, back), exact=False)
    assert ok_s and ok_l
    assert bool(torch.isfinite(short).all()) and bool(short.abs().max() > 0)
    lo = front // stride
    assert torch.equal(long_[:, :, lo: lo + short.shape[2]], short)


@pytest.mark.parametrize("form,t", [("s1", 40), ("s2", 61)])
def test_batch_invariance_bitwise(form, t):
    d = _case(form, 25, 24, 128, t, "conv" if form == "s2" else "identity", 24, 11, floats=True)
    full, ok = _launch(d, exact=False)
    one = dict(d, y=d["y"][1:2].contiguous(), x=d["x"][1:2].contiguous())
    alone, ok1 = _launch(one, exact=False)
    assert ok and ok1 and bool(torch.isfinite(full).all())
    assert torch.equal(alone, full[1:2])
