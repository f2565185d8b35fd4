"""The K loop of the Winograd clip temporal convs (csrc/tcn_wino.hip) with its operands read ahead in registers, pinned on the
device.  The integer operands of tests/wino_kloop_fixture.py make every product and partial sum exact in fp32 in any order (bound
asserted below and in tests/test_wino_kloop_fixture_cpu.py), so every launch must equal an fp64 conv BIT FOR BIT: one, two and
three chunks, border and interior tiles, both workgroup shapes, stride 2 with and without the conv residual, the valid form with
the identity and the conv residual.  y, x_res and the output lie between NaN guards and the direct conv weight is NaN (a launch
the Winograd gate left to the direct kernels would show).  On top: the wide and the tall shape agree bitwise, and a sequence
launched alone (n_seg = 1) agrees bitwise with itself inside the batch of three.

The workgroup shape is forced with the diagnostic switch (CSK_DIAG=1, CSK_TCN_WINO=2 wide / =3 tall), which the library honours
only if CSK_DIAG was set when it was loaded: one child process computes every output once, the tests compare them."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import wino_kloop_fixture as fx  # noqa: E402

DEV = "cuda:0"
GUARD = 1 << 14
NAN = float("nan")
CASES = fx.cases()
IDS = [fx.case_id(c) for c in CASES]
ARMS = {"wide": "2", "tall": "3"}

assert fx.partial_sum_bound() < 2 ** 24


def _arms(case):
    return ("wide", "tall") if case[3] % 128 == 0 else ("wide",)


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


def _launch(pkg, d):
    """the Winograd entry of the form on guarded operands -> (output on the host, guards intact)"""
    fold = pkg.fold
    ones = torch.ones(d["co"], dtype=torch.float64)
    s2 = d["form"] == "s2"
    img = (fold.pack_conv_weight_wino_s2 if s2 else fold.pack_conv_weight_wino)(d["w"], ones)
    assert torch.equal(img, img.round())                                  # the transformed weights are integers
    direct = torch.full((9,) + tuple(img.shape[1:]), NAN, device=DEV)       # never read: the Winograd kernels take these shapes
    y = _Guarded(d["y"].shape, d["y"])
    x = _Guarded(d["x"].shape, d["x"]) if "x" in d else None
    wres = fold.pack_conv_weight(d["wres"], ones).to(DEV) if "wres" in d else None
    t_out = {"s1": d["t"], "valid": d["t"] - 8, "s2": (d["t"] - 1) // 2 + 1}[d["form"]]
    out = _Guarded((d["y"].shape[0], d["co"], t_out, d["v"]))
    kw = dict(relu=True, res_mode={"none": 0, "identity": 1, "conv": 2}[d["res"]], x_res=x.t if x else None, w_res=wres, out=out.t)
    bias = fold.pad_vec(d["bias"]).to(DEV)
    img = img.to(DEV)
    if d["form"] == "valid" and d["res"] == "conv":
        pkg.blocks.tcn_stage(y.t, direct, bias, d["co"], 9, 1, 0, res_off=4, w_wino_valid_res=img, **kw)
    elif d["form"] == "valid":
        pkg.blocks.tcn_stage(y.t, direct, bias, d["co"], 9, 1, 0, res_off=4, w_wino_valid=img, **kw)
    elif s2:
        pkg.blocks.tcn_stage(y.t, direct, bias, d["co"], 9, 2, 4, w_wino_ext=img, **kw)
    else:
        pkg.blocks.tcn_stage(y.t, direct, bias, d["co"], 9, 1, 4, w_wino=img, **kw)
    torch.cuda.synchronize()
    return out.t.cpu(), all(b.guards_intact() for b in (y, out) + ((x,) if x else ()))


def _child(path):
    """Every output the tests compare, keyed by (case index, arm) and (case index, arm + '_alone')."""
    os.environ["CSK_DIAG"] = "1"
    import _bootstrap
    pkg = _bootstrap.load()
    out = {}
    for i, case in enumerate(CASES):
        d = fx.operands(case, 100 + i)
        one = dict(d, y=d["y"][1:2].contiguous())
        if "x" in d:
            one["x"] = d["x"][1:2].contiguous()
        for arm in _arms(case):
            os.environ["CSK_TCN_WINO"] = ARMS[arm]
            out[(i, arm)] = _launch(pkg, d)
            out[(i, arm + "_alone")] = _launch(pkg, one)
    os.environ.pop("CSK_TCN_WINO", None)
    torch.save(out, path)


@pytest.fixture(scope="module")
def outs(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("wino_kloop") / "outs.pt")
    env = {k: val for k, val in os.environ.items() if k != "CSK_TCN_WINO"}
    subprocess.check_call([sys.executable, os.path.abspath(__file__), path], env=env)
    return torch.load(path)


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_equals_fp64_bit_for_bit(outs, i):
    want = fx.reference(fx.operands(CASES[i], 100 + i))
    for arm in _arms(CASES[i]):
        got, intact = outs[(i, arm)]
        assert intact, f"a guard was overwritten: {IDS[i]} {arm}"
        assert bool(torch.isfinite(got).all()), f"read outside the operands, or the direct kernels ran: {IDS[i]} {arm}"
        assert bool(got.abs().max() > 0)
        assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} outputs differ from fp64: {IDS[i]} {arm}"


@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if len(_arms(c)) == 2], ids=[IDS[i] for i, c in enumerate(CASES) if len(_arms(c)) == 2])
def test_wide_and_tall_agree_bitwise(outs, i):
    assert torch.equal(outs[(i, "wide")][0], outs[(i, "tall")][0])
    assert torch.equal(outs[(i, "wide_alone")][0], outs[(i, "tall_alone")][0])


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_one_sequence_alone_agrees_with_the_batch_bitwise(outs, i):
    for arm in _arms(CASES[i]):
        alone, intact = outs[(i, arm + "_alone")]
        assert intact and bool(torch.isfinite(alone).all())
        assert torch.equal(alone, outs[(i, arm)][0][1:2]), f"{IDS[i]} {arm}"


if __name__ == "__main__":
    _child(sys.argv[1])
