"""The Winograd F(2, 3) clip temporal convs (csrc/tcn_wino.hip: csk_tcn_stage_wino_f32, csk_tcn_stage_wino_ext_f32,
csk_tcn_stage_wino_valid_f32, csk_tcn_stage_wino_valid_res_f32) pinned on the device, at the ABI, with the cases of
tests/tcn_wino_fixture.py.  Which instantiation each case runs, and that the cases reach all 28 of them and every kind of tile, is
shown on the CPU (tests/test_tcn_wino_fixture_cpu.py).  No kernel is compared with another kernel: every reference is the fp64
definition.

Every launch the gate is expected to take gets a DIRECT weight image full of NaN: a silent fall-back to the direct kernels fails
the test instead of passing it.  y, x_res and the output lie between NaN guards, the output is NaN before the launch.

1. Exact tier: integer operands make the transformed problem exact in halves, so every launch -- ReLU off but for one case per
   entry, both signs compared -- must equal the fp64 conv BIT FOR BIT; and each case launched with its first sequence alone gives
   that sequence's bits.
2. Routing tier: unique ids under one-hot weights, one case per tap and kernel and one per residual form alone.
3. NaN tier: one NaN in y under ReLU comes out at exactly the outputs the algorithm lets it reach (at stride 2 a strict superset
   of the definition's window), the rest bit-identical to the clean launch.
4. Rounding tier: random fp32 operands, |got - fp64| <= gamma(n) S everywhere (derived in the fixture, not measured); the ratios
   are printed.
5. Launches the gate refuses run the direct kernels on the real direct weight and equal fp64 too."""
import pytest
import torch

import _bootstrap
from tests import tcn_wino_fixture as fx

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
fold = pkg.fold
DEV = "cuda:0"
GUARD = 1 << 14
NAN = float("nan")


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


def _launch(case, d=None, first_only=False):
    """the case's entry through pkg.blocks.tcn_stage on guarded operands -> (output on the host, guards intact); first_only: the
    first sequence alone"""
    d = d or fx.operands(case)
    if first_only:
        d = {k: (v[:1] if k in ("y", "x") else v) for k, v in d.items()}
    n = d["y"].shape[0]
    taken = not fx.sel_of(case._replace(n=n)).reject
    ones = torch.ones(case.co, dtype=torch.float64)
    w = fold.pack_conv_weight(d["w"], ones)
    image = (fold.pack_conv_weight_wino_s2 if case.stride == 2 else fold.pack_conv_weight_wino)(d["w"], ones).to(DEV)
    if taken:
        w = torch.full_like(w, NAN)                                  # the direct kernels must not run
    bias = fold.pad_vec(d["bias"]).to(DEV)
    y = _Guarded(d["y"].shape, d["y"])
    x = _Guarded(d["x"].shape, d["x"]) if "x" in d else None
    wres = fold.pack_conv_weight(d["wres"], ones).to(DEV) if "wres" in d else None
    out = _Guarded((n, case.co, case.t_out, case.v))
    kw = dict(relu=bool(case.relu), res_mode=fx.RES_MODE[case.res], x_res=x.t if x else None, w_res=wres, res_off=case.res_off,
              out=out.t)
    kw[fx.ENTRY_KW[case.entry]] = image
    pkg.blocks.tcn_stage(y.t, w.to(DEV), bias, case.co, 9, case.stride, case.pad, **kw)
    torch.cuda.synchronize()
    return out.t.cpu(), all(b.guards_intact() for b in (y, out) + ((x,) if x else ()))


def _compare(case, got, intact, want=None):
    if want is None:
        want = fx.reference(case) if case.tier == "exact" else fx.routing_expected(case)
    assert intact, f"a guard was overwritten: {case.name}"
    assert bool(torch.isfinite(got).all()), f"the direct kernels ran, or a read outside the operands, or outputs left unwritten: {case.name}"
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} outputs differ from fp64: {case.name}"


@pytest.mark.parametrize("group", fx.EXACT_GROUPS)
def test_launch_equals_fp64(group):
    for case in fx.GROUPS[group]:
        assert fx.partial_sum_bound(case) < 2 ** 23
        got, intact = _launch(case)
        _compare(case, got, intact)
        solo, intact = _launch(case, first_only=True)                # tiles do not cross sequences
        _compare(case, solo, intact, got[:1])


@pytest.mark.parametrize("group", fx.ROUTE_GROUPS)
def test_every_output_comes_from_the_right_input(group):
    for case in fx.GROUPS[group]:
        _compare(case, *_launch(case))


@pytest.mark.parametrize("which", range(len(fx.NAN_CASES)), ids=[c.group for c, _ in fx.NAN_CASES])
def test_one_nan_reaches_exactly_the_outputs_the_algorithm_lets_it_reach(which):
    case, idxs = fx.NAN_CASES[which]
    clean, intact = _launch(case)
    _compare(case, clean, intact)
    for idx in idxs:
        d = dict(fx.operands(case))
        d["y"] = d["y"].clone()
        d["y"][idx] = NAN
        got, intact = _launch(case, d)
        mask = fx.nan_mask(case, idx)
        assert intact and bool(mask.any())
        wrong = int((torch.isnan(got) != mask).sum())
        assert wrong == 0, f"{wrong} outputs are NaN or not against the algorithm's reach: {case.name} {idx}"
        assert torch.equal(got[~mask], clean[~mask]), (case.name, idx)


def test_rounding_stays_inside_the_derived_bound(capsys):
    lines, worst = [], 0.0
    for case in fx.GROUPS["round"]:
        got, intact = _launch(case)
        assert intact and bool(torch.isfinite(got).all()), case.name
        ratio = ((got.double() - fx.reference(case)).abs() / fx.error_bound(case)).max().item()
        lines.append(f"  {case.name:62s} n {fx.roundings(case):4d}  err / bound {ratio:.4f}")
        worst = max(worst, ratio)
    with capsys.disabled():
        print("\nlargest err / bound per rounding case\n" + "\n".join(lines))
    assert worst <= 1.0, "\n".join(lines)


def test_refused_launches_run_the_direct_kernels():
    for case in fx.REJECTED:
        assert fx.sel_of(case).reject
        _compare(case, *_launch(case))
    case = fx.Case("gate", 8, "valid", 12, 64, 8, 25)               # 8 frames, pad 0: no output frame; the host refuses it first
    assert fx.sel_of(case).reject
    with pytest.raises(RuntimeError):
        _launch(case)
