"""The direct clip temporal conv (csk_tcn_stage_f32 / csk_tcn_stage_splitk_f32: tcn_stage_kernel and tcn_reduce_kernel of
csrc/tcn.hip, tcn_stage16_kernel of csrc/tcn16.hip) pinned on the device, at the ABI, with the cases of tests/tcn_direct_fixture.py.
Which instantiation each case runs, and that the cases reach all of them, is shown on the CPU (tests/test_tcn_direct_fixture_cpu.py).

1. Exact tier: integer operands make every partial sum exact in fp32 in any order, so every launch -- ReLU off, both signs
   compared -- must equal the fp64 conv BIT FOR BIT; y, x_res and the output lie between NaN guards.
2. Split-K: the same, with the partial-sum buffer full of NaN before the launch; and bit for bit the unsplit launch.
3. Routing tier: unique ids as activations under one-hot weights; every output element must be the id of the input element the
   definition names, for every tap and for each residual form alone.  One NaN in y under ReLU must come out at exactly the outputs
   whose window covers it, the rest bit-identical to the NaN-free launch.
4. Both tile families at the shapes both support, each forced in a child process (CSK_TCN16 is read when the library loads) and
   each compared with the fp64 reference, not with the other."""
import os
import subprocess
import sys

import pytest
import torch

import _bootstrap
from tests import tcn_direct_fixture as fx

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
fold = pkg.fold
DEV = "cuda:0"
GUARD = 1 << 14
NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXACT_GROUPS = [g for g in fx.DEFAULT_GROUPS if g != "split" and not g.startswith("route")]
ROUTE_GROUPS = [g for g in fx.DEFAULT_GROUPS if g.startswith("route")]


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


def _launch(case, d=None):
    """csk_tcn_stage_f32 (ksplit > 1: csk_tcn_stage_splitk_f32) on guarded operands -> (output on the host, guards intact)"""
    d = d or fx.operands(case)
    ones = torch.ones(case.co, dtype=torch.float64)
    w = fold.pack_conv_weight(d["w"], ones).to(DEV)
    bias = fold.pad_vec(d["bias"]).to(DEV)
    y = _Guarded(d["y"].shape, d["y"])
    x = _Guarded(d["x"].shape, d["x"]) if "x" in d else None
    wres = fold.pack_conv_weight(d["wres"], ones).to(DEV) if "wres" in d else None
    out = _Guarded((case.n, case.co, case.t_out, case.v))
    kw = dict(relu=bool(case.relu), res_mode=fx.RES_MODE[case.res], x_res=x.t if x else None, w_res=wres, res_off=case.res_off, out=out.t)
    if case.ksplit > 1:
        scratch = pkg.blocks.SplitScratch()
        floats = case.ksplit * out.t.numel()
        part = scratch.get(out.t.device, floats)
        part.fill_(NAN)
        assert scratch.get(out.t.device, floats) is part                     # the launch below takes this very buffer
        kw.update(ksplit=case.ksplit, scratch=scratch)
    pkg.blocks.tcn_stage(y.t, w, bias, case.co, case.k, case.stride, case.pad, **kw)
    torch.cuda.synchronize()
    return out.t.cpu(), all(b.guards_intact() for b in (y, out) + ((x,) if x else ()))


def _compare(case, got, intact):
    want = fx.reference(case) if case.tier == "exact" else fx.routing_expected(case)
    assert intact, f"a guard was overwritten: {case.name}"
    assert bool(torch.isfinite(got).all()), f"read outside the operands, or outputs left unwritten: {case.name}"
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} outputs differ from fp64: {case.name}"


def _default_path():
    assert not (os.environ.get("CSK_DIAG") and os.environ.get("CSK_TCN16")), "the case tables assume the launcher's own choice of family"


@pytest.mark.parametrize("group", EXACT_GROUPS)
def test_launch_equals_fp64(group):
    _default_path()
    for case in fx.GROUPS[group]:
        assert fx.partial_sum_bound(case.c, case.c_res) < 2 ** 24
        _compare(case, *_launch(case))


def test_split_k_equals_fp64_and_the_unsplit_launch():
    _default_path()
    for case in fx.GROUPS["split"]:
        got, intact = _launch(case)
        _compare(case, got, intact)
        whole, intact = _launch(case._replace(ksplit=1))
        assert intact and torch.equal(whole, got), case.name


@pytest.mark.parametrize("group", ROUTE_GROUPS)
def test_every_output_comes_from_the_right_input(group):
    _default_path()
    for case in fx.GROUPS[group]:
        _compare(case, *_launch(case))


@pytest.mark.parametrize("which", range(len(fx.NAN_CASES)), ids=[c.group for c, _ in fx.NAN_CASES])
def test_one_nan_reaches_exactly_the_outputs_whose_window_covers_it(which):
    _default_path()
    case, idx = fx.NAN_CASES[which]
    clean, intact = _launch(case)
    _compare(case, clean, intact)
    d = dict(fx.operands(case))
    d["y"] = d["y"].clone()
    d["y"][idx] = NAN
    got, intact = _launch(case, d)
    mask = fx.nan_mask(case, idx)
    assert intact and bool(mask.any())
    assert torch.equal(torch.isnan(got), mask), f"{int((torch.isnan(got) != mask).sum())} outputs are NaN or not against the definition"
    assert torch.equal(got[~mask], clean[~mask])


def child_main(mode, path):
    """in a child process whose library was loaded with CSK_TCN16=<mode>: the launches of the forced group, saved"""
    assert os.environ.get("CSK_DIAG") and os.environ.get("CSK_TCN16") == str(mode)
    torch.save([_launch(case) for case in fx.GROUPS[f"forced-{mode}"]], path)


def test_each_tile_family_equals_fp64_at_the_shared_shapes(tmp_path):
    """CSK_TCN16=1 keeps every launch on the 32x32x2 kernels (the compile-time-18 instantiations at whole 8-channel chunks), =2 puts
    every launch the 16x16x4 kernel is built for on it (128 and 256 channels at V = 25): children one after the other, each a fresh
    interpreter with its own time limit; a child that fails ends the test."""
    for mode in (1, 2):
        path = str(tmp_path / f"forced_{mode}.pt")
        code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests import test_gpu_tcn_direct as m; m.child_main({mode}, sys.argv[1])"
        env = dict(os.environ, CSK_DIAG="1", CSK_TCN16=str(mode))
        done = subprocess.run([sys.executable, "-c", code, path], env=env, timeout=300)
        assert done.returncode == 0, f"the CSK_TCN16={mode} child exited with {done.returncode}"
        results = torch.load(path)
        cases = fx.GROUPS[f"forced-{mode}"]
        assert len(results) == len(cases)
        for case, (got, intact) in zip(cases, results):
            _compare(case, got, intact)
