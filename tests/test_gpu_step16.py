"""Every instantiation of the slot-balanced 16x16x4 tile family (csrc/step16.hip) against fp64, BIT FOR BIT: the cases of
tests/step16_fixture.py have integer-valued fp32 operands whose sums are exact in fp32 in any order, so the kernel must give the
fp64 reference exactly (torch.equal; no tolerance anywhere in this file).  tests/test_step16_fixture_cpu.py proves on the CPU
that the cases are admissible and that between them they reach all 16 tcn_step16_kernel<NB, E, HS, TAIL> and all 12
gcn16_kernel<NB, F, CONVRES, 8>.  Which instantiation a launch runs is ASSERTED through the host queries
(csk_tcn_step_f32_tile / csk_gcn_stage_f32_tile: the function the launchers switch on), not observed on the device."""
import os
import subprocess
import sys

import pytest
import torch

import _bootstrap
from tests import step16_fixture as fx

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native = pkg.native
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(t):
    return None if t is None else t.to(DEV)


# ---- csk_tcn_step_f32 -----------------------------------------------------------------------------------------------------
def _step(sc, ops, wide_P=None):
    """csk_tcn_step_f32 on the case (its positions repeated up to wide_P) -> the emissions (n_emit, C_out, P) on the host; asserts
    that the spare slot of the output ring is untouched"""
    t, g = fx.step_launch(sc, ops, wide_P)
    P = g["P"]
    ring, w, xres, wres, bias = (_dev(t[k]) for k in ("ring", "w", "xres", "wres", "bias"))
    out = torch.full((g["out_slots"], sc.co, P), float("nan"), device=DEV)
    rc = native.lib().csk_tcn_step_f32(
        native.ptr(ring), g["slots"], g["head"], sc.head_step, sc.n_emit, native.ptr(w), native.ptr(xres), g["x_slots"], g["x_slot0"],
        sc.head_step, native.ptr(wres), native.ptr(bias), native.ptr(out), g["out_slots"], g["out_slot0"], sc.c, sc.co, P, 9,
        fx.RES_MODE[sc.res], sc.c_res, int(sc.relu), 1, None, native.stream_of(out))
    native.check(rc, "csk_tcn_step_f32")
    out = out.cpu()
    spare = (g["out_slot0"] + sc.n_emit) % g["out_slots"]
    assert bool(torch.isnan(out[spare]).all()), "a slot of the output ring that holds no emission was written"
    return torch.stack([out[(g["out_slot0"] + j) % g["out_slots"]] for j in range(sc.n_emit)], 0)


def _want(sc, ops):
    """the fp64 reference cast to fp32, in the layout of the emissions: (n_emit, C_out, N V)"""
    return fx.step_reference(sc, ops).float().permute(2, 1, 0, 3).reshape(sc.n_emit, sc.co, sc.N * sc.V)


def _mismatch(got, want):
    bad = got != want
    return f"{int(bad.sum())} of {bad.numel()} outputs differ, emissions {sorted(set(bad.nonzero()[:, 0].tolist()))}"


@pytest.mark.parametrize("sc", fx.STEP_CASES, ids=lambda c: c.id)
def test_step_kernel_equals_fp64(sc):
    """the NB = 18 instantiations: every (E, HS, TAIL) form, every residual mode, wrapped rings, partial tiles, 1 and 4 m-tiles"""
    assert fx.step_tile(sc) // 1000 == 18
    ops = fx.step_ops(sc)
    got, want = _step(sc, ops)[..., : sc.N * sc.V], _want(sc, ops)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want), _mismatch(got, want)


@pytest.mark.parametrize("wc", fx.WIDE, ids=lambda c: c.id)
def test_wide_step_kernel_equals_fp64_and_the_small_launch(wc):
    """the NB = 25 instantiations, which only a launch of more than 256 narrow tiles picks: the P = 100 case repeated up to the
    smallest P the query gives, ending in a partial tile.  Every repetition equals the fp64 reference and the bits of the small
    (NB = 18) launch"""
    sc, P = wc.sc, fx.wide_P(wc)
    assert fx.step_tile(sc, P) == fx.step_tile(sc) + 7000 and fx.step_tile(sc, P) // 1000 == 25
    ops = fx.step_ops(sc)
    want = _want(sc, ops)
    small, big = _step(sc, ops), _step(sc, ops, P)
    assert bool(torch.isfinite(big).all())
    assert torch.equal(small, want), _mismatch(small, want)
    idx = torch.arange(P) % 100
    assert torch.equal(big, want[..., idx]), _mismatch(big, want[..., idx])
    assert torch.equal(big, small[..., idx])


@pytest.mark.parametrize("wc", fx.WIDE, ids=lambda c: c.id)
def test_step_results_do_not_depend_on_the_launch_size(wc):
    """what step16.hip promises -- only the tile WIDTH follows the launch shape, an output's summation order does not -- on
    real-valued data (torch.rand activations, fan-in scaled normal weights: sums that DO round): the wide NB = 25 launch equals the
    P = 100 NB = 18 launch bit for bit on every repetition, for one case per (E, HS, TAIL)"""
    sc, P = wc.sc, fx.wide_P(wc)
    assert fx.step_tile(sc, P) // 1000 == 25 and fx.step_tile(sc) // 1000 == 18
    ops = fx.step_ops(sc, real=True)
    small, big = _step(sc, ops), _step(sc, ops, P)
    assert bool(torch.isfinite(small).all()) and float(small.abs().max()) > 0.1
    assert not torch.equal(small, small.round())                           # (not the integer case again)
    assert torch.equal(big, small[..., torch.arange(P) % 100])


# ---- csk_gcn_stage_f32 ----------------------------------------------------------------------------------------------------
def _gcn(gc, ops):
    """csk_gcn_stage_f32 on channel-major frames (ring-slot arguments of the plain call) -> y (n_seg, C_out, skel V) on the host"""
    t = fx.gcn_launch(gc, ops)
    P = gc.P
    x, w, bias, src, val = (_dev(t[k]) for k in ("x", "w", "bias", "ell_src", "ell_val"))
    y = torch.full((gc.n_seg, gc.co, P), float("nan"), device=DEV)
    rc = native.lib().csk_gcn_stage_f32(native.ptr(x), native.ptr(y), native.ptr(w), native.ptr(bias), native.ptr(src), native.ptr(val),
                                        native.ptr(t["ell_cnt"]), t["ell_w"], 0, 0, gc.n_seg, gc.ci, gc.co, gc.skel, gc.V, gc.ci * P, P,
                                        gc.co * P, P, fx.RES_MODE[gc.res], native.stream_of(x))
    native.check(rc, "csk_gcn_stage_f32")
    return y[:, :, : gc.skel * gc.V].cpu()


def _gcn_want(gc, ops):
    want = fx.gcn_expand(gc, fx.gcn_reference(gc.base, ops)).float()       # (n_seg, C_out, skel, V)
    return want.reshape(gc.n_seg, gc.co, gc.skel * gc.V)


def gcn_child(path):
    """(child process) every small graph-conv case under the switches of the environment -> torch.save(list of outputs)"""
    torch.save([_gcn(gc, fx.gcn_ops(gc)) for gc in fx.GCN_CASES], path)


CHILD_SECONDS = 240      # import, 19 small launches, save: a child that is still running after that is hung


@pytest.fixture(scope="module")
def gcn_families(tmp_path_factory):
    """the small cases once on the 16x16x4 tiles (CSK_GCN16=2: whenever the shape is supported) and once on the 32x32x2 kernel (=1);
    the switches are read when the library is loaded, so each run is a child process, under its own time limit; the second starts
    only if the first exited 0"""
    code = "import sys; sys.path.insert(0, %r); from tests import test_gpu_step16 as t; t.gcn_child(sys.argv[1])" % ROOT
    outs = {}
    for mode in ("2", "1"):
        path = str(tmp_path_factory.mktemp("gcn16") / f"family_{mode}.pt")
        env = dict(os.environ, CSK_DIAG="1", CSK_GCN16=mode)
        env.pop("CSK_GCN_GENERAL", None)
        rc = subprocess.call(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, "-c", code, path], env=env)
        assert rc == 0, f"the child with CSK_GCN16={mode} exited {rc}"
        outs[mode] = torch.load(path)
        assert len(outs[mode]) == len(fx.GCN_CASES)
    return outs


@pytest.mark.parametrize("i", range(len(fx.GCN_CASES)), ids=[gc.id for gc in fx.GCN_CASES])
def test_graph_conv_equals_fp64_on_either_tile_family(i, gcn_families):
    """gcn16_kernel<NB, F, CONVRES, 8> for V = 25 / 18, F = 4 / 2 / 1, identity and conv gcn_residual, ragged channel counts, ragged last
    tiles and more than one segment group -- and the 32x32x2 kernel the policy keeps at these sizes -- both equal the fp64
    reference exactly"""
    gc = fx.GCN_CASES[i]
    want = _gcn_want(gc, fx.gcn_ops(gc))
    for mode, name in (("2", "16x16x4"), ("1", "32x32x2")):
        got = gcn_families[mode][i]
        assert bool(torch.isfinite(got).all()), name
        assert torch.equal(got, want), (name, _mismatch(got, want))


@pytest.mark.parametrize("gc", fx.GCN_PRODUCTION, ids=lambda c: c.id)
def test_graph_conv_production_size_equals_fp64(gc):
    """launches the policy itself gives to the family (asserted through the query): 4 frames of 2048 / 2047 skeletons, 64 -> 64 and
    3 -> 64; the operands repeat a 7-skeleton case, whose reference is repeated"""
    assert fx.gcn_tile(gc) == gc.V * 1000 + 400 + (10 if gc.res == "conv" else 0)
    ops = fx.gcn_ops(gc.base)
    got, want = _gcn(gc, ops), _gcn_want(gc, ops)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want), _mismatch(got, want)
