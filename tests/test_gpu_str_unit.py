"""The S-TR attention unit (csrc/str.hip) stage by stage, through the C ABI with the packed operands of tests/str_unit_fixture.py: the
qkv and o images of the caller's scratch and y, each against the fp64 restatement of its stage.  Exact cases (designed tie sets and
unique ids; one-hot weights) bit for bit at all three images in both layouts; rounding cases element-wise under the derived bound,
every stage judged on its actual input (the image the previous launch left).  Operands, x, y and the scratch lie between NaN guards,
y and the scratch are NaN before the call and the scratch has exactly n_seg (2 dk + 2 dv) frames V floats: after the call exactly the
elements of qkv, o and y that belong to the launch are finite.  Which kernels run is asserted through csk_str_unit_f32_route."""
import ctypes

import numpy as np
import pytest
import torch

import _bootstrap
from tests import str_unit_fixture as fx
from tests.test_gpu_dense_gcn import Guarded, _stream

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native = pkg.native
f32, f64 = np.float32, np.float64


def run_unit(c, ops):
    """one csk_str_unit_f32 call -> (qkv [n, M, ncols], o [n, dv, ncols], the flat scratch, the flat y buffer); route and guards asserted"""
    lib = native.lib()
    dk, dkh, dvh, M, ncols = fx.dims(c)
    xs, ys = fx.xy_strides(c)
    route = (ctypes.c_int32 * 12)()
    assert lib.csk_str_unit_f32_route(c.n_seg, c.c_in, c.c_out, c.frames, c.V, c.has_res, route) == 0 and list(route) == fx.select(c), fx.name(c)
    assert (ops["res_scale"] is not None) == bool(c.has_res)
    x = Guarded(fx.place(ops["x"], xs))
    y = Guarded(size=fx.body(c.n_seg, c.c_out, ncols, ys))
    scratch = Guarded(size=fx.scratch_floats(c))
    g = {k: Guarded(ops[k]) for k in ("w_qkv", "b_qkv", "s_in", "t_in", "w_out", "b_out", "res_scale") if ops[k] is not None}
    rc = lib.csk_str_unit_f32(x.ptr(), y.ptr(), scratch.ptr(), fx.scratch_floats(c), g["w_qkv"].ptr(), g["b_qkv"].ptr(), g["s_in"].ptr(), g["t_in"].ptr(),
                              g["w_out"].ptr(), g["b_out"].ptr(), g["res_scale"].ptr() if c.has_res else None, c.n_seg, c.c_in, c.c_out, c.frames, c.V,
                              xs[0], xs[1], ys[0], ys[1], _stream())
    native.check(rc, "csk_str_unit_f32")
    torch.cuda.synchronize()
    for b in [x, y, scratch] + list(g.values()):
        b.assert_bands()
    s, yf = scratch.numpy(), y.numpy()
    assert np.isfinite(s).all(), (fx.name(c), "an element of the qkv / o image is missing or poisoned")
    belongs = np.zeros(yf.shape, dtype=bool)
    belongs[fx.index(c.n_seg, c.c_out, ncols, ys)] = True
    assert np.array_equal(np.isfinite(yf), belongs), (fx.name(c), "y: a hole, or a store outside (seg, c < C_out, col < frames V)")
    cut = c.n_seg * M * ncols
    return s[:cut].reshape(c.n_seg, M, ncols), s[cut:].reshape(c.n_seg, c.c_out, ncols), s, yf


def _equal(got, want64, what):
    assert fx.is_f32(want64), ("the expected value is no fp32", what)
    want = np.where(np.isnan(want64), np.nan, want64).astype(f32)
    assert torch.equal(torch.from_numpy(np.nan_to_num(got, nan=-7.5)), torch.from_numpy(np.nan_to_num(want, nan=-7.5))), what


@pytest.mark.parametrize("c", fx.CASES, ids=fx.name)
def test_exact_stage_by_stage(c):
    """designed tie sets + unique ids: qkv, o and y bit for bit; then the one-hot forms of the two GEMM stages"""
    ops = fx.exact_operands(c, "designed")
    fx.admissible(c, ops)
    qkv, o, s, yf = run_unit(c, ops)
    want_qkv = fx.qkv64(c, ops)[0]
    want_o = fx.o64(c, want_qkv)[0]
    want_y = fx.y64(c, ops, want_o)[0]
    _equal(qkv, want_qkv, (fx.name(c), "qkv"))
    _equal(o, want_o, (fx.name(c), "o: if only this fails, expf(0.f) != 1 or 1.f / 2^n is inexact in this build"))
    _equal(yf, fx.expected_image(c, 3, want_y)[0], (fx.name(c), "y"))

    ops = fx.exact_operands(c, "onehot1")
    fx.admissible(c, ops)
    qkv, _, _, _ = run_unit(c, ops)
    _equal(qkv, fx.qkv64(c, ops)[0], (fx.name(c), "qkv, one-hot weights"))

    ops = fx.exact_operands(c, "onehot3")
    fx.admissible(c, ops)
    qkv, o, s, yf = run_unit(c, ops)
    _equal(qkv, want_qkv, (fx.name(c), "qkv (onehot3)"))
    _equal(o, want_o, (fx.name(c), "o (onehot3)"))
    _equal(yf, fx.expected_image(c, 3, fx.y64(c, ops, want_o)[0])[0], (fx.name(c), "y, one-hot weights"))


@pytest.mark.parametrize("c,flavour", fx.ROUND, ids=[fx.name(c, fl) for c, fl in fx.ROUND])
def test_rounding_stage_by_stage(c, flavour):
    """|got - ref| <= bound element-wise per stage, the reference of stage 2 / 3 formed from the image the device left for it"""
    ops = fx.round_operands(c, flavour)
    qkv, o, s, yf = run_unit(c, ops)
    ref1, bnd1, _ = fx.qkv64(c, ops)
    ref2, bnd2 = fx.o64(c, qkv)
    ref3, bnd3 = fx.y64(c, ops, o)[:2]
    r = [fx.worst(s, *fx.expected_image(c, 2, ref2, bnd2, qkv=qkv)), fx.worst(yf, *fx.expected_image(c, 3, ref3, bnd3))]
    r.insert(0, fx.worst(qkv.reshape(-1), f64(ref1).reshape(-1), bnd1.reshape(-1)))
    print(f"\n{fx.name(c, flavour):52s} err / bound: qkv {r[0]:.3f}  o {r[1]:.3f}  y {r[2]:.3f}", end="")
    assert (np.abs(f64(qkv) - ref1) <= bnd1).all() and (np.abs(f64(o) - ref2) <= bnd2).all(), (fx.name(c, flavour), r)
    assert max(r) <= 1.0, (fx.name(c, flavour), r)
