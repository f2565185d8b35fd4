"""gcn_stage_sparse2_kernel<MT, CONVRES, 8> (csk_gcn_stage_f32 on a skeleton-sparse shared adjacency), its SPLIT form and
gcn_reduce_kernel (csk_gcn_stage_splitk_f32) against the fp64 reference of tests/dense_gcn_fixture.py, through the C ABI, on the cases
of tests/sparse_gcn_fixture.py.  Exact tier (integer operands): the output BITS equal the reference's, and a split launch equals its
unsplit twin bit for bit.  Float tier (positive operands, one case per instantiation): |y - fp64| <= depth 2^-24 sum |term| with the
depth derived in the fixture, which tests/test_sparse_gcn_fixture_cpu.py shows to be below half of any term.  Which kernel runs is
asserted before every launch through csk_gcn_stage_f32_route / csk_gcn_stage_splitk_f32_route with the launch's own pointers.

x, ell_val, w and bias lie between NaN bands, NaN fills the pads between the rows and segments of x, the tails of ell_val past ell_cnt
are NaN; y and the partial-sum buffer start as NaN.  After the launch every output is finite, every pad and band word of y still
holds the NaN bit pattern it started with, and the partial buffer of a split launch has no NaN in a word the reduction reads and
nothing but that NaN anywhere else.  Not covered: the slow epilogue addressing (fast_epi == 0: channel strides of 2^27 floats)."""
import ctypes

import numpy as np
import pytest
import torch

import _bootstrap
from tests import dense_gcn_fixture as dx
from tests import sparse_gcn_fixture as fx
from tests.test_gpu_dense_gcn import Guarded, _stream

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native = pkg.native
DEV = "cuda:0"
f32 = np.float32
NAN_BITS = torch.full((1,), float("nan"), dtype=torch.float32).view(torch.int32).item()


def untouched(g, mask=None):
    """every band word of the guarded buffer, and every word of its payload under `mask`, still holds the NaN it was filled with"""
    bits = g.buf.view(torch.int32).cpu().numpy()
    keep = np.ones(bits.shape, dtype=bool)
    keep[g.lo: g.lo + g.n] = False if mask is None else mask
    return bool((bits[keep] == NAN_BITS).all())


def launch(lib, c, ops, ksplit=None, before=None):
    """the launch alone -> (guarded operands, y, partial or None); ksplit None: csk_gcn_stage_f32.  before(x, y, ell, partial) runs on
    the guarded buffers ahead of the launch"""
    xc, xs, yc, ys = dx.strides(c)
    w_img, b_img = dx.pack_w(ops["w"], ops["bias"])
    x = Guarded(dx.strided(ops["x"], xc, xs), offset=c.x_off)
    ell, w, b = Guarded(ops["ell_val"]), Guarded(w_img), Guarded(b_img)
    y = Guarded(size=dx.out_size(c))
    src = torch.from_numpy(ops["ell_src"].reshape(-1)).to(DEV)
    cnt = ctypes.cast((ctypes.c_int32 * 3)(*c.ell_cnt), ctypes.c_void_p)
    part = None if ksplit is None else Guarded(size=c.n_seg * ksplit * c.c_out * yc)
    if before is not None:
        before(x, y, ell, part)
    if ksplit is None:
        rc = lib.csk_gcn_stage_f32(x.ptr(), y.ptr(), w.ptr(), b.ptr(), native.ptr(src), ell.ptr(), cnt, c.ell_w, 0, 0, c.n_seg, c.c_in, c.c_out,
                                   c.frames, c.V, xs, xc, ys, yc, c.res, _stream())
    else:
        rc = lib.csk_gcn_stage_splitk_f32(x.ptr(), y.ptr(), w.ptr(), b.ptr(), native.ptr(src), ell.ptr(), cnt, c.ell_w, c.n_seg, c.c_in, c.c_out,
                                          c.frames, c.V, xs, xc, ys, yc, c.res, ksplit, part.ptr(), _stream())
    native.check(rc, "csk_gcn_stage_f32" if ksplit is None else "csk_gcn_stage_splitk_f32")
    torch.cuda.synchronize()
    return (x, ell, w, b), y, part


def run(c, ops, ksplit=None):
    """One launch of the case -> y [n, c_out, T, V]; the route is asserted before it, bands, pads and the partial buffer after it"""
    lib = native.lib()

    def route(x, y, ell, part):
        if ksplit is None:
            assert dx.route_query(lib, c, x.addr(), y.addr(), ell.addr()) == c.route, (c.name, lib.csk_last_error())
        else:
            assert fx.split_query(lib, c, ksplit, x.addr(), y.addr(), ell.addr(), part.addr()) == fx.split_route(c, ksplit), \
                (c.name, ksplit, lib.csk_last_error())
    operands, y, part = launch(lib, c, ops, ksplit, route)
    xc, xs, yc, ys = dx.strides(c)
    got, pad = dx.unstrided(y.numpy(), (c.n_seg, c.c_out, c.frames, c.V), yc, ys)
    assert untouched(y, pad), (c.name, "a band or pad word of y was written")
    for g in operands:
        g.assert_bands()
    assert np.isfinite(got).all(), (c.name, "an output is missing or poisoned")
    if part is not None:
        ranges, Q = fx.cper_ranges(c.c_in, ksplit)[1], c.frames * c.V
        read = np.zeros(part.n, dtype=bool)
        if ranges > 1:                                                          # a collapsed request runs no reduction
            read[: c.n_seg * ranges * c.c_out * yc].reshape(-1, yc)[:, :Q] = True
        assert not np.isnan(part.numpy()[read]).any(), (c.name, "the reduction reads a word no workgroup wrote")
        assert untouched(part, ~read), (c.name, "a word of the partial buffer outside the partial rows was written")
    return got


def same_bits(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)).view(torch.int32), torch.from_numpy(np.ascontiguousarray(b)).view(torch.int32))


@pytest.mark.parametrize("route", sorted({c.route for c in fx.UNSPLIT_CASES}))
def test_unsplit_exact(route):
    """every case of the instantiation bit for bit against the exact sum"""
    for c in fx.UNSPLIT_CASES:
        if c.route == route:
            ops = dx.operands(c, "exact")
            want, _ = dx.reference(c, ops)
            assert same_bits(run(c, ops), want.astype(f32)), c.name


@pytest.mark.parametrize("s", fx.SPLIT_CASES, ids=lambda s: f"{s.c.name}-k{s.ksplit}")
def test_split_exact(s):
    """the split launch bit for bit against the exact sum and against its unsplit twin"""
    ops = dx.operands(s.c, "exact")
    want, _ = dx.reference(s.c, ops)
    got = run(s.c, ops, s.ksplit)
    assert same_bits(got, want.astype(f32)), s.c.name
    assert same_bits(got, run(s.c, ops)), s.c.name


@pytest.mark.parametrize("c,ksplit", [(c, None) for c in fx.FLOAT_CASES] + [(s.c, s.ksplit) for s in fx.FLOAT_SPLITS],
                         ids=lambda v: v.name if isinstance(v, dx.Case) else f"k{v}")
def test_float(c, ksplit):
    from tests.head_fixture import check_bound
    ops = dx.operands(c, "float")
    want, mag = dx.reference(c, ops)
    k = ksplit or 1
    route = c.route if ksplit is None else fx.split_route(c, ksplit)
    worst = check_bound(run(c, ops, ksplit), want, fx.bound(c, mag, k), n_terms=fx.depth(c, k), kernel=c.name, route=route)
    print(f"sparse-gcn float tier {c.name} ksplit={ksplit} route={route}: worst err / bound = {worst:.4f}")
