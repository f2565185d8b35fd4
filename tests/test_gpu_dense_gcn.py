"""The graph conv on a dense adjacency (csrc/gcn_dense.hip; gcn_stage_dense_kernel and gcn_stage_kernel of csrc/gcn.hip) and the bare
1 x 1 conv csk_conv1x1_f32 against fp64 references of their own, through the C ABI.  Cases, operands, references and the bound come
from tests/dense_gcn_fixture.py: the exact tier (integer operands, order-independent sums) is compared bit for bit, the float tier
(positive terms) against fp64 under depth * 2^-24 * sum |term|, which tests/test_dense_gcn_fixture_cpu.py shows to be below half of
any term.  Before every launch the kernel it is going to run is asserted through csk_gcn_stage_f32_route with the launch's own
pointers.  x, ell_val and w lie between NaN bands (x with NaN between its rows as well, where the stride exceeds the row), y is NaN
before the launch: afterwards every output is finite, the bands and the padding between output rows still NaN."""
import ctypes

import numpy as np
import pytest
import torch

import _bootstrap
from tests import dense_gcn_fixture as fx

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native = pkg.native
DEV = "cuda:0"
PAD = 64                      # floats in a guard band: a multiple of 4, so that the operand inside is 16-byte aligned
f32 = np.float32


class Guarded:
    """`data` (flat float32; None: `size` NaNs, an output) inside a NaN-filled device buffer, `offset` floats off 16-byte alignment"""

    def __init__(self, data=None, size=None, offset=0):
        n = int(data.size if data is not None else size)
        self.buf = torch.full((n + 2 * PAD + offset,), float("nan"), device=DEV, dtype=torch.float32)
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.n = PAD + offset, n
        self.t = self.buf[self.lo: self.lo + n]
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=f32).reshape(-1)))

    def addr(self):
        return self.t.data_ptr()

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def numpy(self):
        return self.t.cpu().numpy()

    def assert_bands(self):
        b = self.buf.cpu().numpy()
        assert np.isnan(b[: self.lo]).all() and np.isnan(b[self.lo + self.n:]).all(), "a guard band was written"


def _stream():
    return native.stream_of(torch.empty(1, device=DEV))


def run_stage(c, ops):
    """One csk_gcn_stage_f32 launch of the case -> y [n, c_out, T, V]; route, guards and output padding asserted"""
    lib = native.lib()
    xc, xs, yc, ys = fx.strides(c)
    w_img, b_img = fx.pack_w(ops["w"], ops["bias"])
    x = Guarded(fx.strided(ops["x"], xc, xs), offset=c.x_off)
    ell = Guarded(ops["ell_val"], offset=c.ell_off)
    w, b = Guarded(w_img), Guarded(b_img)
    y = Guarded(size=fx.out_size(c))
    src = torch.from_numpy(ops["ell_src"].reshape(-1)).to(DEV)
    cnt = (ctypes.c_int32 * 3)(*c.ell_cnt)
    stride, per_frame = fx.adj_args(c)
    assert fx.route_query(lib, c, x.addr(), y.addr(), ell.addr()) == c.route, (c.name, lib.csk_last_error())
    native.check(lib.csk_gcn_stage_f32(x.ptr(), y.ptr(), w.ptr(), b.ptr(), native.ptr(src), ell.ptr(), ctypes.cast(cnt, ctypes.c_void_p),
                                       c.ell_w, stride, per_frame, c.n_seg, c.c_in, c.c_out, c.frames, c.V, xs, xc, ys, yc, c.res,
                                       _stream()), "csk_gcn_stage_f32")
    torch.cuda.synchronize()
    got, pad = fx.unstrided(y.numpy(), (c.n_seg, c.c_out, c.frames, c.V), yc, ys)
    assert np.isnan(y.numpy()[pad]).all(), (c.name, "padding between output rows was written")
    for g in (x, ell, w, b, y):
        g.assert_bands()
    assert np.isfinite(got).all(), (c.name, "an output is missing or poisoned")
    return got


@pytest.mark.parametrize("group", sorted(fx.EXACT_GROUPS))
def test_stage_exact(group):
    """every case of the group bit for bit against the exact sum"""
    cases = fx.boundary_routes(native.lib()) if group == "boundary" else fx.EXACT_GROUPS[group]
    for c in cases:
        ops = fx.operands(c, "exact")
        want, _ = fx.reference(c, ops)
        got = run_stage(c, ops)
        assert torch.equal(torch.from_numpy(got), torch.from_numpy(want.astype(f32))), c.name


def test_leaving_dense2_gives_the_aligned_launch_its_bits():
    """the misaligned V = 18 launches (dense128 / general <64, 5>) against the aligned launch (dense2) of the same operands"""
    for co, base in fx.LEAVE_BASE.items():
        ops = fx.operands(base, "exact")
        want = run_stage(base, ops)
        for c in fx.LEAVE_CASES:
            if c.c_out == co:
                assert torch.equal(torch.from_numpy(run_stage(c, fx.operands(c, "exact"))), torch.from_numpy(want)), c.name


@pytest.mark.parametrize("c", fx.FLOAT_CASES, ids=lambda c: c.name)
def test_stage_float(c):
    from tests.head_fixture import check_bound
    ops = fx.operands(c, "float")
    want, mag = fx.reference(c, ops)
    check_bound(run_stage(c, ops), want, fx.bound(c, mag), n_terms=fx.depth(c), kernel=c.name, route=c.route)


def run_conv(c, ops):
    lib = native.lib()
    xc, xs, yc, ys = fx.strides(c)
    w_img, b_img = fx.pack_w(ops["w"], ops["bias"])
    x, w, b, y = Guarded(fx.strided(ops["x"], xc, xs)), Guarded(w_img), Guarded(b_img), Guarded(size=fx.out_size(c))
    native.check(lib.csk_conv1x1_f32(x.ptr(), y.ptr(), w.ptr(), b.ptr(), c.n_seg, c.c_in, c.c_out, c.frames, c.V, xs, xc, ys, yc, _stream()),
                 "csk_conv1x1_f32")
    torch.cuda.synchronize()
    got, pad = fx.unstrided(y.numpy(), (c.n_seg, c.c_out, c.frames, c.V), yc, ys)
    assert np.isnan(y.numpy()[pad]).all(), (c.name, "padding between output rows was written")
    for g in (x, w, b, y):
        g.assert_bands()
    assert np.isfinite(got).all(), (c.name, "an output is missing or poisoned")
    return got


@pytest.mark.parametrize("V", (18, 25))
def test_conv1x1_exact(V):
    """W x + bias with both signs kept, bit for bit: c_in below, at and past a 16-channel chunk, 64- and 128-row tiles, a ragged
    last position tile"""
    for c in fx.CONV_CASES:
        if c.V == V:
            ops = fx.conv_operands(c, "exact")
            want, _ = fx.conv_reference(c, ops)
            assert torch.equal(torch.from_numpy(run_conv(c, ops)), torch.from_numpy(want.astype(f32))), c.name


@pytest.mark.parametrize("c", fx.CONV_FLOAT, ids=lambda c: c.name)
def test_conv1x1_float(c):
    from tests.head_fixture import check_bound
    ops = fx.conv_operands(c, "float")
    want, mag = fx.conv_reference(c, ops)
    check_bound(run_conv(c, ops), want, fx.bound(c, mag), n_terms=fx.depth(c), kernel=c.name)
