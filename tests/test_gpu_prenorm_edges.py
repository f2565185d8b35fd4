"""Skeleton pre-normalisation on the device at its degenerate geometries (tests/prenorm_edge_fixture.py, proved on the CPU by
tests/test_prenorm_edge_fixture_cpu.py): vanishing and antiparallel bones, the axis and angle shortcuts at +-10 % of their
thresholds, exact right angles, null anchors, a null centre joint and an x-bone that exists only because the z-rotated anchors
are rounded to fp32 -- every branch outcome of ``align_to_axis`` and every decision of ``latch_rotations`` in front of it.

Nothing here compares two routes through the same device code.  The clip entry is held to the fp64 numpy oracle: bit for bit
where both stages are the identity (the centred, masked input formed in fp32 numpy) or the one rotating matrix is exact, within
3 * 2^-23 * r per element otherwise (r: fp64 norm of the joint's centred position; derivation in the fixture).  The step entry
must then equal the clip entry bit for bit, set ``has_rot`` for every stream, and hold exact identities or matrices within 2^-30
of the oracle's in ``rot_state`` -- 2^-30 is the matrix error the output bound has paid for.  Cases the reference computes the
same way are also held to what its own function wrote (tests/golden/g19_prenorm_edges.npz), at 1e-5 absolute, |want| <= 8.

Measured on an MI355X: see DESIGN.md section 3c."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _bootstrap
from tests import prenorm_edge_fixture as fx
from tests.helpers import GOLDEN, check_parity

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native = pkg.native
DEV = "cuda:0"
PAD = 1024                      # guard elements on either side of every operand (a multiple of 4: alignment is kept)
GROUP_NAMES = tuple(fx.GROUPS)


def _guarded(shape, dtype, values=None):
    """A tensor of ``shape`` in the middle of a buffer whose PAD elements on either side are NaN (int32: -7)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), -7 if dtype == torch.int32 else float("nan"), device=DEV, dtype=dtype)
    view = buf[PAD:PAD + n].view(shape)
    if values is not None:
        view.copy_(values)
    return buf, view


def _intact(buf, n):
    edge = torch.cat([buf[:PAD], buf[PAD + n:]])
    return bool((edge == -7).all()) if buf.dtype == torch.int32 else bool(torch.isnan(edge).all())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _Run:
    """One shape group on the device, every operand between guards: the clip entry in one launch, the step entry with r = 1
    per frame and with one r = 3 cycle.  Guards are checked after the launches."""

    def __init__(self, x_np, joints):
        self.bufs = []
        n, _, t, v, m = x_np.shape
        x = self._g(x_np.shape, torch.float32, torch.from_numpy(x_np.copy()))
        out = self._g(x_np.shape, torch.float32)
        rc = native.lib().csk_prenorm_f32(native.ptr(x), native.ptr(out), n, t, v, m, *joints, native.stream_of(x))
        torch.cuda.synchronize()
        assert rc == 0
        self.clip = out.cpu().numpy()
        frames = [self._g((n, 3, v, m), torch.float32, x[:, :, f]) for f in range(t)]
        self.steps = {}
        for r in (1, t):
            rot = self._g((n, 18), torch.float64, torch.zeros((n, 18), dtype=torch.float64))
            flags = self._g((n,), torch.int32, torch.zeros((n,), dtype=torch.int32))
            dsts = [self._g((n, 3, v, m), torch.float32) for _ in range(t)]
            for f in range(0, t, r):
                src = (ctypes.c_void_p * r)(*[a.data_ptr() for a in frames[f:f + r]])
                dst = (ctypes.c_void_p * r)(*[a.data_ptr() for a in dsts[f:f + r]])
                rc = native.lib().csk_prenorm_frames_f32(src, dst, r, native.ptr(rot), native.ptr(flags), 1, n, v, m, *joints,
                                                         native.stream_of(x))
                torch.cuda.synchronize()
                assert rc == 0, (r, f)
            self.steps[r] = (torch.stack(dsts, dim=2).cpu().numpy(), rot.cpu().numpy().reshape(n, 2, 3, 3), flags.cpu().numpy())
        self.guards_intact = all(_intact(buf, k) for buf, k in self.bufs)

    def _g(self, shape, dtype, values=None):
        buf, view = _guarded(shape, dtype, values)
        self.bufs.append((buf, view.numel()))
        return view


@pytest.fixture(scope="module")
def world():
    """Per group: the cases, the oracle's output, matrices and bound (computed once, read-only) and the device's results."""
    out = {}
    for group, g in fx.GROUPS.items():
        ids, x = fx.batch(group)
        centred, null = fx.centred(x)
        d = dict(ids=ids, cases=[fx.BY_ID[i] for i in ids], x=x, joints=g["joints"], want=fx.oracle(x, g["joints"]),
                 mats=fx.matrices(x, g["joints"]), bound=fx.bound(x), centred=centred, null=null)
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        d["run"] = _Run(x, g["joints"])
        out[group] = d
    return out


def _ratio(got, want, bound):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    zero = np.broadcast_to(bound == 0, err.shape)
    if got[zero].any():
        return float("inf")
    return float((err[~zero] / np.broadcast_to(bound, err.shape)[~zero]).max())


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_clip_entry_at_every_degenerate_geometry(world, group):
    w = world[group]
    got = w["run"].clip
    assert w["run"].guards_intact and np.isfinite(got).all()
    null = np.broadcast_to(w["null"][:, None], got.shape)
    assert null.any() and not _bits(got)[null].any()                                    # null joints: +0, sign included
    worst, n_bits = {}, 0
    for n, c in enumerate(w["cases"]):
        ident = (c.z != "rotate", c.x != "rotate")
        if all(ident):
            assert np.array_equal(_bits(got[n]), _bits(w["centred"][n])), (c.id, "both stages are the identity: the centred input, bit for bit")
            n_bits += 1
            continue
        if any(ident) and fx.matrix_exact(w["mats"][n, 0 if ident[1] else 1]):
            assert np.array_equal(_bits(got[n]), _bits(w["want"][n])), (c.id, "one exact stage: the oracle, bit for bit")
            n_bits += 1
            continue
        ratio = _ratio(got[n], w["want"][n], w["bound"][n])
        kind = "one identity stage" if any(ident) else "oracle only" if not c.reference_exact else "both stages rotate"
        if ratio >= worst.get(kind, (0.0, ""))[0]:
            worst[kind] = (ratio, c.id)
        assert ratio <= 1.0, f"{c.id}: max err / bound = {ratio:.3f} (bound {fx.BOUND_ULPS:g} * 2^-23 * r)"
    print(f"\n{group}: {n_bits} cases bit for bit; " + "; ".join(f"{k}: max err / bound = {v[0]:.3f} ({v[1]})" for k, v in worst.items()))
    assert n_bits >= sum(c.z != "rotate" and c.x != "rotate" for c in w["cases"]) >= 1


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_step_entry_latches_what_the_clip_entry_used(world, group):
    w = world[group]
    run = w["run"]
    assert run.guards_intact
    worst = 0.0
    for r, (got, rot, flags) in run.steps.items():
        assert np.array_equal(_bits(got), _bits(run.clip)), r
        assert flags.dtype == np.int32 and (flags == 1).all(), r                        # streams that latched identities included
        assert np.array_equal(rot, run.steps[1][1]), r
        for n, c in enumerate(w["cases"]):
            for i, outcome in enumerate((c.z, c.x)):
                if outcome != "rotate":
                    assert np.array_equal(rot[n, i], np.eye(3)) and not np.signbit(rot[n, i]).any(), (c.id, "zx"[i], "exactly 1.0 / 0.0")
                else:
                    diff = float(np.abs(rot[n, i] - w["mats"][n, i]).max())
                    worst = max(worst, diff)
                    assert diff <= fx.ROT_TOL, (c.id, "zx"[i], diff)
    print(f"\n{group}: max |rot_state - oracle matrix| = {worst:.3e} (condition: 2^-30 = {fx.ROT_TOL:.3e})")


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_clip_entry_equals_what_the_reference_wrote_at_the_edges(world, group):
    g = np.load(os.path.join(GOLDEN, "g19_prenorm_edges.npz"))
    w = world[group]
    ids = [str(i) for i in g[f"{group}/ids"]]
    pick = [w["ids"].index(i) for i in ids]
    assert ids == [c.id for c in w["cases"] if c.reference_exact] and np.array_equal(_bits(g[f"{group}/x"]), _bits(w["x"][pick]))
    err = check_parity(w["run"].clip[pick], g[f"{group}/want"], tol=1e-5, ref_cap=8.0, tag=group,
                       what="csk_prenorm_f32 vs preprocess.pre_normalization, degenerate geometries")
    print(f"\n{group}: {len(ids)} cases, max |device - reference| = {err:.3e}")
