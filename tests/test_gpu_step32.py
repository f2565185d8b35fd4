"""Every instantiation of the 32x32x2 continual temporal step (csrc/step.hip: tcn_step_kernel<MT, E, HS, SPLIT, K9, OCC> and
step_reduce_kernel) against fp64.  The exact and route cases of tests/step32_fixture.py have integer operands whose sums are exact in
fp32 in any order, split or not: csk_tcn_step_f32 must give the fp64 reference BIT FOR BIT.  The real-valued tests pin what the path
promises -- a stream's latency-mode results do not depend on the slab width, nor on how many frames a launch carries -- bit for bit,
and the fp32 result against fp64 under a derived bound.  tests/test_step32_fixture_cpu.py proves on the CPU that the cases are
admissible, reach all 15 instantiations and catch the seeded defects.  Which instantiation a launch runs is restated in
``step32_fixture.select`` and the library is asked (csk_tcn_step_f32_tile) that the 16x16x4 family does not take it."""
import ctypes
from dataclasses import replace

import pytest
import torch

import _bootstrap
from tests import head_fixture as hf
from tests import step32_fixture as fx

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native = pkg.native
DEV = "cuda:0"
GUARD = 4096             # NaN floats on either side of the partial-sum buffer
ROUTE = fx.one_per_instantiation()
SPLIT_FORMS = {k: c for k, c in fx.one_per_instantiation([c for c in fx.CASES if c.NV == 100]).items() if k[3]}


def _dev(t):
    return None if t is None else t.to(DEV)


def _step(cs, tier="exact", wide_P=None, j_lo=0, n=None, mutate=None):
    """csk_tcn_step_f32 on emissions j_lo .. j_lo + n - 1 of the case (all of them by default; its positions repeated up to wide_P)
    -> the emissions (n, C_out, P) on the host.  Asserts that the slots of the output ring that hold no emission of the launch and the
    guards on both sides of the partial buffer are still NaN.  ``mutate``: edits the argument dict (the guard tests); then -> (rc, out)"""
    t, g = fx.launch(cs, tier, wide_P)
    n = cs.n_emit if n is None else n
    sub = replace(cs, n_emit=n)
    sel = fx.select(sub)
    P = g["P"]
    ring, w, xres, wres, bias = (_dev(t[k]) for k in ("ring", "w", "xres", "wres", "bias"))
    out = torch.full((g["out_slots"], cs.co, P), float("nan"), device=DEV)
    n_part = n * sel.eff * cs.co * P
    buf = torch.full((n_part + 2 * GUARD,), float("nan"), device=DEV)
    a = dict(slots=g["slots"], head=(g["head"] + j_lo * cs.head_step) % g["slots"], head_step=cs.head_step, n_emit=n,
             x_slot0=(g["x_slot0"] + j_lo * cs.head_step) % g["x_slots"], out_slot0=(g["out_slot0"] + j_lo) % g["out_slots"], k=cs.k,
             ksplit=cs.ksplit, partial=buf.data_ptr() + 4 * GUARD if cs.ksplit > 1 else None)
    if mutate:
        mutate(a)
    rc = native.lib().csk_tcn_step_f32(
        native.ptr(ring), a["slots"], a["head"], a["head_step"], a["n_emit"], native.ptr(w), native.ptr(xres), g["x_slots"], a["x_slot0"],
        cs.head_step, native.ptr(wres), native.ptr(bias), native.ptr(out), g["out_slots"], a["out_slot0"], cs.c, cs.co, P, a["k"],
        fx.RES_MODE[cs.res], cs.c_res, int(cs.relu), a["ksplit"], None if a["partial"] is None else ctypes.c_void_p(a["partial"]),
        native.stream_of(out))
    if mutate:
        torch.cuda.synchronize()
        return rc, out.cpu()
    native.check(rc, "csk_tcn_step_f32")
    out, buf = out.cpu(), buf.cpu()
    mine = [(a["out_slot0"] + j) % g["out_slots"] for j in range(n)]
    for s in range(g["out_slots"]):
        if s not in mine:
            assert bool(torch.isnan(out[s]).all()), "a slot of the output ring that holds no emission was written"
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n_part:]).all()), "a write outside the partial buffer"
    if sel.split:
        assert bool(torch.isfinite(buf[GUARD: GUARD + n_part].view(-1, P)[:, : cs.NV]).all()), "a partial slab was not fully written"
    return torch.stack([out[s] for s in mine], 0)


def _mismatch(got, want):
    bad = got != want
    return f"{int(bad.sum())} of {bad.numel()} outputs differ, emissions {sorted(set(bad.nonzero()[:, 0].tolist()))}"


def _not16(cs):
    assert fx.tile16(cs) == 0, "the 16x16x4 family takes this launch"


# ---- exact ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", fx.CASES, ids=lambda c: c.id)
def test_step_kernel_equals_fp64(cs):
    _not16(cs)
    got, want = _step(cs)[..., : cs.NV], fx.reference(cs).float()
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want), _mismatch(got, want)


@pytest.mark.parametrize("cs", fx.COLLAPSE, ids=lambda c: c.id)
def test_collapsed_split_request_equals_fp64_on_either_family(cs):
    """c = 8, ksplit 2: one range.  k = 9 runs on the 16x16x4 tiles, k = 5 stays on the 32x32x2 kernel; neither touches the partial"""
    assert fx.select(cs).eff == 1 and (fx.tile16(cs) != 0) == (cs.k == 9)
    got, want = _step(cs)[..., : cs.NV], fx.reference(cs).float()
    assert torch.equal(got, want), _mismatch(got, want)


@pytest.mark.parametrize("cs", list(ROUTE.values()), ids=lambda c: c.id)
def test_every_output_names_its_source(cs):
    """route tier, one case per instantiation: ids with a full 24-bit significand through one-hot weights"""
    _not16(cs)
    got, want = _step(cs, "route")[..., : cs.NV], fx.reference(cs, "route").float()
    assert torch.equal(got, want), _mismatch(got, want)


def _set(**kw):
    return lambda a: a.update(kw)


@pytest.mark.parametrize("name,mutate,text", [
    ("null-partial", _set(partial=None), b"partial-sum buffer"),
    ("misaligned-partial", lambda a: a.update(partial=a["partial"] + 4), b"16-byte aligned"),
    ("ksplit-0", _set(ksplit=0), b"ksplit"), ("ksplit-33", _set(ksplit=33), b"ksplit"),
    ("ring-too-shallow", lambda a: a.update(slots=a["k"] - 1 + (a["n_emit"] - 1) * a["head_step"], head=0), b"too shallow"),
    ("k-0", _set(k=0), b"k/slots"), ("k-10", _set(k=10), b"k/slots"), ("n-emit-65", _set(n_emit=65), b"emission geometry")],
    ids=lambda v: v if isinstance(v, str) else "")
def test_argument_errors_launch_nothing(name, mutate, text):
    cs = next(c for c in fx.GROUPS["split"] if c.n_emit == 3 and c.ksplit == 2)
    rc, out = _step(cs, mutate=mutate)
    assert rc == -1 and text in native.lib().csk_last_error(), native.lib().csk_last_error()
    assert bool(torch.isnan(out).all())


# ---- real-valued: bit for bit ----------------------------------------------------------------------------------------------------------
def test_split_forms_for_the_slab_width_test():
    assert len(SPLIT_FORMS) == 6 and all(c.P == 100 for c in SPLIT_FORMS.values())


@pytest.mark.parametrize("cs", list(SPLIT_FORMS.values()), ids=lambda c: c.id)
def test_latency_mode_results_do_not_depend_on_the_slab_width(cs):
    """a split-K launch at P = 100 and the same positions repeated to 700 (several tiles of 64 / 128 / 256, the last one partial):
    identical bits on every repetition"""
    P = 700
    wide = fx.select_dims(cs.c, cs.co, P, cs.k, cs.head_step, cs.n_emit, cs.ksplit)
    assert wide.key == fx.select(cs).key and P // wide.NP >= 2 and P % wide.NP
    small, big = _step(cs, "real"), _step(cs, "real", wide_P=P)
    assert bool(torch.isfinite(small).all()) and float(small.abs().max()) > 0.1 and not torch.equal(small, small.round())
    assert torch.equal(big, small[..., torch.arange(P) % 100])


def _grouped(cs, per):
    """the case's emissions computed `per` per launch"""
    assert cs.n_emit % per == 0
    return torch.cat([_step(cs, "real", j_lo=j, n=per) for j in range(0, cs.n_emit, per)], 0)


FRAMES = [c for c in (
    next(c for c in fx.GROUPS["folded"] if fx.select(c).key == (64, 4, 1, False, True, 2) and c.res == r) for r in ("none", "ident", "conv"))] + [
    next(c for c in fx.GROUPS["folded"] if fx.select(c).key[:3] == (128, 2, hs)) for hs in (1, 2)] + [
    next(c for c in fx.GROUPS["split"] if fx.select(c).key[:3] == (128, 2, hs) and c.NV == 100) for hs in (1, 2)]


@pytest.mark.parametrize("cs", FRAMES, ids=lambda c: c.id)
def test_results_do_not_depend_on_the_frames_per_launch(cs):
    """E and OCC change the column mapping only, never the K order: the same emissions one per launch (E = 1), in pairs (E = 2) and in
    fours (E = 4, MT = 64) are identical bits"""
    sel = fx.select(cs)
    _not16(cs)
    whole = _step(cs, "real")
    assert bool(torch.isfinite(whole[..., : cs.NV]).all()) and not torch.equal(whole, whole.round())
    for per in (1, 2, 4):
        if per >= cs.n_emit or cs.n_emit % per:
            continue
        sub = replace(cs, n_emit=per)
        assert fx.select(sub).E == min(per, sel.E) and fx.select(sub).MT == sel.MT and fx.tile16(sub) == 0
        got = _grouped(cs, per)
        assert torch.equal(got[..., : cs.NV], whole[..., : cs.NV]), (per, _mismatch(got[..., : cs.NV], whole[..., : cs.NV]))


def test_results_do_not_depend_on_the_occupancy_twin():
    """the same emissions through <64, 4, 1, ., K9, OCC = 3> (64 emissions: 528 workgroups) and OCC = 2 (60: 495), and one group of
    four on its own"""
    hi, lo = fx.GROUPS["occ"]
    assert fx.select(hi).OCC == 3 and fx.select(lo).OCC == 2
    a, b = _step(hi, "real"), _step(hi, "real", n=lo.n_emit)
    assert bool(torch.isfinite(a[..., : hi.NV]).all()) and not torch.equal(a, a.round())
    assert torch.equal(a[: lo.n_emit, :, : hi.NV], b[..., : hi.NV])
    one = _step(hi, "real", j_lo=8, n=1)
    assert torch.equal(one[0, :, : hi.NV], a[8, :, : hi.NV])


# ---- real-valued: the derived bound --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", list(ROUTE.values()), ids=lambda c: c.id)
def test_step_kernel_within_the_derived_fp64_bound(cs):
    """|got - ref64| <= (n_terms + 4) 2**-24 sum |term|, n_terms = k c + c_res + 2: recursive fp32 summation in any order, split or not
    (tests/test_step32_fixture_cpu.py: a result truncated to bf16 misses this bound)"""
    _not16(cs)
    got = _step(cs, "real")[..., : cs.NV]
    hf.check_bound(got.numpy(), fx.reference(cs, "real").numpy(), fx.bound(cs).numpy(), n_terms=fx.n_terms(cs), case=cs.id,
                   kernel="tcn_step_kernel<%d,%d,%d,%s,%s,%d>" % fx.select(cs).key)
