"""The cases of tests/test_gpu_step16.py, checked without a GPU (tests/step16_fixture.py): every case is admissible for exact
comparison (integer operands, sum |w| |x| + |bias| + |res| < 2**24 per output), a repeated case has the repeated reference, and --
the coverage proof -- the host queries csk_tcn_step_f32_tile / csk_gcn_stage_f32_tile, which return what the launchers of
csrc/step16.hip switch on, answer with EVERY instantiation of tcn_step16_kernel (16) and gcn16_kernel (12) over the cases."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import _bootstrap
from tests import step16_fixture as fx
from tests import step_split_fixture as ssf

pkg = _bootstrap.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = [(4, 1), (2, 1), (2, 2), (1, 1)]


@pytest.mark.parametrize("sc", fx.STEP_CASES + [w.sc for w in fx.WIDE], ids=lambda c: c.id)
def test_step_case_is_admissible(sc):
    ops = fx.step_ops(sc)
    bound = fx.step_admissible(sc, ops)
    fx.step_handed_integers(sc, ops)
    want = fx.step_reference(sc, ops)
    assert tuple(want.shape) == (sc.N, sc.co, sc.n_emit, sc.V) and float(want.abs().max()) <= bound
    assert torch.equal(want, want.round()) and torch.equal(want.float().double(), want)        # the cast to fp32 is exact
    assert float((want != 0).double().mean()) > 0.9                                           # the ReLU leaves the values to compare
    g = ssf.launch_geometry(sc)                                                                # a wrapping case really wraps
    assert ((g["head"] - 8) % g["slots"] + 8 >= g["slots"]) == sc.wrap
    assert (g["out_slot0"] + sc.n_emit > g["out_slots"]) == (sc.wrap and sc.n_emit > 1)
    assert 0 <= g["head"] < g["slots"] and g["slots"] >= 9 + (sc.n_emit - 1) * sc.head_step


@pytest.mark.parametrize("gc", fx.GCN_CASES + [p.base for p in fx.GCN_PRODUCTION[::2]], ids=lambda c: c.id)
def test_gcn_case_is_admissible(gc):
    ops = fx.gcn_ops(gc)
    bound = fx.gcn_admissible(gc, ops)
    fx.gcn_handed_integers(gc, ops)
    want = fx.gcn_reference(gc, ops)
    assert tuple(want.shape) == (gc.n_seg, gc.co, gc.skel, gc.V) and float(want.max()) <= bound
    assert torch.equal(want.float().double(), want) and float((want != 0).double().mean()) > 0.8


def test_reference_of_a_repeated_case_is_the_repeated_reference():
    """positions (temporal step) and skeletons (graph conv) are independent: the fp64 reference computed on repeated operands
    equals the small case's reference, repeated -- so the wide launches need no large fp64 product"""
    wc = fx.WIDE[1]                                                    # conv residual
    sc, ops = wc.sc, fx.step_ops(wc.sc)
    rep = fx.StepCase(**{**sc.__dict__, "N": 3 * sc.N})
    rops = fx.StepOps(*[None if t is None else t.repeat(3, 1, 1, 1) if t.dim() == 4 and t.shape[0] == sc.N else t
                        for t in (ops.x, ops.w, ops.bias, ops.x_res, ops.w_res)])
    assert torch.equal(fx.step_reference(rep, rops), fx.step_reference(sc, ops).repeat(3, 1, 1, 1))
    # and in the launch layout: position p of the wide ring is position p % 100 of the small one
    small, _ = fx.step_launch(sc, ops)
    big, g = fx.step_launch(sc, ops, wide_P=252)
    assert g["P"] == 252 and torch.equal(big["ring"][..., 200:252].nan_to_num(-1), small["ring"][..., :52].nan_to_num(-1))
    for pc in fx.GCN_PRODUCTION[:4:3]:
        b = pc.base
        ops = fx.gcn_ops(b)
        idx = torch.arange(23) % b.skel
        wide = fx.GcnOps(ops.x[:, :, idx], ops.w, ops.bias, ops.A)
        wc23 = fx.GcnCase(pc.ci, pc.co, pc.V, pc.n_seg, 23, pc.seed, base_skel=7)
        assert torch.equal(fx.gcn_reference(wc23.base, wide), fx.gcn_expand(wc23, fx.gcn_reference(b, ops)))
        x = fx.gcn_launch(wc23, ops)["x"]
        assert torch.equal(x[:, :, 7 * pc.V: 14 * pc.V], x[:, :, : 7 * pc.V]) and bool(torch.isnan(x[:, :, 23 * pc.V:]).all())


def test_every_temporal_instantiation_is_reached():
    """the coverage proof: the query returns NB * 1000 + E * 100 + HS * 10 + TAIL of the kernel the launcher picks (one function
    decides for both); over the cases that is all 16 of {25, 18} x {(4, 1), (2, 1), (2, 2), (1, 1)} x {TAIL 0, 1}"""
    small = {c.id: fx.step_tile(c) for c in fx.STEP_CASES}
    wide = {w.id: fx.step_tile(w.sc, fx.wide_P(w)) for w in fx.WIDE}
    every = {nb * 1000 + e * 100 + hs * 10 + t for nb in (25, 18) for e, hs in FORMS for t in (0, 1)}
    assert set(small.values()) == {t for t in every if t // 1000 == 18}
    assert set(wide.values()) == {t for t in every if t // 1000 == 25} and len(wide) == 8
    assert set(small.values()) | set(wide.values()) == every and len(every) == 16
    for w in fx.WIDE:                                                   # a wide launch: the P = 100 case runs the narrow twin
        P, t = fx.wide_P(w), wide[w.id]
        assert w.sc.P == 100 == w.sc.N * w.sc.V and fx.step_tile(w.sc) == t - 7000
        assert P % fx.tile_positions(t) and P >= fx.smallest_P25(w) > 100       # ends in a partial tile
    groups = [("18", [(c, small[c.id]) for c in fx.STEP_CASES]), ("25", [(w.sc, wide[w.id]) for w in fx.WIDE])]
    for nb, cs in groups:
        assert {c.res for c, _ in cs} == {"none", "ident", "conv"} and {c.wrap for c, _ in cs} == {False, True}, nb
        assert any(c.n_emit // (t // 100 % 10) > 1 for c, t in cs), nb             # gz > 1: j0 = bz * E
        assert any(c.co > 64 for c, _ in cs), nb                                    # more than one m-tile
    cs = fx.STEP_CASES
    # TAIL by the channel count (a partial chunk: 6; a chunk of padding only: 4, 12, 24) and by the residual alone
    assert {c.c for c in cs} == {16, 32, 4, 6, 12, 24} and {c.c_res for c in cs if c.c == 16 and c.res == "conv"} >= {3, 24}
    assert all(fx.step_tile(c) % 10 == 1 for c in cs if c.c == 16 and c.c_res in (3, 24))
    assert {c.P for c in cs} == {100, 72, 428} and {c.co for c in cs} == {64, 256}
    assert all(c.res != "ident" or (c.head_step == 1 and c.c_res == c.co) for c in cs)
    for e, hs in FORMS:                                                 # every form with and without ReLU, at one and more tiles
        form = [c for c in cs if small[c.id] // 10 % 100 == e * 10 + hs]
        assert {c.relu for c in form} == {False, True} and {c.P for c in form} == {100, 72, 428}, (e, hs)
    # the launches of the 1024-stream NTU cycle (P = 51 200) run the wide tiles
    lib = pkg.native.lib()
    assert [lib.csk_tcn_step_f32_tile(16, hs, n, 12, 8, c, co, 51200, 9, 2, c, 1) for hs, n, c, co in ((1, 4, 64, 64), (2, 2, 64, 128),
                                                                                                        (2, 1, 128, 256))] == [25410, 25220, 25110]


def test_temporal_query_follows_the_dispatch_and_reports_argument_errors():
    lib = pkg.native.lib()

    def tile(slots=12, head_step=1, n_emit=1, x_res_slots=0, out_slots=4, c=16, c_out=64, P=100, k=9, res_mode=0, c_res=0, ksplit=1):
        return lib.csk_tcn_step_f32_tile(slots, head_step, n_emit, x_res_slots, out_slots, c, c_out, P, k, res_mode, c_res, ksplit)
    assert tile() == 18110
    # the launches the family does not take go to the 32x32x2 kernels: split-K, k != 9, P < 8, head_step 0 (a bare
    # CoTemporalConvolution), a ring of 4 GB or more
    assert tile(ksplit=2, c=64) == 0 and tile(k=3) == 0 and tile(P=4) == 0 and tile(head_step=0) == 0
    assert tile(c=256, P=1 << 19, slots=16) == 0 and tile(c=256, P=1 << 17, slots=16) == 18110
    assert tile(ksplit=2, c=8) == 18111                                 # fewer channels than one range of a split: unsplit
    for kw, text in ((dict(P=102), b"bad dims"), (dict(c=0), b"bad dims"), (dict(c_out=-1), b"bad dims"), (dict(k=10), b"k/slots"),
                     (dict(slots=8), b"k/slots"), (dict(n_emit=2, out_slots=1), b"emission geometry"), (dict(n_emit=4, slots=11), b"too shallow"),
                     (dict(ksplit=0), b"ksplit"), (dict(res_mode=1, c_res=64), b"residual ring"),
                     (dict(res_mode=1, c_res=16, x_res_slots=4), b"c_res == c_out"), (dict(P=1 << 31), b"P too large")):
        assert tile(**kw) == -1 and text in lib.csk_last_error(), (kw, lib.csk_last_error())


GCN_CHILD = (
    "import sys, json; sys.path.insert(0, %r)\n"
    "from tests import step16_fixture as fx\n"
    "print(json.dumps([[fx.gcn_tile(g) for g in fx.GCN_CASES], [fx.gcn_tile(g) for g in fx.GCN_PRODUCTION]]))\n") % ROOT


def _gcn_tiles(**switches):
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("CSK_DIAG", "CSK_GCN16", "CSK_GCN_GENERAL")}
    env.update(switches)
    out = subprocess.run([sys.executable, "-c", GCN_CHILD], env=env, check=True, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def test_every_graph_conv_instantiation_is_reached():
    """With the family forced on (CSK_DIAG=1 CSK_GCN16=2; the switches are read when the library is loaded: a child process) the
    query answers with all 12 of {25, 18} x {F = 4, 2, 1} x {identity, conv gcn_residual} over the small cases; without the switch
    the policy keeps the 32x32x2 kernel for them and hands the production sizes to the family; CSK_GCN16=1 switches it off."""
    forced, forced_prod = _gcn_tiles(CSK_DIAG="1", CSK_GCN16="2")
    assert set(forced) == {nb * 1000 + f * 100 + r * 10 for nb in (25, 18) for f in (4, 2, 1) for r in (0, 1)} and len(set(forced)) == 12
    for gc, t in zip(fx.GCN_CASES, forced):
        assert t // 1000 == gc.V and (t // 10 % 10 == 1) == (gc.res == "conv") and gc.n_seg % (t // 100 % 10) == 0, gc.id
    own, own_prod = [[fx.gcn_tile(g) for g in cs] for cs in (fx.GCN_CASES, fx.GCN_PRODUCTION)]
    assert own == [0] * len(fx.GCN_CASES)
    assert own_prod == forced_prod == [gc.V * 1000 + 400 + (10 if gc.res == "conv" else 0) for gc in fx.GCN_PRODUCTION]
    assert {(gc.ci, gc.skel, gc.V) for gc in fx.GCN_PRODUCTION} == {(ci, s, v) for ci in (64, 3) for s in (2048, 2047) for v in (25, 18)}
    off, off_prod = _gcn_tiles(CSK_DIAG="1", CSK_GCN16="1")
    assert not any(off) and not any(off_prod)
    # segment groups (n_seg / F > 1), ragged last tiles and single whole tiles, for either joint count
    for V in (25, 18):
        cs = [(gc, t) for gc, t in zip(fx.GCN_CASES, forced) if gc.V == V]
        assert any(gc.n_seg // (t // 100 % 10) > 1 for gc, t in cs)
        npg = [(gc, 16 * V // (t // 100 % 10)) for gc, t in cs]
        assert any((gc.skel * V) % n for gc, n in npg) and any(gc.skel * V == n for gc, n in npg)
        assert {(gc.ci, gc.co) for gc, _ in cs} == {(64, 64), (16, 16), (3, 64), (12, 24), (128, 256)}


def test_graph_conv_query_reads_what_the_launcher_reads():
    lib = pkg.native.lib()
    gc = fx.GCN_PRODUCTION[0]
    P = gc.P
    assert fx.gcn_tile(gc) == 25400
    # 16-byte alignment of x and y, strides that are whole quads, a shared skeleton-sparse adjacency
    assert fx.gcn_tile(gc, x=ctypes.c_void_p((1 << 12) + 4)) == 0 and fx.gcn_tile(gc, y=ctypes.c_void_p((1 << 12) + 8)) == 0

    def tile(cnt=(1, 1, 4), ell_w=4, adj=0, n_seg=4, ci=64, co=64, skel=2048, V=25, xs=64 * P, xc=P, res=1):
        c = (ctypes.c_int32 * 3)(*cnt)
        return lib.csk_gcn_stage_f32_tile(fx.ALIGNED, fx.ALIGNED, ctypes.cast(c, ctypes.c_void_p), ell_w, adj, 0, n_seg, ci, co, skel, V, xs, xc,
                                          64 * P, P, res)
    assert tile() == 25400 and tile(n_seg=2) == 25200
    assert tile(n_seg=3) == 0                                           # 384 tiles of 400 columns against 600 of 256: not clearly better
    assert tile(xc=P + 2) == 0 and tile(xs=64 * P + 1) == 0 and tile(cnt=(2, 1, 4)) == 0 and tile(cnt=(1, 1, 5), ell_w=5) == 0
    assert tile(adj=3 * 25 * 4) == 0
    assert tile(V=21) == 0                                              # no tile of the family holds whole skeletons of 21 joints
    for kw, text in ((dict(V=1), b"bad dims"), (dict(V=65), b"bad dims"), (dict(n_seg=0), b"bad dims"), (dict(ci=0), b"bad dims"),
                     (dict(ell_w=0), b"ell_w"), (dict(cnt=(1, 1, 5)), b"ell_cnt"), (dict(res=0), b"res_mode"), (dict(ci=3), b"identity residual")):
        assert tile(**kw) == -1 and text in lib.csk_last_error(), (kw, lib.csk_last_error())
    assert lib.csk_gcn_stage_f32_tile(fx.ALIGNED, fx.ALIGNED, None, 4, 0, 0, 4, 64, 64, 2048, 25, 64 * P, P, 64 * P, P, 1) == -1
    assert b"null pointer" in lib.csk_last_error()
