"""tests/tcn_direct_fixture.py without a GPU: select() reproduces the launcher's figures, the cases of tests/test_gpu_tcn_direct.py
reach every instantiation of tcn_stage_kernel and tcn_stage16_kernel that the launcher can pick (the table is printed: run with
-s), the integer operands keep every partial sum exact, the routing ids are unique, and the step-by-step host model of the
operation differs from the fp64 reference under each seeded defect on every case that exists to catch it."""
import pytest
import torch

from tests import tcn_direct_fixture as fx

SEL = {c: fx.sel_of(c) for c in fx.ALL_CASES}


def _sel(V, stride, c_out, k=9, pad=None, c=12, res_mode=0, c_res=0, ksplit=1, mode=0):
    return fx.select(c, c_out, c_res, 21, V, k, stride, k // 2 if pad is None else pad, res_mode, 0, ksplit, mode)


def test_select_reproduces_the_launchers_figures():
    for V, co, stride, ldb, nj in ((25, 64, 1, 500, 9), (25, 64, 2, 775, 14), (25, 128, 1, 375, 6), (25, 128, 2, 525, 9)):
        s = _sel(V, stride, co)
        assert (s.family, s.mt, s.ldb - s.ldb % V, s.nj) == ("32", co, ldb, nj), (V, co, stride, s)
    assert [_sel(18, st, co).nj for co in (64, 128) for st in (1, 2)] == [9, 14, 6, 9]
    s = _sel(25, 1, 64, k=1)
    assert (s.ldb, s.key) == (300, ("tcn_stage_kernel", 64, 6, False, False, 0))
    s = _sel(40, 2, 128)                              # 128-row tiles would keep 80 columns, 64-row tiles keep 240
    assert fx._narrow(128, 9, 40, 9, 2)[0] == 80 and (s.mt, s.nt, s.nj) == (64, 240, 14)
    s = _sel(64, 2, 128)
    assert fx._narrow(128, 9, 64, 9, 2)[0] == 1 and (s.mt, s.nt) == (64, 128)
    s = _sel(25, 3, 128)                              # 96 of 128 against 192 of 256: a tie, the 128-row tile stays
    assert (s.mt, s.nt, s.nj, s.vt) == (128, 96, 9, 25)
    for V in (25, 18):
        for c_res in (3, 8, 16, 40):
            assert (_sel(V, 1, 128, res_mode=2, c_res=c_res).vt, _sel(V, 1, 128, res_mode=2, c_res=c_res).res_g) == (0, 2)
        for c_res in (24, 32, 64):
            assert (_sel(V, 1, 128, res_mode=2, c_res=c_res).vt, _sel(V, 1, 128, res_mode=2, c_res=c_res).res_g) == (V, 4)
    # the 16x16x4 gate: channel limits at V = 25, none at V = 18, whole chunks, 16-byte window start, both overrides
    assert [_sel(25, st, 64, c=c).family for st, c in ((1, 64), (1, 128), (2, 128), (2, 256))] == ["16", "32", "16", "32"]
    assert _sel(18, 1, 64, c=256).family == "16" and _sel(18, 1, 64, c=12).family == "32"
    assert _sel(25, 1, 64, c=8, pad=3).family == "32" and _sel(18, 1, 64, c=8, pad=2).family == "16"
    assert _sel(25, 1, 64, c=64, res_mode=2, c_res=3).family == "32" and _sel(25, 2, 64, c=64, res_mode=1, c_res=64).family == "32"
    assert _sel(25, 1, 64, c=256, mode=2).family == "16" and _sel(18, 1, 64, c=64, mode=1).key == ("tcn_stage_kernel", 64, 9, True, False, 18)
    # split-K: ranges of whole chunks with a real channel each; one range is the unsplit launch; nj > 9 runs the plain kernel
    assert [(s.ksplit, s.cper) for s in (_sel(25, 1, 64, c=40, ksplit=k) for k in (2, 3, 5, 8, 32))] == [(2, 24), (3, 16), (3, 16), (5, 8), (5, 8)]
    assert (_sel(25, 1, 64, c=64, ksplit=64).ksplit, _sel(25, 1, 64, c=256, ksplit=5).cper) == (8, 56)
    assert _sel(25, 1, 64, c=8, ksplit=2).family == "16"
    s = _sel(18, 2, 64, c=128, ksplit=3)
    assert (s.ldb, s.split, s.ksplit, s.key) == (704, False, 1, ("tcn_stage_kernel", 64, 14, False, False, 0))


def test_cases_reach_every_instantiation_the_launcher_can_pick(capsys):
    want = fx.reachable()
    stage = {k for k in want if k[0] == "tcn_stage_kernel"}
    assert len(stage) == 19 and sum(k[4] for k in stage) == 4                 # 5 generic, 4 nine-tap, 3 + 3 compile-time V, 4 split
    assert {k for k in want if k[0] == "tcn_stage16_kernel"} == {("tcn_stage16_kernel", v, s) for v in (25, 18) for s in (1, 2)}
    # <64, 6> with V = 25 / 18 as a constant is compiled but never picked: a 64-row tile stages at least (11 + 9) V positions
    assert not any(k[1:3] == (64, 6) and k[5] for k in stage)
    default = {SEL[c].key for c in fx.ALL_CASES if c.mode == 0}
    assert default == want, sorted(want - default)
    with capsys.disabled():
        print("\ncase -> kernel (CSK_TCN16 = 1 / 2: the case needs the forced family mode, run in a child process)")
        for c in fx.ALL_CASES:
            s = SEL[c]
            inst = (f"tcn_stage16_kernel<{s.vt}, {s.stride}>" if s.family == "16" else
                    f"tcn_stage_kernel<{s.mt}, {s.nj}, K9={int(s.k9)}, SPLIT={int(s.split)}, VT={s.vt}> RES_G={s.res_g}")
            t = fx.tiles(c, s)
            print(f"  {c.name:78s} {inst:62s} nt={s.nt:3d} ranges={s.ksplit:2d} tiles={len(t)} interior={sum(t)} "
                  f"rows full/ragged={fx.row_tiles(c, s)}" + (f"  [forced CSK_TCN16={c.mode}]" if c.mode else ""))
        print("instantiation -> cases")
        for k in sorted(want, key=str):
            print(f"  {k}: {sum(SEL[c].key == k for c in fx.ALL_CASES)}")


def test_every_group_runs_the_family_it_is_named_for():
    for g, table in fx.GROUPS.items():
        fam = {SEL[c].family for c in table}
        if g.startswith(("f16_", "route16", "forced-2")):
            assert fam == {"16"}, g
        elif g.startswith(("vt_", "runtime", "stride3", "generic", "k9_pads", "route32", "forced-1")):
            assert fam == {"32"}, g
        assert all(c.mode == (int(g[-1]) if g.startswith("forced-") else 0) for c in table)
        assert len(table) <= (60 if g.startswith("forced-") else 40), g      # a parametrised GPU test stays at a few seconds
    assert [fx.sel_of(c).family for c, _ in fx.NAN_CASES] == ["32", "16"]
    # what the forced modes add: the 32x32 compile-time-18 kernels at whole chunks, the 16x16x4 kernel at 128 / 256 channels and V = 25
    assert {SEL[c].key for c in fx.GROUPS["forced-1"] if c.v == 18 and c.c % 8 == 0} >= {("tcn_stage_kernel", mt, nj, True, False, 18)
                                                                                          for mt, nj in ((64, 9), (128, 6), (128, 9))}
    assert {(c.c, c.stride) for c in fx.GROUPS["forced-2"] if c.v == 25 and fx.sel_of(c._replace(mode=0)).family == "32"} == {
        (128, 1), (256, 1), (256, 2)}
    assert [a._replace(mode=0, group="", seed=0) for a in fx.GROUPS["forced-1"]] == [a._replace(mode=0, group="", seed=0) for a in fx.GROUPS["forced-2"]]


def test_cases_reach_the_branch_points():
    cs = fx.ALL_CASES
    f32 = [c for c in cs if SEL[c].family == "32"]
    f16 = [c for c in cs if SEL[c].family == "16"]
    # narrowed tiles: 64-row tiles at V = 40 / 64, the 128-row tile at stride 3; more than one position tile each
    narrowed = {(SEL[c].mt, SEL[c].nt) for c in f32 if SEL[c].nt < 16384 // SEL[c].mt}
    assert narrowed == {(64, 240), (64, 128), (128, 96)}
    assert all(any(SEL[c].nt == nt and len(fx.tiles(c)) > 1 for c in f32) for nt in (240, 128, 96))
    # the split-K fall-back at nj > 9, requests that collapse to one range, fewer ranges than asked
    sp = fx.GROUPS["split"]
    assert sum(SEL[c].key == ("tcn_stage_kernel", 64, 14, False, False, 0) for c in sp) == 2
    assert {c.ksplit for c in sp} >= {2, 3, 5, 8, 32, 64} and {c.c for c in sp} >= {40, 64, 128, 256}
    live = [c for c in sp if SEL[c].split]
    assert {SEL[c].mt for c in live} == {64, 128} and {c.res for c in live} == {"none", "identity", "conv"}
    assert {c.co * c.t_out * c.v % 4 == 0 for c in live} == {True, False}
    assert any(SEL[c].ksplit < c.ksplit for c in live) and any(c.c % SEL[c].cper for c in live) and any(c.c % SEL[c].cper == 0 for c in live)
    assert any(SEL[c].ksplit == 32 for c in live) and sum(c.relu for c in live) >= 2 and any(c.res_off for c in live)
    # epilogues and staging forms in both families, per instantiation family
    for fam in (f32, f16):
        assert any(fx.row_tiles(c)[0] for c in fam) and any(fx.row_tiles(c)[1] for c in fam)
        assert any(fx.row_tiles(c) == (1, 1) for c in fam)                    # c_out 70: a full tile beside a ragged one
        t = [fx.tiles(c) for c in fam]
        assert any(any(x) for x in t) and any(not all(x) for x in t)
        assert sum(c.relu for c in fam if c.tier == "exact") >= 2 and {c.n for c in fam} == {1, 3}
        assert {c.res for c in fam} == {"none", "identity", "conv"} and {c.res_off for c in fam if c.res != "none"} == {0, 4}
    for mt in (64, 128):
        for v in (25, 18):
            assert any(any(fx.tiles(c)) for c in f32 if SEL[c].mt == mt and c.v == v and SEL[c].vt)
    # 16x16x4: three tiles with an interior one and odd T at both V and both strides; rows that end inside a quad
    for v in (25, 18):
        for s in (1, 2):
            fam = [c for c in f16 if c.v == v and c.stride == s]
            assert any(fx.tiles(c) == [False, True, False] and c.t % 2 for c in fam), (v, s)
            assert any(c.t * v % 4 for c in fam) and {c.res for c in fam} >= {"none", "conv"}
    assert {c.c for c in f16 if c.v == 18} >= {8, 64, 128, 256} and {c.c for c in f16 if c.v == 25 and c.mode == 0} == {8, 16, 64, 128}
    # the shapes the issue names
    assert {c.c for c in cs} >= {3, 8, 12, 20, 64, 128, 256} and {c.co for c in cs} >= {12, 64, 70, 128, 256}
    assert {c.v for c in cs} >= {25, 18, 17, 20, 33, 40, 64}
    assert {c.t for c in cs if c.stride == 1} >= set(fx.S1_T16) and {c.t for c in cs if c.stride == 2} >= set(fx.S2_T16)
    assert {(c.k, c.pad) for c in cs} >= {(1, 0), (3, 1), (5, 2), (9, 4), (9, 0), (9, 3)}
    assert {c.c_res for c in f32 if c.res == "conv" and c.stride == 1} >= set(fx.CRES) <= {c.c_res for c in f32 if c.res == "conv" and c.stride == 2}
    assert {SEL[c].res_g for c in f32 if c.res == "conv" and SEL[c].vt} == {4} and any(SEL[c].res_g == 2 and c.v in (25, 18) and c.k == 9 and
                                                                                     SEL[c].nj <= 9 for c in f32 if c.res == "conv")
    # routing: every tap per family and stride; each residual form alone
    for fam in ("32", "16"):
        for s in (1, 2):
            g = fx.GROUPS[f"route{fam}-s{s}"]
            assert sorted(c.tap for c in g if c.tier == "route_tap") == list(range(9))
            assert {c.tier for c in g} >= {"route_tap", "route_conv"} and len(fx.tiles(g[0])) >= 2
        assert any(c.tier == "route_ident" for c in fx.GROUPS[f"route{fam}-s1"])


def test_partial_sums_are_exact_in_fp32():
    for c in fx.ALL_CASES + [c for c, _ in fx.NAN_CASES]:
        assert fx.partial_sum_bound(c.c, c.c_res) < 2 ** 24, c.name
        if c.tier == "exact":
            d = fx.operands(c)
            for key, bound in (("y", fx.ACT), ("w", fx.W_MAX), ("bias", fx.BIAS), ("x", fx.ACT), ("wres", fx.W_RES)):
                if key in d:
                    assert torch.equal(d[key], d[key].round()) and float(d[key].abs().max()) <= bound, (c.name, key)
    assert fx.partial_sum_bound(256, 64) == 28235


def test_routing_ids_are_unique_and_exact():
    for c in fx.ALL_CASES:
        if c.tier == "exact":
            continue
        d = fx.operands(c)
        ids = torch.cat([d[k].flatten() for k in ("y", "x") if k in d])
        assert float(ids.min()) >= 1 and float(ids.max()) < 2 ** 24 and torch.equal(ids, ids.double().float())
        assert ids.unique().numel() == ids.numel(), c.name
        assert set(d["w"].unique().tolist()) <= {0.0, 1.0} and float(d["bias"].abs().max()) == 0
        want = fx.routing_expected(c)
        assert torch.equal(fx.reference(c), want), c.name                      # the gather is what the fp64 conv gives
        if c.tier == "route_tap":
            assert int(d["w"].sum()) == c.co and (c.pad == 0 or c.tap == c.pad or bool((want == 0).any()))
        nz = want[:, 0][want[:, 0] != 0]
        assert nz.numel() > 0 and nz.unique().numel() == nz.numel()              # within a channel no id comes twice


def test_nan_cases_name_the_outputs_a_nan_reaches():
    for c, idx in fx.NAN_CASES:
        mask = fx.nan_mask(c, idx)
        d = fx.operands(c)
        y = d["y"].clone()
        y[idx] = float("nan")
        out = torch.zeros(mask.shape, dtype=torch.float64)                    # 0 x NaN is NaN: a sum over every channel and tap
        yp = torch.nn.functional.pad(y.double(), (0, 0, c.pad, c.pad))
        for r in range(c.k):
            out += torch.einsum("oc,nctv->notv", d["w"].double()[:, :, r, 0], yp[:, :, torch.arange(c.t_out) * c.stride + r])
        assert torch.equal(torch.isnan(out), mask) and 0 < int(mask.sum()) < mask.numel() // c.n
        assert int(mask.sum()) == c.co * len({tt for tt in range(c.t_out) if 0 <= idx[2] - (c.stride * tt - c.pad) < c.k})


def test_host_model_is_the_reference():
    for c in fx.ALL_CASES:
        assert torch.equal(fx.model(c), fx.reference(c)), c.name


@pytest.mark.parametrize("defect", fx.DEFECTS)
def test_every_seeded_defect_is_caught_on_all_of_its_cases(defect):
    targets = [c for c in fx.ALL_CASES if fx.applies(defect, c)]
    assert len(targets) >= 6, defect
    fams = {SEL[c].family for c in targets}
    assert fams == ({"32"} if defect in ("range_twice", "narrow_tile_skipped", "ragged_channel") else {"32", "16"}), (defect, fams)
    for c in targets:
        assert not torch.equal(fx.model(c, defect), fx.reference(c)), (defect, c.name)
