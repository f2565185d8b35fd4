"""tests/tcn_wino_fixture.py without a GPU: select() reproduces the launchers' figures and their gate, the cases of
tests/test_gpu_tcn_wino.py reach every instantiation of tcn_stage_wino_kernel and tcn_stage_wino_s2_kernel that the launchers can
pick and every kind of tile, the integer operands keep the transformed problem exact in halves, the step-by-step host model of the
Winograd computation equals the fp64 definition bit for bit and differs from it under each seeded defect in every group that
exists to catch it, the NaN mask is the definition's window at stride 1 and a strict superset of it at stride 2, and the derived
rounding bound holds for an fp32 emulation and is broken by a reduced-precision operand."""
import pytest
import torch

from tests import tcn_wino_fixture as fx

fold = fx.fold
TABLE = [c for c in fx.ALL_CASES if c.tier in ("exact", "route_tap", "route_res")]
SEL = {c: fx.sel_of(c) for c in fx.ALL_CASES}


def test_select_reproduces_the_launchers_figures():
    s = fx.select("ext", 12, 128, 0, 11, 25)                         # 150 pair columns: 192 tall against 256 wide
    assert (s.mw, s.qp, s.qtiles, s.mtiles, s.grid) == (2, 150, 3, 1, 9)
    s = fx.select("ext", 12, 128, 0, 9, 25)                          # 125: one tile either way, the wide shape stays
    assert (s.mw, s.qp, s.qtiles, s.mtiles, s.grid) == (1, 125, 1, 2, 6)
    assert (fx.select("ext", 12, 128, 0, 20, 18).mw, fx.select("ext", 12, 128, 0, 14, 18).mw) == (2, 1)       # 180 and 126 columns
    assert [fx.pick_mw(q, 128, 1) for q in (950, 3750, 684, 64, 65)] == [2, 1, 2, 2, 1]
    assert fx.pick_mw(950, 192, 1) == 1 and fx.pick_mw(3750, 128, 2) == 2 and fx.pick_mw(100, 64, 2) == 1
    s = fx.select("ext", 64, 64, 0, 75, 25)
    assert (s.qp, s.qtiles, s.chunks, s.phantom, s.partial_last) == (950, 8, 8, True, True)
    assert [t.interior for t in s.tiles] == [False] + [True] * 5 + [False] * 2 and s.tiles[1][:2] == (5, 10)
    s = fx.select("ext", 20, 128, 24, 75, 25, stride=2, res_mode=2)
    assert (s.key, s.t_out, s.qp, s.qtiles, s.chunks, s.res_chunks) == (("tcn_stage_wino_s2_kernel", 25, True, 2), 38, 475, 8, 4, 3)
    s = fx.select("valid_res", 3, 192, 48, 30, 18, pad=0, res_mode=2, res_off=4)
    assert (s.key, s.t_out, s.chunks, s.res_chunks, s.mtiles) == (("tcn_stage_wino_kernel", 18, False, 1, True, True), 22, 2, 6, 3)
    assert not any(t.front for t in s.tiles)                          # pad 0: no tile starts in front of the sequence


def test_gate_table():
    """every -2 condition; the four shapes of test_wino_gate_falls_back_to_the_direct_kernels (tests/test_gpu_winograd.py) among them"""
    for ci, co, s, res, v in [(64, 128, 2, True, 25), (64, 64, 1, False, 25), (40, 40, 1, True, 25), (64, 64, 1, True, 20)]:
        conv = ci != co or s != 1
        mode = 2 if (res and conv) else 1 if res else 0
        assert fx.select("id", co, co, ci if res else 0, 20, v, 9, s, 4, mode, 0, n_seg=2).reject, (ci, co, s, res, v)
    for case in fx.REJECTED:
        assert fx.sel_of(case).reject, case.name
    ok = dict(entry="id", c=12, c_out=64, c_res=64, t_in=11, V=25, k=9, stride=1, pad=4, res_mode=1, res_off=0)
    assert not fx.select(**ok).reject
    for change in (dict(k=3), dict(stride=2), dict(pad=3), dict(res_mode=0), dict(res_mode=2), dict(res_off=1), dict(c_res=32),
                   dict(t_res=12), dict(has_x=False), dict(V=20), dict(c_out=96, c_res=96), dict(c=0), dict(n_seg=0),
                   dict(t_in=1 << 22, t_res=1 << 22)):
        assert fx.select(**dict(ok, **change)).reject, change
    ok = dict(entry="ext", c=12, c_out=64, c_res=8, t_in=11, V=18, k=9, stride=2, pad=4, res_mode=2, res_off=0)
    assert not fx.select(**ok).reject and not fx.select(**dict(ok, res_mode=0, c_res=0)).reject
    for change in (dict(stride=3), dict(res_mode=1, c_res=64), dict(res_off=2), dict(c_res=0), dict(t_res=6), dict(has_wres=False),
                   dict(has_x=False), dict(pad=0), dict(V=17)):
        assert fx.select(**dict(ok, **change)).reject, change
    assert fx.select("ext", 12, 64, 64, 11, 25, res_mode=1).reject and not fx.select("ext", 12, 64, 0, 11, 25).reject
    ok = dict(entry="valid", c=12, c_out=64, c_res=64, t_in=9, V=25, k=9, stride=1, pad=0, res_mode=1, res_off=4)
    assert not fx.select(**ok).reject and not fx.select(**dict(ok, res_mode=0, c_res=0, res_off=0)).reject
    for change in (dict(t_in=8, t_res=8), dict(res_mode=2), dict(res_off=0), dict(c_res=32), dict(t_res=10), dict(pad=4), dict(stride=2)):
        assert fx.select(**dict(ok, **change)).reject, change
    ok = dict(entry="valid_res", c=12, c_out=64, c_res=16, t_in=10, V=18, k=9, stride=1, pad=0, res_mode=2, res_off=4)
    assert not fx.select(**ok).reject
    for change in (dict(t_in=8, t_res=8), dict(res_mode=1), dict(res_mode=0), dict(res_off=0), dict(c_res=8), dict(c_res=24),
                   dict(t_res=11), dict(has_wres=False)):
        assert fx.select(**dict(ok, **change)).reject, change


def test_cases_reach_every_instantiation_the_launchers_can_pick(capsys):
    want = fx.reachable()
    s1 = {k for k in want if k[0] == "tcn_stage_wino_kernel" and not k[4]}
    valid = {k for k in want if k[0] == "tcn_stage_wino_kernel" and k[4]}
    s2 = {k for k in want if k[0] == "tcn_stage_wino_s2_kernel"}
    assert (len(want), len(s1), len(valid), len(s2)) == (28, 8, 12, 8)
    assert s1 == {("tcn_stage_wino_kernel", v, r, m, False, False) for v in (25, 18) for r in (False, True) for m in (1, 2)}
    assert valid == {("tcn_stage_wino_kernel", v, r, m, True, rc) for v in (25, 18) for m in (1, 2)
                     for r, rc in ((False, False), (True, False), (False, True))}
    assert s2 == {("tcn_stage_wino_s2_kernel", v, cv, m) for v in (25, 18) for cv in (False, True) for m in (1, 2)}
    got = {SEL[c].key for c in TABLE}
    assert got == want, sorted(want - got)
    assert {SEL[c].key for c in TABLE if c.tier == "exact"} == want       # the exact tier alone reaches them all
    relu = {(c.entry, c.stride) for c in TABLE if c.tier == "exact" and c.relu}                # ReLU on: one case per entry and form
    assert relu == {("id", 1), ("ext", 1), ("ext", 2), ("valid", 1), ("valid_res", 1)}
    assert sum(c.relu for c in TABLE if c.tier == "exact") * 10 < sum(c.tier == "exact" for c in TABLE)
    with capsys.disabled():
        print("\ncase -> kernel <template arguments>, grid, tiles (F front border, I interior, B back border, FB both)")
        for c in TABLE:
            s = SEL[c]
            kinds = " ".join("I" if t.interior else ("F" if t.front else "") + ("B" if t.back else "") for t in s.tiles)
            print(f"  {c.name:78s} {s.key[0]}<{', '.join(str(a).lower() for a in s.key[1:])}>  grid {s.grid:3d}  {kinds}")


def test_cases_reach_every_kind_of_tile_length_and_grid():
    for kern in ("s1", "valid", "s2"):
        for mw in (1, 2):
            sels = [SEL[c] for c in TABLE if c.tier == "exact" and fx.kernel_of(c) == kern and SEL[c].mw == mw]
            tiles = [t for s in sels for t in s.tiles]
            assert any(t.interior for t in tiles) and any(t.back and not t.front for t in tiles), (kern, mw)
            assert any(t.front for t in tiles) == (kern != "valid"), (kern, mw)      # pad 0: no span starts in front of a sequence
            assert any(s.partial_last and len(s.tiles) > 1 for s in sels) and any(len(s.tiles) == 1 for s in sels), (kern, mw)
            assert {s.phantom for s in sels} == {False, True}, (kern, mw)
            assert {s.phantom for s in sels if len(s.tiles) > 1} == {False, True}, (kern, mw)
            assert any(s.chunks == 32 for s in sels) or mw == (2 if kern == "s1" else 1), (kern, mw)
            for v in (25, 18):                                       # the tile kinds again per joint count
                tv = [t for s in sels if s.vt == v for t in s.tiles]
                assert any(t.interior for t in tv) and any(not t.interior for t in tv), (kern, mw, v)
        cases = [c for c in TABLE if c.tier == "exact" and fx.kernel_of(c) == kern]
        assert {1, 2, 3} <= {c.t_out for c in cases}, kern
        assert {3, 12, 16, 20, 64, 256} <= {c.c for c in cases}, kern
        assert {SEL[c].mtiles for c in cases} >= {1, 2, 3}, kern
    assert {9, 10, 11} <= {c.t for c in TABLE if c.pad == 0}
    assert {c.c_res for c in TABLE if c.stride == 2 and c.res == "conv" and c.tier == "exact"} >= {3, 8, 24, 64}
    assert {c.c_res for c in TABLE if c.entry == "valid_res" and c.tier == "exact"} == {16, 48}
    assert all(c.n == 3 for c in fx.ALL_CASES)
    assert any(c.c != c.co for c in TABLE if c.res == "identity")
    # xcd_contiguous_id remaps block ids by grid % 8: grids below 8, of 8, and above 8 that are no multiple of 8 (with three
    # sequences a grid is a multiple of 3: the grid of 8 is that of an exact case launched with one sequence, which the GPU test does)
    grids = {SEL[c].grid for c in TABLE} | {SEL[c].grid // 3 for c in TABLE if c.tier == "exact"}
    assert {3, 6, 8, 9, 15, 24, 27} <= grids
    assert {g % 8 for g in grids} == set(range(8))


@pytest.mark.parametrize("group", fx.EXACT_GROUPS + fx.ROUTE_GROUPS)
def test_model_equals_the_definition(group):
    for case in fx.GROUPS[group]:
        want = fx.reference(case) if case.tier == "exact" else fx.routing_expected(case)
        got = fx.model(case)
        assert torch.equal(got, want), case.name
        if case.tier != "exact":
            y = fx.operands(case)["y"]
            assert y.unique().numel() == y.numel() and float(y.max()) < 1 << 22


# the groups that exist to catch each defect (prefixes of group names)
DEFECT_GROUPS = {
    "m3_sign": ("s1-", "valid-", "s2-", "route-"),
    "group_offset": ("s1-", "valid-", "s2-", "route-"),
    "front_clamp": ("s1-", "s2-", "route-s1", "route-s2"),
    "back_reads_on": ("s1-", "s2-", "route-s1", "route-s2"),
    "phantom_stored": ("s1-", "valid-", "s2-", "route-s1", "route-valid"),
    "clamped_lane_stored": ("s1-", "valid-", "s2-", "route-"),
    "channel_tail": ("s1-", "valid-", "s2-"),
    "valid_res_frame": ("valid-", "route-valid"),
    "s2_inf_product": ("s2-",),
    "s2_res_d1": ("s2-", "route-s2"),
    "seg_stride_cpad": ("s1-", "valid-", "s2-", "route-"),
    "decode_swapped": ("s1-", "valid-", "s2-", "route-"),
}


@pytest.mark.parametrize("defect", fx.DEFECTS)
def test_every_seeded_defect_is_caught_in_every_group_that_exists_for_it(defect):
    groups = [g for g in fx.EXACT_GROUPS + fx.ROUTE_GROUPS if any(fx.applies(defect, c, SEL[c]) for c in fx.GROUPS[g])]
    assert groups and {g for g in fx.EXACT_GROUPS + fx.ROUTE_GROUPS if g.startswith(DEFECT_GROUPS[defect])} == set(groups), groups
    for g in groups:
        for case in fx.GROUPS[g]:
            if not fx.applies(defect, case, SEL[case]):
                continue
            want = fx.reference(case) if case.tier == "exact" else fx.routing_expected(case)
            got = fx.model(case, defect)
            if not torch.equal(got, want) and not torch.equal(torch.nan_to_num(got, nan=-7.0), want):
                break
        else:
            pytest.fail(f"{defect} changes no case of {g}")


def test_m3_sign_and_group_offset_fail_the_exact_and_the_routing_tier():
    """the two defects of the kernel-side sensitivity check: every exact case of more than one frame, and the routing cases of the
    taps they touch"""
    for case in TABLE:
        want = fx.reference(case) if case.tier == "exact" else fx.routing_expected(case)
        if case.tier == "exact" and case.t_out >= 2 and case.seed < 6:
            assert not torch.equal(fx.model(case, "m3_sign"), want), case.name
            assert not torch.equal(fx.model(case, "group_offset"), want), case.name
        if case.tier == "route_tap":
            assert not torch.equal(fx.model(case, "group_offset"), want), case.name


def test_exact_operands_keep_the_transformed_problem_exact():
    for case in TABLE:
        if case.tier != "exact":
            continue
        assert fx.partial_sum_bound(case) < 2 ** 23, case.name
        d = fx.operands(case)
        assert bool((d["w"] % 2 != 0).any())                         # odd weights: half-integer image entries
        u, _ = fx.images(case)
        assert u.shape[0] == (13 if case.stride == 2 else 12)
        assert torch.equal(u * 2, (u * 2).round()) and float(u.abs().max()) <= 1.5 * fx.W_MAX
        assert bool(((u * 2) % 2 != 0).any()), case.name               # and some are half-integers
        g = torch.tensor(fold.WINO_G, dtype=torch.float64)
        w = d["w"].double()[:, :, :, 0]
        if case.stride == 1:
            exact = torch.einsum("ir,ocgr->gico", g, w.view(case.co, case.c, 3, 3)).reshape(12, case.c, case.co)
            assert torch.equal(u[:, :case.c, :case.co].double(), exact)              # survives the rounding to fp32
        assert torch.equal(u.double().float(), u) and not bool(u[:, case.c:].any())


def test_transforms_are_those_of_the_weight_image():
    """A^T [(G w) . (B^T d)] is the 3-tap conv of two output frames: WINO_BT / WINO_AT belong to fold.WINO_G"""
    g = torch.tensor(fold.WINO_G, dtype=torch.float64)
    bt, at = torch.tensor(fx.WINO_BT, dtype=torch.float64), torch.tensor(fx.WINO_AT, dtype=torch.float64)
    gen = torch.Generator().manual_seed(5)
    w, d = torch.randn(3, generator=gen).double(), torch.randn(4, generator=gen).double()
    got = at @ ((g @ w) * (bt @ d))
    want = torch.stack([(w * d[0:3]).sum(), (w * d[1:4]).sum()])
    assert torch.allclose(got, want, rtol=1e-13, atol=1e-13)
    assert fold.WINO_S2_GROUPS == ((0, 3), (6, 2), (1, 2), (5, 2))


def test_nan_mask_is_the_window_at_stride_1_and_a_superset_at_stride_2():
    for case, idxs in fx.NAN_CASES:
        sel = fx.sel_of(case)
        assert not sel.reject and len(sel.tiles) >= 3
        clean = fx.model(case)
        assert torch.equal(clean, fx.reference(case))
        for idx in idxs:
            mask, window = fx.nan_mask(case, idx), fx.window_mask(case, idx)
            assert bool(mask.any()) and bool((mask | ~window).all())               # never less than the window
            if case.stride == 1:
                assert torch.equal(mask, window), (case.name, idx)
            y = fx.operands(case)["y"].clone()
            y[idx] = float("nan")
            got = fx.model(case, y=y)
            assert torch.equal(torch.isnan(got), mask), (case.name, idx)
            assert torch.equal(got[~mask], clean[~mask])
        assert idxs[0][2] < 4 and idxs[2][2] == case.t - 1
    # stride 2: E1 and O1 feed raw frames 4 j + 6 and 4 j + 5 into out(2 j), whose window ends at frame 4 j + 4
    case = fx.NAN_CASES[2][0]
    for f0 in range(case.t):
        extra = (fx.nan_mask(case, (0, 0, f0, 0)) & ~fx.window_mask(case, (0, 0, f0, 0)))[0, 0, :, 0].nonzero().flatten().tolist()
        want = [(f0 - 4 - f0 % 4) // 2] if f0 % 4 in (1, 2) and f0 >= 5 else []
        assert extra == [t for t in want if t < case.t_out], (f0, extra)


def test_rounding_bound_holds_for_fp32_and_is_broken_by_reduced_precision(capsys):
    """an fp32 emulation of the algorithm stays inside gamma(n) S everywhere; with the activations cut to bf16 it does not, and
    neither with 10 significand bits at 64 channels (at 256 channels gamma(n) has grown past that error: not asserted)"""
    lines = []
    for case in fx.GROUPS["round"]:
        ref, bound = fx.reference(case), fx.error_bound(case)
        assert bool((bound > 0).all()) and fx.roundings(case) * fx.U32 < 1e-3
        ratio = ((fx.model(case, dtype=torch.float32).double() - ref).abs() / bound).max().item()
        y = fx.operands(case)["y"]
        cut = {bits: ((fx.model(case, dtype=torch.float32, y=fx.truncated(y, bits)).double() - ref).abs() / bound).max().item()
               for bits in (7, 10)}
        lines.append(f"  {case.name:62s} n {fx.roundings(case):4d}  fp32 {ratio:.3f}  bf16 {cut[7]:.1f}  10 bits {cut[10]:.2f}")
        assert ratio <= 1.0, lines[-1]
        assert cut[7] > 1.0, lines[-1]
        if case.c == 64:
            assert cut[10] > 1.0, lines[-1]
    with capsys.disabled():
        print("\nlargest err / bound per rounding case (host emulation)\n" + "\n".join(lines))
