"""tests/str_unit_fixture.py without a GPU: through the host query csk_str_unit_f32_route (the function the launchers switch on) the
case table reaches all 4 + 8 instantiations of csrc/str.hip and every tile kind; every exact case is admissible and its designed tie
sets are what the fp64 logits give; the op-for-op fp32 host model equals the fp64 references on the exact cases and stays within the
derived bounds on the rounding cases; every seeded defect changes its stage's image on an exact case and exceeds the bound on a
rounding case (the 2^-18 exponential: the bound only)."""
import ctypes as C

import numpy as np
import pytest

import _bootstrap
from tests import str_unit_fixture as fx

pkg = _bootstrap.load()
f32, f64 = np.float32, np.float64


def _route(c=None, **kw):
    a = dict(n_seg=2, c_in=64, c_out=64, frames=4, V=25, has_res=1) if c is None else c._asdict()
    a.update(kw)
    out = (C.c_int32 * 12)(*([-7] * 12))
    rc = pkg.native.lib().csk_str_unit_f32_route(a["n_seg"], a["c_in"], a["c_out"], a["frames"], a["V"], a["has_res"], out)
    return rc, list(out)


def test_route_query_is_declared_bound_and_refuses_what_the_entry_refuses():
    assert "csk_str_unit_f32_route" in pkg.native.SIGNATURES and len(pkg.native.SIGNATURES["csk_str_unit_f32_route"]) == 7
    lib = pkg.native.lib()
    assert _route()[0] == 0
    assert lib.csk_str_unit_f32_route(2, 64, 64, 4, 25, 1, None) == -1
    for kw, rc, msg in ((dict(n_seg=0), -1, b"positive"), (dict(frames=0), -1, b"positive"), (dict(V=20), -2, b"V in {18, 25}"),
                        (dict(c_out=48, c_in=48), -2, b"C_out"), (dict(c_out=512, c_in=512), -2, b"C_out"), (dict(c_in=24, has_res=0), -2, b"multiple of 16"),
                        (dict(c_in=32), -1, b"skip"), (dict(n_seg=1 << 20, frames=1 << 12), -1, b"too large")):
        got, out = _route(**kw)
        assert got == rc and msg in lib.csk_last_error() and out == [-7] * 12, kw
        fake = C.c_void_p(1 << 20)                      # the entry says the same (never dereferenced: validation fails first)
        a = dict(n_seg=2, c_in=64, c_out=64, frames=4, V=25, has_res=1)
        a.update(kw)
        assert lib.csk_str_unit_f32(fake, fake, fake, 1 << 62, fake, fake, fake, fake, fake, fake, fake if a["has_res"] else None, a["n_seg"], a["c_in"],
                                    a["c_out"], a["frames"], a["V"], 1 << 40, 1 << 32, 1 << 40, 1 << 32, None) == rc, kw


def test_table_reaches_every_instantiation_and_tile_kind():
    inst, kinds, grids = {}, set(), ([], [])
    for c in fx.CASES:
        rc, r = _route(c)
        assert rc == 0 and r == fx.select(c), (fx.name(c), r, fx.select(c))
        for k in fx.instantiations(c):
            inst.setdefault(k, []).append(fx.name(c))
        kinds |= fx.tile_kinds(c)
        grids[0].append(r[3])
        grids[1].append(r[11])
        print(f"\n{fx.name(c):44s} qkv <{r[0]},1,0,0> {r[1]}x{r[2]} grid {r[3]:3d} | att <{r[4]},{r[5]}> grid {r[6]:3d} | out <{r[8]},0,{r[7]},1> {r[9]}x{r[10]} grid {r[11]:3d}", end="")
    want = {("gemm", 4, 1, 0, 0), ("gemm", 2, 1, 0, 0), ("gemm", 2, 0, 1, 1), ("gemm", 2, 0, 0, 1)} | {("att", v, d) for v in (18, 25) for d in (1, 2, 4, 8)}
    assert set(inst) == want and len(want) == 12
    print(f"\ninstantiations reached: {len(inst)} of 12; tile kinds: {sorted(kinds)}")
    assert kinds >= {"ragged_rows", "ragged_rows_upper_half", "ragged_cols", "full_cols", "one_column_tile", "one_wave_stores", "frame_straddles_seam",
                     "one_chunk", "odd_chunks", "grid_1", "grid_mult_8", "grid_rem_8"}
    for g in grids:
        assert 1 in g and any(v % 8 == 0 for v in g) and any(v > 8 and v % 8 for v in g) and len({v % 8 for v in g} - {0}) >= 4, g
    # the issue's matrix
    for co in (32, 64, 128, 256):
        assert {c.has_res for c in fx.CASES if c.c_out == co} == {0, 1}
    assert {c.c_in for c in fx.CASES} >= {16, 32, 48, 256} and all(c.c_in == c.c_out for c in fx.CASES if c.has_res)
    assert {c.n_seg for c in fx.CASES} == {1, 3} and {c.layout for c in fx.CASES} == {"dense", "ring"}
    cols = {(c.V, c.frames) for c in fx.CASES}
    assert cols >= {(18, 1), (25, 1), (25, 11), (18, 15), (25, 41)} and any(v * t % 256 == 0 for v, t in cols)
    assert max(c.n_seg * c.frames * c.V * fx.dims(c)[3] for c in fx.CASES) == 3 * 1025 * 384
    for c in fx.CASES:                              # ring: x channel stride != y channel stride, a segment stride beyond C * channel stride
        (xs, xc), (ys, yc) = fx.xy_strides(c)
        assert c.layout == "dense" or (xc != yc and xs > c.c_in * xc and ys > c.c_out * yc)


@pytest.fixture(scope="module")
def exact():
    """(case, form) -> (operands, qkv64, o64, y64), computed once"""
    out = {}
    for c in fx.CASES:
        for form in ("designed", "onehot1", "onehot3"):
            ops = fx.exact_operands(c, form)
            qkv = fx.qkv64(c, ops)[0]
            o = fx.o64(c, qkv)[0] if form != "onehot1" else None
            out[c, form] = (ops, qkv, o, fx.y64(c, ops, o)[0] if o is not None else None)
    return out


def test_exact_cases_are_admissible_and_tie_as_designed(exact):
    sizes, per_case = set(), []
    for c in fx.CASES:
        for form in ("designed", "onehot1", "onehot3"):
            fx.admissible(c, exact[c, form][0])
        ops, qkv, o, y = exact[c, "designed"]
        l, _ = fx.logits64(c, qkv)
        tie = l == l.max(-1, keepdims=True)
        assert np.array_equal(tie, ops["J"]), fx.name(c)
        cnt = tie.sum(-1)
        sizes |= set(np.unique(cnt).tolist())
        per_case.append(set(np.unique(cnt).tolist()))
        assert tie[..., 0].any() and tie[..., c.V - 1].any()                       # tie sets that hold joint 0 / joint V - 1
        flat = tie.reshape(c.n_seg, fx.NH, c.frames, c.V * c.V)
        assert (flat[:, 0] != flat[:, 1]).any() and len({tuple(np.packbits(flat[0, h, 0])) for h in range(fx.NH)}) >= 2       # J differs per head
        for s in range(c.n_seg):                                                   # >= 2 tie sets among the queries of one head
            for h in range(fx.NH):
                assert len({tuple(r) for r in tie[s, h, 0].tolist()}) >= 2
        dk = fx.dims(c)[0]
        v = qkv[:, 2 * dk:]
        assert np.unique(v).size == v.size                                          # unique ids: (row, joint, frame, segment)
        # onehot forms: every output the copy of one input element
        ops1, qkv1, _, _ = exact[c, "onehot1"]
        assert np.array_equal(qkv1, f64(ops1["x"])[:, ops1["src"]]) and np.unique(ops1["x"]).size == ops1["x"].size
        ops3, _, o3, y3 = exact[c, "onehot3"]
        assert np.array_equal(y3, o3[:, ops3["src"]]) and (o3 > 0).all()
    assert sizes == {1, 2, 4, 8, 16} and all(len(s) >= 4 for s in per_case)


def _same(got, want):
    return np.array_equal(f64(got), want, equal_nan=True)


def test_model_without_a_defect_equals_the_exact_references(exact):
    for (c, form), (ops, qkv, o, y) in exact.items():
        assert _same(fx.model_stage(c, ops, 1), fx.expected_image(c, 1, qkv)[0]), (fx.name(c), form)
        if form != "onehot1":
            assert _same(fx.model_stage(c, ops, 2, qkv=qkv), fx.expected_image(c, 2, o, qkv=qkv)[0]), (fx.name(c), form)
            assert _same(fx.model_stage(c, ops, 3, o=o), fx.expected_image(c, 3, y)[0]), (fx.name(c), form)


@pytest.fixture(scope="module")
def rounding():
    """(case, flavour) -> (operands, the model's qkv and o images [n, rows, ncols]): every stage judged on its actual input"""
    out = {}
    for c, fl in fx.ROUND:
        dk, dkh, dvh, M, ncols = fx.dims(c)
        ops = fx.round_operands(c, fl)
        s1 = fx.model_stage(c, ops, 1)
        qkv = s1[: c.n_seg * M * ncols].reshape(c.n_seg, M, ncols)
        s2 = fx.model_stage(c, ops, 2, qkv=qkv)
        out[c, fl] = (ops, s1, qkv, s2, s2[c.n_seg * M * ncols:].reshape(c.n_seg, c.c_out, ncols))
    return out


def _judge(c, ops, stage, img, qkv, o):
    if stage == 1:
        ref, bnd, _ = fx.qkv64(c, ops)
    elif stage == 2:
        ref, bnd = fx.o64(c, qkv)
    else:
        ref, bnd = fx.y64(c, ops, o)[:2]
    return fx.worst(img, *fx.expected_image(c, stage, ref, bnd, qkv=qkv))


def test_model_without_a_defect_meets_the_bound_on_every_rounding_case(rounding):
    top = [0.0, 0.0, 0.0]
    for (c, fl), (ops, s1, qkv, s2, o) in rounding.items():
        r = [_judge(c, ops, 1, s1, qkv, o), _judge(c, ops, 2, s2, qkv, o), _judge(c, ops, 3, fx.model_stage(c, ops, 3, o=o), qkv, o)]
        print(f"\n{fx.name(c, fl):52s} host model err / bound: qkv {r[0]:.3f}  o {r[1]:.3f}  y {r[2]:.3f}", end="")
        assert max(r) <= 1.0, (fx.name(c, fl), r)
        top = [max(a, b) for a, b in zip(top, r)]
    print(f"\nlargest err / bound of the fp32 host model: qkv {top[0]:.3f}, o {top[1]:.3f}, y {top[2]:.3f}")
    assert 0 < min(top)


@pytest.mark.parametrize("stage,defect", [(s, d) for s, ds in fx.DEFECTS.items() for d in ds])
def test_each_seeded_defect_is_caught_both_ways(stage, defect, exact, rounding):
    if defect != "exp_rel_2^-18":
        for c in fx.CASES:
            ops, qkv, o, y = exact[c, "designed"]
            ref = {1: qkv, 2: o, 3: y}[stage]
            if not _same(fx.model_stage(c, ops, stage, defect, qkv=qkv, o=o), fx.expected_image(c, stage, ref, qkv=qkv)[0]):
                break
        else:
            pytest.fail(f"{defect}: no exact case changes")
    for (c, fl), (ops, s1, qkv, s2, o) in rounding.items():
        if _judge(c, ops, stage, fx.model_stage(c, ops, stage, defect, qkv=qkv, o=o), qkv, o) > 1.0:
            return
    pytest.fail(f"{defect}: within the bound on every rounding case")
