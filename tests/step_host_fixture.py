"""The host path of the continual temporal step, pinned without a GPU: what csk_tcn_step_f32 / csk_tcn_step_bf16x3 and their queries
(csk_tcn_step_f32_tile, csk_tcn_step_f32_route, csk_tcn_step_bf16x3_tile) REFUSE, with which text, and which tile the two _tile queries
report over a grid of launch shapes.  tests/golden/step_refusals.json holds both as the library answered BEFORE the host path was
rewritten around one StepCall / step_check / step_route (csrc/step_params.h); tests/test_step_host_cpu.py replays it.

ROWS          one call per row: the valid BASE call of the function with ONE argument changed so that exactly one requirement is violated
              (where two requirements overlap by construction -- slots < k is also a ring too shallow -- the row sits at the first of them
              in either order).  The pointers are stand-ins that are never dereferenced: a refused call launches nothing.  The BASE calls of
              the two entries themselves are never made.
SITES         per entry, every place of its code path that refuses a call (one name per CSK_FAIL of the entry, its check and its
              launcher); the rows must reach every one but UNREACHABLE, which lists those no argument list can reach and why.
record()      asks the loaded library for the return code and text of every row and for the tile grid; run once, against the build
              that is the reference.
csk_tcn_step_f32_route did not exist when the table was recorded: it must refuse what csk_tcn_step_f32_tile refuses, with the same text
(both are the shape level of the same check), which the test asserts row by row.

ctypes and json only; nothing is read from csrc."""
import ctypes as C
import itertools
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_refusals.json")
FAKE = 0x10000                              # a 16-byte aligned stand-in pointer
F32, BF, TILE, ROUTE, BF_TILE = "csk_tcn_step_f32", "csk_tcn_step_bf16x3", "csk_tcn_step_f32_tile", "csk_tcn_step_f32_route", "csk_tcn_step_bf16x3_tile"

_SHAPE = ("slots", "head_step", "n_emit", "x_res_slots", "out_slots", "c", "c_out", "P", "k", "res_mode", "c_res", "ksplit")
ARGS = {
    F32: ("ring", "slots", "head", "head_step", "n_emit", "w", "x_res", "x_res_slots", "x_res_slot0", "x_res_step", "w_res", "bias", "out",
          "out_slots", "out_slot0", "c", "c_out", "P", "k", "res_mode", "c_res", "relu", "ksplit", "partial", "stream"),
    TILE: _SHAPE,
    BF_TILE: ("n_emit", "c_out", "P"),
}
ARGS[BF] = tuple(a for a in ARGS[F32] if a not in ("ksplit", "partial"))
POINTERS = ("ring", "w", "x_res", "w_res", "bias", "out", "partial", "stream")
# four emissions of a 64 -> 64 channel block with a conv residual at 200 positions: every requirement is met and is one change away
_ENTRY = dict(ring=FAKE, slots=16, head=0, head_step=1, n_emit=4, w=FAKE, x_res=FAKE, x_res_slots=16, x_res_slot0=0, x_res_step=1, w_res=FAKE,
              bias=FAKE, out=FAKE, out_slots=16, out_slot0=0, c=64, c_out=64, P=200, k=9, res_mode=2, c_res=64, relu=1, ksplit=1, partial=0,
              stream=0)
BASE = {F32: _ENTRY, BF: {k: v for k, v in _ENTRY.items() if k in ARGS[BF]}, TILE: {k: _ENTRY[k] for k in _SHAPE},
        BF_TILE: dict(n_emit=4, c_out=64, P=200)}
ROUTE_WORDS = 3                             # CSK_STEP_ROUTE_WORDS


def call(lib, fn, change):
    """-> (return code, text of csk_last_error): the BASE call of fn with `change` applied"""
    a = dict(BASE[fn], **change)
    vals = [C.c_void_p(a[n] or None) if n in POINTERS else a[n] for n in ARGS[fn]]
    rc = getattr(lib, fn)(*vals)
    return rc, lib.csk_last_error().decode()


def route(lib, **shape):
    """csk_tcn_step_f32_route -> (return code, [family, code, workgroups])"""
    a = dict(BASE[TILE], **shape)
    words = (C.c_int32 * ROUTE_WORDS)()
    rc = lib.csk_tcn_step_f32_route(*[a[n] for n in _SHAPE], words)
    return rc, list(words)


# ---- the refusals --------------------------------------------------------------------------------------------------------------------
def _rows(fn, site, *changes):
    return [(fn, site, c) for c in changes]


ROWS_GRID = dict(P=1 << 30, c_out=1 << 16, n_emit=64, slots=80, out_slots=80, res_mode=0, x_res=0, w_res=0)      # 2**24 x 512 x 32 workgroups
_SHAPE_ROWS = (
    ("ksplit_range", (dict(ksplit=0), dict(ksplit=33))),
    ("dims", (dict(c=0), dict(c_out=0), dict(c_out=-1), dict(P=0), dict(P=202), dict(P=-4))),
    ("k_slots", (dict(k=0), dict(k=10), dict(slots=8))),
    ("emission", (dict(n_emit=0), dict(n_emit=65, slots=80, out_slots=80), dict(head_step=-1), dict(out_slots=3))),
    ("shallow", (dict(slots=11), dict(head_step=2, slots=14))),
    ("p_large", (dict(P=(1 << 31) - 256),)),
    ("res_ring_shape", (dict(x_res_slots=0),)),
    ("ident_c_res", (dict(res_mode=1, c_res=32),)),
)
ROWS = (
    # ---- csk_tcn_step_f32
    _rows(F32, "null", dict(ring=0), dict(w=0), dict(bias=0), dict(out=0))
    + _rows(F32, "no_x_res", dict(x_res=0), dict(x_res=0, res_mode=1))
    + [(F32, site, c) for site, cs in _SHAPE_ROWS for c in cs]
    + _rows(F32, "ksplit_partial_null", dict(ksplit=2), dict(ksplit=32))
    + _rows(F32, "head", dict(head=-1), dict(head=16))
    + _rows(F32, "out_slot0", dict(out_slot0=-1), dict(out_slot0=16))
    + _rows(F32, "res_ring_slot", dict(x_res_slot0=-1), dict(x_res_slot0=16), dict(x_res_step=-1))
    + _rows(F32, "conv_no_w_res", dict(w_res=0))
    + _rows(F32, "align", dict(ring=FAKE + 4), dict(ring=FAKE + 8), dict(ring=FAKE + 12), dict(x_res=FAKE + 4), dict(x_res=FAKE + 8))
    + _rows(F32, "partial_align", dict(ksplit=2, partial=FAKE + 4), dict(ksplit=4, partial=FAKE + 8))
    + _rows(F32, "grid", ROWS_GRID, dict(ROWS_GRID, ksplit=2, partial=FAKE))
    # ---- csk_tcn_step_bf16x3
    + _rows(BF, "null", dict(ring=0), dict(w=0), dict(bias=0), dict(out=0))
    + _rows(BF, "dims", dict(c=0), dict(c_out=0), dict(P=0), dict(P=202))
    + _rows(BF, "k", dict(k=8), dict(k=3, slots=16), dict(k=10))
    + _rows(BF, "head_step", dict(head_step=0), dict(head_step=3, slots=32), dict(head_step=-1))
    + _rows(BF, "slots_head", dict(slots=8), dict(head=-1), dict(head=16))
    + _rows(BF, "emission", dict(n_emit=0), dict(n_emit=65, slots=80, out_slots=80), dict(out_slots=3), dict(out_slot0=-1), dict(out_slot0=16))
    + _rows(BF, "shallow", dict(slots=11), dict(head_step=2, slots=14))
    + _rows(BF, "res_mode", dict(res_mode=3), dict(res_mode=-1))
    + _rows(BF, "no_x_res", dict(x_res=0), dict(x_res=0, res_mode=1))
    + _rows(BF, "res_ring", dict(c_res=0), dict(x_res_slots=0), dict(x_res_slot0=-1), dict(x_res_slot0=16), dict(x_res_step=-1))
    + _rows(BF, "ident_c_res", dict(res_mode=1, c_res=32))
    + _rows(BF, "conv_no_w_res", dict(w_res=0))
    + _rows(BF, "align", dict(ring=FAKE + 4), dict(x_res=FAKE + 8), dict(out=FAKE + 4), dict(out=FAKE + 8), dict(out=FAKE + 12))
    + _rows(BF, "w_align", dict(w=FAKE + 8), dict(w_res=FAKE + 4))
    + _rows(BF, "ring_4gb", dict(c=1024, c_res=16, c_out=16, P=1 << 16), dict(c=16, c_res=1024, c_out=16, P=1 << 16),
            dict(c=16, c_res=16, c_out=1024, P=1 << 16))
    # ---- the queries
    + [(TILE, site, c) for site, cs in _SHAPE_ROWS for c in cs]
    + _rows(BF_TILE, "dims", dict(n_emit=0), dict(n_emit=65), dict(c_out=0), dict(P=0), dict(P=202))
)
SITES = {
    F32: ("null", "no_x_res", "ksplit_range", "dims", "k_slots", "emission", "shallow", "p_large", "res_ring_shape", "ident_c_res",
          "ksplit_partial_null", "head", "out_slot0", "res_ring_slot", "conv_no_w_res", "align", "partial_align", "grid", "grid16"),
    BF: ("null", "dims", "k", "head_step", "slots_head", "emission", "shallow", "res_mode", "no_x_res", "res_ring", "ident_c_res",
         "conv_no_w_res", "align", "w_align", "ring_4gb", "grid"),
    TILE: tuple(s for s, _ in _SHAPE_ROWS),
    BF_TILE: ("dims",),
}
UNREACHABLE = {
    (F32, "grid16"): "the 16x16x4 launcher takes rings below 4 GB only: out_slots * c_out * P < 2**30 bounds its grid far below 2**31",
    (BF, "grid"): "every ring is below 4 GB by then: out_slots * c_out * P < 2**30 bounds the grid far below 2**31",
}

# ---- the tile sweep ------------------------------------------------------------------------------------------------------------------
SWEEP = dict(c_out=(4, 64, 128, 256), P=(8, 52, 100, 400, 25600), n_emit=tuple(range(1, 9)), head_step=(1, 2), ksplit=(1, 4), k=(3, 9))


def sweep_points():
    keys = tuple(SWEEP)
    return [dict(zip(keys, v)) for v in itertools.product(*SWEEP.values())]


def sweep_tiles(lib):
    """-> (csk_tcn_step_f32_tile, csk_tcn_step_bf16x3_tile) at every point: 64 input channels, no residual, the shallowest legal rings"""
    f32, bf = [], []
    for s in sweep_points():
        slots = s["k"] + (s["n_emit"] - 1) * s["head_step"]
        f32.append(lib.csk_tcn_step_f32_tile(slots, s["head_step"], s["n_emit"], 0, s["n_emit"], 64, s["c_out"], s["P"], s["k"], 0, 0, s["ksplit"]))
        bf.append(lib.csk_tcn_step_bf16x3_tile(s["n_emit"], s["c_out"], s["P"]))
    return f32, bf


def record(lib, path=GOLDEN):
    """writes the golden file from the loaded library: the reference build"""
    rows = []
    for fn, site, change in ROWS:
        rc, text = call(lib, fn, change)
        assert rc == -1, (fn, site, change, rc)
        rows.append(dict(fn=fn, site=site, change=change, rc=rc, text=text))
    f32, bf = sweep_tiles(lib)
    with open(path, "w") as f:                  # one row per line
        f.write('{"refusals": [\n' + ",\n".join(json.dumps(r) for r in rows) + '],\n"sweep": ' + json.dumps({k: list(v) for k, v in SWEEP.items()})
                + ',\n"f32_tile": ' + json.dumps(f32) + ',\n"bf16x3_tile": ' + json.dumps(bf) + "}\n")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)
