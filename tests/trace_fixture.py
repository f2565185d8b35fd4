"""Launch-trace recorder of the continual driver (test infrastructure, needs no GPU).

The Python engine of ``CoStGcn`` / ``CoSpatioTemporalBlock`` decides WHAT is launched -- which entry, on which ring slots,
with which weight image, how many emissions -- and the kernels decide the numbers.  This module pins the first half: it
replaces ``native.lib`` by an object whose every ``csk_*`` attribute records ``(name, args)`` and returns 0, drives a model
bound to CPU memory through ``_python_cycle`` / ``_flush`` (and a stand-alone block through ``engine_advance``), and turns every
pointer argument into ``"<tensor name>+<byte offset>"`` against a table of the model's state tensors, packed operands, input
frames and the logits a cycle returned.  A pointer that resolves to nothing raises.  A driver that launches the same kernels
on the same operands in the same order produces the same trace; tests/golden/continual_trace.json holds the trace of the
driver before its arithmetic was gathered into one copy each (tests/test_continual_trace_cpu.py).

``python tests/trace_fixture.py PATH`` writes the trace of the checked-out tree to PATH.
"""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import _bootstrap  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "continual_trace.json")
CPU = torch.device("cpu")
CYCLE_MIX = (1, 2, 4, 8, 3, 4, 4)


class _FakeLib:
    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        if not name.startswith("csk_"):
            raise AttributeError(name)
        return lambda *args: self._rec.call(name, args)


class Recorder:
    """Context manager: while active, every library call of the package is recorded instead of made."""

    def __init__(self, pkg):
        self.pkg, self.calls, self._pending, self._via = pkg, [], [], None

    def __enter__(self):
        native, blocks = self.pkg.native, self.pkg.blocks
        self._saved = (native.lib, native.stream_of, blocks.tcn_step_launch, blocks.tcn_step_split_launch)
        fake = _FakeLib(self)
        native.lib = lambda: fake
        native.stream_of = lambda t: "stream"
        blocks.tcn_step_launch = self._through("tcn_step_launch", blocks.tcn_step_launch)
        blocks.tcn_step_split_launch = self._through("tcn_step_split_launch", blocks.tcn_step_split_launch)
        return self

    def __exit__(self, *exc):
        native, blocks = self.pkg.native, self.pkg.blocks
        native.lib, native.stream_of, blocks.tcn_step_launch, blocks.tcn_step_split_launch = self._saved
        return False

    def _through(self, name, orig):
        def launch(*args):
            self._via = name
            try:
                return orig(*args)
            finally:
                self._via = None
        return launch

    def call(self, name, args):
        self._pending.append([name, self._via or "", [_raw(a) for a in args]])
        return 0

    def settle(self, table, note=None):
        """Resolve the pointers of the calls made since the last settle against ``table`` ({name: tensor}); ``note`` (what the
        driver returned) is appended as a pseudo-call."""
        ranges = _ranges(table)
        for name, via, args in self._pending:
            self.calls.append([name, via] + [_resolve(a, ranges, name) for a in args])
        self._pending = []
        if note is not None:
            self.calls.append(["return", ""] + list(note))


class _Ptr(int):
    pass


def _raw(a):
    """Argument as recorded at call time: pointers as _Ptr (resolved by settle), everything else by value."""
    if a is None or isinstance(a, (str, float)):
        return a
    if isinstance(a, bool):
        return int(a)
    if isinstance(a, int):
        return a
    if isinstance(a, C.c_void_p):
        return None if a.value is None else _Ptr(a.value)
    if isinstance(a, C.Array):
        if issubclass(a._type_, C.Structure):
            return [_raw_struct(s) for s in a]
        if a._type_ is C.c_void_p:
            return [None if v is None else _Ptr(v) for v in a]
        return [int(v) for v in a]
    if isinstance(a, C.Structure):
        return _raw_struct(a)
    if isinstance(a, C._SimpleCData):
        return a.value
    if hasattr(a, "_obj"):                      # ctypes.byref(x)
        return _raw(a._obj)
    raise TypeError(f"trace recorder: argument of type {type(a).__name__}")


def _raw_struct(s):
    out = {}
    for field in s._fields_:
        name, ctype = field[0], field[1]
        v = getattr(s, name)
        if ctype is C.c_void_p:
            out[name] = None if v is None else _Ptr(v)
        elif isinstance(v, C.Array):
            out[name] = [int(e) for e in v]
        else:
            out[name] = v
    return out


def _ranges(table):
    out = []
    for name, t in table.items():
        if t is None or t.numel() == 0:
            continue
        assert t.is_contiguous(), name
        out.append((name, t.data_ptr(), t.numel() * t.element_size()))
    return out


def _resolve(a, ranges, where):
    if isinstance(a, _Ptr):
        hits = [(size, i, name, a - start) for i, (name, start, size) in enumerate(ranges) if start <= a < start + size]
        if not hits:
            raise AssertionError(f"{where}: pointer {int(a):#x} belongs to no tensor of the table")
        _, _, name, off = min(hits)             # a view inside a larger buffer: the narrowest owner
        return f"{name}+{off}"
    if isinstance(a, list):
        return [_resolve(e, ranges, where) for e in a]
    if isinstance(a, dict):
        return {k: _resolve(v, ranges, where) for k, v in a.items()}
    return a


# ---- pointer tables -----------------------------------------------------------------------------------------------------
def _ops(module, prefix, table):
    for k, v in module._packed_ops(CPU).items():
        if isinstance(v, torch.Tensor):
            table[f"{prefix}{k}"] = v


def block_table(blk, prefix="", table=None):
    table, st = {} if table is None else table, blk._state
    table[prefix + "y"], table[prefix + "out"] = st.y, st.out
    if st.owns_xin:
        table[prefix + "xin"] = st.xin
    if st.owns_partial:
        table[prefix + "partial"] = st.partial
    _ops(blk, prefix + "tcn.", table)
    _ops(blk.gcn, prefix + "gcn.", table)
    return table


def model_table(net, frames):
    table = {"frames": frames, "xin0": net._xin0, "pool_ring": net._pool_ring, "pooled": net._pooled, "scratch": net._scratch,
             "fc.weight": net.fc.weight, "fc.bias": net.fc.bias}
    _ops(net, "ops.", table)
    for name, blk in net.layers.items():
        block_table(blk, name + ".", table)
    return table


# ---- scenarios ----------------------------------------------------------------------------------------------------------
def _model(pkg, setup=None):
    net = pkg.CoStGcn(pkg.ntu_graph().A, pool_size=4, pool_padding=1).eval()
    net.use_native_plan = False
    net.set_max_cycle(8)
    if setup is not None:
        setup(net)
    return net


def _drive_model(pkg, net, cycles, flush):
    total = sum(cycles)
    c, _, v, m = net.input_shape
    x = torch.zeros((total, 1, c, v, m), dtype=torch.float32)
    with Recorder(pkg) as rec:
        net._bind(1, CPU)
        pos = 0
        for r in cycles:
            slot, nf, outs = net._python_cycle([x[pos + j] for j in range(r)])
            pos += r
            table = model_table(net, x)
            table.update({f"logits{j}": o for j, o in enumerate(outs)})
            rec.settle(table, (slot, nf, len(outs)))
        if flush:
            outs = net._flush()
            table = model_table(net, x)
            table.update({f"logits{j}": o for j, o in enumerate(outs)})
            rec.settle(table, ("flush", len(outs)))
        rec.calls.append(["counters", ""] + net._counters())
    return rec.calls


def _mixed(total):
    cycles = []
    while sum(cycles) < total:
        cycles.append(min(CYCLE_MIX[len(cycles) % len(CYCLE_MIX)], total - sum(cycles)))
    return cycles


def _fusion_off(net):
    for blk in net.layers.values():
        blk.fuse_step = False


def scenario_default(pkg):
    return _drive_model(pkg, _model(pkg), _mixed(96), flush=True)


def scenario_fusion_off(pkg):
    return _drive_model(pkg, _model(pkg, _fusion_off), _mixed(96), flush=True)


def scenario_latency(pkg):
    return _drive_model(pkg, _model(pkg, lambda net: net.set_latency_mode(2)), [4] * 12, flush=True)


def scenario_bf16x3_step(pkg):
    return _drive_model(pkg, _model(pkg, lambda net: pkg.continual.set_step_precision(net, "bf16x3")), [4] * 12, flush=False)


def scenario_block(pkg):
    blk = pkg.CoSpatioTemporalBlock(4, 8, pkg.ntu_graph().A, stride=2).eval()
    assert blk.kind == "conv"
    with Recorder(pkg) as rec:
        blk.bind_state(176, CPU)
        for i in range(20):
            res = blk.engine_advance(i % 8 + 1, 7, 25)
            rec.settle(block_table(blk), ("none",) if res is None else res)
        for r in (1, 2, 3, 4):
            res = blk.engine_advance(r, 7, 25, flush=True)
            rec.settle(block_table(blk), ("none",) if res is None else res)
        rec.calls.append(["counters", "", blk._state.s, blk._state.e])
    return rec.calls


def scenario_layer_structs(pkg):
    net = _model(pkg)
    x = torch.zeros((1, 1) + (net.input_shape[0], net.input_shape[2], net.input_shape[3]), dtype=torch.float32)
    with Recorder(pkg) as rec:
        net._bind(1, CPU)
        arr, keep, ops, fcw, fcb = net._layer_structs(CPU)
        ranges = _ranges(model_table(net, x))
        rec.calls += [["csk_co_layer", str(i), _resolve(_raw_struct(arr[i]), ranges, f"layer {i}")] for i in range(10)]
        rec.calls.append(["model operands", ""] + _resolve([_Ptr(t.data_ptr()) for t in (ops["scale"], ops["shift"], fcw, fcb)],
                                                             ranges, "model operands"))
    return rec.calls


SCENARIOS = {"default": scenario_default, "fusion_off": scenario_fusion_off, "latency": scenario_latency,
             "bf16x3_step": scenario_bf16x3_step, "block": scenario_block, "layer_structs": scenario_layer_structs}


def record(name):
    return json.loads(json.dumps(SCENARIOS[name](_bootstrap.load())))       # through JSON: what the fixture can hold


# ---- fixture format -----------------------------------------------------------------------------------------------------
# Most arguments of a launch are the same on every cycle (operand pointers, shapes); what moves is a handful of ring slots.  The
# fixture stores "templates" -- a call with every number (pointer offsets included) taken out, plus the numbers that are the same
# in all calls of that shape -- and per scenario the rows [template index, the remaining numbers...], one line per cycle.
# ``decode`` gives back the full call list; nothing is lost.
def _split(x, values):
    """Call -> skeleton with "#" where a number stood; the numbers go to ``values`` in order."""
    if isinstance(x, (int, float)) and not isinstance(x, bool):
        values.append(x)
        return "#"
    if isinstance(x, str) and "+" in x and x.rsplit("+", 1)[1].isdigit():
        values.append(int(x.rsplit("+", 1)[1]))
        return x.rsplit("+", 1)[0] + "+#"
    if isinstance(x, list):
        return [_split(e, values) for e in x]
    if isinstance(x, dict):
        return {k: _split(v, values) for k, v in x.items()}
    return x


def _join(skel, values):
    if skel == "#":
        return next(values)
    if isinstance(skel, str) and skel.endswith("+#"):
        return f"{skel[:-1]}{next(values)}"
    if isinstance(skel, list):
        return [_join(e, values) for e in skel]
    if isinstance(skel, dict):
        return {k: _join(v, values) for k, v in skel.items()}
    return skel


def encode(traces):
    """{scenario: calls} -> {"templates": [[skeleton, fixed numbers (None: moving)], ...], "scenarios": {scenario: rows}}."""
    shapes, rows = {}, {}
    for name, calls in traces.items():
        rows[name] = []
        for c in calls:
            values = []
            key = json.dumps(_split(c, values))
            shapes.setdefault(key, []).append(values)
            rows[name].append((key, values))
    index = {key: i for i, key in enumerate(shapes)}
    fixed = {key: [v if all(o[j] == v for o in vs) else None for j, v in enumerate(vs[0])] for key, vs in shapes.items()}
    return {"templates": [[json.loads(key), fixed[key]] for key in shapes],
            "scenarios": {name: [[index[key]] + [v for v, f in zip(values, fixed[key]) if f is None] for key, values in rs]
                          for name, rs in rows.items()}}


def decode(enc, name):
    calls = []
    for tid, *moving in enc["scenarios"][name]:
        skel, fixed = enc["templates"][tid]
        moving = iter(moving)
        calls.append(_join(skel, iter([next(moving) if f is None else f for f in fixed])))
    return calls


def dump(path):
    def compact(x):
        return json.dumps(x, separators=(",", ":"))
    enc = encode({name: record(name) for name in SCENARIOS})
    ends = {i for i, (skel, _) in enumerate(enc["templates"]) if skel[0] in ("return", "counters")}
    with open(path, "w") as f:
        f.write('{"templates": [\n' + ",\n".join(" " + compact(t) for t in enc["templates"]) + '\n], "scenarios": {\n')
        for i, (name, rows) in enumerate(enc["scenarios"].items()):
            f.write(f' "{name}": [\n  ')
            f.write("".join(compact(c) + ("" if j + 1 == len(rows) else ",\n  " if c[0] in ends else ",") for j, c in enumerate(rows)))
            f.write("\n ]" + ("," if i + 1 < len(SCENARIOS) else "") + "\n")
        f.write("}}\n")


if __name__ == "__main__":
    dump(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
