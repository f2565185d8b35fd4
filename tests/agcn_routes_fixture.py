"""Launch-trace recorder of the A-GCN graph conv and of the clip drivers (test infrastructure, needs no GPU).

``AdaptiveGraphConvolution`` decides on the host which launches form a per-sample adjacency -- the fused embed-attention entry
or the 1x1 conv + attention pair -- on which geometry, with which allocations; the clip drivers decide the order of the input
norm and the ten blocks.  This module pins those decisions: it replaces ``native.lib`` by an object whose every ``csk_*``
attribute records ``[name, args...]`` and returns 0, ``native.ptr`` by a holder of the tensor itself, ``native.stream_of`` and
``native.require_device_f32`` by stubs, and drives the modules on CPU memory.  Integers and floats are recorded by value.  A
pointer argument is recorded as ``[role, byte offset, shape, bytes of its storage]``: the role is the name the scenario's table
gives the tensor that owns the storage (the input, a packed operand), the offset is relative to that tensor -- a chunk's view
shows here -- and a tensor the code under test allocated itself is ``t<k>``, numbered in order of first appearance (its shape
and storage size are the allocation's: the slack behind a buffer shows in the last number).  tests/golden/agcn_routes_trace.json
holds the traces of the drivers before their launch sequences were gathered into one copy each (tests/test_agcn_routes_cpu.py).

``python tests/agcn_routes_fixture.py PATH`` writes the traces of the checked-out tree to PATH.
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "agcn_routes_trace.json")
CPU = torch.device("cpu")


class _Arg:
    """What the stand-in of ``native.ptr`` returns: the tensor, not its address."""

    def __init__(self, tensor):
        self.tensor = tensor


class _FakeLib:
    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        if not name.startswith("csk_"):
            raise AttributeError(name)
        return lambda *args: self._rec.call(name, args)


class Recorder:
    """Context manager: while active, every library call of the package is recorded instead of made.  ``table``: {role: tensor}
    of the tensors the scenario knows by name; ``route``: what the ``*_route`` queries answer (0: no kernel for the shape)."""

    def __init__(self, pkg, table, route=0):
        self.pkg, self.calls, self.route = pkg, [], route
        self._roles, self._by_address, self._keep, self._fresh = {}, {}, [], 0
        for role, t in table.items():
            if isinstance(t, torch.Tensor) and t.numel():
                self._roles.setdefault(t.untyped_storage().data_ptr(), (role, t.data_ptr()))
                self._keep.append(t)

    def __enter__(self):
        native = self.pkg.native
        self._saved = (native.lib, native.ptr, native.stream_of, native.require_device_f32)
        fake = _FakeLib(self)
        native.lib = lambda: fake
        native.ptr = lambda t: None if t is None else _Arg(t)
        native.stream_of = lambda t: "stream"
        native.require_device_f32 = lambda t, name: None
        return self

    def __exit__(self, *exc):
        native = self.pkg.native
        native.lib, native.ptr, native.stream_of, native.require_device_f32 = self._saved
        return False

    def call(self, name, args):
        self.calls.append([name] + [self._value(a) for a in args])
        return self.route if name.endswith("_route") else 0

    def _tensor(self, t):
        storage = t.untyped_storage()
        if storage.data_ptr() not in self._roles:        # allocated by the code under test: kept alive, so no address comes twice
            self._roles[storage.data_ptr()] = (f"t{self._fresh}", storage.data_ptr())
            self._fresh += 1
        self._keep.append(t)
        role, base = self._roles[storage.data_ptr()]
        seen = [role, t.data_ptr() - base, list(t.shape), storage.nbytes()]
        self._by_address.setdefault(t.data_ptr(), seen[:3])
        return seen

    def _value(self, a):
        if a is None or isinstance(a, (str, float)):
            return a
        if isinstance(a, (bool, int)):
            return int(a)
        if isinstance(a, _Arg):
            return self._tensor(a.tensor)
        if hasattr(a, "_obj"):                           # ctypes.byref(x)
            return self._value(a._obj)
        if isinstance(a, C.Array) and issubclass(a._type_, C.Structure):
            return [self._struct(s) for s in a]
        raise TypeError(f"trace recorder: argument of type {type(a).__name__}")

    def _struct(self, s):
        """A job struct: numbers by value, an address as the tensor an earlier call has shown at it."""
        out = {}
        for name, ctype in s._fields_:
            v = getattr(s, name)
            out[name] = v if ctype is not C.c_void_p else (None if v is None else self._by_address[v])
        return out


def _ops(module, prefix, table):
    for k, v in module._packed_ops(CPU).items():
        if isinstance(v, torch.Tensor):
            table[f"{prefix}{k}"] = v
    return table


# ---- the adaptive graph conv ----------------------------------------------------------------------------------------------
N = 2
JOINTS = (18, 25)
CHANNELS = ((3, 64), (64, 64), (64, 128))        # inter 16, 16, 32; conv, identity and conv gcn_residual
FRAMES = (1, 5)


def _graph_conv(pkg, v, ci, co, fuse):
    A = pkg.kinetics_graph().A if v == 18 else pkg.ntu_graph().A
    g = pkg.AdaptiveGraphConvolution(ci, co, A).eval()
    g.fuse_embed_attention = fuse
    g.fuse_framewise = False
    return g


def _run(pkg, g, table, call, route=0):
    with Recorder(pkg, _ops(g, "ops.", table), route) as rec:
        call()
    return rec.calls


def _clip_input(ci, t, v):
    return torch.zeros((N, ci, t, v), dtype=torch.float32)


def chunked_budget(g, v, fuse):
    """A ``framewise_budget_bytes`` that holds two frames and a half of what ``forward_framewise`` keeps per frame of N
    sequences: the 3 V V adjacency floats, and on the two-launch route the 6 * inter embedding rows of V floats."""
    per_frame = 4 * N * (3 * v * v + (0 if fuse else 6 * g.inter_c * v))
    return 2 * per_frame + per_frame // 2


def graph_conv_scenarios(pkg):
    """{name: thunk -> calls}: forward, forward_framewise (composed, one chunk and 2 + 2 + 1 frames; the frame-wise kernel where
    the route query names one) and stage, over JOINTS x CHANNELS x FRAMES x fused / two-launch."""
    out = {}
    for v in JOINTS:
        for ci, co in CHANNELS:
            for t in FRAMES:
                for fuse in (True, False):
                    tag = f"V{v}-{ci}x{co}-T{t}-{'fused' if fuse else 'two'}"

                    def forward(v=v, ci=ci, co=co, t=t, fuse=fuse):
                        g, x = _graph_conv(pkg, v, ci, co, fuse), _clip_input(ci, t, v)
                        return _run(pkg, g, {"x": x}, lambda: g.forward(x))

                    def framewise(v=v, ci=ci, co=co, t=t, fuse=fuse, chunked=False):
                        g, x = _graph_conv(pkg, v, ci, co, fuse), _clip_input(ci, t, v)
                        if chunked:
                            g.framewise_budget_bytes = chunked_budget(g, v, fuse)
                        return _run(pkg, g, {"x": x}, lambda: g.forward_framewise(x))

                    def stage(v=v, ci=ci, co=co, t=t, fuse=fuse):
                        # t ring slots of N skeletons each, channel-major with the row padded to a multiple of 4 floats
                        g, p = _graph_conv(pkg, v, ci, co, fuse), (N * v + 3) // 4 * 4
                        x, y = torch.zeros((t, ci, p)), torch.zeros((t, co, p))
                        return _run(pkg, g, {"x": x, "y": y}, lambda: g.stage(x, y, n_seg=t, frames=N, x_strides=(ci * p, p),
                                                                               y_strides=(co * p, p)))

                    out[f"forward-{tag}"], out[f"framewise-{tag}"], out[f"stage-{tag}"] = forward, framewise, stage
                    if t == 5:
                        out[f"framewise-chunked-{tag}"] = lambda framewise=framewise: framewise(chunked=True)
            if (ci, co) == (64, 128):

                def kernel(v=v, ci=ci, co=co):
                    g, x = _graph_conv(pkg, v, ci, co, True), _clip_input(ci, 5, v)
                    g.fuse_framewise = g.framewise_everywhere = True
                    return _run(pkg, g, {"x": x}, lambda: g.forward_framewise(x), route=32000 + v * 10 + 1)

                out[f"framewise-kernel-V{v}-{ci}x{co}-T5"] = kernel
    return out


# ---- the clip drivers: input norm, then the ten blocks -----------------------------------------------------------------------
SHAPE = (3, 16, 25, 2)                            # input_shape (C, T, V, M) of the driver scenarios
PRIME_FRAMES = 80                                 # a history every block of a fresh model has emitted from (D(10) = 76), stride phase 0


def _model(pkg, cls, **kwargs):
    net = cls(pkg.ntu_graph().A, input_shape=SHAPE, **kwargs).eval()
    table = _ops(net, "ops.", {"fc.weight": net.fc.weight, "fc.bias": net.fc.bias})
    for name, blk in net.layers.items():
        _ops(blk, f"{name}.tcn.", table)
        _ops(blk.gcn, f"{name}.gcn.", table)
    return net, table


def _clip(t=SHAPE[1], v=SHAPE[2]):
    return torch.zeros((1, SHAPE[0], t, v, SHAPE[3]), dtype=torch.float32)


def _drive(pkg, cls, call, x, route=0, **kwargs):
    net, table = _model(pkg, cls, **kwargs)
    with Recorder(pkg, dict(table, x=x), route) as rec:
        call(net, x)
    return rec.calls


def _prime(net, x):
    net._prime_chunk(x, torch.zeros((x.shape[0], net.record_floats()), dtype=torch.float32))


def _prime_framewise(net, x):
    net._prime_chunk(x, torch.zeros((x.shape[0], net.record_floats()), dtype=torch.float32), net._framewise_parts)


POOL = dict(pool_size=4, pool_padding=1)
# name -> (model class, its keywords, the call, frames of the clip, the route answer)
DRIVERS = {
    "StGcn.features": ("StGcn", {}, lambda net, x: net.features(x), SHAPE[1], 0),
    "CoStGcn._clip_stack": ("CoStGcn", POOL, lambda net, x: net._clip_stack(x), SHAPE[1], 0),
    "CoAGcn.features_clip_as_steps": ("CoAGcn", POOL, lambda net, x: net.features_clip_as_steps(x), SHAPE[1], 0),
    "CoAGcn.features_clip_as_steps-kernel": ("CoAGcn", POOL, lambda net, x: net.features_clip_as_steps(x), SHAPE[1], 1),
    "CoStGcn._prime_chunk": ("CoStGcn", POOL, _prime, PRIME_FRAMES, 0),
    "CoAGcn._prime_chunk-framewise": ("CoAGcn", POOL, _prime_framewise, PRIME_FRAMES, 0),
}


def drive(pkg, name, x=None):
    cls, kwargs, call, t, route = DRIVERS[name]
    return _drive(pkg, getattr(pkg, cls), call, _clip(t) if x is None else x, route, **kwargs)


def scenarios(pkg):
    out = graph_conv_scenarios(pkg)
    out.update({name: (lambda name=name: drive(pkg, name)) for name in DRIVERS})
    return out


def record(thunk):
    return json.loads(json.dumps(thunk()))          # through JSON: what the fixture can hold


def dump(path):
    pkg = _bootstrap.load()
    with open(path, "w") as f:
        rows = []
        for name, thunk in scenarios(pkg).items():
            calls = ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in record(thunk))
            rows.append(f' "{name}": [\n{calls}\n ]')
        f.write("{\n" + ",\n".join(rows) + "\n}\n")


if __name__ == "__main__":
    dump(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
