"""A stored clip at the steps' arithmetic, the parts that need no GPU: the index map of every continual
family against a frame-by-frame simulation of the counters and the pooling window, the refusals ``prime_state`` keeps, the host
checks of ``CoAGcn.prime_state_as_steps`` (no launch), and the symbol, signature and argument checks of csk_co_head_clip_f32."""
import ctypes as C
import os
import re

import pytest
import torch

import _bootstrap

pkg = _bootstrap.load()
native = pkg.native
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = pkg.ntu_graph().A


# ---- the index map ---------------------------------------------------------------------------------------------------------
def _simulate(net, t, pad_end):
    """A fresh model stepped through ``t`` frames, one at a time, on counters alone: every block follows
    ``continual.emissions``; with ``pad_end`` the flush of ``CoStGcn._flush`` (block by block, its ``padding`` zero frames, what
    it releases travelling down the rest of the stack), then ``pool_padding`` zero entries.  The head of ``_head_step``: entry
    number ``feats`` releases a prediction when feats >= pool_size - pool_padding, over the min(feats, pool_size) newest
    entries.  Returns (layer-10 frames emitted, [(first, last) entry of every prediction])."""
    blocks = net._blocks
    received = [0] * len(blocks)
    state = {"feats": 0, "real": 0}
    preds = []

    def head(real):
        state["feats"] += 1
        state["real"] += real
        f = state["feats"]
        if f >= net.pool_size - net.pool_padding:
            preds.append((f - min(f, net.pool_size), f - 1))

    def push(i0, r):
        for i in range(i0, len(blocks)):
            _, e = pkg.continual.emissions(received[i], r, blocks[i].delay, blocks[i].stride)
            received[i] += r
            if not e:
                return 0
            r = e
        return r

    for _ in range(t):
        for _ in range(push(0, 1)):
            head(1)
    if pad_end and t > 0:
        for i, blk in enumerate(blocks):
            for _ in range(blk.padding):
                for _ in range(push(i, 1)):
                    head(1)
        for _ in range(net.pool_padding):
            head(0)
    return state["real"], preds


POOLS = [(4, 0), (4, 1), (1, 0), (3, 2), (7, 7), (-1, -1)]            # (pool_size, pool_padding); -1: the defaults of the head


def _net(cls, pool, t_shape=300):
    return cls(A, input_shape=(3, t_shape, 25, 2), pool_size=pool[0], pool_padding=pool[1]).eval()


@pytest.mark.parametrize("pad_end", [False, True])
@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("t", [0, 75, 76, 80, 96])
def test_padded_map_equals_a_frame_by_frame_simulation(t, pool, pad_end):
    net = _net(pkg.CoStGcn, pool)
    assert (net.receptive_field, net.padding, net.stride) == (153, 76, 4)
    frames, entries = pkg.CoStGcn.clip_as_steps_map(net, t, pad_end)
    assert (frames, entries) == _simulate(net, t, pad_end)
    assert frames == (net.prime_clip_frames(t)[-1] if pad_end and t else net.prime_counts(t)[-1])
    # CoAGcn's own derivation is unchanged and gives the same values for the padded table
    agcn = _net(pkg.CoAGcn, pool)
    assert "clip_as_steps_map" in vars(pkg.CoAGcn) and agcn.clip_as_steps_map(t, pad_end) == (frames, entries)
    assert pkg.CoSTr.clip_as_steps_map is pkg.CoStGcn.clip_as_steps_map


@pytest.mark.parametrize("pad_end", [False, True])
@pytest.mark.parametrize("pool", POOLS + [(16, 0)])
@pytest.mark.parametrize("t", [80, 81, 84, 96])
def test_unpadded_map_equals_a_frame_by_frame_simulation(t, pool, pad_end):
    """Delay 8 per block, stride 1, padding 0: the flush of ``pad_end`` pushes nothing through the blocks (read off
    ``CoStGcn._flush``: ``blk.padding`` frames per block), so only the window's ``pool_padding`` zero entries follow."""
    net = _net(pkg.CoStGcnMod, pool, t_shape=96)
    assert (net.receptive_field, net.padding, net.stride) == (81, 0, 1) and all(b.padding == 0 and b.delay == 8 for b in net._blocks)
    if pool == (-1, -1):
        assert (net.pool_size, net.pool_padding) == (16, 0)
    frames, entries = net.clip_as_steps_map(t, pad_end)
    assert (frames, entries) == _simulate(net, t, pad_end)
    assert frames == max(0, t - 80)
    for cls in (pkg.agcn.CoAGcnMod, pkg.str.CoSTrMod):
        assert cls.clip_as_steps_map is pkg.CoStGcn.clip_as_steps_map and cls.forward_clip_as_steps is pkg.CoStGcn.forward_clip_as_steps


def test_a_history_too_short_to_predict_is_empty_without_a_launch(monkeypatch):
    monkeypatch.setattr(native, "lib", lambda: _NoLaunch())
    _NoLaunch.calls = 0
    cases = ((_net(pkg.CoStGcn, (4, 0)), 88, (False,)),                          # 3 entries of 4 (the flush would release 22)
             (_net(pkg.CoStGcnMod, (4, 0), 96), 83, (False, True)), (_net(pkg.CoStGcnMod, (4, 0), 96), 40, (False, True)))
    for net, t, flags in cases:
        for pad_end in flags:
            out = net.forward_clip_as_steps(torch.zeros((2, 3, t, 25, 2)), pad_end)
            assert tuple(out.shape) == (2, 60, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _net(pkg.CoStGcn, (4, 0)).forward_clip_as_steps(torch.zeros((2, 3, 96, 25, 2)))
    with pytest.raises(ValueError, match="needs T >= 81"):
        _net(pkg.CoStGcnMod, (4, 0), 96).features_clip_as_steps(torch.zeros((2, 3, 80, 25, 2)))
    split = pkg.set_precision(_net(pkg.CoStGcn, (4, 0)), "bf16x3")
    with pytest.raises(NotImplementedError, match="clip precision of this model is 'bf16x3'"):
        split.forward_clip_as_steps(torch.zeros((2, 3, 96, 25, 2)))
    with pytest.raises(NotImplementedError, match="clip precision of this model is 'bf16x3'"):
        split.features_clip_as_steps(torch.zeros((2, 3, 96, 25, 2)))
    with pytest.raises(RuntimeError, match="inference-only"):
        _net(pkg.CoStGcn, (4, 0)).train().forward_clip_as_steps(torch.zeros((2, 3, 96, 25, 2)))
    assert _NoLaunch.calls == 0


# ---- priming ------------------------------------------------------------------------------------------------------------
class _NoLaunch:
    """Stands in for the library: any call is a failure of the test."""
    calls = 0

    def __getattr__(self, name):
        def entry(*a, **k):
            _NoLaunch.calls += 1
            raise AssertionError(f"{name} was called")
        return entry


def _hist(t, n=1, c=3, v=25, m=2):
    return torch.zeros((n, c, t, v, m))


def test_prime_state_keeps_its_refusals():
    with pytest.raises(NotImplementedError, match="one\\s+adjacency over all T frames"):
        _net(pkg.CoAGcn, (4, 0)).prime_state(_hist(96))
    with pytest.raises(NotImplementedError, match="one\\s+adjacency over all T frames"):
        _net(pkg.CoAGcn, (4, 0)).prime_streams(_hist(96), [0])
    for cls in (pkg.CoStGcnMod, pkg.agcn.CoAGcnMod, pkg.str.CoSTrMod):
        with pytest.raises(NotImplementedError, match=r"unpadded '\*' models.*follow-up"):
            _net(cls, (4, 0)).prime_state(_hist(96))
        assert not hasattr(cls, "prime_state_as_steps")
    assert not hasattr(pkg.CoStGcn, "prime_state_as_steps")


def test_prime_state_as_steps_checks_on_the_host_before_any_launch(monkeypatch):
    monkeypatch.setattr(native, "lib", lambda: _NoLaunch())
    _NoLaunch.calls = 0
    net = _net(pkg.CoAGcn, (4, 0))
    for call in (net.prime_state_as_steps, lambda x: net.prime_streams_as_steps(x, [0])):
        for t in (77, 78, 98):
            with pytest.raises(ValueError, match="not a multiple of the total stride 4"):
                call(_hist(t))
        for t in (4, 72):
            with pytest.raises(ValueError, match=r"younger than the 76 frames"):
                call(_hist(t))
        with pytest.raises(RuntimeError, match="does not match input_shape"):
            call(_hist(96, v=18))
        with pytest.raises(RuntimeError, match=r"\(n, C, T, V, M\) history tensor"):
            call(torch.zeros((3, 96, 25, 2)))
        with pytest.raises(RuntimeError, match="no CPU fallback"):                # a history that passes every other check
            call(_hist(96))
    for blk in net._blocks:                                                          # what set_precision marks on a block
        blk.precision = "bf16x3"
    with pytest.raises(NotImplementedError, match="clip precision of this model is 'bf16x3'"):
        net.prime_state_as_steps(_hist(96))
    with pytest.raises(RuntimeError, match="inference-only"):
        _net(pkg.CoAGcn, (4, 0)).train().prime_state_as_steps(_hist(96))
    assert _NoLaunch.calls == 0


def test_prime_streams_as_steps_runs_the_import_checks_before_any_launch(monkeypatch):
    monkeypatch.setattr(native, "lib", lambda: _NoLaunch())
    monkeypatch.setattr(native, "require_device_f32", lambda t, name: None)
    _NoLaunch.calls = 0
    net = _net(pkg.CoAGcn, (4, 0))
    net.use_native_plan = False
    with pytest.raises(RuntimeError, match="no state slab is bound"):
        net.prime_streams_as_steps(_hist(96), [0])
    net._bind(3, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="step it through its warm-up first"):
        net.prime_streams_as_steps(_hist(96), [0])
    assert _NoLaunch.calls == 0


# ---- csk_co_head_clip_f32 ----------------------------------------------------------------------------------------------------
def test_head_clip_symbol_signature_and_abi():
    hdr = open(os.path.join(ROOT, "include", "cskel.h")).read()
    decl = re.search(r"int csk_co_head_clip_f32\(([^;]*)\);", hdr)
    assert decl, "csk_co_head_clip_f32 is not declared in include/cskel.h"
    params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
    kinds = [C.c_void_p if "*" in p else (C.c_int64 if p.startswith("int64_t") else C.c_int) for p in params]
    assert native.SIGNATURES["csk_co_head_clip_f32"] == kinds and len(kinds) == 17
    assert hasattr(C.CDLL(native.LIB_PATH), "csk_co_head_clip_f32")
    assert native.lib().csk_abi_version() == native.ABI_VERSION == 16            # additive: the version stays
    assert int(re.search(r"#define CSK_ABI_VERSION (\d+)", hdr).group(1)) == 16
    comment = hdr[: hdr.index("#define CSK_ABI_VERSION")].rsplit("/*", 1)[1]
    assert "csk_co_head_clip_f32" in comment


def _head(h=0x10000, t_src=7, frames=5, entries=0x20000, window=4, first_entry=3, n_pred=3, fc_w=0x30000, fc_b=0x40000, pooled=0x50000,
          logits=0x60000, n=2, m=2, c=256, v=25, classes=60):
    p = C.c_void_p
    return native.lib().csk_co_head_clip_f32(p(h), t_src, frames, p(entries), window, first_entry, n_pred, p(fc_w), p(fc_b), p(pooled),
                                             p(logits), n, m, c, v, classes, None)


@pytest.mark.parametrize("kwargs, needle", [
    (dict(h=0), "null pointer"), (dict(fc_w=0), "null pointer"), (dict(fc_b=0), "null pointer"), (dict(pooled=0), "null pointer"),
    (dict(logits=0), "null pointer"), (dict(entries=0), "null pointer (entries"),
    (dict(h=0x10002), "not 4-byte aligned"), (dict(entries=0x20001), "not 4-byte aligned"), (dict(fc_b=0x40002), "not 4-byte aligned"),
    (dict(logits=0x60002), "not 4-byte aligned"),
    (dict(fc_w=0x30004), "16-byte aligned when C is a multiple of 4"), (dict(pooled=0x50008), "16-byte aligned when C is a multiple of 4"),
    (dict(n=0), "bad dims"), (dict(m=0), "bad dims"), (dict(c=0), "bad dims"), (dict(v=0), "bad dims"), (dict(classes=0), "bad dims"),
    (dict(t_src=0, frames=0), "bad dims"),
    (dict(frames=-1), "-1 real frames of a source of 7"), (dict(frames=8), "8 real frames of a source of 7"),
    (dict(window=0), "a window of 0"), (dict(first_entry=-1), "first_entry -1 < 0"), (dict(n_pred=-1), "n_pred -1 < 0"),
    (dict(c=8193), "at most 8192 channels"), (dict(window=8192), "a window of 8192 entries (at most 8177)"), (dict(n=65536), "at most 65535 streams"),
])
def test_head_clip_refuses_bad_arguments_without_a_gpu(kwargs, needle):
    lib = native.lib()
    assert _head(**kwargs) == -1
    assert needle in lib.csk_last_error().decode(), lib.csk_last_error().decode()


def test_head_clip_with_no_prediction_launches_nothing():
    assert _head(n_pred=0) == 0
    assert _head(n_pred=0, frames=0, entries=0) == 0                             # no real frame: no scratch needed
    assert _head(n_pred=0, c=3, fc_w=0x30004, pooled=0x50008) == 0               # off the multiple of 4: rows may sit at any 4 bytes
    assert _head(n_pred=0, window=0) == -1                                       # the checks come first
