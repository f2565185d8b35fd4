"""Priming CoAGcn streams from buffered history at the steps' arithmetic (``prime_state_as_steps`` / ``prime_streams_as_steps``,
agcn.py).  The yardstick is the stream that was STEPPED through the same history: its exported record, job by
job, and what it goes on to predict -- the patterns of tests/test_gpu_stream_prime.py, restated for the family whose clip pass
must form its attention per frame.  Small states and structural zeros bit for bit; activations per job within
max|primed - stepped| <= 1e-4 max|stepped| (the bound of 3e).  The observed ratios are printed (run with -s)."""
import contextlib
import functools

import pytest
import torch

import _bootstrap
from tests.helpers import randomise_unit_

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native = pkg.native
DEV = "cuda:0"
AGC = pkg.agcn.AdaptiveGraphConvolution
T_MORE = 16
SMALL = ("mod_prev", "mod_flags", "pn_rot", "pn_flags")


def _small_states(net):
    pkg.set_input_modality(net, "bone_motion")
    pkg.set_pre_normalization(net)


def _make(graph, sizes, small=False, seed=7):
    """One CoAGcn per entry of ``sizes`` with the same seeded weights, on the device."""
    a = (pkg.ntu_graph() if graph == "ntu" else pkg.kinetics_graph()).A
    v = a.shape[-1]
    nets = [pkg.CoAGcn(a, (3, 300, v, 2), 60, pool_size=4, pool_padding=0).eval() for _ in sizes]
    randomise_unit_(nets[0], seed, attn_scale=1 / v)
    for net in nets[1:]:
        net.load_state_dict(nets[0].state_dict())
    for net in nets:
        if small:
            _small_states(net)
    return [net.to(DEV) for net in nets], v


def _frames(t, n, v, seed):
    return torch.rand((t, n, 3, v, 2), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _steps(net, frames, t0, t1, r=4):
    out = []
    for t in range(t0, t1, r):
        out += net._cycle([frames[t + f] for f in range(r)])[2]
    return out


def _history(frames, t):
    return frames[:t].permute(1, 2, 0, 3, 4).contiguous()


@functools.lru_cache(maxsize=None)
def _stepped(graph, small, t):
    """Slab A: 3 streams stepped through ``t`` frames of a seeded history, left at frame ``t``; computed once per configuration
    and put back by whoever steps it on (``_restored``)."""
    (A,), v = _make(graph, (3,), small)
    frames = _frames(t + T_MORE, 3, v, 100 + t)
    _steps(A, frames, 0, t)
    return A, frames, v


@contextlib.contextmanager
def _restored(net):
    tensors = net._state_tensors()
    keep, position = [x.clone() for x in tensors], net._position()
    try:
        yield
    finally:
        for x, k in zip(tensors, keep):
            x.copy_(k)
        net._set_position(position)


def _compare_records(net, primed, stepped, t, label):
    table = {name: (count, first, window) for name, _, count, first, window in net.prime_table(t)}
    offset, worst = 0, 0.0
    p, s = primed.cpu(), stepped.cpu()
    for name, rows, seg, window in net._move_windows():
        size = rows * seg * window
        a, b = p[:, offset: offset + size], s[:, offset: offset + size]
        if name in SMALL:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (label, name)
            assert bool((b.view(torch.int32) != 0).any()), (label, name, "the stepped state is empty: nothing was compared")
        else:
            count, first, _ = table[name]
            lead = max(0, -first) * (size // window)                                # words of the frames in front of the clip
            assert int(a[:, :lead].view(torch.int32).abs().max() if lead else 0) == 0, (label, name, "leading frames are not +0")
            assert torch.equal(a[:, :lead].view(torch.int32), b[:, :lead].view(torch.int32)), (label, name)
            scale = float(b.abs().max())
            ratio = float((a - b).abs().max()) / scale if scale else 0.0
            worst = max(worst, ratio)
            print(f"agcn prime-vs-steps {label} T={t} {name}: max|primed-stepped|/max|stepped| = {ratio:.3e} (bound 1e-4), "
                  f"count {count}, first {first}")
            assert count == 0 or scale > 0, (label, name, "the stepped window is empty: nothing was compared")
            assert ratio <= 1e-4, (label, name, ratio)
        offset += size
    assert offset == net.record_floats()
    print(f"agcn prime-vs-steps {label} T={t}: worst ratio {worst:.3e}")
    return worst


RECORD_CASES = [("ntu", True, 96), ("ntu", True, 76), ("kinetics", False, 80)]


@pytest.mark.parametrize("graph,small,t", RECORD_CASES, ids=[f"{g}-{'small' if s else 'plain'}-T{t}" for g, s, t in RECORD_CASES])
def test_primed_record_equals_the_stepped_streams_record(graph, small, t):
    """Slab A steps the history and exports; ``prime_state_as_steps`` of the same history gives the same record, job by job.
    With bone_motion and pre-normalisation on, the previous raw frame, both flags and the latched rotations match bit for bit.
    ``prime_state`` keeps refusing the class; the model's continual state and position are untouched."""
    A, frames, v = _stepped(graph, small, t)
    x = _history(frames, t)
    with pytest.raises(NotImplementedError, match="one\\s+adjacency over all T frames"):
        A.prime_state(x)
    before, position = [s.clone() for s in A._state_tensors()], A._position()
    state = A.prime_state_as_steps(x)
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(A._state_tensors(), before))
    assert A._position() == position
    assert state.ages.tolist() == [t] * 3 and state.signature == A.move_signature() and state.packed.shape == (3, A.record_floats())
    _compare_records(A, state.packed, A._export([0, 1, 2]).packed, t, f"{graph}-{'small' if small else 'plain'}")


def test_a_primed_stream_continues_as_the_stepped_stream():
    """Slab B (and its twin B') is warmed on other frames to frame 100; ``prime_streams_as_steps(x[1:2], [1])`` makes its stream
    1 the stream A stepped through x.  Both step 16 further frames in cycles of 4: B's logits of stream 1 are allclose (rtol
    1e-4, atol 1e-5) to A's, B's streams 0 and 2 are bit for bit B''s."""
    t = 96
    A, frames, v = _stepped("ntu", True, t)
    (B, Bt), _ = _make("ntu", (3, 3), True)
    warm = _frames(100 + T_MORE, 3, v, 55)
    for net in (B, Bt):
        _steps(net, warm, 0, 100)
    x = _history(frames, t)
    with pytest.raises(ValueError, match="outside a slab of 3"):
        B.prime_streams_as_steps(x[1:2], [3])
    B.prime_streams_as_steps(x[1:2], [1])
    assert B.stream_ages().tolist() == [100, t, 100] and B._counters() == Bt._counters() and B.streams_ready().tolist() == [True] * 3
    compared = 0
    with _restored(A):
        for s in range(0, T_MORE, 4):
            cyc_a = [frames[t + s + f] for f in range(4)]
            cyc_bt = [warm[100 + s + f] for f in range(4)]
            cyc_b = []
            for xa, xb in zip(cyc_a, cyc_bt):
                y = xb.clone()
                y[1] = xa[1]
                cyc_b.append(y)
            la, lb, lbt = A._cycle(cyc_a)[2], B._cycle(cyc_b)[2], Bt._cycle(cyc_bt)[2]
            assert len(la) == len(lb) == len(lbt) == 1
            assert torch.equal(lb[0][[0, 2]], lbt[0][[0, 2]]), (s, "the neighbours of the primed stream")
            compared += 1
            assert torch.allclose(lb[0][1], la[0][1], rtol=1e-4, atol=1e-5), (s, float((lb[0][1] - la[0][1]).abs().max()))
            assert not torch.equal(lb[0][1], lbt[0][1])                            # ... and it is the primed stream that answers
    assert compared == 4


def test_the_record_does_not_depend_on_the_framewise_route_or_the_chunking():
    """The fused frame-wise kernel wherever it is built, the composed launches everywhere, adjacency chunks of one frame, and
    one stream per prime chunk: the same bits as the default routing."""
    A, frames, v = _stepped("ntu", False, 96)
    x = _history(frames, 96)[:2]
    want = A.prime_state_as_steps(x).packed.view(torch.int32)
    saved = (AGC.framewise_everywhere, AGC.fuse_framewise, AGC.framewise_budget_bytes)
    try:
        AGC.framewise_everywhere = True
        assert torch.equal(A.prime_state_as_steps(x).packed.view(torch.int32), want), "framewise_everywhere"
        AGC.framewise_everywhere, AGC.fuse_framewise = False, False
        assert torch.equal(A.prime_state_as_steps(x).packed.view(torch.int32), want), "fuse_framewise = False"
        AGC.framewise_budget_bytes = 1 << 20                                       # a few frames of adjacencies per chunk
        (fresh,), _ = _make("ntu", (1,))
        fresh.prime_budget_bytes = 1                                               # one stream per chunk
        assert fresh._n is None
        assert torch.equal(fresh.prime_state_as_steps(x).packed.view(torch.int32), want), "chunks"
        assert fresh._n is None
    finally:
        AGC.framewise_everywhere, AGC.fuse_framewise, AGC.framewise_budget_bytes = saved


def test_stream_shards_prime_streams_as_steps_equals_the_unsharded_slab():
    """2 shards x 2 streams against one slab of 4: global streams 2 (shard 1) and 1 (shard 0) are primed from the same
    histories; every prediction of the next 8 frames is bit for bit the unsharded slab's."""
    A, frames, v = _stepped("ntu", False, 96)
    nets, _ = _make("ntu", (2, 2, 4))
    pool = nets[:2]
    shards = pkg.parallel.StreamShards(lambda: pool.pop(0), 4, 2, torch.device(DEV))
    whole = nets[2]
    warm = _frames(100 + 8, 4, v, 57)
    for t in range(0, 100, 4):
        cyc = [warm[t + f] for f in range(4)]
        shards.forward_cycle(cyc)
        whole.forward_cycle(cyc)
    x = _history(frames, 96)
    with pytest.raises(NotImplementedError, match="one\\s+adjacency over all T frames"):
        shards.prime_streams(x[:2], [2, 1])
    with pytest.raises(ValueError, match="not a multiple of the total stride"):
        shards.prime_streams_as_steps(x[:2, :, :94].contiguous(), [2, 1])
    shards.prime_streams_as_steps(x[:2], [2, 1])
    whole.prime_streams_as_steps(x[:2], [2, 1])
    assert shards.stream_ages().tolist() == whole.stream_ages().tolist() == [100, 96, 96, 100]
    for t in range(100, 108, 4):
        cyc = [warm[t + f] for f in range(4)]
        got, want = shards.forward_cycle(cyc), whole.forward_cycle(cyc)[-1]
        assert torch.equal(got, want), t
