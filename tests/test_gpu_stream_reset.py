"""Per-stream reset of the continual slab (CoStGcn.reset_streams, csk_co_scrub_streams_f32).

The yardstick is a FRESH model: a stream that is reset while its neighbours run on must, from the fresh model's first
emission on, give layer-10 features and logits that are ``torch.equal`` to those of a fresh model fed the stream's frames
since the reset.  Bitwise is the derived expectation: the project holds stream-position invariance bitwise, the head sums
its window oldest-first in one chain (leading zeros are exact, the features are non-negative), and after the per-cycle
scrub the stream's rings hold what a fresh model's hold."""
import pytest
import torch

import _bootstrap
from tests.helpers import randomise_unit_

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native = pkg.native
DEV = "cuda:0"
N = 5


# ---- the kernel alone ------------------------------------------------------------------------------------------------
def _scrub(jobs, streams, n_total):
    idx = torch.tensor(streams, dtype=torch.int32, device=DEV)
    arr = (native.ScrubJob * len(jobs))(*jobs)
    import ctypes
    native.check(native.lib().csk_co_scrub_streams_f32(ctypes.byref(arr), len(jobs), native.ptr(idx), len(streams), n_total,
                                                       native.stream_of(idx)), "csk_co_scrub_streams_f32")
    torch.cuda.synchronize()


def _pattern(shape, lead=0):
    """Non-zero everywhere; ``lead`` floats in front put the ring's base on a 4-byte boundary only."""
    numel = shape[0] * shape[1] * shape[2]
    buf = (torch.arange(numel + lead, dtype=torch.float32) % 8191.0 + 1.0).to(DEV)
    return buf, buf[lead:].view(shape)


STREAM_SETS = ([0], [1, 3], [4], [0, 1, 2, 3, 4], [3, 0])


def _block_ring_cases():
    """(depth, rows, mv, lead): the segment lengths of the models at 0 / 4 bytes of lead over three row counts, then -- over
    rows 3 and 65 -- what they leave out of mv in (50, 36, 25, 2, 1) x lead in (0, 1, 2, 3): the segments shorter than their
    own head (mv = 2, 1) and the other two base alignments."""
    cases = [(depth, rows, mv, lead) for lead in (0, 1) for mv in (50, 36, 25) for rows in (3, 64, 65) for depth in (12, 5)]
    return cases + [(depth, rows, mv, lead) for lead in (0, 1, 2, 3) for mv in (50, 36, 25, 2, 1) for rows in (3, 65) for depth in (12, 5)
                    if (depth, rows, mv, lead) not in cases]


@pytest.mark.parametrize("depth,rows,mv,lead", _block_ring_cases())
def test_scrub_kernel_block_ring_writes_the_named_segments_only(depth, rows, mv, lead):
    """Ring [depth][rows][P], P = N * mv rounded up to 4 (NTU 250 -> 252 and M = 1 125 -> 128 leave a padding tail): segment
    starts 8-byte aligned for odd streams at mv = 50, 16-byte at 36, 4-byte at 25, and at mv = 2 and 1 a segment can be shorter
    than the floats in front of its first 16-byte boundary -- and everything 4, 8 or 12 bytes further with ``lead``; slot runs
    that wrap, a single slot, the whole ring, an empty run.  The result equals the CPU-built expectation bit for bit, so every
    float outside the named segments (neighbours, padding, other slots, the lead) is unchanged."""
    p = (N * mv + 3) // 4 * 4
    for streams in STREAM_SETS:
        for slot0, n_slots in ((depth - 2, 4), (3, 1), (0, depth), (depth - 1, depth), (1, 0)):
            buf, ring = _pattern((depth, rows, p), lead)
            want = buf.cpu().clone()
            w = want[lead:].view(depth, rows, p)
            for j in range(n_slots):
                for n in streams:
                    w[(slot0 + j) % depth, :, n * mv:(n + 1) * mv] = 0.0
            _scrub([native.ScrubJob(ring.data_ptr(), p, depth, rows, slot0, n_slots, mv, native.SCRUB_BLOCK_RING)], streams, N)
            assert torch.equal(buf.cpu(), want), (streams, slot0, n_slots)


@pytest.mark.parametrize("c", [256, 70, 3])
@pytest.mark.parametrize("depth", [12, 5, 3])
def test_scrub_kernel_pool_ring_and_a_table_of_jobs(depth, c):
    """Pooling ring [depth][N][C]: stream n is row n.  One launch with a table of three jobs -- the pooling ring and two block
    rings of different shape and slot run -- equals the CPU-built expectation for all three."""
    for streams in STREAM_SETS:
        for slot0, n_slots in ((depth - 2, 3), (0, depth), (depth - 1, 1)):
            pbuf, pool = _pattern((depth, N, c))
            b1, r1 = _pattern((12, 64, 252))
            b2, r2 = _pattern((5, 65, 128), lead=1)
            wp, w1, w2 = pbuf.cpu().clone().view(depth, N, c), b1.cpu().clone().view(12, 64, 252), b2.cpu().clone()
            w2v = w2[1:].view(5, 65, 128)
            for n in streams:
                for j in range(n_slots):
                    wp[(slot0 + j) % depth, n] = 0.0
                for j in range(4):
                    w1[(10 + j) % 12, :, n * 50:(n + 1) * 50] = 0.0
                w2v[4, :, n * 25:(n + 1) * 25] = 0.0
            _scrub([native.ScrubJob(r1.data_ptr(), 252, 12, 64, 10, 4, 50, native.SCRUB_BLOCK_RING),
                    native.ScrubJob(pool.data_ptr(), c, depth, N, slot0, n_slots, c, native.SCRUB_POOL_RING),
                    native.ScrubJob(r2.data_ptr(), 128, 5, 65, 4, 1, 25, native.SCRUB_BLOCK_RING)], streams, N)
            assert torch.equal(pool.cpu(), wp) and torch.equal(r1.cpu(), w1) and torch.equal(b2.cpu(), w2), (streams, slot0)


def test_scrub_kernel_ignores_an_index_outside_the_slab():
    """The indices live on the device, so the host cannot see them: one outside [0, n_total) writes nothing."""
    buf, ring = _pattern((5, 3, 128))
    want = buf.cpu().clone().view(5, 3, 128)
    want[:, :, 50:75] = 0.0
    _scrub([native.ScrubJob(ring.data_ptr(), 128, 5, 3, 0, 5, 25, native.SCRUB_BLOCK_RING)], [5, 2, -1], N)
    assert torch.equal(ring.cpu(), want)


# ---- fresh-model equivalence -------------------------------------------------------------------------------------------
def _graph(name):
    return (pkg.ntu_graph() if name == "ntu" else pkg.kinetics_graph()).A


def _make(model, graph, native_plan, n_copies, seed=7):
    """``n_copies`` models with the same randomised weights (BN statistics, graph attention, every conv) on the device."""
    a = _graph(graph)
    v = a.shape[-1]
    cls = {"stgcn": pkg.CoStGcn, "agcn": pkg.CoAGcn, "str": pkg.CoSTr}[model]
    nets = [cls(a, (3, 300, v, 2), 60, pool_size=3, pool_padding=1).eval() for _ in range(n_copies)]
    randomise_unit_(nets[0], seed, attn_scale=1 / v if model == "agcn" else 1.0)
    for net in nets[1:]:
        net.load_state_dict(nets[0].state_dict())
    for net in nets:
        net.use_native_plan = native_plan
    return [net.to(DEV) for net in nets], v


def _feat(net, slot, j, stream, mv):
    out = net.layers["layer10"]._state.out
    return out[(slot + j) % out.shape[0], :, stream * mv:(stream + 1) * mv]


T_RESET, T_AGAIN, T_END = 80, 120, 228      # reset {1, 4} at 80; reset 4 again at 120 (stream 1 is 40 frames old: two cohorts)


def _run(model, graph, native_plan, r, scrub=True):
    """Slab of 5 streams with the resets, the same slab without any reset, a fresh 2-stream model on streams {1, 4} from frame
    80 on and a fresh 1-stream model on stream 4 from frame 120 on, all stepped in cycles of ``r`` frames.  Returns the
    number of (features or logits) comparisons of reset streams against their fresh models and how many of them failed;
    everything else is asserted on the way."""
    (slab, plain, fresh_a, fresh_b), v = _make(model, graph, native_plan, 4)
    slab._scrub_warming = scrub
    mv = 2 * v
    frames = torch.rand((T_END, N, 3, v, 2), generator=torch.Generator().manual_seed(21)).to(DEV)
    answered = {"a": False, "b": False}
    compared = failed = 0
    for t in range(0, T_END, r):
        if t == T_RESET:
            slab.reset_streams([1, 4])
            assert slab.stream_ages().tolist() == [80, 0, 80, 80, 0]
        if t == T_AGAIN:
            slab.reset_streams((4,))
            assert slab.stream_ages().tolist() == [120, 40, 120, 120, 0] and sorted(slab._cohorts) == [80, 120]
        cyc = [frames[t + f] for f in range(r)]
        slot, nf, logits = slab._cycle(cyc)
        pslot, pnf, plogits = plain._cycle(cyc)
        # the streams nobody touched: the slab without any reset, on every step
        assert nf == pnf and len(logits) == len(plogits)
        for s in (0, 2, 3):
            assert all(torch.equal(_feat(slab, slot, j, s, mv), _feat(plain, pslot, j, s, mv)) for j in range(nf)), (t, s)
            assert all(torch.equal(a[s], b[s]) for a, b in zip(logits, plogits)), (t, s)
        # the reset streams: their fresh models, from the fresh model's first emission on
        pairs = []
        if t >= T_RESET:
            pairs.append(("a", fresh_a, [1, 4] if t < T_AGAIN else [1], [0, 1] if t < T_AGAIN else [0], [frames[t + f][[1, 4]] for f in range(r)]))
        if t >= T_AGAIN:
            pairs.append(("b", fresh_b, [4], [0], [frames[t + f][[4]] for f in range(r)]))
        for tag, fresh, streams, rows, fcyc in pairs:
            fslot, fnf, flogits = fresh._cycle([f.contiguous() for f in fcyc])
            if fnf:
                assert nf == fnf, (t, tag)
                for s, row in zip(streams, rows):
                    for j in range(fnf):
                        compared += 1
                        failed += not torch.equal(_feat(slab, slot, j, s, mv), _feat(fresh, fslot, j, row, mv))
            if flogits:
                assert len(logits) == len(flogits), (t, tag)
                for s, row in zip(streams, rows):
                    for a, b in zip(logits, flogits):
                        compared += 1
                        failed += not torch.equal(a[s], b[row])
            answered[tag] = answered[tag] or bool(flogits)
        # ready exactly from the step on which the fresh model first answers; the never-reset streams as a fresh slab would be
        ready = slab.streams_ready().tolist()
        assert ready[0] == ready[2] == ready[3] == (t + r > 80), t
        if t >= T_RESET:
            assert ready[1] == answered["a"], t
            assert ready[4] == (answered["a"] if t < T_AGAIN else answered["b"]), t
    assert answered["a"] and answered["b"] and not slab._warming() and slab.streams_ready().all()
    assert (slab.__dict__.get("_plan") is not None) == (native_plan and model != "str")
    return compared, failed


@pytest.mark.parametrize("graph", ["ntu", "kinetics"])
@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("native_plan", [True, False])
def test_reset_streams_equal_a_fresh_model_bitwise(native_plan, r, graph):
    """CoStGcn, every combination of {native plan, Python engine} x {per frame, aligned 4-frame cycles} x {NTU, Kinetics
    graph} (none omitted): 80 frames, reset {1, 4}, 40 frames, reset 4 again while stream 1 still warms (two cohorts of
    different age), on to frame 228.  Reset streams == their fresh models (features and logits, torch.equal) from the fresh
    model's first emission on; ``streams_ready()`` flips with the fresh model's first answer; streams {0, 2, 3} == the slab
    that was never reset, on every step."""
    compared, failed = _run("stgcn", graph, native_plan, r)
    assert compared >= 50 and failed == 0, (compared, failed)


@pytest.mark.parametrize("model,native_plan,r", [("agcn", True, 1), ("str", False, 4)])
def test_reset_streams_of_the_sibling_models_equal_their_own_fresh_models(model, native_plan, r):
    """CoAGcn (native plan with the adaptive graph conv, per frame) and CoSTr (Python engine, 4-frame cycles) inherit the
    reset: same protocol, each stream against a fresh model of its own kind."""
    compared, failed = _run(model, "ntu", native_plan, r)
    assert compared >= 50 and failed == 0, (compared, failed)


def test_zeroing_alone_does_not_give_a_fresh_model():
    """The same run with the per-cycle scrub switched off (the naive reset: zero the stream's slices once): the reset
    streams then DIFFER from their fresh models -- the blocks below a filling window were fed ReLU(bias + partial window)
    -- while every assertion about the untouched streams and the ages still holds.  The scrub, not the zeroing, carries the
    equivalence."""
    compared, failed = _run("stgcn", "ntu", True, 4, scrub=False)
    assert compared >= 50 and failed > 0, (compared, failed)


# ---- rules that need a device slab --------------------------------------------------------------------------------------
def _stepped(native_plan, frames, n=N, t_end=80):
    (net,), v = _make("stgcn", "ntu", native_plan, 1)
    for t in range(0, t_end, 4):
        net.forward_cycle([frames[t + f][:n] for f in range(4)])
    return net


@pytest.mark.parametrize("native_plan", [True, False])
def test_cycle_rules_while_a_stream_warms(native_plan):
    """While a reset stream warms: 8-frame and misaligned cycles and ``pad_end`` raise before any launch (the counters and every
    state tensor are untouched); aligned 1-, 2- and 4-frame cycles run; a reset off the stride grid raises; once every stream
    is ready any cycle runs again; ``clean_state()`` clears ages and cohorts."""
    frames = torch.rand((200, N, 3, 25, 2), generator=torch.Generator().manual_seed(3)).to(DEV)
    net = _stepped(native_plan, frames)
    net.reset_streams([2])
    before, keep = net._counters(), [t.clone() for t in net._state_tensors()]
    with pytest.raises(ValueError, match="crosses a multiple of 4"):
        net.forward_cycle([frames[80 + f] for f in range(8)])
    with pytest.raises(ValueError, match="crosses a multiple of 4"):
        net.forward_cycle([frames[80 + f] for f in range(5)])
    with pytest.raises(RuntimeError, match="pad_end"):
        net.forward_steps(frames[80:84].permute(1, 2, 0, 3, 4).contiguous(), pad_end=True)
    with pytest.raises(RuntimeError, match="pad_end"):
        net.forward_steps(frames[80:84].permute(1, 2, 0, 3, 4).contiguous(), pad_end=True, update_state=False)
    assert net._counters() == before and all(torch.equal(a, b) for a, b in zip(net._state_tensors(), keep))
    net.forward_cycle([frames[80]])                                   # frame 81: phase 1
    with pytest.raises(RuntimeError, match="multiple of 4"):
        net.reset_streams([3])
    with pytest.raises(ValueError, match="crosses a multiple of 4"):
        net.forward_cycle([frames[81 + f] for f in range(4)])         # a misaligned 4-frame cycle
    net.forward_cycle([frames[81], frames[82]])
    net.forward_cycle([frames[83]])
    net.forward_cycle([frames[84], frames[85]])
    net.forward_cycle([frames[86], frames[87]])
    assert net.stream_ages().tolist() == [88, 88, 8, 88, 88] and net._counters()[0] == 88
    for t in range(88, 164, 4):
        net.forward_cycle([frames[t + f] for f in range(4)])
    assert net.streams_ready().all() and not net._warming()
    assert len(net.forward_cycle([frames[164 + f] for f in range(8)])) == 2       # nothing warms: an 8-frame cycle again
    net.reset_streams(range(N))
    assert net.stream_ages().tolist() == [0] * N and net._warming()
    net.clean_state()
    assert net.stream_ages().tolist() == [0] * N and not net._warming() and net._counters() == [0] * 22
    net.forward_cycle([frames[f] for f in range(8)])                  # a clean slab takes any cycle


@pytest.mark.parametrize("native_plan", [True, False])
def test_peeks_leave_ages_and_later_results_unchanged(native_plan):
    """update_state=False while a stream warms: the single-step peek neither scrubs nor ages, the multi-frame peek restores
    ages and cohorts with the slab; a model that was peeked at goes on bit for bit like a twin that was not."""
    frames = torch.rand((180, N, 3, 25, 2), generator=torch.Generator().manual_seed(4)).to(DEV)
    peeker, twin = _stepped(native_plan, frames), _stepped(native_plan, frames)
    for net in (peeker, twin):
        net.reset_streams([0, 3])
    n_pred = 0
    for t in range(80, 180):
        f = frames[t]
        if t in (80, 83, 100, 159, 160, 161):
            ages, cohorts = peeker.stream_ages().tolist(), {k: list(v[0]) for k, v in peeker._cohorts.items()}
            p1 = peeker.forward_step(f, update_state=False)
            if t in (100, 160):                                        # a look-ahead across the moment the streams get ready
                ahead = peeker.forward_steps(frames[t:t + 12].permute(1, 2, 0, 3, 4).contiguous(), update_state=False)
                assert ahead.shape[2] == 3
            assert peeker.stream_ages().tolist() == ages and {k: list(v[0]) for k, v in peeker._cohorts.items()} == cohorts
        got, want = peeker.forward_step(f), twin.forward_step(f)
        assert (got is None) == (want is None)
        if want is not None:
            assert torch.equal(got, want), t
            n_pred += 1
            if t in (100, 160):
                assert torch.equal(p1, want), t
    assert n_pred == 25 and peeker._counters() == twin._counters()
    assert all(torch.equal(a, b) for a, b in zip(peeker._state_tensors(), twin._state_tensors()))
    assert peeker.streams_ready().all() and not peeker._warming() and not twin._warming()


def test_stream_shards_reset_equals_the_unsharded_slab():
    """Two shards of a 6-stream slab, global streams {2, 3} reset (one per shard): predictions and readiness equal the
    unsharded slab's, bit for bit."""
    def make():
        return _make("stgcn", "ntu", True, 1)[0][0]
    from continual_skeletons_amd import parallel
    eng = parallel.StreamShards(make, 6, 2, torch.device(DEV))
    whole = make()
    frames = torch.rand((176, 6, 3, 25, 2), generator=torch.Generator().manual_seed(5)).to(DEV)
    with pytest.raises(RuntimeError, match="no state slab is bound"):
        eng.reset_streams([2, 3])
    n_pred = 0
    for t in range(0, 176, 4):
        if t == 84:
            for bad in ([2, 2], [6], torch.tensor([2])):
                with pytest.raises(ValueError):
                    eng.reset_streams(bad)
            eng.reset_streams([2, 3])
            whole.reset_streams([2, 3])
        cyc = [frames[t + f] for f in range(4)]
        got, want = eng.forward_cycle(cyc), whole.forward_cycle(cyc)
        assert (got is None) == (not want)
        if want:
            torch.cuda.synchronize()
            assert torch.equal(got, want[-1]), t
            n_pred += 1
        assert torch.equal(eng.streams_ready(), whole.streams_ready()) and torch.equal(eng.stream_ages(), whole.stream_ages()), t
        if t == 84:
            assert eng.stream_ages().tolist() == [88, 88, 4, 4, 88, 88]
    assert n_pred >= 20 and eng.streams_ready().all()
