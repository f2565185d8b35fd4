"""csk_co_head_clip_f32 (csrc/head.hip) alone: the continual head over a clip tensor in one call, BIT FOR BIT
against the composition of the entries it replaces -- the CSK_PRIME_POOL job of csk_co_prime_pack_f32 (the head step's pool on
the clip layout), csk_co_window_mean_f32 once per prediction on an array of entries with a zero tail, csk_fc_f32 on all
predictions -- never against itself.  One integer-valued case is held against an fp64 reference by equality."""
import ctypes

import pytest
import torch

import _bootstrap

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native = pkg.native
DEV = "cuda:0"
GROUP = 16                              # predictions of one workgroup at C <= 512 (CLIP_G of csrc/head.hip)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _composed(h, frames, window, first_entry, n_pred, w, b, n, m, c, v, classes):
    """(pooled [n_pred][n][c], logits [n_pred][n][classes]) by the existing entries."""
    lib, stream = native.lib(), native.stream_of(h)
    total = first_entry + n_pred
    ring = torch.zeros((total + window, n, c), device=DEV)                      # entries >= frames: +0.0, the window's end padding
    if frames:
        packed = torch.empty((n, frames * c), device=DEV)
        job = (native.PrimeJob * 1)(native.PrimeJob(h.data_ptr(), 0, native.PRIME_POOL, c, h.shape[2], 0, frames, 0))
        native.check(lib.csk_co_prime_pack_f32(ctypes.byref(job), 1, native.ptr(packed), frames * c, n, m, v, stream), "pack")
        ring[:frames] = packed.view(n, frames, c).permute(1, 0, 2)
    pooled = torch.empty((n_pred, n, c), device=DEV)
    for k in range(n_pred):
        e = first_entry + k
        lo = max(0, e + 1 - window)
        native.check(lib.csk_co_window_mean_f32(native.ptr(ring[lo]), native.ptr(pooled[k]), n * c, window, e - lo, e - lo + 1, stream), "mean")
    logits = torch.empty((n_pred, n, classes), device=DEV)
    native.check(lib.csk_fc_f32(native.ptr(pooled), native.ptr(w), native.ptr(b), native.ptr(logits), n_pred * n, c, classes, stream), "fc")
    return pooled, logits


def _one_call(h, frames, window, first_entry, n_pred, w, b, n, m, c, v, classes):
    """The entry under test, its three buffers between NaN guard rows: (pooled, logits) and the whole guarded buffers."""
    bufs = [torch.full((rows + 2, n, width), float("nan"), device=DEV) for rows, width in ((frames, c), (n_pred, c), (n_pred, classes))]
    entries, pooled, logits = (buf[1: buf.shape[0] - 1] for buf in bufs)
    rc = native.lib().csk_co_head_clip_f32(native.ptr(h), h.shape[2], frames, native.ptr(entries) if frames else None, window, first_entry,
                                           n_pred, native.ptr(w), native.ptr(b), native.ptr(pooled), native.ptr(logits), n, m, c, v,
                                           classes, native.stream_of(h))
    native.check(rc, "csk_co_head_clip_f32")
    torch.cuda.synchronize()
    for buf in bufs:                                                              # the guard rows are untouched
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())
    return pooled, logits


def _data(n, m, c, v, classes, frames, t_src, seed):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn((n * m, c, t_src, v), generator=g) * 3.0 + 0.5
    h[:, :, frames:] = float("nan")                                             # the frames behind the real ones are never read
    w, b = torch.randn((classes, c), generator=g), torch.randn((classes,), generator=g)
    return h.to(DEV), w.to(DEV), b.to(DEV)


def _kinds(frames, window, first_entry, n_pred):
    """Which kinds of window the predictions hold."""
    kinds = set()
    for e in range(first_entry, first_entry + n_pred):
        lo = max(0, e + 1 - window)
        if e + 1 < window:
            kinds.add("partial")
        elif lo >= frames:
            kinds.add("zero tail")
        elif e >= frames:
            kinds.add("sliding out")
        else:
            kinds.add("full")
    return kinds


SHAPES = [(25, 2, 256, 60), (18, 2, 256, 400), (25, 1, 3, 5), (18, 2, 64, 7)]


@pytest.mark.parametrize("window", [1, 4, 7])
@pytest.mark.parametrize("frames", [0, 1, 5])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("v,m,c,classes", SHAPES)
def test_one_call_equals_the_composed_entries_bit_for_bit(v, m, c, classes, n, frames, window):
    """Real-valued data.  From entry 0: partly filled windows (window > 1), full ones, windows sliding from the real entries
    into the zero tail, and windows wholly in it; from entry 2 the same range entered mid-way.  The two frames behind ``frames``
    hold NaN and every output is finite; the guard rows around entries, pooled and logits stay NaN."""
    h, w, b = _data(n, m, c, v, classes, frames, frames + 2, 1000 * v + 10 * c + frames + window)
    for first_entry, n_pred in ((0, frames + window + 2), (2, frames + window)):
        kinds = _kinds(frames, window, first_entry, n_pred)
        if first_entry == 0:
            assert kinds >= {"zero tail"} | ({"partial"} if window > 1 else set()) | ({"sliding out"} if frames and window > 1 else set())
            assert "full" in kinds or frames < window
        want = _composed(h, frames, window, first_entry, n_pred, w, b, n, m, c, v, classes)
        got = _one_call(h, frames, window, first_entry, n_pred, w, b, n, m, c, v, classes)
        for a, r, name in zip(got, want, ("pooled", "logits")):
            assert bool(torch.isfinite(a).all()), name
            assert torch.equal(_bits(a), _bits(r)), (name, first_entry, float((a - r).abs().max()))


@pytest.mark.parametrize("v,m,c,classes,frames,window,first_entry,n_pred", [
    (25, 2, 256, 60, 5, 7, 3, 2 * GROUP + 5),        # three groups, the last of 5 predictions
    (18, 2, 64, 7, 5, 4, 0, 3 * GROUP + 1),          # four groups, the last of one
    (25, 2, 256, 60, 80, 75, 70, GROUP + 3),         # the union of a group's windows in 64-channel slices (90 entries x 256 > 32 KB)
    (18, 2, 256, 400, 40, 150, 0, 41),               # ... in slices of 49 channels, the last one ragged; partly filled windows only
    (25, 1, 3, 5, 9, 4, 1, 2 * GROUP + 2),           # more than one group of frames in the pool pass (8 per wave), C off the multiple of 4
], ids=["three-groups", "four-groups", "slices-64", "slices-49", "c3"])
def test_groups_of_predictions_and_channel_slices(v, m, c, classes, frames, window, first_entry, n_pred):
    """Prediction counts that are no multiple of the group of 16 and span three groups and more; windows so long that a
    workgroup stages its entries slice by slice."""
    n = 3
    h, w, b = _data(n, m, c, v, classes, frames, frames + 2, 77 * v + c + window)
    want = _composed(h, frames, window, first_entry, n_pred, w, b, n, m, c, v, classes)
    got = _one_call(h, frames, window, first_entry, n_pred, w, b, n, m, c, v, classes)
    for a, r, name in zip(got, want, ("pooled", "logits")):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(_bits(a), _bits(r)), (name, float((a - r).abs().max()))


def test_integer_valued_case_equals_the_fp64_reference():
    """Features that are multiples of M V, integer weights, a window of 4: every partial sum is exact in fp32, so the fp64
    reference is matched by equality -- the semantics themselves, not an order."""
    v, m, c, classes, n, frames, window, first_entry, n_pred = 25, 2, 256, 60, 3, 5, 4, 1, 10
    g = torch.Generator().manual_seed(5)
    h = (torch.randint(-8, 9, (n * m, c, frames + 2, v), generator=g) * (m * v)).float()
    w, b = torch.randint(-4, 5, (classes, c), generator=g).float(), torch.randint(-9, 10, (classes,), generator=g).float()
    pooled, logits = _one_call(h.to(DEV), frames, window, first_entry, n_pred, w.to(DEV), b.to(DEV), n, m, c, v, classes)
    ent = torch.zeros((first_entry + n_pred, n, c), dtype=torch.float64)
    ent[:frames] = h[:, :, :frames].double().view(n, m, c, frames, v).mean(dim=(1, 4)).permute(2, 0, 1)
    for k in range(n_pred):
        e = first_entry + k
        want = ent[max(0, e + 1 - window): e + 1].sum(0) / window
        assert torch.equal(pooled[k].cpu().double(), want), k
        assert torch.equal(logits[k].cpu().double(), want @ w.double().t() + b.double()), k
    assert bool((pooled[:3] != 0).any()) and not bool(pooled[frames + window - 1 - first_entry:].any())


def test_a_nan_reaches_exactly_the_windows_that_hold_its_entry():
    """A NaN in channel 1 of feature frame 2 of stream 1: pooled[k][1][1] and all logits of (k, stream 1) are NaN for exactly the
    predictions whose windows hold entry 2; every other value is finite and bit for bit the clean run's."""
    v, m, c, classes, n, frames, window, first_entry, n_pred, bad = 18, 2, 64, 7, 3, 5, 4, 0, 12, 2
    h, w, b = _data(n, m, c, v, classes, frames, frames + 2, 9)
    clean = _one_call(h, frames, window, first_entry, n_pred, w, b, n, m, c, v, classes)
    h[1 * m + 1, 1, bad, 3] = float("nan")
    pooled, logits = _one_call(h, frames, window, first_entry, n_pred, w, b, n, m, c, v, classes)
    holds = torch.tensor([max(0, first_entry + k + 1 - window) <= bad <= first_entry + k for k in range(n_pred)])
    assert holds.tolist() == [False, False] + [True] * 4 + [False] * 6
    want_p = torch.zeros((n_pred, n, c), dtype=torch.bool)
    want_p[holds, 1, 1] = True
    want_l = torch.zeros((n_pred, n, classes), dtype=torch.bool)
    want_l[holds, 1] = True
    for got, ref, want in ((pooled, clean[0], want_p), (logits, clean[1], want_l)):
        nan = torch.isnan(got).cpu()
        assert torch.equal(nan, want)
        assert torch.equal(_bits(got).cpu()[~want], _bits(ref).cpu()[~want])
