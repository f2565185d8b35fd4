"""Parity at BASELINE.json's full sizes (configs[1] and configs[2]) on the GPU.

The oracle is too slow for 256 clips / 1024 streams, so it checks a slice, and the rest is covered by a
size-independent property of the path: every clip / stream is independent of its batch neighbours (eval-mode BN,
no cross-sample op), hence row i of the full-size result must equal -- bit for bit -- the same clip run
in a small batch."""
import pytest
import torch

import _bootstrap
from oracle import stgcn_oracle as o
from tests import str_oracle as so
from tests.helpers import check_parity, g6_state_dict, model_fixture, randomise_unit_

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
DEV = "cuda:0"
A = pkg.ntu_graph().A
TOL = 1e-4


def test_config2_batch256_clip_forward():
    """Full 10-block ST-GCN clip forward, batch 256, NTU-60 shape: logits of a 32-clip slice vs the oracle,
    and batch invariance over all 256 clips."""
    a, sd, _ = g6_state_dict("ntu")
    net = pkg.StGcn(A).eval()
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV)
    x = torch.rand((256, 3, 300, 25, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    full = net(x)
    assert full.shape == (256, 60) and bool(torch.isfinite(full).all())
    idx = [0, 1, 254, 255] + list(range(5, 256, 9))[:28]          # 32 clips spread over the batch, both ends included
    assert len(idx) == 32 == len(set(idx))
    with torch.no_grad():
        want = o.stgcn_forward(x[idx].cpu(), sd)
    check_parity(full[idx].cpu(), want)
    for lo in range(0, 256, 64):                                  # batch invariance, bitwise
        part = net(x[lo:lo + 64].contiguous())
        assert torch.equal(part, full[lo:lo + 64])


def test_config3_1024_streams_online():
    """CoST-GCN online inference with 1024 concurrent streams: predictions of 8 streams vs the oracle stepping
    those streams alone; stream invariance (bitwise) between the 1024-stream slab and a 4-stream slab; and
    the 4-frame cycle launches vs per-frame stepping."""
    a, sd, _ = g6_state_dict("ntu")
    T = 76 + 4 * 4 + 1
    g = torch.Generator(device=DEV).manual_seed(2)
    frames = torch.rand((T, 1024, 3, 25, 2), device=DEV, generator=g)
    big = pkg.CoStGcn(A, pool_size=3, pool_padding=1).eval()
    big.load_state_dict(sd, strict=True)
    big = big.to(DEV)
    got = []
    t = 0
    while t < T:
        r = min(4, T - t)
        got += big.forward_cycle([frames[t + f] for f in range(r)])
        t += r
    assert len(got) >= 3 and all(gv.shape == (1024, 60) for gv in got)
    pick = [0, 5, 255, 256, 511, 777, 1000, 1023]             # both stream shards' ends and interiors
    orc = o.CoStGcnOracle(sd, pool_size=3, pool_padding=1)
    want = []
    with torch.no_grad():
        for t in range(T):
            r = orc.forward_step(frames[t][pick].cpu())
            if r is not None:
                want.append(r)
    assert len(want) == len(got)
    for gv, wv in zip(got, want):
        check_parity(gv[pick].cpu(), wv)
    small = pkg.CoStGcn(A, pool_size=3, pool_padding=1).eval()
    small.load_state_dict(sd, strict=True)
    small = small.to(DEV)
    sel = [5, 6, 999, 1000]
    got_small = [r for r in (small.forward_step(frames[t][sel].contiguous()) for t in range(T)) if r is not None]
    for gv, sv in zip(got, got_small):
        assert torch.equal(gv[sel], sv)
    # per-layer ring depths (8 + max_in post-GCN slots, 4 + max_in history slots): ~5.7 GB for 1024 streams (16-slot rings
    # everywhere were 9.3 GB; SURVEY 8a's per-frame minimum is 3.25 GB)
    assert 5.0 < big.state_bytes() / 1e9 < 6.5


def _randomise_agcn(m, seed):
    randomise_unit_(m, seed, attn_scale=1 / 18)        # O(1) activations through all ten blocks, non-uniform attention


def test_config4_agcn_clip_batch64_kinetics_shape():
    """BASELINE configs[3], clip form: A-GCN (per-sample adaptive adjacency), Kinetics-400 shape (V = 18, T = 300),
    batch 64: logits of an 8-clip slice vs the oracle; the attention is per sample, so rows of the full batch must
    equal -- bit for bit -- the same clips run in batches of 16."""
    Ak = pkg.kinetics_graph().A
    net = pkg.AGcn(Ak, input_shape=(3, 300, 18, 2), num_classes=400).eval()
    _randomise_agcn(net, 21)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net = net.to(DEV)
    x = torch.rand((64, 3, 300, 18, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    full = net(x)
    assert full.shape == (64, 400) and bool(torch.isfinite(full).all())
    idx = [0, 9, 17, 31, 32, 47, 55, 63]
    with torch.no_grad():
        want = o.stgcn_forward(x[idx].cpu(), sd, gcn=o.adaptive_graph_conv)
    check_parity(full[idx].cpu(), want)
    for lo in range(0, 64, 16):
        assert torch.equal(net(x[lo:lo + 16].contiguous()), full[lo:lo + 16])


def test_config4_coagcn_1024_streams_kinetics_shape():
    """BASELINE configs[3], online form: CoAGCN (per-frame attention) with 1024 concurrent streams, V = 18:
    predictions of 8 streams vs the oracle stepping them alone, and stream invariance (bitwise) against a
    3-stream slab driven frame by frame (the big slab runs 4-frame launch cycles)."""
    Ak = pkg.kinetics_graph().A
    T = 76 + 4 * 4 + 1

    def make():
        net = pkg.CoAGcn(Ak, input_shape=(3, 300, 18, 2), num_classes=400, pool_size=3, pool_padding=1).eval()
        _randomise_agcn(net, 22)
        return net
    big = make()
    sd = {k.replace("0.1.", "").replace("0.0.residual", "residual"): v.clone() for k, v in big.state_dict().items()}
    big = big.to(DEV)
    frames = torch.rand((T, 1024, 3, 18, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    got, t = [], 0
    while t < T:
        r = min(4, T - t)
        got += big.forward_cycle([frames[t + f] for f in range(r)])
        t += r
    assert len(got) >= 3 and all(gv.shape == (1024, 400) for gv in got)
    pick = [0, 7, 340, 341, 682, 683, 1001, 1023]             # ends and interiors of the three stream shards' ranges
    orc = o.CoStGcnOracle(sd, pool_size=3, pool_padding=1)
    for b in orc.blocks:
        b.gcn = o.adaptive_graph_conv
    want = []
    with torch.no_grad():
        for t in range(T):
            r = orc.forward_step(frames[t][pick].cpu())
            if r is not None:
                want.append(r)
    assert len(want) == len(got)
    for gv, wv in zip(got, want):
        check_parity(gv[pick].cpu(), wv)
    small = make()
    small.load_state_dict(big.state_dict(), strict=True)       # make() draws fresh conv weights
    small = small.to(DEV)
    sel = [7, 8, 1001]
    got_small = [r for r in (small.forward_step(frames[t][sel].contiguous()) for t in range(T)) if r is not None]
    assert len(got_small) == len(got)
    for gv, sv in zip(got, got_small):
        assert torch.equal(gv[sel], sv)


def _default_head_case(make_big, make_small, sd, V, classes, seed, oracle_gcn=None):
    """1024 streams with the model-level DEFAULT head (models/base.py:84-101 -> AvgPool1d(75, stride 1, padding 19) over the
    layer-10 features, what bench.py times): 304 frames = the first prediction (56th feature, frame 296) and one slide of the
    75-entry window; 8 picked streams vs the oracle with the same 75 / 19 window, and stream invariance (bitwise) against a
    4-stream slab stepped frame by frame."""
    T = 304
    frames = torch.rand((T, 1024, 3, V, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    big = make_big().to(DEV)
    assert (big.pool_size, big.pool_padding) == (75, 19)
    got, t = [], 0
    while t < T:
        got += big.forward_cycle([frames[t + f] for f in range(4)])
        t += 4
    assert len(got) == 2 and all(gv.shape == (1024, classes) for gv in got)      # features 56 and 57 of 57
    pick = [0, 3, 255, 256, 511, 640, 1000, 1023]
    orc = o.CoStGcnOracle(sd, pool_size=75, pool_padding=19)
    if oracle_gcn is not None:
        for b in orc.blocks:
            b.gcn = oracle_gcn
    want = []
    with torch.no_grad():
        for t in range(T):
            r = orc.forward_step(frames[t][pick].cpu())
            if r is not None:
                want.append(r)
    assert len(want) == len(got)
    for gv, wv in zip(got, want):
        check_parity(gv[pick].cpu(), wv)
    small = make_small(big).to(DEV)
    sel = [3, 4, 640, 1023]
    got_small = [r for r in (small.forward_step(frames[t][sel].contiguous()) for t in range(T)) if r is not None]
    assert len(got_small) == len(got)
    for gv, sv in zip(got, got_small):
        assert torch.equal(gv[sel], sv)


def test_config3_1024_streams_default_head():
    a, sd, _ = g6_state_dict("ntu")

    def make():
        net = pkg.CoStGcn(A).eval()                 # pool_size / pool_padding left at their defaults
        net.load_state_dict(sd, strict=True)
        return net
    _default_head_case(make, lambda big: make(), sd, 25, 60, 6)


def test_config4_coagcn_1024_streams_default_head():
    Ak = pkg.kinetics_graph().A

    def make():
        net = pkg.CoAGcn(Ak, input_shape=(3, 300, 18, 2), num_classes=400).eval()
        _randomise_agcn(net, 23)
        return net
    big = make()
    sd = {k.replace("0.1.", "").replace("0.0.residual", "residual"): v.clone() for k, v in big.state_dict().items()}

    def make_small(b):
        small = make()
        small.load_state_dict(b.state_dict(), strict=True)       # make() draws fresh conv weights
        return small
    _default_head_case(lambda: big, make_small, sd, 18, 400, 7, oracle_gcn=o.adaptive_graph_conv)


def test_config5_per_gpu_shard_of_1024_clips():
    """BASELINE configs[4] shards 8192 clips over 8 GPUs: one rank's 1024-clip shard in a single forward (3.9 GB
    activations per 64-channel layer) must reproduce, bit for bit, the same clips run 256 at a time, which is what
    makes the all-gathered logits independent of the world size (tests/test_parallel_cpu.py covers the gather)."""
    a, sd, _ = g6_state_dict("ntu")
    net = pkg.StGcn(A).eval()
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV)
    x = torch.rand((1024, 3, 300, 25, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    full = net(x)
    assert full.shape == (1024, 60) and bool(torch.isfinite(full).all())
    for lo in (0, 768):
        assert torch.equal(net(x[lo:lo + 256].contiguous()), full[lo:lo + 256])


def test_str_batch256_clip_forward():
    """S-TR clip forward, batch 256, NTU-60 shape (512 segments x 7500 columns in layer 4, 2.4 GB of unit scratch): logits of a
    32-clip slice vs the oracle with the attention unit as the graph conv of layers 4-10, and batch invariance over all 256 clips."""
    a, sd, _ = model_fixture("g12_str_ntu", 25)
    net = pkg.STr(A).eval()
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV)
    x = torch.rand((256, 3, 300, 25, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))
    full = net(x)
    assert full.shape == (256, 60) and bool(torch.isfinite(full).all())
    idx = [0, 1, 254, 255] + list(range(5, 256, 9))[:28]          # 32 clips spread over the batch, both ends included
    assert len(idx) == 32 == len(set(idx))
    with torch.no_grad():
        want = o.stgcn_forward(x[idx].cpu(), sd, gcn=so.gcn)
    check_parity(full[idx].cpu(), want, note="STr batch 256")
    for lo in range(0, 256, 64):                                  # batch invariance, bitwise
        part = net(x[lo:lo + 64].contiguous())
        assert torch.equal(part, full[lo:lo + 64])


def _costr_1024_streams(v, classes, fixture, seed, pick, sel):
    """CoS-TR online inference with 1024 concurrent streams in 4-frame cycles: predictions of 8 streams vs the oracle stepping
    those streams alone (CoStGcnOracle with the attention unit as every block's graph conv), and stream invariance (bitwise)
    against a 4-stream model stepped frame by frame."""
    graph = A if v == 25 else pkg.kinetics_graph().A
    a, sd, _ = model_fixture(fixture, v)
    T = 76 + 4 * 4 + 1

    def make():
        net = pkg.CoSTr(graph, (3, 300, v, 2), classes, pool_size=3, pool_padding=1).eval()
        net.load_state_dict(net.map_state_dict(sd), strict=True)
        return net.to(DEV)
    frames = torch.rand((T, 1024, 3, v, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    big = make()
    got, t = [], 0
    while t < T:
        r = min(4, T - t)
        got += big.forward_cycle([frames[t + f] for f in range(r)])
        t += r
    assert len(got) >= 3 and all(gv.shape == (1024, classes) for gv in got)
    orc = o.CoStGcnOracle(sd, pool_size=3, pool_padding=1)
    for b in orc.blocks:
        b.gcn = so.gcn
    want = []
    with torch.no_grad():
        for t in range(T):
            r = orc.forward_step(frames[t][pick].cpu())
            if r is not None:
                want.append(r)
    assert len(want) == len(got)
    for gv, wv in zip(got, want):
        check_parity(gv[pick].cpu(), wv, note=f"CoSTr 1024 streams V={v}")
    small = make()
    got_small = [r for r in (small.forward_step(frames[t][sel].contiguous()) for t in range(T)) if r is not None]
    assert len(got_small) == len(got)
    for gv, sv in zip(got, got_small):
        assert torch.equal(gv[sel], sv)


def test_costr_1024_streams_online():
    _costr_1024_streams(25, 60, "g12_str_ntu", 12, pick=[0, 5, 255, 256, 511, 777, 1000, 1023], sel=[5, 6, 999, 1000])


def test_costr_1024_streams_kinetics_shape():
    """The same at Kinetics shape (V = 18, 400 classes): 36 864 ring columns per slot, 18-joint attention."""
    _costr_1024_streams(18, 400, "g12_str_kin", 13, pick=[0, 7, 340, 341, 682, 683, 1001, 1023], sel=[7, 8, 1001, 1023])
