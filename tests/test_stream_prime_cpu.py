"""Priming streams from buffered history, the parts that need no GPU: the symbol and its signature, the argument checks of
csk_co_prime_pack_f32 (made on the host side of the entry), the frame table against a brute-force simulation of a fresh
stream's ring counters, the record offsets, and every refusal of prime_state / prime_streams (no launch)."""
import ctypes as C
import os
import re

import pytest
import torch

import _bootstrap

pkg = _bootstrap.load()
native = pkg.native
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, K = pkg.ntu_graph().A, pkg.kinetics_graph().A


def test_symbol_signature_and_abi():
    hdr = open(os.path.join(ROOT, "include", "cskel.h")).read()
    decl = re.search(r"int csk_co_prime_pack_f32\(([^;]*)\);", hdr)
    assert decl, "csk_co_prime_pack_f32 is not declared in include/cskel.h"
    params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
    kinds = [C.c_void_p if "*" in p else (C.c_int64 if p.startswith("int64_t") else C.c_int) for p in params]
    assert native.SIGNATURES["csk_co_prime_pack_f32"] == kinds and len(kinds) == 8
    assert hasattr(C.CDLL(native.LIB_PATH), "csk_co_prime_pack_f32")
    assert native.lib().csk_abi_version() == native.ABI_VERSION == 16            # additive: the version stays
    body = re.search(r"typedef struct csk_prime_job \{(.*?)\} csk_prime_job;", hdr, re.S).group(1)
    names = [n.strip(" *") for line in body.split(";") if line.strip() for n in line.strip().split(None, 1)[1].replace("void *", "").split(",")]
    assert names == [f[0] for f in native.PrimeJob._fields_]
    assert C.sizeof(native.PrimeJob) == 8 + 8 + 6 * 4
    for name, value in (("RING", native.PRIME_RING), ("POOL", native.PRIME_POOL), ("WORDS", native.PRIME_WORDS)):
        assert int(re.search(rf"#define CSK_PRIME_{name} (\d+)", hdr).group(1)) == value
    assert "stream_prime.hip" in os.listdir(os.path.join(ROOT, "continual-skeletons_amd", "csrc"))


def _job(src=0x1000, offset=0, kind=native.PRIME_RING, rows=64, t_src=12, first=4, window=8):
    return native.PrimeJob(src, offset, kind, rows, t_src, first, window, 0)


def _call(jobs, n_jobs=None, packed=0x2000, record=1 << 20, n_streams=2, m=2, v=25):
    arr = (native.PrimeJob * max(1, len(jobs)))(*jobs)
    return native.lib().csk_co_prime_pack_f32(C.byref(arr) if jobs else None, len(jobs) if n_jobs is None else n_jobs,
                                              C.c_void_p(packed), record, n_streams, m, v, None)


@pytest.mark.parametrize("kwargs, needle", [
    (dict(jobs=[]), "null pointer (jobs)"),
    (dict(jobs=[_job()], n_jobs=0), "jobs per launch"),
    (dict(jobs=[_job()], n_jobs=native.MOVE_MAX_JOBS + 1), "jobs per launch"),
    (dict(jobs=[_job()], n_streams=-1), "n_streams < 0"),
    (dict(jobs=[_job()], m=0), "M >= 1"),
    (dict(jobs=[_job()], v=0), "V >= 1"),
    (dict(jobs=[_job()], record=0), "record of 0"),
    (dict(jobs=[_job()], packed=0), "null pointer (packed)"),
    (dict(jobs=[_job()], packed=0x2002), "4-byte aligned"),
    (dict(jobs=[_job(kind=3)]), "unknown job kind"),
    (dict(jobs=[_job(src=0)]), "null pointer (source"),
    (dict(jobs=[_job(src=0x1002)]), "source of job 0 is not 4-byte aligned"),
    (dict(jobs=[_job(rows=0)]), "bad dims"),
    (dict(jobs=[_job(t_src=0)]), "bad dims"),
    (dict(jobs=[_job(window=-1)]), "a window of -1"),
    (dict(jobs=[_job(first=5)]), "takes frames [5, 13) of a source of 12"),
    (dict(jobs=[_job(kind=native.PRIME_POOL, first=5)]), "takes frames [5, 13) of a source of 12"),
    (dict(jobs=[_job(kind=native.PRIME_WORDS, rows=36, t_src=1, first=0, window=2)]), "a words job copies one array"),
    (dict(jobs=[_job(kind=native.PRIME_WORDS, rows=36, t_src=2, first=0, window=1)]), "a words job copies one array"),
    (dict(jobs=[_job(offset=-1)]), "of a record of"),
    (dict(jobs=[_job()], record=8 * 64 * 50 - 1), "of a record of"),
    (dict(jobs=[_job(offset=1)], record=8 * 64 * 50), "of a record of"),
    (dict(jobs=[_job(kind=native.PRIME_POOL, offset=1)], record=8 * 64), "of a record of"),
    (dict(jobs=[_job(), _job(src=0)]), "source of job 1"),
])
def test_pack_entry_refuses_bad_arguments_without_a_gpu(kwargs, needle):
    lib = native.lib()
    assert _call(**kwargs) < 0
    assert needle in lib.csk_last_error().decode(), lib.csk_last_error().decode()


def test_pack_entry_with_nothing_to_do_launches_nothing():
    assert _call([_job()], n_streams=0, packed=0) == 0
    assert _call([_job(window=0, first=12), _job(kind=native.PRIME_POOL, window=0), _job(kind=native.PRIME_WORDS, t_src=1, first=0, window=0)]) == 0
    assert _call([_job(first=-3, window=0)]) == 0                                # a negative first frame is legal


def _brute_force_counts(net, t):
    """Feed a fresh stream ``t`` frames, one at a time, through counters that follow ``continual.emissions``: [frames each
    ring-feeding stage has pushed: input, then every block's emissions]."""
    received = [0] * len(net._blocks)
    counts = [0] * (len(net._blocks) + 1)
    for _ in range(t):
        counts[0] += 1
        push = 1
        for i, blk in enumerate(net._blocks):
            if not push:
                break
            _, e = pkg.continual.emissions(received[i], push, blk.delay, blk.stride)
            received[i] += push
            counts[i + 1] += e
            push = e
    return counts, received


def _models():
    return {"ntu": pkg.CoStGcn(A, pool_size=4, pool_padding=0).eval(),
            "kinetics": pkg.CoStGcn(K, input_shape=(3, 300, 18, 2), num_classes=400).eval()}


@pytest.mark.parametrize("which", ["ntu", "kinetics"])
@pytest.mark.parametrize("t", [76, 80, 96, 300])
def test_frame_table_against_a_brute_force_stream(which, t):
    net = _models()[which]
    counts, received = _brute_force_counts(net, t)
    assert net.prime_counts(t) == counts
    table = {name: (source, count, first, window) for name, source, count, first, window in net.prime_table(t)}
    clip = net.prime_clip_frames(t)
    windows = {name: window for name, _, _, window in net._move_windows()}
    assert table["xin0"] == ("xin0", t, t - windows["xin0"], windows["xin0"])
    for i in range(10):
        # the post-GCN ring of block i has received what the block has received; its clip tensor has the frames of its input
        assert table[f"y{i}"] == (f"y{i}", received[i], received[i] - 8, 8) and received[i] == counts[i] <= clip[i]
        if i < 9:
            assert table[f"out{i}"] == (f"out{i}", counts[i + 1], counts[i + 1] - 4, 4)
        assert counts[i + 1] <= clip[i + 1]                                  # never a frame behind the clip tensor
        # ... and never a clip frame the right padding touched: output frame j of block i reads post-GCN frames up to
        # j * stride + 4, which the block has received
        blk = net._blocks[i]
        assert counts[i + 1] == 0 or (counts[i + 1] - 1) * blk.stride + blk.delay <= received[i] - 1
    assert table["pool"] == ("out9", counts[10], counts[10] - net.pool_size, net.pool_size)
    assert [name for name, *_ in net.prime_table(t)] == [name for name, *_ in net._move_windows()][:21]


def test_youngest_history_has_an_empty_pooling_window_and_leading_zero_frames():
    net = _models()["ntu"]
    assert net._cum_delays()[10] == 76
    table = {name: (count, first, window) for name, _, count, first, window in net.prime_table(76)}
    assert table["pool"] == (0, -4, 4)                  # no entry yet: four zero entries
    assert table["y9"] == (4, -4, 8)                    # four leading zero frames, then layer 10's four post-GCN frames
    assert table["out8"] == (4, 0, 4) and table["y8"] == (8, 0, 8)
    assert all(first >= 0 for name, (_, first, _) in table.items() if name not in ("pool", "y9"))
    assert all(first >= 0 for name, _, _, first, _ in net.prime_table(96) if name != "pool")
    assert {name: first for name, _, _, first, _ in net.prime_table(96)}["pool"] == 1      # 5 emissions, a window of 4


def test_record_offsets_agree_with_the_move_windows():
    net = _models()["ntu"]
    pkg.set_input_modality(net, "bone_motion")
    pkg.set_pre_normalization(net)
    windows = net._move_windows()
    assert net.record_floats() == sum(rows * seg * window for _, rows, seg, window in windows)
    assert [name for name, *_ in windows][21:] == ["mod_prev", "mod_flags", "pn_rot", "pn_flags"] and len(windows) <= native.MOVE_MAX_JOBS
    ring = net.prime_table(96)
    assert len(ring) == 21 and [w for *_, w in ring] == [window for _, _, _, window in windows[:21]]
    c, _, v, m = net.input_shape
    assert net.prime_stream_bytes(300) == 4 * (2 * c * 300 * v * m + v * m * sum(
        blk.out_channels * (a + b) for blk, a, b in zip(net._blocks, net.prime_clip_frames(300), net.prime_clip_frames(300)[1:])))
    assert 60e6 < net.prime_stream_bytes(300) < 100e6


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


def test_every_refusal_is_made_on_the_host_without_a_launch(monkeypatch):
    monkeypatch.setattr(native, "lib", lambda: _NoLaunch())
    _NoLaunch.calls = 0
    net = _models()["ntu"]
    for t in (77, 78, 79, 98):
        with pytest.raises(ValueError, match="not a multiple of the total stride 4"):
            net.prime_state(_hist(t))
    for t in (4, 72):
        with pytest.raises(ValueError, match=r"younger than the 76 frames.*reset_streams"):
            net.prime_state(_hist(t))
    with pytest.raises(RuntimeError, match="does not match input_shape"):
        net.prime_state(_hist(96, v=18))
    with pytest.raises(RuntimeError, match=r"\(n, C, T, V, M\) history tensor"):
        net.prime_state(torch.zeros((3, 96, 25, 2)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                   # a history that passes every other check
        net.prime_state(_hist(96))
    with pytest.raises(NotImplementedError, match="one\\s+adjacency over all T frames"):
        pkg.CoAGcn(A, pool_size=4, pool_padding=0).eval().prime_state(_hist(96))
    for cls in (pkg.CoStGcnMod, pkg.agcn.CoAGcnMod, pkg.str.CoSTrMod):
        with pytest.raises(NotImplementedError, match=r"unpadded '\*' models.*follow-up"):
            cls(A, pool_size=4, pool_padding=0).eval().prime_state(_hist(96))
    split = pkg.set_precision(pkg.CoStGcn(A, pool_size=4, pool_padding=0).eval(), "bf16x3")
    with pytest.raises(NotImplementedError, match="clip precision of this model is 'bf16x3'"):
        split.prime_state(_hist(96))
    with pytest.raises(RuntimeError, match="inference-only"):
        pkg.CoStGcn(A).train().prime_state(_hist(96))
    # prime_streams: the history's checks come first, then import_streams' own, all before a launch
    with pytest.raises(ValueError, match="not a multiple of the total stride"):
        net.prime_streams(_hist(78), [0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.prime_streams(_hist(96), [0])
    assert _NoLaunch.calls == 0


def test_prime_streams_runs_the_import_checks_before_any_launch(monkeypatch):
    """A device history cannot exist here, so the device check is taken out of the way: what must then refuse, without a
    launch, is ``import_streams``' own list."""
    monkeypatch.setattr(native, "lib", lambda: _NoLaunch())
    monkeypatch.setattr(native, "require_device_f32", lambda t, name: None)
    _NoLaunch.calls = 0
    net = _models()["ntu"]
    net.use_native_plan = False
    with pytest.raises(RuntimeError, match="no state slab is bound"):
        net.prime_streams(_hist(96), [0])
    net._bind(3, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="step it through its warm-up first"):
        net.prime_streams(_hist(96), [0])
    r, ctr, per_block = 200, [200], []
    for blk in net._blocks:
        _, e = pkg.continual.emissions(0, r, blk.delay, blk.stride)
        per_block += [r, e]
        r = e
    net._set_counters(ctr + [r] + per_block)
    with pytest.raises(ValueError, match="2 indices for 1 records"):
        net.prime_streams(_hist(96), [0, 1])
    with pytest.raises(ValueError, match="outside a slab of 3"):
        net.prime_streams(_hist(96), [3])
    net._frames = 201
    with pytest.raises(RuntimeError, match="multiple of 4"):
        net.prime_streams(_hist(96), [0])
    net._frames = 200
    twin = _models()["ntu"]
    twin.use_native_plan = False
    ens = pkg.fusion.OnlineEnsemble([net, twin])
    with pytest.raises(RuntimeError, match="no state slab is bound"):           # the second member refuses: the first has not launched
        ens.prime_streams(_hist(96), [0])
    with pytest.raises(ValueError, match="younger than"):
        ens.prime_streams(_hist(40), [0])
    assert _NoLaunch.calls == 0
