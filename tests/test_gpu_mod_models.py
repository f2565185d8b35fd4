"""StGcnMod / CoStGcnMod on the GPU: the clip model against the reference's own StGcnMod (tests/golden/g15_stgcn_mod.npz) and the
composed oracle (tests/mod_oracle.py), with the valid Winograd route and with the direct kernels; the continual model's features
against the clip model's at frame s - 80 and its logits against the composed step oracle; native plan, Python engine, cycle
length and slab size bitwise; the state-dict map; stream reset, bone modality and pre-normalisation bitwise against the fresh /
twin constructions of their own test files; and the refusal of clips shorter than 81 frames."""
import numpy as np
import pytest
import torch

import _bootstrap
from closed_form import closed_form_input
from tests import mod_oracle as mo
from tests import modality_oracle as modo
from tests.helpers import check_parity

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
co = pkg.continual
DEV = "cuda:0"
T_CO, POOL = 92, dict(pool_size=4, pool_padding=0)
_cache = {}


def _graph(v):
    return (pkg.ntu_graph() if v == 25 else pkg.kinetics_graph()).A


def _clip_model(tag):
    """(fixture arrays, state dict, input, StGcnMod on the device) -- built once per shape."""
    if ("clip", tag) not in _cache:
        a, sd, x = mo.g15(tag)
        v = int(a["v"])
        net = pkg.StGcnMod(_graph(v), (3, int(a["t"]), v, 2), a["logits"].shape[1]).eval()
        net.load_state_dict(sd, strict=True)
        _cache["clip", tag] = (a, sd, x, net.to(DEV))
    return _cache["clip", tag]


def _co_model(tag, native_plan=True):
    a, sd, x, clip = _clip_model(tag)
    v = int(a["v"])
    net = pkg.CoStGcnMod(_graph(v), (3, 300, v, 2), a["logits"].shape[1], **POOL).eval()
    net.load_state_dict(net.map_state_dict(clip.state_dict()), strict=True)
    net.use_native_plan = native_plan
    return net.to(DEV)


def _co_input(tag, n=2):
    v = 25 if tag == "ntu" else 18
    return torch.from_numpy(closed_form_input((n, 3, T_CO, v, 2), salt=33.0 + v))       # (N, C, T, V, M)


def _step_run(net, x, r):
    """Step over x (N, C, T, V, M) on the device in cycles of r -> ([(step, layer-10 features (N*M, 256, V))], [(step, logits)])."""
    n, c, t, v, m = x.shape
    feats, logits = [], []
    for s0 in range(0, t, r):
        slot, nf, outs = net._cycle([x[:, :, s0 + f].contiguous() for f in range(r)])
        ring = net.layers["layer10"]._state.out
        for j in range(nf):
            feats.append(co.slot_to_frame(ring[(slot + j) % ring.shape[0]], n * m, v).clone())
        logits += [o.clone() for o in outs]
    return feats, logits


def _reference_run(tag):
    """The native plan, one frame per call, two streams: the run every other configuration is compared with."""
    if ("run", tag) not in _cache:
        net = _co_model(tag)
        _cache["run", tag] = _step_run(net, _co_input(tag).to(DEV), 1) + (net.__dict__.get("_plan") is not None,)
    return _cache["run", tag]


# ---- clip model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wino", [True, False])
@pytest.mark.parametrize("tag", ["ntu", "kin"])
def test_stgcn_mod_equals_the_reference_and_the_oracle(tag, wino):
    """The 1e-4 of tests/test_gpu_clip_parity.py, with the seven identity-residual blocks on the valid Winograd kernel and on the
    direct kernels: logits and layer 1 / 5 / 8 / 10 taps against g15, layer-10 features against the composed oracle."""
    a, sd, x, net = _clip_model(tag)
    taps = {}
    hooks = [net.layers[f"layer{i}"].register_forward_hook(lambda mod, inp, out, i=i: taps.__setitem__(i, out)) for i in (1, 5, 8, 10)]
    for b in net.layers.values():
        b.wino_valid = wino
    try:
        with torch.no_grad():
            logits = net(x.to(DEV)).cpu()
            want_feat = mo.stgcn_mod_features(x, sd)
    finally:
        for h in hooks:
            h.remove()
        for b in net.layers.values():
            b.wino_valid = True
    check_parity(logits, a["logits"], tag=tag, wino=wino, what="logits")
    for i in (1, 5, 8, 10):
        assert tuple(taps[i].shape) == tuple(a[f"layer{i}_shape"])
        check_parity(taps[i].cpu().reshape(-1)[::97], a[f"layer{i}_sub"], tag=tag, wino=wino, what=f"layer{i}")
    check_parity(taps[10].cpu(), want_feat, tag=tag, wino=wino, what="features")
    _cache["logits", tag, wino] = logits
    if ("logits", tag, not wino) in _cache:                      # the rerouted blocks are a difference, and the only one
        other = _cache["logits", tag, not wino]
        assert not torch.equal(other, logits) and float((other - logits).abs().max()) <= 1e-4


@pytest.mark.parametrize("tag", ["ntu", "kin"])
def test_stgcn_mod_batch_invariance(tag):
    a, sd, x, net = _clip_model(tag)
    more = torch.from_numpy(closed_form_input((2,) + tuple(x.shape[1:]), salt=77.0))
    with torch.no_grad():
        alone, batch = net(x.to(DEV)), net(torch.cat([x, more]).to(DEV))
    assert tuple(batch.shape) == (3, alone.shape[1]) and torch.equal(batch[0], alone[0])


def test_short_clip_raises_and_launches_nothing(monkeypatch):
    a, sd, x, net = _clip_model("ntu")

    def no_launch():
        raise AssertionError("a library call was made")
    monkeypatch.setattr(pkg.native, "lib", no_launch)
    with pytest.raises(ValueError, match="T >= 81"):
        net(x[:, :, :80].contiguous().to(DEV))


# ---- continual model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["ntu", "kin"])
def test_costgcn_mod_features_lag_the_clip_model_by_80_and_logits_equal_the_step_oracle(tag):
    a, sd, _, clip = _clip_model(tag)
    x = _co_input(tag)
    feats, logits, planned = _reference_run(tag)
    assert planned and len(feats) == T_CO - 80 and len(logits) == T_CO - 80 - 3
    with torch.no_grad():
        want = clip.features(x.to(DEV)).cpu()                                        # (N * M, 256, 12, V)
        oracle = mo.CoStGcnModOracle(sd, **POOL)
        outs = [o_ for o_ in (oracle.forward_step(x[:, :, s]) for s in range(T_CO)) if o_ is not None]
    for j, f in enumerate(feats):                                                    # emission of step s = 80 + j
        check_parity(f.cpu(), want[:, :, j], tag=tag, what="features", step=80 + j)
    assert len(outs) == len(logits)
    for j, (g, w) in enumerate(zip(logits, outs)):
        check_parity(g.cpu(), w, tag=tag, what="logits", step=83 + j)


@pytest.mark.parametrize("native_plan,r", [(False, 1), (True, 4), (False, 4)])
@pytest.mark.parametrize("tag", ["ntu", "kin"])
def test_costgcn_mod_engines_and_cycle_lengths_are_bitwise_equal(tag, native_plan, r):
    feats, logits, _ = _reference_run(tag)
    net = _co_model(tag, native_plan)
    f2, l2 = _step_run(net, _co_input(tag).to(DEV), r)
    assert (net.__dict__.get("_plan") is not None) == native_plan
    assert len(f2) == len(feats) and all(torch.equal(a_, b_) for a_, b_ in zip(f2, feats))
    assert len(l2) == len(logits) and all(torch.equal(a_, b_) for a_, b_ in zip(l2, logits))


@pytest.mark.parametrize("tag", ["ntu", "kin"])
def test_costgcn_mod_stream_0_of_a_larger_slab_is_stream_0_alone(tag):
    x = _co_input(tag, 3).to(DEV)
    f3, l3 = _step_run(_co_model(tag), x, 4)
    f1, l1 = _step_run(_co_model(tag), x[:1].contiguous(), 4)
    assert len(f1) == len(f3) == T_CO - 80 and all(torch.equal(a_[:2], b_) for a_, b_ in zip(f3, f1))      # M = 2 skeletons of stream 0
    assert len(l1) == len(l3) and all(torch.equal(a_[0], b_[0]) for a_, b_ in zip(l3, l1))


def test_stgcn_mod_state_dict_loads_into_costgcn_mod_and_clip_forwards_agree():
    """The continual model's clip forward runs the same blocks on the same weights: its layer-10 features are the clip model's."""
    a, sd, x, clip = _clip_model("ntu")
    net = _co_model("ntu")
    with torch.no_grad():
        assert torch.equal(net._clip_features(x.to(DEV)), clip.features(x.to(DEV)))


# ---- inherited switches -----------------------------------------------------------------------------------------------------
def _predictions(net, frames, r, rows=None, lo=0):
    out = []
    for t in range(lo, len(frames), r):
        cyc = [frames[t + f] if rows is None else frames[t + f][rows].contiguous() for f in range(r)]
        out += [(t + r, o.clone()) for o in net.forward_cycle(cyc)]
    return out


def _same(a_, b_):
    return len(a_) == len(b_) and all(ta == tb and torch.equal(p, q) for (ta, p), (tb, q) in zip(a_, b_))


def test_bone_modality_equals_the_twin_stepped_on_host_derived_frames():
    net, twin = _co_model("ntu"), _co_model("ntu")
    pkg.set_input_modality(net, "bone")
    x = torch.randn((T_CO, 2, 3, 25, 2), generator=torch.Generator().manual_seed(21))                     # (T, N, C, V, M)
    der = modo.derive_steps(x.permute(1, 2, 0, 3, 4).numpy(), "bone", pkg.modality.bone_parents(25))
    der = torch.from_numpy(np.ascontiguousarray(der.transpose(2, 0, 1, 3, 4)))
    got, want = _predictions(net, x.to(DEV), 4), _predictions(twin, der.to(DEV), 4)
    assert len(want) == T_CO - 83 and _same(got, want) and net.__dict__.get("_plan") is not None


def test_pre_normalisation_equals_the_twin_stepped_on_the_clip_form():
    from tests.test_gpu_prenorm import _raw
    net, twin = _co_model("ntu"), _co_model("ntu")
    pkg.set_pre_normalization(net)
    x = _raw(2, T_CO, 25, 2, 21).to(DEV)                                                                   # (N, 3, T, V, M)
    raw, normed = x.permute(2, 0, 1, 3, 4).contiguous(), pkg.pre_normalize_clip(x).permute(2, 0, 1, 3, 4).contiguous()
    got, want = _predictions(net, raw, 4), _predictions(twin, normed, 4)
    assert len(want) == T_CO - 83 and _same(got, want)


def test_reset_stream_is_a_fresh_model():
    """Stream 1 of three is reset at frame 8 and stepped on (one frame per cycle while it warms: the total stride is 1): from the
    fresh model's first emission on its features and logits are the fresh one-stream model's, bit for bit; stream 0 runs on as
    in a slab that was never reset."""
    slab, plain, fresh = _co_model("ntu"), _co_model("ntu"), _co_model("ntu")
    x = torch.rand((8 + T_CO, 3, 3, 25, 2), generator=torch.Generator().manual_seed(23)).to(DEV)          # (T, N, C, V, M)
    mv, compared = 50, 0
    for t in range(len(x)):
        if t == 8:
            slab.reset_streams([1])
        slot, nf, logits = slab._cycle([x[t]])
        pslot, pnf, plogits = plain._cycle([x[t]])
        assert nf == pnf and len(logits) == len(plogits)
        ring, pring = slab.layers["layer10"]._state.out, plain.layers["layer10"]._state.out
        if nf:
            assert torch.equal(ring[slot][:, :mv], pring[pslot][:, :mv])
        assert all(torch.equal(p[0], q[0]) for p, q in zip(logits, plogits))
        if t >= 8:
            fslot, fnf, flogits = fresh._cycle([x[t][[1]].contiguous()])
            if fnf:
                assert nf == 1
                compared += 1
                assert torch.equal(ring[slot][:, mv: 2 * mv], fresh.layers["layer10"]._state.out[fslot][:, :mv]), t
            if flogits:
                compared += 1
                assert len(logits) == 1 and torch.equal(logits[0][1], flogits[0][0]), t
            assert bool(slab.streams_ready()[1]) == bool(flogits), t
    assert compared == (T_CO - 80) + (T_CO - 83)
