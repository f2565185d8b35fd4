"""AGcnMod / STrMod / CoAGcnMod / CoSTrMod on the GPU, as tests/test_gpu_mod_models.py does for StGcnMod / CoStGcnMod: the clip
models against the reference's own classes (tests/golden/g16_agcn_mod.npz, g17_str_mod.npz) and the literal oracle
(tests/mod_family_oracle.py) with the conv-residual blocks (layers 5 and 8) on csk_tcn_stage_wino_valid_res_f32 and on the direct
kernel; batch invariance; the continual models' features against the clip models' at frame s - 80 (A-GCN*'s graph conv is per
frame, so this holds for it as it cannot for A-GCN) and their logits against the step oracle; engines, cycle lengths and slab
sizes bitwise; one stream reset."""
import pytest
import torch

import _bootstrap
from closed_form import closed_form_input
from tests import mod_family_oracle as fo
from tests.helpers import check_parity
from tests.test_gpu_mod_models import _graph, _step_run

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
DEV = "cuda:0"
T_CO, POOL = 100, dict(pool_size=4, pool_padding=0)
MODELS = {"agcn": (fo.g16, pkg.agcn.AGcnMod, pkg.agcn.CoAGcnMod), "str": (fo.g17, pkg.str.STrMod, pkg.str.CoSTrMod)}
CASES = [(m, tag) for m in MODELS for tag in ("ntu", "kin")]
_cache = {}


def _clip_model(model, tag):
    """(fixture arrays, state dict, input, clip model on the device) -- built once per model and shape."""
    if ("clip", model, tag) not in _cache:
        a, sd, x = MODELS[model][0](tag)
        v = int(a["v"])
        net = MODELS[model][1](_graph(v), (3, int(a["t"]), v, 2), a["logits"].shape[1]).eval()
        net.load_state_dict(sd, strict=True)
        _cache["clip", model, tag] = (a, sd, x, net.to(DEV))
    return _cache["clip", model, tag]


def _co_model(model, tag, native_plan=True):
    a, sd, x, clip = _clip_model(model, tag)
    v = int(a["v"])
    net = MODELS[model][2](_graph(v), (3, 300, v, 2), a["logits"].shape[1], **POOL).eval()
    net.load_state_dict(net.map_state_dict(clip.state_dict()), strict=True)
    net.use_native_plan = native_plan
    return net.to(DEV)


def _co_input(tag, n=2):
    v = 25 if tag == "ntu" else 18
    return torch.from_numpy(closed_form_input((n, 3, T_CO, v, 2), salt=35.0 + v))       # (N, C, T, V, M)


def _reference_run(model, tag):
    """The model's default engine, one frame per call, two streams: the run every other configuration is compared with."""
    if ("run", model, tag) not in _cache:
        net = _co_model(model, tag)
        _cache["run", model, tag] = _step_run(net, _co_input(tag).to(DEV), 1) + (net.__dict__.get("_plan") is not None,)
    return _cache["run", model, tag]


# ---- clip models ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wino_res", [True, False])
@pytest.mark.parametrize("model,tag", CASES)
def test_clip_model_equals_the_reference_and_the_oracle(model, tag, wino_res):
    a, sd, x, net = _clip_model(model, tag)
    taps = {}
    hooks = [net.layers[f"layer{i}"].register_forward_hook(lambda mod, inp, out, i=i: taps.__setitem__(i, out)) for i in (1, 5, 8, 10)]
    assert [i + 1 for i, b in enumerate(net.layers.values()) if b.wino_valid_res] == [5, 8]
    for i in (5, 8):
        net.layers[f"layer{i}"].wino_valid_res = wino_res
    try:
        with torch.no_grad():
            logits = net(x.to(DEV)).cpu()
            want_feat = fo.mod_features(x, sd)
    finally:
        for h in hooks:
            h.remove()
        for i in (5, 8):
            net.layers[f"layer{i}"].wino_valid_res = True
    check_parity(logits, a["logits"], model=model, tag=tag, wino_res=wino_res, what="logits")
    for i in (1, 5, 8, 10):
        assert tuple(taps[i].shape) == tuple(a[f"layer{i}_shape"])
        check_parity(taps[i].cpu().reshape(-1)[::97], a[f"layer{i}_sub"], model=model, tag=tag, wino_res=wino_res, what=f"layer{i}")
    check_parity(taps[10].cpu(), want_feat, model=model, tag=tag, wino_res=wino_res, what="features")
    _cache["out", model, tag, wino_res] = (logits, taps[5].cpu(), taps[8].cpu())
    if ("out", model, tag, not wino_res) in _cache:              # the rerouted blocks are a difference, and the only one
        other = _cache["out", model, tag, not wino_res]
        for got, ref in zip((logits, taps[5].cpu(), taps[8].cpu()), other):
            check_parity(got, ref, model=model, tag=tag, what="wino_valid_res on vs off")
        assert not torch.equal(other[1], taps[5].cpu()) and not torch.equal(other[0], logits)


@pytest.mark.parametrize("model,tag", CASES)
def test_clip_model_batch_invariance(model, tag):
    a, sd, x, net = _clip_model(model, tag)
    more = torch.from_numpy(closed_form_input((1,) + tuple(x.shape[1:]), salt=77.0))
    with torch.no_grad():
        alone, batch = net(x.to(DEV)), net(torch.cat([x, more]).to(DEV))
    assert tuple(batch.shape) == (3, alone.shape[1]) and torch.equal(batch[:2], alone)


def test_agcn_mod_launches_no_embedding_or_attention(monkeypatch):
    """AGcnMod's graph convs are csk_gcn_stage_f32 alone, and layers 5 and 8 reach the new entry."""
    a, sd, x, net = _clip_model("agcn", "ntu")
    lib, seen = pkg.native.lib(), []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith("csk_") or name == "csk_last_error":
                return fn
            return lambda *args: (seen.append(name), fn(*args))[1]
    monkeypatch.setattr(pkg.native, "lib", lambda: Spy())
    with torch.no_grad():
        net(x.to(DEV))
    assert seen.count("csk_gcn_stage_f32") == 10 and seen.count("csk_tcn_stage_wino_valid_res_f32") == 2
    assert seen.count("csk_tcn_stage_wino_valid_f32") == 7 and seen.count("csk_tcn_stage_f32") == 0      # no -2 fallback ran
    assert not any("agcn" in s or "conv1x1" in s for s in seen)


# ---- continual models -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,tag", CASES)
def test_features_lag_the_clip_model_by_80_and_logits_equal_the_step_oracle(model, tag):
    a, sd, _, clip = _clip_model(model, tag)
    x = _co_input(tag)
    feats, logits, planned = _reference_run(model, tag)
    assert planned == (model == "agcn") and len(feats) == T_CO - 80 and len(logits) == T_CO - 80 - 3
    with torch.no_grad():
        want = clip.features(x.to(DEV)).cpu()                                        # (N * M, 256, 20, V)
        oracle = fo.CoModOracle(sd, **POOL)
        outs = [o_ for o_ in (oracle.forward_step(x[:, :, s]) for s in range(T_CO)) if o_ is not None]
    for j, f in enumerate(feats):                                                    # emission of step s = 80 + j
        check_parity(f.cpu(), want[:, :, j], model=model, tag=tag, what="features", step=80 + j)
    assert len(outs) == len(logits)
    for j, (g, w) in enumerate(zip(logits, outs)):
        check_parity(g.cpu(), w, model=model, tag=tag, what="logits", step=83 + j)


@pytest.mark.parametrize("native_plan,r", [(False, 1), (True, 3), (True, 4), (False, 4)])
@pytest.mark.parametrize("model,tag", CASES)
def test_engines_and_cycle_lengths_are_bitwise_equal(model, tag, native_plan, r):
    feats, logits, _ = _reference_run(model, tag)
    net = _co_model(model, tag, native_plan)
    x = _co_input(tag)
    f2, l2 = _step_run(net, x[:, :, :T_CO // r * r].to(DEV), r)
    assert (net.__dict__.get("_plan") is not None) == (native_plan and model == "agcn")     # CoSTrMod: the Python engine
    k = T_CO // r * r - 80
    assert len(f2) == k and all(torch.equal(a_, b_) for a_, b_ in zip(f2, feats))
    assert len(l2) == k - 3 and all(torch.equal(a_, b_) for a_, b_ in zip(l2, logits))


@pytest.mark.parametrize("model,tag", CASES)
def test_stream_0_of_a_larger_slab_is_stream_0_alone(model, tag):
    x = _co_input(tag, 3).to(DEV)
    f3, l3 = _step_run(_co_model(model, tag), x, 4)
    f1, l1 = _step_run(_co_model(model, tag), x[:1].contiguous(), 4)
    assert len(f1) == len(f3) == T_CO - 80 and all(torch.equal(a_[:2], b_) for a_, b_ in zip(f3, f1))      # M = 2 skeletons of stream 0
    assert len(l1) == len(l3) and all(torch.equal(a_[0], b_[0]) for a_, b_ in zip(l3, l1))


def test_coagcn_mod_reset_stream_is_a_fresh_model():
    """Stream 1 of three is reset at frame 8 and stepped on: from the fresh model's first emission on its features and logits are
    the fresh one-stream model's, bit for bit."""
    slab, fresh = _co_model("agcn", "ntu"), _co_model("agcn", "ntu")
    x = torch.rand((8 + 88, 3, 3, 25, 2), generator=torch.Generator().manual_seed(23)).to(DEV)            # (T, N, C, V, M)
    mv, compared = 50, 0
    for t in range(len(x)):
        if t == 8:
            slab.reset_streams([1])
        slot, nf, logits = slab._cycle([x[t]])
        if t >= 8:
            fslot, fnf, flogits = fresh._cycle([x[t][[1]].contiguous()])
            if fnf:
                compared += 1
                ring = slab.layers["layer10"]._state.out
                assert nf == 1 and torch.equal(ring[slot][:, mv: 2 * mv], fresh.layers["layer10"]._state.out[fslot][:, :mv]), t
            if flogits:
                compared += 1
                assert len(logits) == 1 and torch.equal(logits[0][1], flogits[0][0]), t
            assert bool(slab.streams_ready()[1]) == bool(flogits), t
    assert compared == (88 - 80) + (88 - 83)
