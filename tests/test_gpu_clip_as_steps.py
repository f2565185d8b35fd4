"""``forward_clip_as_steps`` / ``features_clip_as_steps`` of every continual family but CoAGcn (co_clip.py; CoAGcn's
own are held by tests/test_gpu_agcn_framewise.py): one clip pass and one csk_co_head_clip_f32 call against a fresh twin that
STEPS the same clip, within the project's clip-versus-steps bound -- max|clip - steps| <= 1e-4 max|steps|.
The observed ratios are printed (run with -s)."""
import pytest
import torch

import _bootstrap
from tests.helpers import randomise_unit_

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native = pkg.native
DEV = "cuda:0"
N, T = 2, 96
CLASSES = {"stgcn": pkg.CoStGcn, "str": pkg.CoSTr, "stgcnmod": pkg.CoStGcnMod, "agcnmod": pkg.agcn.CoAGcnMod, "strmod": pkg.str.CoSTrMod}


def _pair(model, graph, pool, seed=11):
    """(net, twin): the same seeded weights; ``pool`` = (pool_size, pool_padding), -1: the head's defaults for T = 96."""
    a = (pkg.ntu_graph() if graph == "ntu" else pkg.kinetics_graph()).A
    v = a.shape[-1]
    nets = [CLASSES[model](a, (3, T, v, 2), 60, pool_size=pool[0], pool_padding=pool[1]).eval() for _ in range(2)]
    randomise_unit_(nets[0], seed)
    nets[1].load_state_dict(nets[0].state_dict())
    return [net.to(DEV) for net in nets], v


def _clip(v, t=T, seed=3):
    return torch.rand((N, 3, t, v, 2), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _close(got, want, label):
    assert got.shape == want.shape, (label, tuple(got.shape), tuple(want.shape))
    scale = float(want.abs().max())
    ratio = float((got - want).abs().max()) / scale if scale else 0.0
    print(f"clip-as-steps {label}: {tuple(got.shape)} max|clip-steps|/max|steps| = {ratio:.3e} (bound 1e-4)")
    assert scale > 0 and ratio <= 1e-4, (label, ratio)


CASES = [("stgcn", "ntu", (4, 0)), ("stgcn", "ntu", (4, 1)), ("stgcn", "kinetics", (4, 1)), ("str", "ntu", (4, 1)),
         ("stgcnmod", "ntu", (-1, -1)), ("stgcnmod", "ntu", (4, 1)), ("agcnmod", "ntu", (-1, -1)), ("agcnmod", "ntu", (4, 0)),
         ("strmod", "ntu", (-1, -1)), ("strmod", "ntu", (4, 1))]


@pytest.mark.parametrize("model,graph,pool", CASES, ids=[f"{m}-{g}-pool{p[0]}-{p[1]}" for m, g, p in CASES])
def test_clip_as_steps_equals_a_stepped_twin(model, graph, pool):
    """T = 96.  The padded models release 5 layer-10 frames without ``pad_end`` and 24 with it; the '*' models 16 either way
    (their flush pushes nothing), with the default head of T = 96 -- a window of 16, one prediction -- and with a window of 4."""
    (net, twin), v = _pair(model, graph, pool)
    if pool == (-1, -1):
        assert (net.pool_size, net.pool_padding) == (16, 0)
    x = _clip(v)
    for pad_end in (False, True):
        twin.clean_state()
        want = twin.forward_steps(x, pad_end)
        got = net.forward_clip_as_steps(x, pad_end)
        assert want.shape[2] == len(net.clip_as_steps_map(T, pad_end)[1]) > 0
        _close(got, want, f"{model}-{graph}-pool{pool} pad_end={pad_end}")
        assert net._n is None                                                      # no slab was bound on the way


@pytest.mark.parametrize("model,t", [("stgcn", 84), ("stgcnmod", 83)])
def test_a_history_too_short_to_predict_gives_an_empty_result(model, t):
    (net, twin), v = _pair(model, "ntu", (4, 0))
    x = _clip(v, t)
    twin.clean_state()
    want, got = twin.forward_steps(x), net.forward_clip_as_steps(x)
    assert tuple(want.shape) == tuple(got.shape) == (N, 60, 0) and got.device == x.device


def test_the_call_touches_no_continual_state():
    """On a bound model in mid-stream: the state tensors and the position are bit for bit what they were, and the model steps
    on bit for bit like a twin that never made the call."""
    (net, twin), v = _pair("stgcn", "ntu", (4, 1))
    frames = torch.rand((104, N, 3, v, 2), generator=torch.Generator().manual_seed(5)).to(DEV)
    for t in range(0, 96, 4):
        for m in (net, twin):
            m.forward_cycle([frames[t + f] for f in range(4)])
    before, position = [s.clone() for s in net._state_tensors()], net._position()
    out = net.forward_clip_as_steps(_clip(v), pad_end=True)
    assert out.shape[2] > 0
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(net._state_tensors(), before))
    assert net._position() == position
    for t in range(96, 104, 4):
        a, b = (m.forward_cycle([frames[t + f] for f in range(4)]) for m in (net, twin))
        assert len(a) == len(b) == 1 and torch.equal(a[0], b[0])


def _bone_motion(net):
    pkg.set_input_modality(net, "bone_motion")


def _prenorm(net):
    pkg.set_pre_normalization(net)


def _keypoints(net):
    pkg.keypoints.set_keypoint_intake(net, 5)


@pytest.mark.parametrize("setup,graph", [(_bone_motion, "ntu"), (_prenorm, "ntu"), (_keypoints, "kinetics")],
                         ids=["bone_motion", "prenorm", "keypoints"])
def test_input_variants_follow_the_steps(setup, graph):
    """A motion modality (the steps take the BACKWARD difference), the pre-normalisation (rotations latched from frame 0) and
    the keypoint intake ((N, T, P, V, 3) clips), each against the stepped twin."""
    (net, twin), v = _pair("stgcn", graph, (4, 1))
    for m in (net, twin):
        setup(m)
    if setup is _keypoints:
        x = torch.rand((N, T, 5, v, 3), generator=torch.Generator().manual_seed(8)).to(DEV)
    else:
        x = _clip(v, seed=8)
    twin.clean_state()
    _close(net.forward_clip_as_steps(x, True), twin.forward_steps(x, True), setup.__name__)


@pytest.mark.parametrize("model", ["stgcn", "stgcnmod"])
def test_features_are_the_models_clip_features(model):
    """Joint modality, no pre-pass: the stepped-form input is the clip itself, so the features are ``_clip_features`` bit for
    bit; with a motion modality they are ``_clip_stack`` of the backward difference."""
    (net, _), v = _pair(model, "ntu", (4, 0))
    x = _clip(v)
    got = net.features_clip_as_steps(x)
    assert tuple(got.shape) == (N * 2, 256, 16 if model == "stgcnmod" else 24, v)
    assert torch.equal(got.view(torch.int32), net._clip_features(x).view(torch.int32))
    pkg.set_input_modality(net, "joint_motion")
    back = torch.zeros_like(x)
    back[:, :, 1:] = x[:, :, 1:] - x[:, :, :-1]
    plain = _pair(model, "ntu", (4, 0))[0][0]
    assert torch.equal(net.features_clip_as_steps(x).view(torch.int32), plain._clip_features(back).view(torch.int32))
