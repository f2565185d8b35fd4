"""The three step pre-passes on at once (input_stage.py): ``CoStGcn`` on the 18-joint graph, 2 streams, ``max_cycle`` 4, keypoint
intake (P = 5), pre-normalisation and the bone-motion modality -- against the same model with every switch off, fed the frames
the public clip functions give in chain order: ``select_people_clip``, ``pre_normalize_clip``, ``derive_clip`` shifted by one
frame (the steps' backward difference).  The history is the shortest after which the head has emitted twice, ``_ready_age() +
stride`` frames (from ``_cum_delays``); the moves happen at the last multiple of the stride in front of it.

Bit for bit (``torch.equal``) wherever both sides run the step kernels.  A primed stream's activations come from the clip
kernels: its small states are bit for bit, its logits within the project's clip-versus-steps bound (rtol 1e-4, atol 1e-5:
tests/test_gpu_continual_parity.py, tests/test_gpu_stream_prime.py)."""
import pytest
import torch

import _bootstrap
from tests.helpers import randomise_unit_

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
keypoints = pkg.keypoints
DEV = "cuda:0"
N, P, V, M = 2, 5, 18, 2
CO = dict(pool_size=3, pool_padding=1)


def _net(weights=None, on=True):
    net = pkg.CoStGcn(pkg.kinetics_graph().A, (3, 300, V, M), 60, **CO).eval()
    if weights is None:
        randomise_unit_(net, 7)
    else:
        net.load_state_dict(weights)
    net = net.to(DEV)
    net.set_max_cycle(4)
    if on:
        keypoints.set_keypoint_intake(net, P)
        pkg.set_input_modality(pkg.set_pre_normalization(net), "bone_motion")
    return net


def _step(net, frames, lo, hi):
    """Frames lo .. hi - 1 in aligned cycles of at most 4 -> [(frames received, logits)]."""
    out = []
    for t in range(lo, hi, 4):
        cyc = list(frames[t:min(t + 4, hi)])
        out += [(t + len(cyc), o.clone()) for o in net.forward_cycle(cyc)]
    return out


def _same(a, b):
    return len(a) == len(b) and all(ta == tb and torch.equal(x, y) for (ta, x), (tb, y) in zip(a, b))


def _stage_state(net):
    return {name: t for stage in net.stages for name, t in stage.state()}


@pytest.fixture(scope="module")
def world():
    """The history, the model stepped to the move point (read only: the tests export from it and read its state), and the
    logits of a second copy stepped through the whole history."""
    net = _net()
    weights = net.state_dict()
    twice = net._ready_age() + net.stride               # frames after which the head has emitted twice
    move_at = (twice - 1) // net.stride * net.stride    # streams move at multiples of the stride
    assert net._ready_age() == net._cum_delays()[10] + net.stride + 1 and move_at >= net._ready_age()
    g = torch.Generator().manual_seed(5)
    k = torch.rand((N, twice, P, V, 3), generator=g).to(DEV)               # (N, T, P, V, 3) keypoint history
    raw = k.permute(1, 0, 2, 3, 4).contiguous()                             # [T](N, P, V, 3)
    _step(net, raw, 0, move_at)
    full = _step(_net(weights), raw, 0, twice)
    return dict(net=net, weights=weights, twice=twice, move_at=move_at, k=k, raw=raw, full=full)


def test_the_chain_equals_the_plain_model_on_the_public_clip_functions(world):
    net, k, twice = world["net"], world["k"], world["twice"]
    assert [type(s).__name__ for s in net.stages] == ["KeypointIntake", "PreNorm", "InputModality"] and all(s.enabled for s in net.stages)
    d = pkg.modality.derive_clip(pkg.pre_normalize_clip(keypoints.select_people_clip(k, M)), "bone_motion")
    stepped = torch.zeros_like(d)
    stepped[:, :, 1:] = d[:, :, :-1]
    frames = stepped.permute(2, 0, 1, 3, 4).contiguous()
    plain = _net(world["weights"], on=False)
    assert not any(s.enabled for s in plain.stages)
    want = _step(plain, frames, 0, twice)
    assert [t for t, _ in want] == [world["move_at"], twice] and _same(world["full"], want)


def _continued(world):
    """A second slab that holds the model's streams at the move point (export -> import), ready for the frames behind it."""
    net, other = world["net"], _net(world["weights"])
    g = torch.Generator().manual_seed(6)
    _step(other, torch.rand((world["move_at"], 3, P, V, 3), generator=g).to(DEV), 0, world["move_at"])     # 3 other streams
    other.import_streams(net.export_streams([0, 1]), [2, 0])
    return _Rows(other, [2, 0])


class _Rows:
    """``forward_cycle`` of a slab on frames for the streams ``rows`` (the others get seeded noise), returning those rows."""

    def __init__(self, net, rows):
        self.net, self.rows, self.g = net, rows, torch.Generator().manual_seed(9)

    def forward_cycle(self, cyc):
        full = []
        for x in cyc:
            f = torch.rand((self.net._n,) + tuple(x.shape[1:]), generator=self.g).to(DEV)
            f[self.rows] = x
            full.append(f)
        return [o[self.rows] for o in self.net.forward_cycle(full)]


def test_exported_streams_continue_bitwise_on_a_second_slab(world):
    net, raw, move_at, twice = world["net"], world["raw"], world["move_at"], world["twice"]
    moved = _continued(world)
    mine, theirs = _stage_state(net), _stage_state(moved.net)
    assert sorted(mine) == ["mod_flags", "mod_prev", "pn_flags", "pn_rot"]
    assert all(torch.equal(theirs[name][moved.rows], mine[name]) for name in mine)
    assert _same(_step(moved, raw, move_at, twice), world["full"][-1:])


def test_a_peek_leaves_the_stage_state_bit_identical(world):
    net, raw, move_at = _net(world["weights"]), world["raw"], world["move_at"]
    assert _same(_step(net, raw, 0, move_at), world["full"][:-1])
    keep = {name: t.clone() for name, t in _stage_state(net).items()}
    peeked = net.forward_step(raw[move_at], update_state=False)
    assert len(keep) == 4 and all(torch.equal(t, keep[name]) for name, t in _stage_state(net).items())
    assert torch.equal(peeked, net.forward_step(raw[move_at])) and torch.equal(peeked, world["full"][-1][1])
    assert not torch.equal(_stage_state(net)["mod_prev"], keep["mod_prev"])         # the real step did update


def test_reset_streams_clears_exactly_that_streams_flags(world):
    net, raw, move_at = _net(world["weights"]), world["raw"], world["move_at"]
    _step(net, raw, 0, move_at)
    flags = [stage.flags for stage in net.stages if stage.flags is not None]
    rot = net.stage("prenorm").rot.clone()
    assert len(flags) == 2 and all(f.tolist() == [1, 1] for f in flags)
    net.reset_streams([1])
    assert all(f.tolist() == [1, 0] for f in flags) and torch.equal(net.stage("prenorm").rot, rot)


def test_prime_streams_from_the_history_equals_stepping_it(world):
    net, k, raw, move_at, twice = world["net"], world["k"], world["raw"], world["move_at"], world["twice"]
    primed = _net(world["weights"])
    g = torch.Generator().manual_seed(8)
    _step(primed, torch.rand((move_at, N, P, V, 3), generator=g).to(DEV), 0, move_at)
    primed.prime_streams(k[:, :move_at].contiguous(), [0, 1])
    mine, theirs = _stage_state(net), _stage_state(primed)
    assert all(torch.equal(theirs[name], mine[name]) for name in mine)              # the small states: bit for bit
    t_want, want = world["full"][-1]
    (t_got, got), = _step(primed, raw, move_at, twice)
    assert t_got == t_want == twice and torch.allclose(got, want, rtol=1e-4, atol=1e-5)
