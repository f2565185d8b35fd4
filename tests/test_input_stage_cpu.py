"""The input pre-passes as a chain of stages (input_stage.py), host only: the record layout of every combination of switches
against the values the per-stage hooks gave before the chain existed, the chain order, "off is the identity", the shared
setter on a two-shard ``StreamShards`` whose second shard refuses, and the one-intake rule from both directions.

RINGS, SIGNATURE_AROUND, TAILS and REFUSED are data: ``move_signature()``, ``_move_windows()`` and ``record_floats()`` of
``CoStGcn(graph, (3, 300, V, 2))`` as the commit in front of the chain returned them, for 4 modalities x pre-normalisation off /
default joints / zaxis (2, 3), xaxis (24, 0) x keypoint intake off / on (P = 5) at V = 25 and V = 18, written out with pprint.
The ring windows and the signature entries around the two stage entries are the same for every combination of one V and stand
once; at V = 18 joint 24 does not exist and that commit refused the custom joints with the texts of REFUSED."""
import ctypes
import itertools
import types

import pytest

import _bootstrap

pkg = _bootstrap.load()
from continual_skeletons_amd import input_stage, keypoints, ntu_intake  # noqa: E402

RINGS = {18: [('xin0', 3, 36, 4),
      ('y0', 64, 36, 8),
      ('out0', 64, 36, 4),
      ('y1', 64, 36, 8),
      ('out1', 64, 36, 4),
      ('y2', 64, 36, 8),
      ('out2', 64, 36, 4),
      ('y3', 64, 36, 8),
      ('out3', 64, 36, 4),
      ('y4', 128, 36, 8),
      ('out4', 128, 36, 4),
      ('y5', 128, 36, 8),
      ('out5', 128, 36, 4),
      ('y6', 128, 36, 8),
      ('out6', 128, 36, 4),
      ('y7', 256, 36, 8),
      ('out7', 256, 36, 4),
      ('y8', 256, 36, 8),
      ('out8', 256, 36, 4),
      ('y9', 256, 36, 8),
      ('pool', 1, 256, 75)],
 25: [('xin0', 3, 50, 4),
      ('y0', 64, 50, 8),
      ('out0', 64, 50, 4),
      ('y1', 64, 50, 8),
      ('out1', 64, 50, 4),
      ('y2', 64, 50, 8),
      ('out2', 64, 50, 4),
      ('y3', 64, 50, 8),
      ('out3', 64, 50, 4),
      ('y4', 128, 50, 8),
      ('out4', 128, 50, 4),
      ('y5', 128, 50, 8),
      ('out5', 128, 50, 4),
      ('y6', 128, 50, 8),
      ('out6', 128, 50, 4),
      ('y7', 256, 50, 8),
      ('out7', 256, 50, 4),
      ('y8', 256, 50, 8),
      ('out8', 256, 50, 4),
      ('y9', 256, 50, 8),
      ('pool', 1, 256, 75)]}

SIGNATURE_AROUND = {18: ((('graph_convs',
        ('GraphConvolution',
         'GraphConvolution',
         'GraphConvolution',
         'GraphConvolution',
         'GraphConvolution',
         'GraphConvolution',
         'GraphConvolution',
         'GraphConvolution',
         'GraphConvolution',
         'GraphConvolution')),
       ('layers',
        ((3, 64, 1, 9, 4, 'none'),
         (64, 64, 1, 9, 4, 'identity'),
         (64, 64, 1, 9, 4, 'identity'),
         (64, 64, 1, 9, 4, 'identity'),
         (64, 128, 2, 9, 4, 'conv'),
         (128, 128, 1, 9, 4, 'identity'),
         (128, 128, 1, 9, 4, 'identity'),
         (128, 256, 2, 9, 4, 'conv'),
         (256, 256, 1, 9, 4, 'identity'),
         (256, 256, 1, 9, 4, 'identity'))),
       ('input_cvm', (3, 18, 2)),
       ('pool_size', 75),
       ('pool_padding', 19)),
      (('split_k', ((1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1))),
       ('step_precision', ('f32', 'f32', 'f32', 'f32', 'f32', 'f32', 'f32', 'f32', 'f32', 'f32')))),
 25: ((('graph_convs',
        ('GraphConvolution',
         'GraphConvolution',
         'GraphConvolution',
         'GraphConvolution',
         'GraphConvolution',
         'GraphConvolution',
         'GraphConvolution',
         'GraphConvolution',
         'GraphConvolution',
         'GraphConvolution')),
       ('layers',
        ((3, 64, 1, 9, 4, 'none'),
         (64, 64, 1, 9, 4, 'identity'),
         (64, 64, 1, 9, 4, 'identity'),
         (64, 64, 1, 9, 4, 'identity'),
         (64, 128, 2, 9, 4, 'conv'),
         (128, 128, 1, 9, 4, 'identity'),
         (128, 128, 1, 9, 4, 'identity'),
         (128, 256, 2, 9, 4, 'conv'),
         (256, 256, 1, 9, 4, 'identity'),
         (256, 256, 1, 9, 4, 'identity'))),
       ('input_cvm', (3, 25, 2)),
       ('pool_size', 75),
       ('pool_padding', 19)),
      (('split_k', ((1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1))),
       ('step_precision', ('f32', 'f32', 'f32', 'f32', 'f32', 'f32', 'f32', 'f32', 'f32', 'f32'))))}

TAILS = {(18, 'bone', 'default', False): ((('input_modality', 'bone'), ('pre_normalization', (1, 0, 1, 8, 4))),
                                  [('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                  591061),
 (18, 'bone', 'default', True): ((('input_modality', 'bone'), ('pre_normalization', (1, 0, 1, 8, 4))),
                                 [('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                 591061),
 (18, 'bone', 'off', False): ((('input_modality', 'bone'), ('pre_normalization', (0, 0, 1, 8, 4))), [], 591024),
 (18, 'bone', 'off', True): ((('input_modality', 'bone'), ('pre_normalization', (0, 0, 1, 8, 4))), [], 591024),
 (18, 'bone_motion', 'default', False): ((('input_modality', 'bone_motion'), ('pre_normalization', (1, 0, 1, 8, 4))),
                                         [('mod_prev', 1, 108, 1), ('mod_flags', 1, 1, 1), ('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                         591170),
 (18, 'bone_motion', 'default', True): ((('input_modality', 'bone_motion'), ('pre_normalization', (1, 0, 1, 8, 4))),
                                        [('mod_prev', 1, 108, 1), ('mod_flags', 1, 1, 1), ('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                        591170),
 (18, 'bone_motion', 'off', False): ((('input_modality', 'bone_motion'), ('pre_normalization', (0, 0, 1, 8, 4))),
                                     [('mod_prev', 1, 108, 1), ('mod_flags', 1, 1, 1)],
                                     591133),
 (18, 'bone_motion', 'off', True): ((('input_modality', 'bone_motion'), ('pre_normalization', (0, 0, 1, 8, 4))),
                                    [('mod_prev', 1, 108, 1), ('mod_flags', 1, 1, 1)],
                                    591133),
 (18, 'joint', 'default', False): ((('input_modality', 'joint'), ('pre_normalization', (1, 0, 1, 8, 4))),
                                   [('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                   591061),
 (18, 'joint', 'default', True): ((('input_modality', 'joint'), ('pre_normalization', (1, 0, 1, 8, 4))),
                                  [('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                  591061),
 (18, 'joint', 'off', False): ((('input_modality', 'joint'), ('pre_normalization', (0, 0, 1, 8, 4))), [], 591024),
 (18, 'joint', 'off', True): ((('input_modality', 'joint'), ('pre_normalization', (0, 0, 1, 8, 4))), [], 591024),
 (18, 'joint_motion', 'default', False): ((('input_modality', 'joint_motion'), ('pre_normalization', (1, 0, 1, 8, 4))),
                                          [('mod_prev', 1, 108, 1), ('mod_flags', 1, 1, 1), ('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                          591170),
 (18, 'joint_motion', 'default', True): ((('input_modality', 'joint_motion'), ('pre_normalization', (1, 0, 1, 8, 4))),
                                         [('mod_prev', 1, 108, 1), ('mod_flags', 1, 1, 1), ('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                         591170),
 (18, 'joint_motion', 'off', False): ((('input_modality', 'joint_motion'), ('pre_normalization', (0, 0, 1, 8, 4))),
                                      [('mod_prev', 1, 108, 1), ('mod_flags', 1, 1, 1)],
                                      591133),
 (18, 'joint_motion', 'off', True): ((('input_modality', 'joint_motion'), ('pre_normalization', (0, 0, 1, 8, 4))),
                                     [('mod_prev', 1, 108, 1), ('mod_flags', 1, 1, 1)],
                                     591133),
 (25, 'bone', 'custom', False): ((('input_modality', 'bone'), ('pre_normalization', (1, 2, 3, 24, 0))),
                                 [('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                 813437),
 (25, 'bone', 'custom', True): ((('input_modality', 'bone'), ('pre_normalization', (1, 2, 3, 24, 0))),
                                [('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                813437),
 (25, 'bone', 'default', False): ((('input_modality', 'bone'), ('pre_normalization', (1, 0, 1, 8, 4))),
                                  [('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                  813437),
 (25, 'bone', 'default', True): ((('input_modality', 'bone'), ('pre_normalization', (1, 0, 1, 8, 4))),
                                 [('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                 813437),
 (25, 'bone', 'off', False): ((('input_modality', 'bone'), ('pre_normalization', (0, 0, 1, 8, 4))), [], 813400),
 (25, 'bone', 'off', True): ((('input_modality', 'bone'), ('pre_normalization', (0, 0, 1, 8, 4))), [], 813400),
 (25, 'bone_motion', 'custom', False): ((('input_modality', 'bone_motion'), ('pre_normalization', (1, 2, 3, 24, 0))),
                                        [('mod_prev', 1, 150, 1), ('mod_flags', 1, 1, 1), ('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                        813588),
 (25, 'bone_motion', 'custom', True): ((('input_modality', 'bone_motion'), ('pre_normalization', (1, 2, 3, 24, 0))),
                                       [('mod_prev', 1, 150, 1), ('mod_flags', 1, 1, 1), ('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                       813588),
 (25, 'bone_motion', 'default', False): ((('input_modality', 'bone_motion'), ('pre_normalization', (1, 0, 1, 8, 4))),
                                         [('mod_prev', 1, 150, 1), ('mod_flags', 1, 1, 1), ('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                         813588),
 (25, 'bone_motion', 'default', True): ((('input_modality', 'bone_motion'), ('pre_normalization', (1, 0, 1, 8, 4))),
                                        [('mod_prev', 1, 150, 1), ('mod_flags', 1, 1, 1), ('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                        813588),
 (25, 'bone_motion', 'off', False): ((('input_modality', 'bone_motion'), ('pre_normalization', (0, 0, 1, 8, 4))),
                                     [('mod_prev', 1, 150, 1), ('mod_flags', 1, 1, 1)],
                                     813551),
 (25, 'bone_motion', 'off', True): ((('input_modality', 'bone_motion'), ('pre_normalization', (0, 0, 1, 8, 4))),
                                    [('mod_prev', 1, 150, 1), ('mod_flags', 1, 1, 1)],
                                    813551),
 (25, 'joint', 'custom', False): ((('input_modality', 'joint'), ('pre_normalization', (1, 2, 3, 24, 0))),
                                  [('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                  813437),
 (25, 'joint', 'custom', True): ((('input_modality', 'joint'), ('pre_normalization', (1, 2, 3, 24, 0))),
                                 [('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                 813437),
 (25, 'joint', 'default', False): ((('input_modality', 'joint'), ('pre_normalization', (1, 0, 1, 8, 4))),
                                   [('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                   813437),
 (25, 'joint', 'default', True): ((('input_modality', 'joint'), ('pre_normalization', (1, 0, 1, 8, 4))),
                                  [('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                  813437),
 (25, 'joint', 'off', False): ((('input_modality', 'joint'), ('pre_normalization', (0, 0, 1, 8, 4))), [], 813400),
 (25, 'joint', 'off', True): ((('input_modality', 'joint'), ('pre_normalization', (0, 0, 1, 8, 4))), [], 813400),
 (25, 'joint_motion', 'custom', False): ((('input_modality', 'joint_motion'), ('pre_normalization', (1, 2, 3, 24, 0))),
                                         [('mod_prev', 1, 150, 1), ('mod_flags', 1, 1, 1), ('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                         813588),
 (25, 'joint_motion', 'custom', True): ((('input_modality', 'joint_motion'), ('pre_normalization', (1, 2, 3, 24, 0))),
                                        [('mod_prev', 1, 150, 1), ('mod_flags', 1, 1, 1), ('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                        813588),
 (25, 'joint_motion', 'default', False): ((('input_modality', 'joint_motion'), ('pre_normalization', (1, 0, 1, 8, 4))),
                                          [('mod_prev', 1, 150, 1), ('mod_flags', 1, 1, 1), ('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                          813588),
 (25, 'joint_motion', 'default', True): ((('input_modality', 'joint_motion'), ('pre_normalization', (1, 0, 1, 8, 4))),
                                         [('mod_prev', 1, 150, 1), ('mod_flags', 1, 1, 1), ('pn_rot', 1, 36, 1), ('pn_flags', 1, 1, 1)],
                                         813588),
 (25, 'joint_motion', 'off', False): ((('input_modality', 'joint_motion'), ('pre_normalization', (0, 0, 1, 8, 4))),
                                      [('mod_prev', 1, 150, 1), ('mod_flags', 1, 1, 1)],
                                      813551),
 (25, 'joint_motion', 'off', True): ((('input_modality', 'joint_motion'), ('pre_normalization', (0, 0, 1, 8, 4))),
                                     [('mod_prev', 1, 150, 1), ('mod_flags', 1, 1, 1)],
                                     813551)}

REFUSED = {(18, 'bone', 'custom', False): 'xaxis = (24, 0) outside [0, 18): the skeleton has 18 joints',
 (18, 'bone', 'custom', True): 'xaxis = (24, 0) outside [0, 18): the skeleton has 18 joints',
 (18, 'bone_motion', 'custom', False): 'xaxis = (24, 0) outside [0, 18): the skeleton has 18 joints',
 (18, 'bone_motion', 'custom', True): 'xaxis = (24, 0) outside [0, 18): the skeleton has 18 joints',
 (18, 'joint', 'custom', False): 'xaxis = (24, 0) outside [0, 18): the skeleton has 18 joints',
 (18, 'joint', 'custom', True): 'xaxis = (24, 0) outside [0, 18): the skeleton has 18 joints',
 (18, 'joint_motion', 'custom', False): 'xaxis = (24, 0) outside [0, 18): the skeleton has 18 joints',
 (18, 'joint_motion', 'custom', True): 'xaxis = (24, 0) outside [0, 18): the skeleton has 18 joints'}

PRENORM = {"off": None, "default": {}, "custom": dict(zaxis=(2, 3), xaxis=(24, 0))}
GRAPHS = {25: pkg.ntu_graph, 18: pkg.kinetics_graph}


def test_records_of_every_switch_combination_are_the_ones_before_the_chain():
    seen = 0
    for v, mod, pn, kp in itertools.product((25, 18), pkg.modality.MODALITIES, PRENORM, (False, True)):
        net = pkg.CoStGcn(GRAPHS[v]().A, (3, 300, v, 2))
        pkg.set_input_modality(net, mod)
        if kp:
            keypoints.set_keypoint_intake(net, 5)
        if (v, mod, pn, kp) in REFUSED:
            with pytest.raises(ValueError) as err:
                pkg.set_pre_normalization(net, True, **PRENORM[pn])
            assert str(err.value) == REFUSED[(v, mod, pn, kp)] and net.pre_normalization is False
            continue
        if PRENORM[pn] is not None:
            pkg.set_pre_normalization(net, True, **PRENORM[pn])
        signature, windows, floats = TAILS[(v, mod, pn, kp)]
        assert net.move_signature() == SIGNATURE_AROUND[v][0] + signature + SIGNATURE_AROUND[v][1], (v, mod, pn, kp)
        assert net._move_windows() == RINGS[v] + windows and net.record_floats() == floats, (v, mod, pn, kp)
        names = [w[0] for w in windows]
        assert names == [n for n in ("mod_prev", "mod_flags", "pn_rot", "pn_flags") if n in names]      # the trailing order
        seen += 1
    assert seen == len(TAILS) == 40 and len(REFUSED) == 8


def _models():
    a25, a18 = pkg.ntu_graph().A, pkg.kinetics_graph().A
    return [pkg.StGcn(a25, (3, 20, 25, 2)), pkg.AGcn(a18, (3, 20, 18, 2)), pkg.STr(a25, (3, 20, 25, 2)),
            pkg.CoStGcn(a25, (3, 300, 25, 2)), pkg.CoAGcn(a18, (3, 300, 18, 2)), pkg.CoSTr(a25, (3, 300, 25, 2))]


def test_the_chain_order_is_one_tuple_intakes_first():
    for net in _models():
        names = [stage.name for stage in net.stages]
        clip_only = [] if isinstance(net, pkg.CoStGcn) else ["ntu"]
        assert names == clip_only + ["keypoints", "prenorm", "modality"]
        assert [type(stage) for stage in net.stages] == list(type(net).STAGES)
        assert [stage.intake for stage in net.stages] == [True] * (len(names) - 2) + [False, False]
        assert all(net.stage(stage.name) is stage and isinstance(stage, input_stage.InputStage) for stage in net.stages)
        # state stands in records in the order the first records had it: the modality's in front of the pre-normalisation's
        assert [stage.name for stage in net._record_stages][:2] == ["modality", "prenorm"]


def test_a_stage_that_is_off_hands_back_the_object_it_was_given():
    for net in _models():
        x, cycle = object(), [object(), object()]           # off means untouched: not even looked at
        for stage in net.stages:
            assert stage.enabled is False and stage.clip(x) is x and stage.clip_as_stepped(x) is x
            assert stage.frames(cycle) is cycle and stage.frames(cycle, update=False) is cycle
            stage.bind(3, "cpu", 4)
            assert stage.scratch is None and stage.flags is None and stage.state() == [] and stage.reset_jobs() == []
            assert stage.windows() == [] and stage.prime(x, 8) == {}
        assert net._intake_clip(x) is x and net._prepare_clip(x) is x and net._stage_frames(cycle) is cycle
        assert net._stage_frames(cycle, update=False) is cycle and net._fed() is net._plain
        assert (net.input_modality, net.pre_normalization, net.keypoint_intake, net.ntu_intake, net.time_axis) == ("joint", False, False, False, 2)


def _stepped(frames):
    net = pkg.CoStGcn(pkg.ntu_graph().A)
    net._ctr = (ctypes.c_int64 * 22)()
    net._n, net._xin0 = 2, types.SimpleNamespace(device="cpu")     # stands for a bound slab (binding needs a device)
    net.bound = []
    for stage in net.stages:
        stage.bind = lambda n, device, max_cycle, name=stage.name: net.bound.append((name, n, device, max_cycle))
    net._frames = frames
    return net


SETTERS = {
    "modality": (lambda target: pkg.set_input_modality(target, "bone"), "input modality", "joint", "bone"),
    "prenorm": (lambda target: pkg.set_pre_normalization(target, xaxis=(9, 5)), "pre-normalisation",
                (False, (0, 1, 8, 4)), (True, (0, 1, 9, 5))),
    "keypoints": (lambda target: keypoints.set_keypoint_intake(target, 6), "keypoint intake", (False, 5), (True, 6)),
}


@pytest.mark.parametrize("name", sorted(SETTERS))
def test_the_shared_setter_switches_no_shard_when_the_second_refuses(name):
    switch, what, before, after = SETTERS[name]
    shards = object.__new__(pkg.parallel.StreamShards)
    shards.models = [_stepped(0), _stepped(8)]
    with pytest.raises(RuntimeError) as err:
        switch(shards)
    assert str(err.value) == f"a shard has stepped: call clean_state() on every shard model before changing the {what}"
    assert [m.stage(name).settings for m in shards.models] == [before, before] and not shards.models[0].bound
    shards.models = [_stepped(0), pkg.GraphConvolution(3, 8, pkg.ntu_graph().A)]
    with pytest.raises(TypeError) as err:
        switch(shards)
    assert str(err.value) == f"GraphConvolution has no {what}" and shards.models[0].stage(name).settings == before
    shards.models = [_stepped(0), _stepped(0)]
    assert switch(shards) is shards and [m.stage(name).settings for m in shards.models] == [after, after]
    assert [m.bound for m in shards.models] == [[(name, 2, "cpu", 8)]] * 2       # a bound slab: that stage alone is re-bound
    single = _stepped(8)
    with pytest.raises(RuntimeError, match=rf"^the model has stepped 8 frames .*call clean_state\(\) before changing the {what}$"):
        switch(single)
    assert single.stage(name).settings == before and not single.bound


def test_a_stepped_model_refuses_before_the_parent_table_is_looked_up():
    """As before the chain: the "has stepped" refusal comes in front of the bone modes' missing-skeleton error."""
    def odd(frames):
        net = _stepped(frames)
        net.stage("modality").shape = (3, 300, 20, 2)       # a skeleton without a parent table
        net.input_shape = (3, 300, 20, 2)
        return net
    with pytest.raises(RuntimeError, match=r"clean_state\(\)"):
        pkg.set_input_modality(odd(8), "bone")
    with pytest.raises(ValueError, match="no bone parent table"):
        pkg.set_input_modality(odd(0), "bone")
    shards = object.__new__(pkg.parallel.StreamShards)
    shards.models = [_stepped(0), odd(8)]
    with pytest.raises(RuntimeError, match="a shard has stepped"):
        pkg.set_input_modality(shards, "bone")
    assert [m.input_modality for m in shards.models] == ["joint", "joint"]


def test_one_intake_per_model_from_both_directions():
    for net in _models()[:3]:
        ntu_intake.set_ntu_intake(net)
        with pytest.raises(ValueError) as err:
            keypoints.set_keypoint_intake(net)
        assert str(err.value) == ("the NTU intake is on: a model runs one intake, switch it off first "
                                  "(ntu_intake.set_ntu_intake(model, enabled=False))")
        assert net.ntu_intake is True and net.keypoint_intake is False and net._fed() is net.stage("ntu")
        keypoints.set_keypoint_intake(net, enabled=False)       # switching the other one off is no conflict
        ntu_intake.set_ntu_intake(net, enabled=False)
        keypoints.set_keypoint_intake(net)
        with pytest.raises(ValueError) as err:
            ntu_intake.set_ntu_intake(net)
        assert str(err.value) == ("the keypoint intake is on: a model runs one intake, switch it off first "
                                  "(keypoints.set_keypoint_intake(model, enabled=False))")
        assert net.keypoint_intake is True and net.ntu_intake is False and net._fed() is net.stage("keypoints") and net.time_axis == 1
