"""CPU tests of the S-TR / CoS-TR layer: the restatement against the reference's fixtures (G11, G12), state_dict layouts,
the folded operands of csk_str_unit_f32, loud refusals of flags and arguments that are not built."""
import ctypes

import numpy as np
import pytest
import torch

import _bootstrap
from closed_form import closed_form_input
from oracle import stgcn_oracle as o
from tests import str_oracle as so
from tests.helpers import load_golden, model_fixture

pkg = _bootstrap.load()
G11 = ("eq25", "neq25", "eq18", "neq18")


def g11(tag):
    a, sd = load_golden(f"g11_str_unit_{tag}")
    ci, co, v, salt = (int(u) for u in a["meta"])
    x = torch.from_numpy(closed_form_input((2, ci, 6, v), salt=float(salt)) * 2 - 1)
    return a, sd, x, ci, co, v


def _graph(v):
    return pkg.ntu_graph().A if v == 25 else pkg.kinetics_graph().A


@pytest.mark.parametrize("tag", G11)
def test_oracle_reproduces_reference_unit(tag):
    a, sd, x, *_ = g11(tag)
    with torch.no_grad():
        y = so.str_unit(x, sd, "")
    assert float((y - torch.from_numpy(a["y"])).abs().max()) <= 1e-6


@pytest.mark.parametrize("tag", ["ntu", "kin"])
def test_oracle_reproduces_reference_str(tag):
    arrays, sd, x = model_fixture(f"g12_str_{tag}", 25 if tag == "ntu" else 18)
    with torch.no_grad():
        logits = o.stgcn_forward(x, sd, gcn=so.gcn)
    assert float((logits - torch.from_numpy(arrays["logits"])).abs().max()) <= 1e-5


@pytest.mark.parametrize("tag", G11)
def test_unit_state_dict_matches_reference(tag):
    a, sd, x, ci, co, v = g11(tag)
    m = pkg.GcnUnitAttention(ci, co, _graph(v), num_point=v)
    assert list(m.state_dict().keys()) == list(sd.keys())
    m.load_state_dict(sd, strict=True)
    back = {k: t.clone() for k, t in m.state_dict().items()}
    m2 = pkg.GcnUnitAttention(ci, co, _graph(v), num_point=v)
    m2.load_state_dict(back, strict=True)
    for k in sd:
        assert torch.equal(m2.state_dict()[k], sd[k]), k


@pytest.mark.parametrize("tag", ["ntu", "kin"])
def test_model_state_dicts_match_reference(tag):
    v = 25 if tag == "ntu" else 18
    arrays, sd, _ = model_fixture(f"g12_str_{tag}", v)
    shape = (3, 300, v, 2)
    classes = 60 if tag == "ntu" else 400
    net = pkg.STr(_graph(v), shape, classes)
    assert list(net.state_dict().keys()) == [str(k) for k in arrays["sd_keys"]]
    assert [str(list(t.shape)) for t in net.state_dict().values()] == [str(s) for s in arrays["sd_shapes"]]
    net.load_state_dict(sd, strict=True)
    assert sum(p.numel() for p in net.parameters()) == int(arrays["nparams"])
    # CoSTr: continual key layout (0.1. / 0.0.residual), regular STr keys map onto it, and back
    co = pkg.CoSTr(_graph(v), shape, classes)
    mapped = co.map_state_dict(sd, strict=True)
    co.load_state_dict(mapped, strict=True)
    assert "layers.layer5.0.1.gcn.attention_conv.qkv_conv.weight" in co.state_dict()
    assert "layers.layer5.0.0.residual.t_conv.weight" in co.state_dict()
    short = {k.replace("0.1.", "").replace("0.0.residual", "residual"): t for k, t in co.state_dict().items()}
    assert set(short) == set(sd)
    net2 = pkg.STr(_graph(v), shape, classes)
    net2.load_state_dict(short, strict=True)
    assert all(torch.equal(net2.state_dict()[k], sd[k]) for k in sd)
    assert isinstance(co.layers.layer4.gcn, pkg.GcnUnitAttention) and type(co.layers.layer3.gcn) is pkg.GraphConvolution
    assert co.layers.layer4.gcn.num == 0.1           # the reference passes bn_momentum positionally as ``num`` (cos_tr.py:25-28)


def test_load_pretrained_maps_costr_checkpoints(tmp_path):
    arrays, sd, _ = model_fixture("g12_str_ntu", 25)
    path = str(tmp_path / "str.pt")
    torch.save(sd, path)
    co = pkg.CoSTr(_graph(25))
    pkg.load_pretrained(co, path)
    for k, t in co.state_dict().items():
        assert torch.equal(t, sd[k.replace("0.1.", "").replace("0.0.residual", "residual")]), k


def test_per_layer_graph_conv_leaves_the_default_stacks_alone():
    A = pkg.ntu_graph().A
    for net in (pkg.StGcn(A), pkg.CoStGcn(A)):
        assert all(type(net.layers[f"layer{i}"].gcn) is pkg.GraphConvolution for i in range(1, 11))
    s = pkg.STr(A)
    assert [type(s.layers[f"layer{i}"].gcn).__name__ for i in range(1, 11)] == ["GraphConvolution"] * 3 + ["GcnUnitAttention"] * 7
    with pytest.raises(ValueError):
        pkg.StGcn(A, GraphConv=[None] * 9)


@pytest.mark.parametrize("tag", G11)
def test_folded_operands_reproduce_reference_unit(tag):
    """data_bn affine, q scale, BN fold and skip of GcnUnitAttention._fold, recomputed in fp64 by torch."""
    a, sd, x, ci, co, v = g11(tag)
    m = pkg.GcnUnitAttention(ci, co, _graph(v), num_point=v).eval()
    m.load_state_dict(sd, strict=True)
    ops = m._fold()
    assert (ops["res_scale"] is not None) == (ci == co)
    assert ops["w_qkv"].shape == (ci, -(-(2 * ops["dk"] + ops["dv"]) // 64) * 64)
    assert float(ops["w_qkv"][:, 2 * ops["dk"] + ops["dv"]:].abs().sum()) == 0.0
    y = so.folded_unit(x, ops)
    assert float((y - torch.from_numpy(a["y"])).abs().max()) <= 2e-6


def test_fold_cache_refolds_on_weight_edit():
    m = pkg.GcnUnitAttention(32, 32, pkg.ntu_graph().A).eval()
    ops = m._packed_ops("cpu")
    with torch.no_grad():
        m.bn.weight.mul_(2)
    ops2 = m._packed_ops("cpu")
    assert ops2 is not ops and torch.allclose(ops2["res_scale"], 2 * ops["res_scale"])


@pytest.mark.parametrize("flag,value", [("relative", True), ("adjacency", True), ("more_channels", True),
                                        ("only_attention", False), ("data_normalization", False), ("skip_conn", False),
                                        ("bn_flag", False), ("kernel_size", 3), ("stride", 2), ("Nh", 4),
                                        ("dk_factor", 0.5)])
def test_unsupported_flags_raise(flag, value):
    with pytest.raises(NotImplementedError):
        pkg.GcnUnitAttention(64, 64, pkg.ntu_graph().A, **{flag: value})


def test_unit_forward_refuses_cpu_tensors():
    m = pkg.GcnUnitAttention(32, 32, pkg.ntu_graph().A).eval()
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 32, 2, 25))


def test_str_unit_entry_rejects_bad_arguments_without_a_gpu():
    lib = pkg.native.lib()
    fake = ctypes.c_void_p(1 << 20)           # never dereferenced: every call below fails validation before any launch

    def call(x=fake, scratch=fake, floats=1 << 40, res=fake, n_seg=2, c_in=64, c_out=64, frames=4, V=25, xc=100, yc=100):
        return lib.csk_str_unit_f32(x, fake, scratch, floats, fake, fake, fake, fake, fake, fake, res, n_seg, c_in, c_out,
                                    frames, V, c_in * xc, xc, c_out * yc, yc, None)

    assert call(x=None) == -1
    assert call(n_seg=0) == -1
    assert call(V=20) == -2 and b"V in {18, 25}" in lib.csk_last_error()
    assert call(c_out=48, c_in=48) == -2
    assert call(c_out=512, c_in=512) == -2
    assert call(c_in=24, res=None) == -2
    assert call(c_in=32, c_out=64) == -1                      # skip scale with C_in != C_out
    assert call(xc=99) == -1                                  # channel stride shorter than frames * V
    assert call(floats=100) == -1 and b"scratch" in lib.csk_last_error()
    assert call(scratch=None) == -1
