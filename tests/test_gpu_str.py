"""GPU parity of the S-TR spatial-attention unit (csk_str_unit_f32) and the STr / CoSTr drivers: golden vectors from the
reference's GcnUnitAttention (G11) and STr (G12), the CPU restatement (tests/str_oracle.py) at the real channel pairs,
the continual ring layout, CoSTr stepping and the clip latency mode.  Tolerance 1e-4 absolute."""
import pytest
import torch

import _bootstrap
from closed_form import closed_form_input
from oracle import stgcn_oracle as o
from tests import str_oracle as so
from tests.helpers import check_parity, load_golden, model_fixture, randomise_unit_

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
DEV = "cuda:0"


def _graph(v):
    return pkg.ntu_graph().A if v == 25 else pkg.kinetics_graph().A


@pytest.mark.parametrize("tag", ["eq25", "neq25", "eq18", "neq18"])
def test_unit_golden(tag):
    a, sd = load_golden(f"g11_str_unit_{tag}")
    ci, co, v, salt = (int(u) for u in a["meta"])
    x = torch.from_numpy(closed_form_input((2, ci, 6, v), salt=float(salt)) * 2 - 1)
    m = pkg.GcnUnitAttention(ci, co, _graph(v), num_point=v).eval()
    m.load_state_dict(sd, strict=True)
    y = m.to(DEV)(x.to(DEV)).cpu()
    check_parity(y, a["y"], note=f"G11 {tag}")


def _unit(ci, co, v, seed):
    m = pkg.GcnUnitAttention(ci, co, _graph(v), num_point=v).eval()
    randomise_unit_(m, seed)
    with torch.no_grad():                    # larger q / k weights: a peaked, non-uniform attention
        m.attention_conv.qkv_conv.weight.mul_(3.0)
    return m


# (C_in, C_out, T, V): the STr layer pairs; frames * V leaves a last column tile of 1 column (41 * 25 = 4 * 256 + 1),
# 28 columns (30 * 18) and 119 columns (15 * 25 = 375)
@pytest.mark.parametrize("ci,co,t,v", [(64, 64, 300, 25), (64, 128, 41, 25), (128, 128, 30, 18), (128, 256, 15, 25),
                                       (256, 256, 75, 25)])
def test_unit_vs_restatement_real_channels(ci, co, t, v):
    m = _unit(ci, co, v, seed=ci + co + t)
    g = torch.Generator().manual_seed(t)
    x = torch.rand((2, ci, t, v), generator=g) * 2 - 1
    sd = {k: t_.clone() for k, t_ in m.state_dict().items()}
    with torch.no_grad():
        want = so.str_unit(x, sd, "")
    y = m.to(DEV)(x.to(DEV)).cpu()
    check_parity(y, want, note=f"unit {ci}->{co} T={t} V={v}")


@pytest.mark.parametrize("ci,co,v", [(64, 64, 25), (128, 256, 18)])
def test_stage_on_ring_slots_equals_clip_form(ci, co, v):
    """The continual layout: ring slots (S, C, P), P > N V, frames = skeletons, a run of slots per launch."""
    m = _unit(ci, co, v, seed=7).to(DEV)
    n, s = 6, 5
    x = torch.rand((n, ci, s, v), generator=torch.Generator().manual_seed(3)).to(DEV) * 2 - 1
    clip = m(x)                                                                     # (n, co, s, v)
    p = (n * v + 3) // 4 * 4 + 4
    ring = torch.full((s, ci, p), float("nan"), device=DEV)
    ring[:, :, : n * v] = x.permute(2, 1, 0, 3).reshape(s, ci, n * v)
    yr = torch.full((s, co, p), float("nan"), device=DEV)
    m.stage(ring[0], yr[0], n_seg=3, frames=n, x_strides=(ci * p, p), y_strides=(co * p, p))
    m.stage(ring[3], yr[3], n_seg=2, frames=n, x_strides=(ci * p, p), y_strides=(co * p, p))
    got = yr[:, :, : n * v].reshape(s, co, n, v).permute(2, 1, 0, 3).cpu()
    check_parity(got, clip.cpu(), tol=1e-6, note="ring slots vs clip")
    assert torch.equal(got, clip.cpu())            # the K order per column is fixed: a column does not depend on its place
    assert torch.isnan(yr[:, :, n * v:]).all()                                     # nothing written past frames * V


@pytest.mark.parametrize("tag", ["ntu", "kin"])
def test_str_golden(tag):
    v = 25 if tag == "ntu" else 18
    arrays, sd, x = model_fixture(f"g12_str_{tag}", v)
    net = pkg.STr(_graph(v), (3, 300, v, 2), 60 if tag == "ntu" else 400).eval()
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV)
    taps = {}
    hooks = [net.layers[f"layer{i}"].register_forward_hook(lambda mod, inp, out, i=i: taps.__setitem__(i, out)) for i in (1, 5, 8, 10)]
    logits = net(x.to(DEV)).cpu()
    for h in hooks:
        h.remove()
    for i in (1, 5, 8, 10):
        check_parity(taps[i].cpu().reshape(-1)[::997], arrays[f"layer{i}_sub"], note=f"STr {tag} layer{i}")
    check_parity(logits, arrays["logits"], note=f"STr {tag} logits")


def test_str_latency_mode_batch1():
    arrays, sd, x = model_fixture("g12_str_ntu", 25)
    net = pkg.STr(_graph(25)).eval()
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV)
    base = net(x.to(DEV)).cpu()
    net.set_latency_mode(4)
    got = net(x[:1].to(DEV)).cpu()
    check_parity(got, arrays["logits"], note="STr latency mode batch 1")
    check_parity(got, base, note="STr latency vs default")
    net.set_latency_mode(0)


def test_costr_forward_steps_pad_end_never_reaches_foreign_stage(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("CoSTr reached _foreign_gcn_stage")
    monkeypatch.setattr(pkg.CoSpatioTemporalBlock, "_foreign_gcn_stage", boom)
    arrays, sd, x = model_fixture("g12_str_ntu", 25)
    x = x[:1, :, :48].contiguous()
    co = pkg.CoSTr(_graph(25), pool_size=6, pool_padding=2).eval()
    co.load_state_dict(co.map_state_dict(sd), strict=True)
    co = co.to(DEV)
    with torch.no_grad():
        want = o.co_stgcn_steps_pad_end(x, sd, 6, 2, gcn=so.gcn)
    got = co.forward_steps(x.to(DEV), pad_end=True).cpu()
    assert "_plan" not in co.__dict__                                              # the Python step engine
    assert got.shape == want.shape
    check_parity(got, want, note="CoSTr pad_end")


def test_continual_block_with_unit_vs_block_oracle():
    """One CoSpatioTemporalBlock with the unit as CoGraphConv, stepped frame by frame, against CoBlockOracle(gcn=...)."""
    blk = pkg.CoSpatioTemporalBlock(64, 64, _graph(25), padding="equal",
                                    CoGraphConv=lambda ci, co, A, bn_momentum=0.1: pkg.GcnUnitAttention(ci, co, A, bn_momentum)).eval()
    randomise_unit_(blk, 11)
    sd = {k.replace("0.1.", ""): t.clone() for k, t in blk.state_dict().items()}
    x = torch.rand((3, 64, 14, 25), generator=torch.Generator().manual_seed(5)) * 2 - 1
    with torch.no_grad():
        want = o.CoBlockOracle(sd, "", 1, True, padding=4, gcn=so.gcn).forward_steps(x, pad_end=True)
    got = blk.to(DEV).forward_steps(x.to(DEV), pad_end=True).cpu()
    check_parity(got, want, note="CoSpatioTemporalBlock + unit")
