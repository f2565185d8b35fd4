"""CPU tests of the host layer: C-ABI symbols, state_dict layouts, folding arithmetic, loud failures."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _bootstrap
from oracle import stgcn_oracle as o
from tests.helpers import load_golden

pkg = _bootstrap.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "cskel.h")).read()
    declared = set(re.findall(r"\b(csk_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed from include/cskel.h"
    lib = ctypes.CDLL(pkg.native.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in cskel.h but not exported"
    assert declared - {"csk_last_error"} == set(pkg.native.SIGNATURES), "ctypes table out of sync with cskel.h"
    assert pkg.native.lib().csk_abi_version() == pkg.native.ABI_VERSION == 16


def test_argument_errors_do_not_need_a_gpu():
    lib = pkg.native.lib()
    rc = lib.csk_tcn_stage_f32(None, None, None, None, None, None, 1, 1, 1, 1, 25, 9, 1, 4, 0, 0, 0, 0, 1, None)
    assert rc == -1 and b"null pointer" in lib.csk_last_error()
    with pytest.raises(RuntimeError, match="null pointer"):
        pkg.native.check(rc, "csk_tcn_stage_f32")


def test_graph_matches_reference_fixture():
    a, _ = load_golden("g0_graphs")
    assert np.array_equal(pkg.ntu_graph().A, a["ntu"]) and np.array_equal(pkg.kinetics_graph().A, a["kinetics"])


def test_state_dict_layouts_match_reference():
    A = pkg.ntu_graph().A
    _, sd = load_golden("g3_block_strided")           # dumped from the reference's SpatioTemporalBlock
    blk = pkg.SpatioTemporalBlock(2, 4, A, stride=2)
    assert list(blk.state_dict().keys()) == list(sd.keys())
    assert all(blk.state_dict()[k].shape == v.shape for k, v in sd.items())
    blk.load_state_dict(sd, strict=True)
    # continual container layouts (tests/test_cost_gcn.py:97-98,145,193-198)
    co = pkg.CoSpatioTemporalBlock(2, 4, A, stride=2, padding=4)
    keys = set(co.state_dict().keys())
    assert {"0.0.residual.t_conv.weight", "0.1.gcn.g_conv.0.weight", "0.1.tcn.bn.running_var"} <= keys
    assert not any(k.startswith(("gcn.", "tcn.", "residual.")) for k in keys)
    mapping = {"res": "0.0.", "gcn": "0.1.", "tcn": "0.1."}
    co.load_state_dict({mapping[k[:3]] + k: v for k, v in sd.items()}, strict=True)    # reference Co layout
    co.load_state_dict(sd, strict=True)                                                # plain layout
    ident = pkg.CoSpatioTemporalBlock(4, 4, A, padding=4)
    assert all(k.startswith("0.1.") for k in ident.state_dict())
    nores = pkg.CoSpatioTemporalBlock(4, 4, A, residual=False, padding=4)
    assert all(k.startswith(("gcn.", "tcn.")) for k in nores.state_dict())
    assert (co.delay, co.receptive_field, co.stride, co.padding) == (4, 9, 2, 4)
    assert pkg.CoSpatioTemporalBlock(4, 4, A).delay == 8                               # padding=0 default


def test_costgcn_keys_and_map_state_dict():
    A = pkg.ntu_graph().A
    reg, co = pkg.StGcn(A), pkg.CoStGcn(A)
    assert "layers.layer2.0.1.gcn.g_conv.0.weight" in co.state_dict()
    assert "layers.layer8.0.0.residual.t_conv.weight" in co.state_dict()
    assert "layers.layer1.gcn.bn.weight" in co.state_dict()
    mapped = co.map_state_dict(reg.state_dict())
    assert set(mapped) == set(co.state_dict())
    co.load_state_dict(mapped, strict=True)
    co.load_state_dict(reg.state_dict(), strict=True)      # regular layout loads directly as well
    assert (co.receptive_field, co.padding, co.stride, co.pool_size, co.pool_padding) == (153, 76, 4, 75, 19)


def test_costgcn_key_map_matches_the_reference_fixture():
    """G9 (tests/golden/make_golden.py): the continual key layout and the output of the reference's own
    CoModelBase.map_state_dict (models/base.py:200-224, executed unbound on a stub with that layout) on the reference
    StGcn's keys.  CoStGcn must expose the same keys in the same order and map a regular state dict the same way:
    strict, non-strict (unknown keys dropped) and already-continual (returned as is)."""
    import numpy as np
    d = np.load(os.path.join(ROOT, "tests", "golden", "g9_key_map.npz"))
    regular, co_keys = [str(k) for k in d["regular_keys"]], [str(k) for k in d["co_keys"]]
    net = pkg.CoStGcn(pkg.ntu_graph().A)
    assert list(net.state_dict().keys()) == co_keys
    assert list(pkg.StGcn(pkg.ntu_graph().A).state_dict().keys()) == regular
    sd = {k: i for i, k in enumerate(regular)}
    strict = net.map_state_dict(dict(sd), strict=True)
    assert list(strict.keys()) == [str(k) for k in d["mapped_strict_keys"]] and list(strict.values()) == list(d["mapped_strict_pos"])
    loose = net.map_state_dict(dict(sd, **{"not.a.key": -1}), strict=False)
    assert list(loose.keys()) == [str(k) for k in d["mapped_loose_keys"]] and list(loose.values()) == list(d["mapped_loose_pos"])
    with pytest.raises(KeyError):                                   # the reference raises on an unknown key when strict
        net.map_state_dict(dict(sd, **{"not.a.key": -1}), strict=True)
    same = net.map_state_dict({k: i for i, k in enumerate(co_keys)}, strict=True)
    assert list(same.keys()) == [str(k) for k in d["mapped_same_keys"]] == co_keys


def test_load_pretrained_pt_and_ckpt(tmp_path):
    """Weight import path: a regular ST-GCN state dict saved as .pt, or inside a Lightning-style
    .ckpt, loads into StGcn and -- through map_loaded_weights (models/base.py:226-227) -- into CoStGcn; a state
    dict already in the continual layout passes through unchanged; junk files are refused."""
    import torch
    A = pkg.ntu_graph().A
    src = pkg.StGcn(A)
    with torch.no_grad():
        for prm in src.parameters():
            prm.add_(0.01)
    pt, ckpt, junk = tmp_path / "w.pt", tmp_path / "w.ckpt", tmp_path / "junk.pt"
    torch.save(src.state_dict(), pt)
    torch.save({"state_dict": src.state_dict(), "epoch": 3}, ckpt)
    torch.save([1, 2, 3], junk)
    reg, co = pkg.StGcn(A), pkg.CoStGcn(A)
    pkg.load_pretrained(reg, str(pt))
    pkg.load_pretrained(co, str(ckpt))
    want = src.state_dict()
    assert all(torch.equal(v, want[k]) for k, v in reg.state_dict().items())
    short = lambda k: k.replace("0.1.", "").replace("0.0.residual", "residual")  # noqa: E731
    assert all(torch.equal(v, want[short(k)]) for k, v in co.state_dict().items())
    assert co.map_loaded_weights(str(pt), co.state_dict()) is not None
    same = co.state_dict()
    assert co.map_state_dict(same) is same                      # already in the continual layout: unchanged
    extra = dict(src.state_dict(), not_a_key=torch.zeros(1))
    torch.save(extra, pt)
    with pytest.raises((RuntimeError, KeyError)):
        pkg.load_pretrained(pkg.CoStGcn(A), str(pt))            # strict: unexpected key
    res = pkg.load_pretrained(pkg.CoStGcn(A), str(pt), strict=False)
    assert not res.missing_keys
    with pytest.raises(RuntimeError, match="not a state dict"):
        pkg.load_pretrained(reg, str(junk))


def test_fold_reproduces_oracle_pointwise():
    """Evaluate the PACKED operands with plain numpy (test-only) and compare with the oracle."""
    a, sd = load_golden("g3_block_strided")
    f = pkg.fold.fold_graph_conv(sd, "gcn.")
    x = torch.from_numpy(a["x"]).double()
    n, ci, t, v = x.shape
    a_eff = (sd["gcn.A"] * sd["gcn.graph_attn"]).double()
    # ELL round trip
    dense = torch.zeros(3, v, v, dtype=torch.float64)
    for i in range(3):
        for w in range(v):
            for e in range(int(f["ell_cnt_host"][i])):
                dense[i, int(f["ell_src"][i, w, e]), w] += float(f["ell_val"][i, w, e])
    assert torch.allclose(dense, a_eff.float().double())
    xa = [torch.einsum("nctv,vw->nctw", x, a_eff[i]) for i in range(3)] + [x]
    y = sum(torch.einsum("nctw,co->notw", xa[r], f["w"][r, :ci, : f["c_out"]].double()) for r in range(4))
    y = torch.relu(y + f["bias"][: f["c_out"]].double()[None, :, None, None])
    with torch.no_grad():
        want = o.graph_conv(torch.from_numpy(a["x"]), sd, "gcn.")
    assert float((y - want.double()).abs().max()) < 1e-5


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: no module of the product package may import or execute it."""
    import ast
    pkg_dir = os.path.join(ROOT, "continual-skeletons_amd")
    for fn in os.listdir(pkg_dir):
        if not fn.endswith(".py"):
            continue
        tree = ast.parse(open(os.path.join(pkg_dir, fn)).read())
        for node in ast.walk(tree):
            mods = []
            if isinstance(node, ast.Import):
                mods = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                mods = [node.module or ""]
            assert not any(m.split(".")[0] == "oracle" for m in mods), f"{fn} imports the oracle"


def _oracle_imports(path):
    """(enclosing top-level function or None, module) for every import of the oracle in a source file."""
    import ast
    tree = ast.parse(open(path).read())
    found = []
    for top in tree.body:
        owner = top.name if isinstance(top, (ast.FunctionDef, ast.ClassDef)) else None
        for node in ast.walk(top):
            mods = [a.name for a in node.names] if isinstance(node, ast.Import) else \
                   [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            found += [(owner, m) for m in mods if m.split(".")[0] == "oracle"]
    return found


def test_oracle_is_only_used_as_checker_or_cpu_baseline():
    """Outside tests/ the oracle may be touched by bench.py's cpu_baseline leg and __graft_entry__.smoke() only;
    the tools never use it."""
    assert {o for o, _ in _oracle_imports(os.path.join(ROOT, "bench.py"))} <= {"cpu_baseline_clip", "cpu_baseline_step"}
    assert {o for o, _ in _oracle_imports(os.path.join(ROOT, "__graft_entry__.py"))} <= {"smoke", "build"}
    tools = os.path.join(ROOT, "tools")
    for fn in os.listdir(tools):
        if fn.endswith(".py"):
            assert not _oracle_imports(os.path.join(tools, fn)), f"tools/{fn} imports the oracle"
    assert not _oracle_imports(os.path.join(ROOT, "_bootstrap.py"))


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(pkg.native, "_lib", None)
    monkeypatch.setattr(pkg.native, "LIB_PATH", "/nonexistent/libcskel_hip.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.native.lib()


class _ForeignHparams:                                       # stands for Ride's AttributeDict & co. in a Lightning checkpoint
    def __init__(self):
        self.learning_rate = 0.1


def test_lightning_style_checkpoint_with_hparams(tmp_path):
    """a real Lightning / Ride .ckpt carries `hyper_parameters` objects.  argparse.Namespace loads under the
    safe unpickler; any other class is refused with a message that says what to do; trusted=True loads it."""
    import argparse

    import torch
    A = pkg.ntu_graph().A
    src = pkg.StGcn(A)
    ns, foreign = tmp_path / "ns.ckpt", tmp_path / "foreign.ckpt"
    torch.save({"state_dict": src.state_dict(), "hyper_parameters": argparse.Namespace(graph="ntu_rgbd", lr=0.1)}, ns)
    torch.save({"state_dict": src.state_dict(), "hyper_parameters": _ForeignHparams()}, foreign)
    pkg.load_pretrained(pkg.CoStGcn(A), str(ns))
    with pytest.raises(RuntimeError, match="trusted=True"):
        pkg.load_pretrained(pkg.CoStGcn(A), str(foreign))
    pkg.load_pretrained(pkg.CoStGcn(A), str(foreign), trusted=True)


def test_fusion_file_loaders(tmp_path):
    """.npy prediction arrays and the pickled (names, labels) label file of scripts/multi_stream_eval.py:16-31."""
    import pickle

    import numpy as np
    from continual_skeletons_amd import fusion
    np.save(tmp_path / "p.npy", np.zeros((3, 5), dtype=np.float32))
    np.save(tmp_path / "bad.npy", np.zeros((3,), dtype=np.float32))
    (tmp_path / "l.pkl").write_bytes(pickle.dumps((["a", "b", "c"], [4, 0, 2]), protocol=2))
    assert fusion.load_preds(tmp_path / "p.npy").shape == (3, 5)
    assert fusion.load_labels(tmp_path / "l.pkl").tolist() == [4, 0, 2]
    # a label file is plain lists of str / int: anything that needs a global (here: os.system) is refused, not executed
    (tmp_path / "evil.pkl").write_bytes(b"cos\nsystem\n(S'true'\ntR.")
    with pytest.raises(pickle.UnpicklingError, match="refusing"):
        fusion.load_labels(tmp_path / "evil.pkl")
    (tmp_path / "np.pkl").write_bytes(pickle.dumps((["a"], np.array([3])), protocol=2))
    with pytest.raises(pickle.UnpicklingError):
        fusion.load_labels(tmp_path / "np.pkl")
    assert fusion.load_labels(tmp_path / "np.pkl", trusted=True).tolist() == [3]
    with pytest.raises(ValueError):
        fusion.load_preds(tmp_path / "bad.npy")
    with pytest.raises(ValueError):
        fusion.load_preds(tmp_path / "p.txt")
    with pytest.raises(FileNotFoundError):
        fusion.load_preds(tmp_path / "missing.npy")


def test_co_block_step_argument_errors_are_reported_without_a_gpu():
    """csk_co_block_step_f32 validates its arguments before it touches the device: bad geometry comes back as a
    negative return code with a message (no launch, so this runs on the CPU-only container)."""
    import ctypes as C
    lib = pkg.native.lib()
    fake = C.c_void_p(0x1000)                    # non-null, 16-byte aligned; never dereferenced on these paths
    cnt = (C.c_int32 * 3)(1, 1, 4)

    def call(c_in=64, c_out=64, y_slots=16, V=25, P=200, n_skel=8, res_mode=1, gcn_res=1, cnt_=cnt):
        return lib.csk_co_block_step_f32(fake, 16, 0, c_in, fake, fake, fake, fake, C.cast(cnt_, C.c_void_p), 4, gcn_res,
                                         fake, y_slots, 0, fake, fake, res_mode, 12, fake, 16, 0, c_out, n_skel, V, P, None)

    for kwargs, needle in [(dict(c_out=128), "c_out <= 64"), (dict(y_slots=9), "too shallow"), (dict(P=202), "multiple of 4"),
                           (dict(c_in=32), "identity gcn residual"), (dict(res_mode=2), "none or identity"),
                           (dict(cnt_=(C.c_int32 * 3)(2, 1, 4)), "skeleton-sparse"), (dict(V=43, P=344), "longer than 128")]:
        assert call(**kwargs) < 0
        assert needle in lib.csk_last_error().decode(), (kwargs, lib.csk_last_error().decode())


def test_no_kernel_spills():
    """Every kernel instantiation a public entry point can select is spill-free: the compiler's resource report, which
    build.sh keeps next to the library, shows 0 bytes of scratch per lane for each of them (a spilling instantiation is a
    2x performance cliff for the shapes that select it)."""
    import os
    import re
    path = os.path.join(os.path.dirname(pkg.native.LIB_PATH), "kernel_resources.txt")
    assert os.path.exists(path), "build with continual-skeletons_amd/csrc/build.sh (it writes kernel_resources.txt)"
    text = open(path).read()
    kernels = re.findall(r"Name: (\S+)\n(?:.*\n)*?ScratchSize \[bytes/lane\]: (\d+)", text)
    assert len(kernels) >= 30, len(kernels)
    spilling = [(n, int(b)) for n, b in kernels if int(b) != 0]
    assert not spilling, spilling


def test_environment_switches_are_only_the_kernel_family_selectors():
    """Under CSK_DIAG=1 the library reads exactly four switches, each choosing between two production kernel families
    that compute the same result; nothing in the sources times kernels from the inside or hands them a device address
    parsed from the environment, and the retired 32x32x2 fused block kernel and its switch are gone."""
    import glob
    srcs = sorted(glob.glob(os.path.join(ROOT, "continual-skeletons_amd", "csrc", "*.hip")) +
                  glob.glob(os.path.join(ROOT, "continual-skeletons_amd", "csrc", "*.h")))
    assert len(srcs) >= 10, srcs
    names = set()
    for path in srcs:
        text = open(path).read()
        assert "csk_diag_stamps" not in text and "s_memtime" not in text, path
        assert "co_block_kernel" not in text and "csk_step16_enabled" not in text, path
        if os.path.basename(path) in ("runtime.hip", "mfma_core.h"):       # the definitions and their declarations
            continue
        # every call names its switch as a literal: a forwarding helper (csk_diag_int(env)) would hide the switches it reads
        calls = re.findall(r"csk_diag_(?:flag|int)\(\s*([^)]*)\)", text)
        literal = [re.fullmatch(r'"([A-Z0-9_]+)"\s*', a) for a in calls]
        assert all(literal), (path, calls)
        names |= {m.group(1) for m in literal}
    assert names == {"CSK_TCN16", "CSK_GCN16", "CSK_TCN_WINO", "CSK_GCN_GENERAL"}, sorted(names)


def test_split_weight_packing_reconstructs_the_fp32_weights():
    """fold.pack_conv_weight_split (operand image of csk_tcn_stage_bf16x3): the three bf16 pieces of every element sum back
    to the fp32 weight the exact path packs (24 significand bits), the nine taps sit in class-major order (residue classes
    modulo the stride), padding channels / rows / slots are zero."""
    from continual_skeletons_amd import fold
    g = torch.Generator().manual_seed(3)
    w = torch.randn(70, 20, 9, 1, generator=g)
    sc = torch.rand(70, generator=g).double() + 0.5
    w32 = (w.double()[:, :, :, 0] * sc[:, None, None]).float()
    for stride, order in ((1, list(range(9))), (2, [0, 2, 4, 6, 8, 1, 3, 5, 7]), (3, [0, 3, 6, 1, 4, 7, 2, 5, 8])):
        img = fold.pack_conv_weight_split(w, sc, stride)
        assert img.dtype == torch.int16 and img.numel() == 2 * 9 * 3 * 2 * 128 * 8        # [c16 = 2][9][3][2][Mpad = 128][8]
        kind = img.view(torch.bfloat16).float().view(2, 9, 3, 2, 128, 8)
        rec = kind.sum(2).permute(3, 0, 2, 4, 1).reshape(128, 32, 9)                      # [co][c][slot]
        assert torch.equal(rec[:70, :20], w32[:, :, order])                               # exact: h + m + l == the fp32 value
        assert float(rec[70:].abs().max()) == 0 and float(rec[:, 20:].abs().max()) == 0
    one = fold.pack_conv_weight_split(torch.randn(8, 5, 1, 1, generator=g), torch.ones(8, dtype=torch.float64), 2)
    assert one.numel() == 1 * 3 * 3 * 2 * 64 * 8                                          # k = 1: tap 0 + two zero slots
    assert float(one.view(torch.bfloat16).float().view(1, 3, 3, 2, 64, 8)[:, 1:].abs().max()) == 0
    three = fold.pack_conv_weight_split(torch.randn(8, 5, 3, generator=g), torch.ones(8, dtype=torch.float64))   # graph-conv subsets
    assert three.numel() == 1 * 3 * 3 * 2 * 64 * 8
    with pytest.raises(ValueError):
        fold.pack_conv_weight_split(torch.randn(8, 5, 5, 1), torch.ones(8, dtype=torch.float64))


def test_new_entry_points_validate_their_arguments_without_a_gpu():
    import ctypes as C
    lib = pkg.native.lib()
    fake = C.c_void_p(0x1000)
    assert lib.csk_conv1x1_f32(None, fake, fake, fake, 1, 4, 4, 3, 25, 300, 75, 300, 75, None) == -1
    assert b"null pointer" in lib.csk_last_error()
    assert lib.csk_conv1x1_f32(fake, fake, fake, fake, 1, 4, 4, 3, 70, 840, 210, 840, 210, None) == -1
    assert b"bad dims" in lib.csk_last_error()
    # the clip form of the attention (T > 1) needs its partial-logit scratch
    assert lib.csk_agcn_attention_f32(fake, fake, fake, None, 2, 4, 6, 18, 100, 10, 2, 0, None) == -1
    assert b"scratch" in lib.csk_last_error()
    # bf16x3 stage: the 9-tap conv only, stride <= 4, 16-byte aligned operand images
    args = dict(y=fake, w=fake, xr=None, wr=None, b=fake, o=fake)
    def split(k=9, stride=1, w=fake):
        return lib.csk_tcn_stage_bf16x3(args["y"], w, args["xr"], args["wr"], args["b"], args["o"], 1, 16, 16, 20, 25, k, stride, 4, 0, 0,
                                        0, 0, 1, None)
    assert split(k=3) == -1 and b"9 x 1" in lib.csk_last_error()
    assert split(stride=5) == -1 and b"stride" in lib.csk_last_error()
    assert split(w=C.c_void_p(0x1008)) == -1 and b"16-byte aligned" in lib.csk_last_error()


def test_gcn_route_query_and_dense_guards_without_a_gpu():
    """csk_gcn_stage_f32_route on bad dimensions, the per-frame V = 64 launch that does not fit 160 KiB of LDS (the stage itself fails
    with the same message before it launches anything), and csk_agcn_attention_f32 at V = 33"""
    import ctypes as C
    lib = pkg.native.lib()
    fake = C.c_void_p(0x10000)

    def route(cnt=(18, 18, 18), ell_w=18, adj=3 * 18 * 18, per_frame=0, n_seg=2, c_in=64, c_out=64, frames=8, V=18, res=1, cnt_ptr=True):
        c = (C.c_int32 * 3)(*cnt)
        return lib.csk_gcn_stage_f32_route(fake, fake, fake, C.cast(c, C.c_void_p) if cnt_ptr else None, ell_w, adj, per_frame, n_seg, c_in, c_out,
                                           frames, V, c_in * frames * V, frames * V, c_out * frames * V, frames * V, res)
    assert route() == 3064180
    assert route(cnt_ptr=False) == -1 and b"null pointer" in lib.csk_last_error()
    for bad in (dict(n_seg=0), dict(c_in=0, c_out=0), dict(frames=0), dict(V=1, ell_w=1, cnt=(1, 1, 1)), dict(V=65, ell_w=65, cnt=(65, 65, 65))):
        assert route(**bad) == -1 and b"bad dims" in lib.csk_last_error(), bad
    assert route(ell_w=19) == -1 and b"ell_w" in lib.csk_last_error()
    assert route(cnt=(18, 19, 18)) == -1 and b"ell_cnt[1]" in lib.csk_last_error()
    assert route(res=0) == -1 and b"res_mode" in lib.csk_last_error()
    assert route(c_in=32) == -1 and b"identity residual" in lib.csk_last_error()
    assert route(per_frame=1, cnt=(1, 1, 4), ell_w=4, adj=0) == -1 and b"per-frame adjacency must be dense" in lib.csk_last_error()
    # per-frame, V = 64: 3 V^2 floats of adjacency for each of the 6 frames a 256-position tile can touch
    v64 = dict(V=64, ell_w=64, cnt=(64, 64, 64), adj=3 * 64 * 64, per_frame=1)
    assert route(**v64) == -1 and b"exceeds 160 KiB" in lib.csk_last_error()
    cnt = (C.c_int32 * 3)(64, 64, 64)
    assert lib.csk_gcn_stage_f32(fake, fake, fake, fake, fake, fake, C.cast(cnt, C.c_void_p), 64, 3 * 64 * 64, 1, 2, 64, 64, 8, 64, 64 * 512, 512,
                                 64 * 512, 512, 1, None) == -1 and b"gcn_stage: LDS tile" in lib.csk_last_error()
    assert route(V=64, ell_w=64, cnt=(64, 64, 64), adj=3 * 64 * 64) == 5000645            # per segment it fits: general <64, 5>
    # the tile query keeps its answers: 0 for everything that is not the 16x16x4 family
    c18 = (C.c_int32 * 3)(18, 18, 18)
    assert lib.csk_gcn_stage_f32_tile(fake, fake, C.cast(c18, C.c_void_p), 18, 3 * 18 * 18, 0, 2, 64, 64, 8, 18, 64 * 144, 144, 64 * 144, 144, 1) == 0
    assert lib.csk_agcn_attention_f32(fake, fake, fake, fake, 2, 4, 6, 33, 6 * 24 * 198, 198, 2, 0, None) == -1
    assert b"V <= 32" in lib.csk_last_error()


def _gcn_route_tables(lib):
    """The answers of the three graph-conv route queries over a shape grid, in grid order: {query: [int or refusal text, ...]}.
    Grid: V x c_out x residual x adjacency x ell_cnt x operand alignment x n_seg x frames (x ksplit for the split query, which
    takes shared adjacencies only); ell_w = max(ell_cnt), contiguous channel-major layouts, conv residual from c_in = 40."""
    import ctypes as C
    import itertools
    out = {"route": [], "tile": [], "split": []}

    def said(rc):
        return rc if rc >= 0 else lib.csk_last_error().decode()
    for V, c_out, res, cnt, off, n_seg, frames in itertools.product((18, 25, 20, 4, 32, 41, 64), (40, 64, 100, 128, 192, 256), (1, 2),
                                                                    ((1, 1, 4), (2, 1, 4), (1, 1, 5), None), (0, 4), (1, 2, 4, 1024),
                                                                    (1, 7, 8, 300)):
        cnt = cnt or (V, V, V)
        ell_w, c_in, q = max(cnt), (c_out if res == 1 else 40), frames * V
        cp = C.cast((C.c_int32 * 3)(*cnt), C.c_void_p)
        x, y, ell = C.c_void_p(0x10000 + off), C.c_void_p(0x10000), C.c_void_p(0x20000 + off)
        geom = (n_seg, c_in, c_out, frames, V, c_in * q, q, c_out * q, q, res)
        for stride, per_frame in ((0, 0), (3 * V * ell_w, 0), (3 * V * ell_w, 1)):          # shared, per segment, per frame
            out["route"].append(said(lib.csk_gcn_stage_f32_route(x, y, ell, cp, ell_w, stride, per_frame, *geom)))
            out["tile"].append(said(lib.csk_gcn_stage_f32_tile(x, y, cp, ell_w, stride, per_frame, *geom)))
        for ksplit in (1, 4, 32, 33):
            out["split"].append(said(lib.csk_gcn_stage_splitk_f32_route(x, y, ell, cp, ell_w, *geom, ksplit, y)))
    return out


# What the library of the commit before GcnCall / GcnRoute answered over _gcn_route_tables' grid: per query the number of cases behind
# every distinct answer (route integers as include/cskel.h defines them, refusals by their full text) and the SHA-256 of the answers
# in grid order, one per line.  Recorded from that library, not from the one under test.
_LDS = "gcn_stage: LDS tile %d B exceeds 160 KiB"
_REFUSED = {**{_LDS % b: 96 for b in (173056, 222764, 227328, 233004, 235520, 335872, 346112)},
            "gcn_stage: ell_w must be in [1, V]": 1152,
            "gcn_stage: per-frame adjacency must be dense (ell_w == V, ell_cnt == V)": 7680}
_GCN_ROUTE_TABLE = {
    "route": ({1000640: 543, 1000641: 543, 1001280: 548, 1001281: 548,
               2018400: 28, 2018410: 28, 2025400: 33, 2025410: 33,
               3064180: 96, 3064181: 96, 3064250: 192, 3064251: 192, 3128180: 96, 3128181: 96, 3128250: 192, 3128251: 192,
               4000000: 336, 4000001: 336,
               5000645: 7968, 5000646: 1536, 5001283: 7392, 5001284: 1728, **_REFUSED},
              "6d35b974c4d933111a63f9e3083e1397e463878c6cf9326bd10a4a34f3f112af"),
    "tile": ({0: 22630, 18400: 28, 18410: 28, 25400: 33, 25410: 33, **_REFUSED},
             "38b1554c77e0049dbe494f29da766a83cd82c1b1395c4046927704ac1a1e9137"),
    "split": ({1000640: 543, 1000641: 543, 1001280: 548, 1001281: 548,
               2018400: 28, 2018410: 28, 2025400: 33, 2025410: 33,
               5000645: 3264, 5000646: 768, 5001283: 3264, 5001284: 768,
               # (1 << 30) | MT128 << 29 | CONVRES << 28 | (ranges - 1) << 23 | cper / 8
               1090519042: 192, 1098907650: 192, 1098907654: 192, 1107296257: 192, 1132462081: 192, 1266679809: 192,
               1358954498: 576, 1375731713: 576, 1635778564: 384, 1635778568: 192, 1711276033: 192, 1736441857: 192,
               1870659585: 192, 1895825410: 576, 1912602625: 576,
               "gcn_stage: ell_w must be in [1, V]": 1152,
               "gcn_stage_splitk: ksplit must be in [1, 32] and needs a partial-sum buffer": 10752,
               "gcn_stage_splitk: split-K is built for the skeleton-sparse kernel (shared adjacency, <= 1/1/4 non-zeros per column)": 16128},
              "2654cfef03c10b2f1f6b47e285e1cc457cdf5ed642c75f3eff95fa195dc4e438"),
}


def test_gcn_route_queries_keep_every_answer_and_refusal_text_over_the_shape_grid():
    """csk_gcn_stage_f32_route, csk_gcn_stage_f32_tile and csk_gcn_stage_splitk_f32_route answer every shape of the grid -- the joint
    counts of every family, ragged and full c_out, both residuals, shared / per-segment / per-frame adjacencies, sparse and dense
    entry counts, misaligned operands, 1 to 1024 segments, 1 to 300 frames, splits in and out of range -- with the literal integers
    and the literal refusal texts recorded before the host path was restructured: the same count of cases behind every answer and
    the same answer for every case (digest of the grid-ordered list)."""
    import collections
    import hashlib
    got = _gcn_route_tables(pkg.native.lib())
    assert set(got) == set(_GCN_ROUTE_TABLE)
    for query, (counts, digest) in _GCN_ROUTE_TABLE.items():
        tally = dict(collections.Counter(got[query]))
        assert tally == counts, (query, sorted(set(tally.items()) ^ set(counts.items()), key=str))
        assert hashlib.sha256("\n".join(map(str, got[query])).encode()).hexdigest() == digest, query


def test_conv1x1_refusals_keep_their_text():
    """csk_conv1x1_f32 shares its tile geometry and guards with the graph-conv stage but speaks under its own name: every refusal
    with its full text, in the order of the checks, nothing launched."""
    import ctypes as C
    lib = pkg.native.lib()
    fake = C.c_void_p(0x1000)

    def conv(x=fake, y=fake, w=fake, b=fake, n_seg=2, c_in=16, c_out=128, frames=8, V=25):
        q = frames * V
        rc = lib.csk_conv1x1_f32(x, y, w, b, n_seg, c_in, c_out, frames, V, c_in * q, q, c_out * q, q, None)
        return rc, lib.csk_last_error()
    for null in "xywb":
        assert conv(**{null: None}) == (-1, b"conv1x1: null pointer"), null
    for bad in (dict(n_seg=0), dict(c_in=0), dict(c_out=0), dict(frames=0), dict(V=1), dict(V=65)):
        assert conv(**bad) == (-1, b"conv1x1: bad dims"), bad
    assert conv(frames=1 << 20, V=64) == (-1, b"conv1x1: frames*V too large for 32-bit position arithmetic")
    # an activation row holds the whole frames a tile touches: 4 x 63 = 252 positions on 128-row tiles, over the 192 staged there
    # (V = 64 fits exactly: 3 x 64 = 192, and would launch); this check comes before the grid's
    assert conv(V=63) == (-1, b"conv1x1: activation tile of 252 positions exceeds the staged maximum")
    assert conv(V=63, n_seg=1 << 30, frames=1 << 10) == (-1, b"conv1x1: activation tile of 252 positions exceeds the staged maximum")
    assert conv(V=25, n_seg=1 << 30, frames=1 << 10) == (-1, b"conv1x1: grid too large")
    assert conv(V=25, c_out=64, n_seg=1 << 30, frames=1 << 10) == (-1, b"conv1x1: grid too large")


def test_set_precision_marks_blocks_and_refolds():
    m = pkg.StGcn(pkg.ntu_graph().A)
    assert all(b.precision == "f32" for b in m.layers.values())
    pkg.set_precision(m, "bf16x3")
    assert all(b.precision == "bf16x3" for b in m.layers.values())
    ops = m.layers["layer5"]._fold()                                  # stride-2 block with a conv residual
    assert ops["w_split"].dtype == torch.int16 and ops["w_res_split"] is not None and ops["w"].dtype == torch.float32
    pkg.set_precision(m, "f32")
    assert m.layers["layer5"]._fold()["w_split"] is None
    with pytest.raises(ValueError):
        pkg.set_precision(m, "fp16")
    # a block the split kernel does not cover anywhere below the module: refused BEFORE any block is switched
    m.layers["layer9"].tcn.kernel_size = 7
    with pytest.raises(NotImplementedError):
        pkg.set_precision(m, "bf16x3")
    assert all(b.precision == "f32" for b in m.layers.values())


def test_gcn_bf16x3_entry_validates_arguments_without_a_gpu():
    import ctypes as C
    lib = pkg.native.lib()
    fake = C.c_void_p(0x1000)
    cnt = (C.c_int32 * 3)(1, 1, 4)

    def call(c_out=128, cnt_=cnt, res=1, c_in=128, wres=None):
        return lib.csk_gcn_stage_bf16x3(fake, fake, fake, wres, fake, fake, fake, C.cast(cnt_, C.c_void_p), 4, 2, c_in, c_out, 10, 25,
                                        res, None)
    assert call(c_out=64) == -1 and b"multiple of 128" in lib.csk_last_error()
    assert call(cnt_=(C.c_int32 * 3)(2, 1, 4)) == -1 and b"skeleton-sparse" in lib.csk_last_error()
    assert call(c_in=64) == -1 and b"identity residual" in lib.csk_last_error()
    assert call(c_in=64, res=2) == -1 and b"conv residual without" in lib.csk_last_error()


def test_fused_attention_entry_and_plan_validate_their_arguments_without_a_gpu():
    """csk_agcn_embed_attention_f32 (shapes it is built for, alignment, scratch of the per-segment form) and the adaptive
    graph-conv fields of csk_co_layer (csk_co_plan_create) are checked before anything is launched."""
    import ctypes as C
    lib = pkg.native.lib()
    fake = C.c_void_p(0x1000)

    def call(x=fake, scratch=None, inter=16, V=18, per_frame=1, seg_stride=1000, chan_stride=100):
        return lib.csk_agcn_embed_attention_f32(x, fake, fake, fake, fake, scratch, 2, 64, inter, 4, V, per_frame, seg_stride, chan_stride, None)
    assert call(x=None) == -1 and b"null pointer" in lib.csk_last_error()
    assert call(V=20) == -1 and b"built for V in {18, 25}" in lib.csk_last_error()
    assert call(inter=24) == -1 and b"inter in {16, 32, 64}" in lib.csk_last_error()
    assert call(x=C.c_void_p(0x1004)) == -1 and b"8-byte aligned" in lib.csk_last_error()
    assert call(chan_stride=101) == -1 and b"8-byte aligned" in lib.csk_last_error()
    assert call(per_frame=0) == -1 and b"scratch" in lib.csk_last_error()
    # plan: an adaptive layer needs all four agcn_* operands and the dense ELL pattern (ell_w = V, ell_cnt = {V, V, V})
    L = (pkg.native.CoLayer * 1)()
    l = L[0]
    l.c_in, l.c_out, l.stride, l.res_kind, l.gcn_res_mode, l.ell_w, l.tcn_ksplit = 3, 64, 1, 0, 2, 18, 1
    for j in range(3):
        l.ell_cnt[j] = 18
    for f in ("gcn_w", "gcn_bias", "ell_src", "tcn_w", "tcn_bias", "y_ring", "out_ring"):
        setattr(l, f, 0x1000)
    l.agcn_inter, l.agcn_w_pairs, l.agcn_b_pairs, l.agcn_a_sum = 16, 0x1000, 0x1000, 0x1000      # agcn_adj missing
    l.y_slots, l.out_slots, l.agcn_adj_frames = 16, 8, 8
    lib.csk_co_plan_create.restype = C.c_void_p

    def create(xin0_slots=12):
        return lib.csk_co_plan_create(1, C.byref(L), fake, xin0_slots, 2, 3, 18, 2, 72, fake, fake, 400, fake, fake, 4, 1, fake, fake)
    assert not create() and b"adaptive graph conv" in lib.csk_last_error()
    l.agcn_adj = 0x1000
    l.ell_w = 6                                          # not the dense pattern
    assert not create() and b"adaptive graph conv" in lib.csk_last_error()
    l.ell_w = 18
    # ring depths (include/cskel.h: CSK_CO_Y_SLOTS / CSK_CO_IN_SLOTS) and scratch capacities are part of the contract
    assert not create(xin0_slots=4) and b"input ring needs >= 5" in lib.csk_last_error()
    # the input ring's depth fixes the largest cycle: 4 + 4 slots = cycles of <= 4 frames, for which a 12-slot y ring and a
    # 4-slot output ring (last layer: its own emissions, >= 4) suffice; the same rings are too shallow for 8-frame cycles
    l.y_slots, l.out_slots, l.agcn_adj_frames = 12, 4, 4
    small = create(xin0_slots=8)
    assert small
    lib.csk_co_plan_destroy(C.c_void_p(small))
    assert not create(xin0_slots=12) and b"rings too shallow" in lib.csk_last_error()
    l.y_slots, l.out_slots, l.agcn_adj_frames = 16, 8, 8
    l.y_slots = 15
    assert not create() and b"rings too shallow" in lib.csk_last_error()
    l.y_slots, l.out_slots = 16, 7
    assert not create() and b"rings too shallow" in lib.csk_last_error()
    l.out_slots, l.agcn_adj_frames = 8, 0
    assert not create() and b"agcn_adj_frames" in lib.csk_last_error()
    l.agcn_adj_frames, l.tcn_ksplit, l.tcn_partial, l.partial_emits = 8, 3, 0x1000, 0
    assert not create() and b"partial_emits" in lib.csk_last_error()
    l.partial_emits = 8
    plan = create()
    assert plan
    lib.csk_co_plan_destroy(C.c_void_p(plan))


def test_plan_cycle_rejects_bad_arguments_and_leaves_the_callers_counters_alone():
    """csk_co_plan_cycle steps on the CALLER's counters ({frames, features, (received, emitted) per layer}): a null or
    mis-sized buffer, a negative counter, a cycle length the rings were not sized for and a null frame are argument errors
    reported before anything is launched (fake pointers here), and after each of them the buffer holds, element by element,
    what was passed in."""
    import ctypes as C
    lib = pkg.native.lib()
    fake = C.c_void_p(0x1000)
    L = (pkg.native.CoLayer * 1)()
    l = L[0]
    l.c_in, l.c_out, l.stride, l.res_kind, l.gcn_res_mode, l.ell_w, l.tcn_ksplit = 3, 64, 1, 0, 2, 3, 1
    for j in range(3):
        l.ell_cnt[j] = 1
    for f in ("gcn_w", "gcn_bias", "ell_src", "ell_val", "tcn_w", "tcn_bias", "y_ring", "out_ring"):
        setattr(l, f, 0x1000)
    l.y_slots, l.out_slots = 16, 8
    plan = lib.csk_co_plan_create(1, C.byref(L), fake, 12, 2, 3, 18, 2, 72, fake, fake, 400, fake, fake, 4, 1, fake, fake)
    assert plan, lib.csk_last_error()
    plan = C.c_void_p(plan)
    start = [9, 1, 9, 5]
    frames = (C.c_void_p * 8)(*[0x1000] * 8)
    no_frame = (C.c_void_p * 8)(0x1000, None, *[0x1000] * 6)
    slot, nf, nl = C.c_int(0), C.c_int(0), C.c_int(0)

    def cycle(counters=start, n=4, null_counters=False, fr=frames, r=2):
        buf = (C.c_int64 * len(counters))(*counters)
        rc = lib.csk_co_plan_cycle(plan, None if null_counters else buf, n, fr, r, fake, C.byref(slot), C.byref(nf),
                                   C.byref(nl), None)
        assert all(buf[i] == counters[i] for i in range(len(counters))), list(buf)
        return rc, lib.csk_last_error()
    try:
        for kwargs, why in ((dict(null_counters=True), b"null pointer"), (dict(n=3), b"expected 4 counters"),
                            (dict(counters=start + [0, 0], n=6), b"expected 4 counters"),
                            (dict(counters=[9, 1, -1, 5]), b"negative counter"), (dict(r=0), b"r must be in [1, 8]"),
                            (dict(r=9), b"r must be in [1, 8]"), (dict(fr=None), b"null pointer"),
                            (dict(fr=no_frame), b"null frame")):
            rc, msg = cycle(**kwargs)
            assert rc == -1 and why in msg, (kwargs, rc, msg)
    finally:
        lib.csk_co_plan_destroy(plan)


def test_plan_staleness_check_is_exact_for_every_kind_of_weight_edit():
    """CoStGcn._weights_changed (host logic of the native plan): exact on the FIRST call after a replaced Parameter, a
    swapped / added sub-module, an in-place edit and ``p.data = ...`` -- checked on the snapshot the plan keeps, without a
    GPU (the plan itself is not built here)."""
    import torch
    pkg = _bootstrap.load()

    def fresh():
        net = pkg.CoStGcn(pkg.ntu_graph().A).eval()
        net.__dict__["_plan_keep"] = (None, net._weight_slots())
        assert net._weights_changed() is False and net._weights_changed() is False
        return net

    net = fresh()
    net.fc.weight = torch.nn.Parameter(net.fc.weight.detach().clone())
    assert net._weights_changed() is True
    net = fresh()
    net.layers["layer3"].tcn.bn = torch.nn.BatchNorm2d(64).eval()
    assert net._weights_changed() is True
    net = fresh()
    with torch.no_grad():
        net.fc.bias.add_(1.0)
    assert net._weights_changed() is True
    net = fresh()
    net.layers["layer10"].tcn.t_conv.weight.data = net.layers["layer10"].tcn.t_conv.weight.data.clone()
    assert net._weights_changed() is True
    net = fresh()
    net.layers["layer1"].gcn.register_buffer("extra", torch.zeros(1))
    net.layers["layer2"].add_module("extra", torch.nn.Identity())
    assert net._weights_changed() is True
    net = fresh()
    net.load_state_dict(net.state_dict())
    net._install_dirty_hooks()
    net.load_state_dict(net.state_dict())
    assert net._weights_changed() is True
    net.__dict__["_plan_keep"] = (None, net._weight_slots())          # what _refresh_plan_weights does after refolding
    assert net._weights_changed() is False


def test_round4_entry_points_validate_their_arguments_without_a_gpu():
    """csk_gcn_stage_splitk_f32, csk_co_head_step_f32, csk_input_norm_frames_f32: argument errors are reported before
    anything is launched."""
    import ctypes as C
    lib = pkg.native.lib()
    fake = C.c_void_p(0x1000)
    cnt = (C.c_int32 * 3)(1, 1, 4)

    def gcn(ksplit=4, partial=fake, ell_cnt=cnt, res=1, c_in=64, c_out=64):
        return lib.csk_gcn_stage_splitk_f32(fake, fake, fake, fake, fake, fake, ell_cnt, 4, 1, c_in, c_out, 1, 25, 1600, 25, 1600, 25, res,
                                            ksplit, partial, None)
    assert gcn(ksplit=0) == -1 and b"ksplit must be in [1, 32]" in lib.csk_last_error()
    assert gcn(ksplit=33) == -1 and b"ksplit must be in [1, 32]" in lib.csk_last_error()
    assert gcn(partial=None) == -1 and b"partial-sum buffer" in lib.csk_last_error()
    assert gcn(res=1, c_out=128) == -1 and b"identity residual" in lib.csk_last_error()
    dense = (C.c_int32 * 3)(4, 4, 4)                       # more than 1 / 1 / 4 non-zeros per column: not the sparse kernel's graph
    assert gcn(ell_cnt=dense) == -1 and b"skeleton-sparse" in lib.csk_last_error()

    def head(ring=fake, emit=1, logits=fake, count=1, head_=0, window=4):
        return lib.csk_co_head_step_f32(fake, ring, fake, fake, fake, logits, 2, 256, 50, 100, window, head_, count, emit, 60, None)
    assert head(ring=None) == -1 and b"null pointer" in lib.csk_last_error()
    assert head(head_=4) == -1 and b"bad dims" in lib.csk_last_error()
    assert head(count=5) == -1 and b"bad dims" in lib.csk_last_error()
    assert head(logits=None) == -1 and b"emitting step needs" in lib.csk_last_error()
    assert head(count=0) == -1 and b"emitting step needs" in lib.csk_last_error()

    srcs, dsts = (C.c_void_p * 2)(0x1000, 0x1000), (C.c_void_p * 2)(0x2000, 0)
    assert lib.csk_input_norm_frames_f32(srcs, dsts, 9, fake, fake, 2, 3, 25, 2, 100, None) == -1 and b"1..8 frames" in lib.csk_last_error()
    assert lib.csk_input_norm_frames_f32(srcs, dsts, 2, fake, fake, 2, 3, 25, 2, 99, None) == -1 and b"bad dims" in lib.csk_last_error()
    assert lib.csk_input_norm_frames_f32(srcs, dsts, 2, fake, fake, 2, 3, 25, 2, 100, None) == -1 and b"null frame" in lib.csk_last_error()


def test_gcn_split_route_query_refuses_what_the_split_entry_refuses():
    """csk_gcn_stage_splitk_f32_route and csk_gcn_stage_splitk_f32 on the same bad requests: ksplit outside [1, 32], no partial-sum
    buffer, a graph or a tile the sparse kernel does not take with ksplit > 1, bad dimensions -- the same message from both, nothing
    launched; and the query's answers for ksplit = 1 and for a request that collapses are csk_gcn_stage_f32_route's."""
    import ctypes as C
    lib = pkg.native.lib()
    fake = C.c_void_p(0x10000)

    def both(ksplit=4, partial=fake, cnt=(1, 1, 4), ell_w=4, n_seg=1, c_in=64, c_out=64, frames=2, V=25, res=1, cnt_ptr=True):
        c = C.cast((C.c_int32 * 3)(*cnt), C.c_void_p) if cnt_ptr else None
        q = frames * V
        a = lib.csk_gcn_stage_splitk_f32_route(fake, fake, fake, c, ell_w, n_seg, c_in, c_out, frames, V, c_in * q, q, c_out * q, q, res, ksplit, partial)
        ma = lib.csk_last_error()
        if a >= 0:
            return a, b""
        b = lib.csk_gcn_stage_splitk_f32(fake, fake, fake, fake, fake, fake, c, ell_w, n_seg, c_in, c_out, frames, V, c_in * q, q, c_out * q, q, res,
                                         ksplit, partial, None)
        assert b == -1 and lib.csk_last_error() == ma, (ma, lib.csk_last_error())
        return a, ma
    for bad in (0, -1, 33):
        rc, msg = both(ksplit=bad)
        assert rc == -1 and b"ksplit must be in [1, 32]" in msg
    rc, msg = both(partial=None)
    assert rc == -1 and b"partial-sum buffer" in msg
    for graph in (dict(cnt=(2, 1, 4)), dict(cnt=(1, 1, 5), ell_w=5), dict(V=50, c_out=128, c_in=128)):     # V = 50: ldb 200 > 192
        rc, msg = both(**graph)
        assert rc == -1 and b"skeleton-sparse" in msg, graph
        assert both(ksplit=1, partial=None, **graph)[0] // 1000000 == 5                                     # unsplit: the general kernel
    assert both(cnt_ptr=False) == (-1, b"gcn_stage: null pointer")
    for bad in (dict(n_seg=0), dict(frames=0), dict(V=1, ell_w=1, cnt=(1, 1, 1)), dict(c_in=0, c_out=0)):
        rc, msg = both(**bad)
        assert rc == -1 and b"bad dims" in msg, bad
    rc, msg = both(c_out=128)
    assert rc == -1 and b"identity residual" in msg
    # answers: (1 << 30) | MT128 << 29 | CONVRES << 28 | (ranges - 1) << 23 | cper / 8
    assert both()[0] == (1 << 30) | 3 << 23 | 2
    assert both(c_in=40, c_out=128, res=2)[0] == (1 << 30) | (1 << 29) | (1 << 28) | 2 << 23 | 2
    assert both(ksplit=32, c_in=256, c_out=256)[0] == (1 << 30) | (1 << 29) | 31 << 23 | 1
    assert both(ksplit=1, partial=None)[0] == 1000640 and both(c_in=3, res=2)[0] == 1000641                # one range: the unsplit route
    cnt = C.cast((C.c_int32 * 3)(1, 1, 4), C.c_void_p)
    assert lib.csk_gcn_stage_f32_route(fake, fake, fake, cnt, 4, 0, 0, 1, 3, 64, 2, 25, 150, 50, 3200, 50, 2) == 1000641


def test_roofline_config_prices_n_ranks_against_n_peaks():
    """bench.py passes the WHOLE JOB's work (per-rank work x world) and the step time; the accounting must price it against
    world x one MI355X's peak.  With the round-4 driver timing (72.222 ms per batch-256 step) the fraction is 0.75 at one
    rank AND at eight (weak scaling, same per-rank time) -- it used to print 6.0 at eight (round-4 review, weak item 6)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import workmodel
    fa, fe, by = workmodel.clip_totals(512)
    one = workmodel.roofline_config(fa, by, 72.222e-3, fe)
    eight = workmodel.roofline_config(8 * fa, 8 * by, 72.222e-3, 8 * fe, n_gpus=8)
    assert abs(one["frac"] - 0.7505) < 2e-3 and abs(one["frac_alg"] - 0.7775) < 2e-3
    assert eight["frac"] == one["frac"] and eight["frac_alg"] == one["frac_alg"] and 0 < eight["frac"] < 1
    assert eight["n_gpus"] == 8 and eight["peak_tflops"] == round(8 * workmodel.PEAK_F32_MFMA_TFLOPS, 1)
    assert abs(eight["achieved_tflops_per_gpu"] - one["achieved_tflops"]) < 0.02
    with pytest.raises(ValueError):
        workmodel.roofline_config(fa, by, 1.0, fe, n_gpus=0)
    # the online leg: 1024 streams, 4-frame cycle at the round-4 rate (4.12 ms per cycle) -> 0.70 at any N
    sa, se, sb = workmodel.step_totals(2048, 4)
    assert abs(workmodel.roofline_config(8 * sa, 8 * sb, 4.12e-3, 8 * se, n_gpus=8)["frac"] - workmodel.roofline_config(sa, sb, 4.12e-3, se)["frac"]) < 1e-9


def test_round5_split_k_tcn_entry_validates_its_arguments_without_a_gpu():
    """csk_tcn_stage_splitk_f32: argument errors are reported before anything is launched."""
    import ctypes as C
    lib = pkg.native.lib()
    fake = C.c_void_p(0x1000)

    def tcn(ksplit=4, partial=fake, k=9, c=64, res=1, c_res=64):
        return lib.csk_tcn_stage_splitk_f32(fake, fake, fake, None, fake, fake, 1, c, 64, 20, 25, k, 1, 4 if k == 9 else 0, res, c_res, 20, 0, 1,
                                            ksplit, partial, None)
    assert tcn(ksplit=0) == -1 and b"ksplit must be in [1, 64]" in lib.csk_last_error()
    assert tcn(ksplit=65) == -1 and b"ksplit must be in [1, 64]" in lib.csk_last_error()
    assert tcn(partial=None) == -1 and b"partial-sum buffer" in lib.csk_last_error()
    assert tcn(partial=C.c_void_p(0x1004)) == -1 and b"16-byte aligned" in lib.csk_last_error()
    assert tcn(k=1) == -1 and b"9-tap" in lib.csk_last_error()
    assert tcn(c_res=32) == -1 and b"identity residual" in lib.csk_last_error()


# The temporal-conv entries below are called with fake pointers and always with at least one fault that the direct entry refuses
# before anything is launched.  Expected messages are the texts the entries have always reported (written out, not composed).
_FAKE = ctypes.c_void_p(0x1000)


def _tcn_args(t_in=20, k=9, stride=1, pad=4, res=1, c=64, c_out=64, c_res=64, t_res=20, res_off=0, v=25, n_seg=1):
    return (n_seg, c, c_out, t_in, v, k, stride, pad, res, c_res, t_res, res_off, 1)


def _wino_entries(lib):
    """(name, call(**kw), shape the entry's Winograd gate would take but for the fault added to it)"""
    def falling_back(fn):
        return lambda y=_FAKE, x_res=_FAKE, w_res=_FAKE, **kw: fn(y, _FAKE, x_res, w_res, _FAKE, _FAKE, *_tcn_args(**kw), _FAKE, None)
    return (("wino", falling_back(lib.csk_tcn_stage_wino_f32), dict(stride=1, pad=4, res=1, res_off=0)),
            ("ext stride 1", falling_back(lib.csk_tcn_stage_wino_ext_f32), dict(stride=1, pad=4, res=0, res_off=0)),
            ("ext stride 2", falling_back(lib.csk_tcn_stage_wino_ext_f32), dict(stride=2, pad=4, res=2, res_off=0)),
            ("valid", falling_back(lib.csk_tcn_stage_wino_valid_f32), dict(stride=1, pad=0, res=1, res_off=4)))


def _both_refuse_faults(base):
    """faults added to a shape `base` (stride, pad, res, res_off) that the Winograd gates and the direct entry both refuse:
    (keywords, the direct entry's message without its prefix)"""
    short = dict(pad=0, t_in=5) if base["pad"] == 0 else dict(pad=3, t_in=2)          # t_in + 2 pad < 9 with t_in >= 1
    ranged = dict(base, t_res=10) if base["res"] else dict(base, res=1, t_res=10)     # 10 residual frames: the last output frame reads past them
    return ((dict(base, y=None), b"null pointer"),
            (dict(base, res=1, c_res=32), b"identity residual needs c_res == c_out"),
            (dict(base, **short), b"t_in too short for kernel"),
            (ranged, b"residual frames out of range"))


def test_winograd_entries_report_the_direct_entrys_errors_without_a_gpu():
    """csk_tcn_stage_wino_f32 / _ext_f32 (both strides) / _valid_f32: a call their gate refuses (-2 inside) goes to csk_tcn_stage_f32,
    and what that refuses comes back as -1 with its message; nothing is launched."""
    lib = pkg.native.lib()
    for name, call, base in _wino_entries(lib):
        for kw, msg in _both_refuse_faults(base):
            assert call(**kw) == -1, (name, kw)
            assert lib.csk_last_error() == b"tcn_stage: " + msg, (name, kw, lib.csk_last_error())
        # two faults: the first in the direct entry's order
        assert call(**dict(base, y=None, res=1, c_res=32)) == -1 and lib.csk_last_error() == b"tcn_stage: null pointer", name
        assert call(**dict(base, res=1, c_res=32, t_res=10)) == -1, name
        assert lib.csk_last_error() == b"tcn_stage: identity residual needs c_res == c_out", name


def test_winograd_valid_res_entry_refuses_without_falling_back_and_without_a_gpu():
    """csk_tcn_stage_wino_valid_res_f32 answers -2 to what its kernel does not take -- the same faults, and c_res = 24 (not whole
    16-channel chunks of the residual image) -- and leaves the direct entry to its caller."""
    lib = pkg.native.lib()

    def call(y=_FAKE, x_res=_FAKE, w_res=_FAKE, **kw):
        return lib.csk_tcn_stage_wino_valid_res_f32(y, x_res, w_res, _FAKE, _FAKE, *_tcn_args(**kw), _FAKE, None)
    base = dict(stride=1, pad=0, res=2, res_off=4)
    for kw, _ in _both_refuse_faults(base):
        assert call(**kw) == -2, kw
    assert call(**dict(base, c_res=24)) == -2
    assert call(**dict(base, c_res=8)) == -2
    assert call(**dict(base, w_res=None)) == -2


def test_direct_and_bf16x3_tcn_entries_share_their_argument_checks_each_under_its_own_name():
    """csk_tcn_stage_f32 and csk_tcn_stage_bf16x3: every shared fault is reported, with the entry's own prefix; for a call with two
    faults the first in the order the entries have always checked them is reported."""
    lib = pkg.native.lib()

    def entry(fn):
        return lambda y=_FAKE, x_res=_FAKE, w_res=_FAKE, **kw: fn(y, _FAKE, x_res, w_res, _FAKE, _FAKE, *_tcn_args(**kw), None)
    huge = dict(t_in=1 << 20, t_res=1 << 20, v=64)                    # t_in * V = 2^26
    for prefix, call in ((b"tcn_stage: ", entry(lib.csk_tcn_stage_f32)), (b"tcn_stage_bf16x3: ", entry(lib.csk_tcn_stage_bf16x3))):
        def first(msg, **kw):
            assert call(**kw) == -1, (prefix, kw)
            assert lib.csk_last_error() == prefix + msg, (prefix, kw, lib.csk_last_error())
        first(b"null pointer", y=None)
        for kw in (dict(n_seg=0), dict(c=0), dict(c_out=0), dict(t_in=0), dict(v=1), dict(v=65)):
            first(b"bad dims", **kw)
        first(b"t_in too short for kernel", pad=3, t_in=2)
        first(b"residual requested without x_res", x_res=None)
        first(b"identity residual needs c_res == c_out", c_res=32)
        first(b"conv residual without w_res", res=2, w_res=None)
        first(b"residual frames out of range", t_res=10)
        first(b"residual frames out of range", res_off=-1)
        first(b"T*V too large for 32-bit position arithmetic", **huge)
        # two faults
        first(b"null pointer", y=None, c=0)
        first(b"bad dims", c=0, pad=9)
        first(b"t_in too short for kernel", pad=3, t_in=2, x_res=None)
        first(b"residual requested without x_res", x_res=None, c_res=32)
        first(b"identity residual needs c_res == c_out", c_res=32, t_res=10)
        first(b"conv residual without w_res", res=2, w_res=None, t_res=10)
        first(b"residual frames out of range", **dict(huge, t_res=10))
    f32, bf = entry(lib.csk_tcn_stage_f32), entry(lib.csk_tcn_stage_bf16x3)
    # the checks that differ sit between the dims and t_in, in each entry
    assert f32(k=10, t_in=1) == -1 and lib.csk_last_error() == b"tcn_stage: bad k/stride/pad (k <= 9)"
    assert f32(stride=0, c=0) == -1 and lib.csk_last_error() == b"tcn_stage: bad dims"
    assert f32(stride=0, pad=3, t_in=2) == -1 and lib.csk_last_error() == b"tcn_stage: bad k/stride/pad (k <= 9)"
    assert bf(k=5, pad=2, stride=5) == -1
    assert lib.csk_last_error() == b"tcn_stage_bf16x3: the split kernel is built for the 9 x 1 temporal conv (k = 5); use csk_tcn_stage_f32"
    assert bf(stride=5, pad=3, t_in=2) == -1 and lib.csk_last_error() == b"tcn_stage_bf16x3: bad stride/pad (stride <= 4)"
    assert bf(k=5, pad=2, c=0) == -1 and lib.csk_last_error() == b"tcn_stage_bf16x3: bad dims"
    # ... and the entries' own later checks come after the shared ones
    assert lib.csk_tcn_stage_bf16x3(_FAKE, ctypes.c_void_p(0x1004), _FAKE, _FAKE, _FAKE, _FAKE, *_tcn_args(**huge), None) == -1
    assert lib.csk_last_error() == b"tcn_stage_bf16x3: T*V too large for 32-bit position arithmetic"
    assert lib.csk_tcn_stage_bf16x3(_FAKE, ctypes.c_void_p(0x1004), _FAKE, _FAKE, _FAKE, _FAKE, *_tcn_args(), None) == -1
    assert lib.csk_last_error() == b"tcn_stage_bf16x3: packed weights must be 16-byte aligned"
    assert lib.csk_tcn_stage_splitk_f32(_FAKE, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, *_tcn_args(**huge), 0, _FAKE, None) == -1
    assert lib.csk_last_error() == b"tcn_stage: T*V too large for 32-bit position arithmetic"


def test_folded_operand_cache_sees_every_kind_of_weight_edit():
    """_Folded._packed_ops re-reads a snapshot of dict slots instead of walking parameters() on every call; every way the
    weights can change must still refold on the NEXT call: in-place edit, p.data = ..., replaced Parameter, swapped
    sub-module, load_state_dict -- and an untouched module must NOT refold."""
    A = pkg.ntu_graph().A
    blk = pkg.SpatioTemporalBlock(4, 8, A, stride=2).eval()
    ops0 = blk._packed_ops("cpu")
    assert blk._packed_ops("cpu") is ops0                                   # cached
    g0 = blk.gcn._packed_ops("cpu")
    with torch.no_grad():
        blk.tcn.bn.weight.mul_(2.0)                                         # in-place: version counter
    ops1 = blk._packed_ops("cpu")
    assert ops1 is not ops0 and not torch.equal(ops1["w"], ops0["w"])
    assert blk.gcn._packed_ops("cpu") is g0                                 # the graph conv's cache watches its own tensors only
    blk.tcn.t_conv.bias.data = torch.ones_like(blk.tcn.t_conv.bias)         # p.data = ...: storage pointer
    ops2 = blk._packed_ops("cpu")
    assert ops2 is not ops1 and not torch.equal(ops2["bias"], ops1["bias"])
    blk.residual.t_conv.weight = torch.nn.Parameter(torch.zeros_like(blk.residual.t_conv.weight))    # replaced Parameter
    ops3 = blk._packed_ops("cpu")
    assert ops3 is not ops2 and float(ops3["w_res"].abs().max()) == 0.0
    blk.tcn.bn = torch.nn.BatchNorm2d(8).eval()                             # swapped sub-module
    ops4 = blk._packed_ops("cpu")
    assert ops4 is not ops3
    blk.load_state_dict({k: v.clone() + 0.25 for k, v in blk.state_dict().items()})
    assert blk._packed_ops("cpu") is not ops4
    assert blk.gcn._packed_ops("cpu") is not g0                             # load_state_dict copied into the graph conv's tensors too
    net = pkg.StGcn(A, input_shape=(3, 20, 25, 2)).eval()
    n0 = net._packed_ops("cpu")
    with torch.no_grad():
        net.fc.weight.add_(1.0)                                             # not one of the driver's folded tensors
    assert net._packed_ops("cpu") is n0
    with torch.no_grad():
        net.data_bn.running_mean.add_(1.0)
    assert net._packed_ops("cpu") is not n0


def test_co_stack_step_argument_errors_and_host_side_policies():
    """csk_co_stack_step_f32 (a run of blocks in one launch) validates the chain before any launch: block i + 1 must read what
    block i emits.  CoStGcn.set_max_cycle / SplitScratch: host-side logic that needs no GPU."""
    import ctypes as C
    import torch
    pkg = _bootstrap.load()
    lib = pkg.native.lib()

    class Args(C.Structure):
        _fields_ = [("xin", C.c_void_p), ("xin_slots", C.c_int32), ("xin_slot0", C.c_int32), ("c_in", C.c_int32),
                    ("gcn_w", C.c_void_p), ("gcn_bias", C.c_void_p), ("ell_src", C.c_void_p), ("ell_val", C.c_void_p),
                    ("ell_cnt", C.c_int32 * 3), ("ell_w", C.c_int32), ("gcn_res_mode", C.c_int32), ("y_ring", C.c_void_p),
                    ("y_slots", C.c_int32), ("y_slot0", C.c_int32), ("tcn_w", C.c_void_p), ("tcn_bias", C.c_void_p),
                    ("res_mode", C.c_int32), ("x_res_slot0", C.c_int32), ("out", C.c_void_p), ("out_slots", C.c_int32),
                    ("out_slot0", C.c_int32), ("c_out", C.c_int32)]
    blocks = (Args * 2)()
    for i, b in enumerate(blocks):
        b.xin, b.xin_slots, b.xin_slot0, b.c_in = 0x1000 * (i + 1), 12, 3, 64
        for f in ("gcn_w", "gcn_bias", "ell_src", "ell_val", "tcn_w", "tcn_bias"):
            setattr(b, f, 0x9000)
        b.ell_cnt[0], b.ell_cnt[1], b.ell_cnt[2], b.ell_w, b.gcn_res_mode = 1, 1, 4, 4, 1
        b.y_ring, b.y_slots, b.y_slot0, b.res_mode, b.x_res_slot0 = 0x5000 * (i + 1), 16, 3, 1, 11
        b.out, b.out_slots, b.out_slot0, b.c_out = 0x1000 * (i + 2), 12, 3, 64
    call = lambda n: lib.csk_co_stack_step_f32(n, C.byref(blocks), 8, 25, 200, None)
    assert call(0) == -1 and b"blocks expected" in lib.csk_last_error()
    assert call(5) == -1 and b"blocks expected" in lib.csk_last_error()
    blocks[1].xin_slot0 = 4                      # block 1 would read a slot block 0 does not write this cycle
    assert call(2) == -1 and b"does not read what block 0 emits" in lib.csk_last_error()
    blocks[1].xin_slot0, blocks[1].c_in = 3, 32
    assert call(2) == -1 and b"does not read what block 0 emits" in lib.csk_last_error()
    # set_max_cycle: range check, re-bind on change
    net = pkg.CoStGcn(pkg.ntu_graph().A).eval()
    assert net.max_cycle == 8
    net._n = 5
    net.set_max_cycle(4)
    assert net.max_cycle == 4 and net._n is None
    for bad in (0, 9, 2.5):
        with pytest.raises(ValueError):
            net.set_max_cycle(bad)
    # SplitScratch: one buffer per (device, stream), superseded buffers stay alive until release()
    from continual_skeletons_amd import blocks as blk
    sc = blk.SplitScratch()
    assert sc.nbytes() == 0
    m = pkg.StGcn(pkg.ntu_graph().A).eval()
    pkg.set_clip_latency_mode(m, 4)
    shared = {id(mod.__dict__["_split_scratch"]) for mod in m.modules() if "_split_scratch" in mod.__dict__}
    assert len(shared) == 1                      # one scratch for the whole tree
    pkg.set_clip_latency_mode(m, 0)
    assert all(mod.__dict__.get("_split_scratch") is None for mod in m.modules() if "_split_scratch" in mod.__dict__)


def test_head_and_input_entry_points_validate_their_arguments_without_a_gpu():
    """csk_input_norm_f32, csk_pool_fc_f32, csk_pool_scaled_f32, csk_fc_f32, csk_co_spatial_pool_f32, csk_co_window_mean_f32:
    null pointers, non-positive dims, streams that do not fit a frame row, a ring position outside the window and the FC's
    alignment rule are reported before anything is launched (every call here fails its guard)."""
    import ctypes as C
    lib = pkg.native.lib()
    fake, skew = C.c_void_p(0x1000), C.c_void_p(0x1004)

    def refused(rc, why):
        assert rc == -1 and why in lib.csk_last_error(), (rc, why, lib.csk_last_error())

    def norm(x=fake, scale=fake, shift=fake, h=fake, N=2, Cc=3, T=5, V=25, M=2):
        return lib.csk_input_norm_f32(x, scale, shift, h, N, Cc, T, V, M, Cc * T * V, T * V, None)
    for kw in (dict(x=None), dict(scale=None), dict(shift=None), dict(h=None)):
        refused(norm(**kw), b"input_norm: null pointer")
    for kw in (dict(N=0), dict(Cc=0), dict(T=0), dict(V=-1), dict(M=0)):
        refused(norm(**kw), b"input_norm: bad dims")

    def pool_fc(h=fake, feat=fake, N=2, M=2, Cc=8, TV=50):
        return lib.csk_pool_fc_f32(h, fake, fake, feat, fake, N, M, Cc, TV, 5, None)
    for kw in (dict(h=None), dict(feat=None)):
        refused(pool_fc(**kw), b"pool_fc: null pointer")
    for kw in (dict(N=0), dict(M=0), dict(Cc=-4), dict(TV=0)):
        refused(pool_fc(**kw), b"pool_fc: bad dims")

    def pool_scaled(h=fake, feat=fake, N=2, M=2, Cc=8, TV=50):
        return lib.csk_pool_scaled_f32(h, feat, N, M, Cc, TV, 0.75, None)
    for kw in (dict(h=None), dict(feat=None)):
        refused(pool_scaled(**kw), b"pool_scaled: null pointer")
    for kw in (dict(N=-1), dict(M=0), dict(Cc=0), dict(TV=0)):
        refused(pool_scaled(**kw), b"pool_scaled: bad dims")

    def fc(feat=fake, w=fake, b=fake, logits=fake, N=2, Cc=8, classes=5):
        return lib.csk_fc_f32(feat, w, b, logits, N, Cc, classes, None)
    for kw in (dict(feat=None), dict(w=None), dict(b=None), dict(logits=None)):
        refused(fc(**kw), b"fc: null pointer")
    for kw in (dict(N=0), dict(Cc=0), dict(classes=0)):
        refused(fc(**kw), b"fc: bad dims")
    for kw in (dict(feat=skew), dict(w=skew), dict(feat=skew, Cc=256), dict(feat=C.c_void_p(0x1008))):
        refused(fc(**kw), b"16-byte aligned when C is a multiple of 4")

    def spatial(h=fake, feat=fake, N=2, Cc=256, MV=50, P=100):
        return lib.csk_co_spatial_pool_f32(h, feat, N, Cc, MV, P, None)
    for kw in (dict(h=None), dict(feat=None)):
        refused(spatial(**kw), b"co_spatial_pool: null pointer")
    for kw in (dict(N=0), dict(Cc=0), dict(MV=0), dict(P=99), dict(N=3)):          # N MV > P: the streams do not fit a row
        refused(spatial(**kw), b"co_spatial_pool: bad dims")

    def mean(ring=fake, pooled=fake, n_elem=512, window=4, head=0, count=1):
        return lib.csk_co_window_mean_f32(ring, pooled, n_elem, window, head, count, None)
    for kw in (dict(ring=None), dict(pooled=None)):
        refused(mean(**kw), b"co_window_mean: null pointer")
    for kw in (dict(n_elem=0), dict(window=0), dict(head=-1), dict(head=4), dict(count=-1), dict(count=5)):
        refused(mean(**kw), b"co_window_mean: bad dims")
