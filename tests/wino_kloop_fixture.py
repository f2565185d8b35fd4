"""Cases, operands and the fp64 reference shared by tests/test_gpu_wino_kloop.py and tests/test_wino_kloop_fixture_cpu.py.

The K loop of the Winograd clip temporal convs (csrc/tcn_wino.hip) reads its LDS operands ahead of the MFMAs that use them: A
fragments two MFMA pairs ahead, raw samples half a K step ahead, across the group segments of an 8-channel chunk, with one
frame per K step handed from a group to the next in a register.  What can go wrong is an operand of the wrong step, group or
chunk, so the cases are the smallest that reach every chunk count pattern (C = 8: the peeled chunk alone; 16: one loop trip and
the peel; 24: two trips), both staging paths (T = 7: odd, every tile a border tile; T = 40 at V = 25 and T = 56 at V = 18:
interior tiles in both workgroup shapes), both workgroup shapes, stride 2 with both patterns of the residual loop (16 and 24
residual channels) and without, and the valid form with the identity and with the conv residual.

Operands are integer valued (the value ranges of tests/tcn_border_fixture.py) so that every product and partial sum is exact in
fp32 in any order: the kernels must equal the fp64 conv bit for bit.  The tile arithmetic restates the launchers' formulas."""
import torch
import torch.nn.functional as F

from tests import tcn_border_fixture as bf

N_SEG = 3
C_IN = (8, 16, 24)
C_OUT = (64, 128)                                    # 64: the wide shape only; 128: wide and tall
SHAPES = ((25, 7), (25, 40), (18, 7), (18, 56))      # (V, output frames of the stride-1 forms)
S2_CRES = (0, 16, 24)                                # stride 2: no residual, conv residual of two and of three chunks
VALID_CRES = 16
ACT, W_EVEN, W_RES, BIAS = bf.ACT, bf.W_EVEN, bf.W_RES, bf.BIAS


def cases():
    """(form, V, C, C_out, T_in, residual, C_res) of every launch"""
    out = []
    for v, t in SHAPES:
        for c in C_IN:
            for co in C_OUT:
                out.append(("s1", v, c, co, t, "identity", co))
                for c_res in S2_CRES:
                    out.append(("s2", v, c, co, 2 * t - 1, "conv" if c_res else "none", c_res))
                out.append(("valid", v, c, co, t + 8, "identity", co))
                out.append(("valid", v, c, co, t + 8, "conv", VALID_CRES))
    return out


def case_id(case):
    form, v, c, co, t, res, c_res = case
    return f"{form}-V{v}-C{c}to{co}-T{t}-{res}{c_res if res == 'conv' else ''}"


def partial_sum_bound():
    return max(bf.partial_sum_bound(c, r) for c in C_IN for r in S2_CRES + (VALID_CRES,))


def _ints(gen, shape, lo, hi, step=1):
    return (torch.randint(0, (hi - lo) // step + 1, shape, generator=gen) * step + lo).float()


def operands(case, seed, floats=False):
    form, v, c, co, t, res, c_res = case
    g = torch.Generator().manual_seed(seed)
    if floats:
        rnd = lambda shape, *_: torch.rand(shape, generator=g) - 0.5
    else:
        rnd = lambda shape, lo, hi, step=1: _ints(g, shape, lo, hi, step)
    d = dict(form=form, v=v, c=c, co=co, t=t, res=res)
    d["y"] = rnd((N_SEG, c, t, v), -ACT, ACT)
    d["w"] = rnd((co, c, 9, 1), -W_EVEN, W_EVEN, 2)
    d["bias"] = rnd((co,), -BIAS, BIAS)
    if res == "identity":
        d["x"] = rnd((N_SEG, co, t, v), -ACT, ACT)
    elif res == "conv":
        d["x"] = rnd((N_SEG, c_res, t, v), -ACT, ACT)
        d["wres"] = rnd((co, c_res, 1, 1), -W_RES, W_RES)
    return d


def stride_pad(form):
    return (2, 4) if form == "s2" else (1, 0) if form == "valid" else (1, 4)


def conv64(d):
    """the temporal conv alone, fp64"""
    stride, pad = stride_pad(d["form"])
    return F.conv2d(d["y"].double(), d["w"].double(), d["bias"].double(), stride=(stride, 1), padding=(pad, 0))


def reference(d):
    """conv + residual, ReLU: fp64 on the host, cast to fp32"""
    stride, _ = stride_pad(d["form"])
    out = conv64(d)
    valid = d["form"] == "valid"
    if d["res"] == "identity":
        out = out + (d["x"][:, :, 4: d["t"] - 4] if valid else d["x"]).double()
    elif d["res"] == "conv":
        x = d["x"].double()
        out = out + F.conv2d(x[:, :, 4: d["t"] - 4] if valid else x, d["wres"].double(), stride=(stride, 1))
    return torch.relu(out).float()


def tiles(form, t_in, v, mw):
    """interior flag of every column tile of one sequence in the wide (mw = 1) or the tall (mw = 2) workgroup shape"""
    t_out = {"s1": t_in, "valid": t_in - 8, "s2": (t_in - 1) // 2 + 1}[form]
    qp, nt = (t_out + 1) // 2 * v, 128 // mw
    out = []
    for q0 in range(0, qp, nt):
        ja, jb = q0 // v, (min(q0 + nt, qp) - 1) // v
        if form == "s2":
            fa, span = 4 * ja - 4, (4 * (jb - ja) + 11) * v
        else:
            fa, span = (2 * ja if form == "valid" else 2 * ja - 4), (2 * (jb - ja) + 10) * v
        out.append(fa >= 0 and fa * v + 4 * ((span + 3) // 4) <= t_in * v)
    return out
