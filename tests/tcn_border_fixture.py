"""Shapes, value ranges and tile arithmetic shared by tests/test_gpu_tcn_border_tiles.py and tests/test_tcn_border_fixture_cpu.py.

The Winograd clip temporal convs (csrc/tcn_wino.hip) stage a tile's activations with 16-byte loads when the staged span lies
inside the sequence (interior tile) and element-wise, with the conv's zero padding filled in, when it crosses either end (border
tile).  The cases below are small sequences that are all border, sequences at which the first interior tile appears, and residual
channel counts that cut the stride-2 residual phase into 16-channel steps with and without an 8-channel remainder (a lone 8, 16,
16 + 8, 16 + 16 + 8: one, two, three and five of the kernel's 8-channel chunks, the 3-channel case with clamped padding rows).

Operands are integer valued so that every product and every partial sum is exact in fp32 in any order (partial_sum_bound): the
kernels must equal an fp64 conv bit for bit.  The tile arithmetic restates the launchers' formulas; nothing is read from csrc."""

N_SEG = 3
JOINTS = (25, 18)
C_IN = (3, 16, 24)
C_OUT = (64, 128)
S1_T = (1, 2, 9, 10, 11, 21, 40)                     # stride 1, pad 4: identity residual and none
S2_T = (1, 2, 3, 5, 19, 20, 21, 22, 61)              # stride 2, pad 4: conv residual and none
S2_CRES = (3, 8, 16, 24, 40)
VALID_T = (9, 10, 17, 30)                            # stride 1, pad 0, conv residual on the centred shrink
VALID_CRES = (16, 32)
LONG_S1 = (61, 8, 8)                                 # (frames, zero frames in front, zero frames behind) of the embedding test
LONG_S2 = (121, 8, 11)

ACT = 3            # activations and block inputs: integers in [-ACT, ACT]
W_EVEN = 4         # conv weights: even integers in [-W_EVEN, W_EVEN], so the F(2, 3) images (w0 +- w1 + w2) / 2 are integers
W_RES = 3          # residual conv weights: integers in [-W_RES, W_RES]
BIAS = 8           # bias: integers in [-BIAS, BIAS]


def partial_sum_bound(c_in, c_res, groups=4):
    """Largest magnitude any partial sum of a launch can reach, over the Winograd kernels (four accumulator sets, `groups` groups
    of c_in products each; the stride-2 residual adds c_res products to two of the sets; the output transform adds three sets,
    the bias and an identity residual) and the direct kernels (9 c_in + c_res products).  Below 2^24 every integer is an fp32."""
    image = max(W_EVEN, 3 * W_EVEN // 2)             # |(w0 +- w1 + w2) / 2| <= 3 W / 2
    operand = 2 * ACT                                # |d0 - d2|, |d1 + d2|, ... <= 2 ACT
    acc = groups * c_in * image * operand + c_res * W_RES * operand
    wino = 3 * acc + BIAS + ACT
    direct = 9 * c_in * W_EVEN * ACT + c_res * W_RES * ACT + BIAS + ACT
    return max(wino, direct)


def _ceil_to(a, b):
    return (a + b - 1) // b * b


def pick_mw(qp, c_out, stride):
    """workgroup shape of a launch with qp pair columns per sequence: 1 = 64 channels x 128 columns, 2 = 128 x 64"""
    if c_out % 128:
        return 1
    if stride == 2:
        return 2
    return 2 if 16 * _ceil_to(qp, 64) <= 15 * _ceil_to(qp, 128) else 1


def tiles(form, t_in, v, c_out):
    """The column tiles of one sequence: form 's1' (stride 1, pad 4), 'valid' (stride 1, pad 0) or 's2' (stride 2, pad 4).  Per
    tile: the first and last output frame pair (ja, jb) and whether the staged span lies inside the sequence."""
    stride = 2 if form == "s2" else 1
    t_out = {"s1": t_in, "valid": t_in - 8, "s2": (t_in - 1) // 2 + 1}[form]
    qp = (t_out + 1) // 2 * v
    nt = 128 // pick_mw(qp, c_out, stride)
    out = []
    for q0 in range(0, qp, nt):
        qend = min(q0 + nt, qp)
        ja, jb = q0 // v, (qend - 1) // v
        if form == "s2":
            fa, span = 4 * ja - 4, (4 * (jb - ja) + 11) * v
        else:
            fa, span = (2 * ja if form == "valid" else 2 * ja - 4), (2 * (jb - ja) + 10) * v
        interior = fa >= 0 and fa * v + 4 * ((span + 3) // 4) <= t_in * v
        out.append(dict(ja=ja, jb=jb, interior=interior, frames=range(2 * ja, min(2 * jb + 2, t_out))))
    return out


def res_chunks(c_res):
    """the residual channels (padded to 8, as the kernel's K loop runs them) as 16-channel steps and a final 8-channel remainder"""
    cend = _ceil_to(c_res, 8)
    return [16] * (cend // 16) + [8] * (cend % 16 == 8)
