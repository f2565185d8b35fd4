"""Host model of the stride-2 polyphase Winograd temporal conv (csrc/tcn_wino.hip, tcn_stage_wino_s2_kernel), shared by the CPU
fold tests and the GPU tests: the kernel's arithmetic -- polyphase groups, input transforms with the skipped point-inf products,
the d2 := d1 form of the 1 x 1 stride-2 residual, the output transform -- from the packed image, in a chosen float type."""
import numpy as np

# (first image row, raw frame offset F of the group's sample d0 relative to frame 4 j - 4, products): E0, E1, O0, O1
GROUPS = ((0, 0, 4), (4, 6, 3), (7, 1, 3), (10, 5, 3))


def direct_s2(y, w, x=None, wres=None):
    """fp64 reference: (C, T, V) input, (Co, C, 9) weight -> (Co, To, V), out[t] = sum_r w[r] y[2 t + r - 4] (+ wres . x[2 t])."""
    c, t, v = y.shape
    to = (t - 1) // 2 + 1
    yp = np.zeros((c, 2 * to + 8, v))
    yp[:, 4:4 + t] = y
    out = sum(np.einsum("oc,ctv->otv", w[:, :, r], yp[:, r:r + 2 * to:2]) for r in range(9))
    if x is not None:
        out = out + np.einsum("oc,ctv->otv", wres, x[:, ::2])
    return out


def wino_s2(y, img, co, x=None, wres=None, dtype=np.float64):
    """The kernel's arithmetic from the packed image [13][Cpad][Mpad]; x (Cres, T, V) / wres (Co, Cres): the conv residual.
    Every operand, transform, product sum and the output transform is held in ``dtype``."""
    c, t, v = y.shape
    to = (t - 1) // 2 + 1
    npair = (to + 1) // 2
    yp = np.zeros((c, 4 * npair + 11, v), dtype=dtype)          # raw frames -4 .. 4 npair + 6
    yp[:, 4:4 + t] = y.astype(dtype)
    u = img[:, :c, :co].astype(dtype)
    m = np.zeros((4, co, npair, v), dtype=dtype)
    for row0, f, npts in GROUPS:
        d = [yp[:, f + 2 * i: f + 2 * i + 4 * npair: 4] for i in range(npts)]       # frames 4 j - 4 + F + 2 i
        b = [d[0] - d[2], d[1] + d[2], d[2] - d[1]] + ([d[1] - d[3]] if npts == 4 else [])
        for i in range(npts):
            m[i] += np.einsum("co,cjv->ojv", u[row0 + i], b[i]).astype(dtype)
    if x is not None:
        cr = x.shape[0]
        xp = np.zeros((cr, 4 * npair + 3, v), dtype=dtype)
        xp[:, :t] = x.astype(dtype)
        d0, d1 = xp[:, 0:4 * npair:4], xp[:, 2:2 + 4 * npair:4]                     # x[4 j], x[4 j + 2]
        wr = wres.astype(dtype)
        m[0] += np.einsum("oc,cjv->ojv", wr, d0 - d1).astype(dtype)
        m[1] += np.einsum("oc,cjv->ojv", wr, d1).astype(dtype)
    out = np.zeros((co, 2 * npair, v), dtype=dtype)
    out[:, 0::2] = m[0] + m[1] + m[2]
    out[:, 1::2] = m[1] - m[2] - m[3]
    return out[:, :to]
