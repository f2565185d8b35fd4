"""numpy restatement of the Kinetics keypoint intake (include/cskel.h: csk_select_people_f32), written
from the definition and independent of the package: per (sample, frame) the people are ordered by their fp64 score sums --
larger first, equal sums by index, NaN sums last and by index among themselves -- the best M are kept, x and y are centred, y
is flipped, and the coordinates of joints whose score compares equal to 0 come out as +0."""
import numpy as np


def score_sums(k):
    """k (..., P, V, 3) fp32 -> (..., P) fp64: the joint scores of a person added in fp64, v ascending."""
    s = np.zeros(k.shape[:-2], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for v in range(k.shape[-2]):
            s = s + k[..., v, 2].astype(np.float64)
    return s


def ranks(sums):
    """(..., P) fp64 sums -> (..., P) int: how many people are placed before person p."""
    p = sums.shape[-1]
    idx = np.arange(p)
    q_first = idx[:, None] < idx[None, :]                           # [q, p]: q has the smaller index
    sq, sp = sums[..., :, None], sums[..., None, :]
    nan_q, nan_p = np.isnan(sq), np.isnan(sp)
    with np.errstate(invalid="ignore"):
        numbers = (sq > sp) | ((sq == sp) & q_first)
    before = np.where(nan_q | nan_p, np.where(nan_q == nan_p, q_first, nan_p), numbers) & ~np.eye(p, dtype=bool)
    return before.sum(axis=-2)


def order_people(sums):
    """(P,) fp64 sums -> list of the P person indices, first placed first."""
    rank = ranks(np.asarray(sums, dtype=np.float64))
    assert sorted(rank.tolist()) == list(range(len(rank)))          # the rule is a total order
    return np.argsort(rank, kind="stable").tolist()


def select_people_clip(k, people_out=2):
    """k (N, T, P, V, 3) fp32 -> (N, 3, T, V, people_out) fp32."""
    k = np.asarray(k)
    assert k.dtype == np.float32 and k.ndim == 5 and k.shape[4] == 3 and 1 <= people_out <= k.shape[2]
    order = np.argsort(ranks(score_sums(k)), axis=-1, kind="stable")[..., :people_out]         # (N, T, M)
    kept = np.take_along_axis(k, order[..., None, None], axis=2)                                 # (N, T, M, V, 3)
    x, y, s = kept[..., 0], kept[..., 1], kept[..., 2]
    half, zero = np.float32(0.5), np.float32(0.0)
    absent = s == 0                                                 # -0.0 counts as 0; a NaN score does not
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.stack([np.where(absent, zero, x - half), np.where(absent, zero, -(y - half)), s], axis=1)      # (N, 3, T, M, V)
    assert out.dtype == np.float32
    return np.ascontiguousarray(out.transpose(0, 1, 2, 4, 3))


def select_frame(k, people_out):
    """k (P, V, 3) fp32 -> (3, V, people_out) fp32."""
    return select_people_clip(k[None, None], people_out)[0, :, 0]
