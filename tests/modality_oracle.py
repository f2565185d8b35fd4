"""numpy restatement of the bone / motion input modalities (test infrastructure).

Clip form = the reference's offline scripts (datasets/data_preparation/bone_data_prep.py:158-163,
motion_data_prep.py:28-30); tests/golden/g13_modalities.npz holds what those scripts themselves wrote, and
tests/test_modality_cpu.py checks this restatement against it bit for bit.  Step form = the causal backward difference
the continual path uses.  All arithmetic in float32: one rounding per subtraction, as numpy does on float32 arrays."""
import numpy as np

MODALITIES = ("joint", "bone", "joint_motion", "bone_motion")


def bone(x, parents):
    """(..., V, M) float32: b[v] = x[v] - x[parents[v]], both read from x."""
    x = np.asarray(x, dtype=np.float32)
    return x - x[..., np.asarray(parents, dtype=np.int64), :]


def motion(x):
    """(N, C, T, V, M): m[t] = x[t+1] - x[t], m[T-1] = 0."""
    x = np.asarray(x, dtype=np.float32)
    m = np.zeros_like(x)
    m[:, :, :-1] = x[:, :, 1:] - x[:, :, :-1]
    return m


def derive_clip(x, modality, parents):
    """The clip a model of ``modality`` is fed, from the joint clip (N, C, T, V, M)."""
    x = np.asarray(x, dtype=np.float32)
    if modality == "joint":
        return x
    if modality == "bone":
        return bone(x, parents)
    if modality == "joint_motion":
        return motion(x)
    if modality == "bone_motion":
        return motion(bone(x, parents))
    raise ValueError(modality)


def derive_steps(x, modality, parents, first=None):
    """Continual form over a whole sequence (N, C, T, V, M): bone per frame; motion as the backward difference
    m'[s] = x[s] - x[s-1] with m'[s] = 0 where ``first[n, s]`` (bool (N, T); default: s == 0 only) marks a stream's first
    frame."""
    x = np.asarray(x, dtype=np.float32)
    if modality in ("joint", "bone"):
        return derive_clip(x, modality, parents)
    base = bone(x, parents) if modality == "bone_motion" else x
    out = np.zeros_like(base)
    out[:, :, 1:] = base[:, :, 1:] - base[:, :, :-1]
    if first is not None:
        first = np.asarray(first, dtype=bool)
        out[np.broadcast_to(first[:, None, :, None, None], out.shape)] = 0.0
    return out
