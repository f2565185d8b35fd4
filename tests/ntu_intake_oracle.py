"""Numpy restatement of the NTU body intake (include/cskel.h: csk_ntu_intake_f32), test infrastructure only.

Written from the definition, not from the kernel: flags by ``any(x != 0)``, energies in fp64 with numpy's own summation, the
order by a sort on (energy, slot), the source frames as explicit lists.  The energies differ from the kernel's in the last
bits (another summation order), so the oracle decides ranks the same way only where energies are well apart or exactly tied
by identical data; ``energy_gaps`` measures that."""
import numpy as np


def null_flags(bodies):
    """(T, P, V, 3) -> (P, T) bool: frame t of body p is non-null (any value != 0; -0.0 is zero, NaN is not)."""
    return (bodies != 0).any(axis=(2, 3)).T


def energies(bodies):
    """(T, P, V, 3) -> (P,) fp64: sum over the coordinates of the population std over (non-null frames x V); 0 if there are none."""
    present = null_flags(bodies)
    out = np.zeros(bodies.shape[1], dtype=np.float64)
    for p in range(bodies.shape[1]):
        x = bodies[present[p], p].astype(np.float64).reshape(-1, 3)
        if len(x):
            mean = x.sum(axis=0) / len(x)
            out[p] = np.sqrt(((x - mean) ** 2).sum(axis=0) / len(x)).sum()
    return out


def order_bodies(energy):
    """Slots by descending energy; equal energies: the higher slot first; NaN behind every number."""
    nan = [p for p in range(len(energy)) if energy[p] != energy[p]]
    num = [p for p in range(len(energy)) if energy[p] == energy[p]]
    return sorted(num, key=lambda p: (energy[p], p), reverse=True) + sorted(nan, reverse=True)


def energy_gaps(energy):
    """Smallest relative distance between two energies of a clip that are not bit-identical (inf if there is none)."""
    e = np.unique(np.asarray(energy, dtype=np.float64))
    return min(((b - a) / b for a, b in zip(e, e[1:])), default=np.inf)


def source_frames(present, frames_out):
    """(T,) bool flags of one body -> (L, frame-0-null, src): src[t] = the input frame of output frame t (None: empty body)."""
    idx = np.flatnonzero(present)
    if len(idx) == 0:
        return 0, True, None
    first_null = not present[0]
    if first_null:
        table = idx                                 # compacted: the non-null frames in order
    else:
        table = np.arange(idx[-1] + 1)              # gaps stay; the clip ends behind its last non-null frame
    return len(table), first_null, table[np.arange(frames_out) % len(table)]


def plan_clip(bodies, frames_out, bodies_out):
    """(T, P, V, 3) -> [(slot, L, frame-0-null)] of the kept bodies, in output order."""
    present = null_flags(bodies)
    order = order_bodies(energies(bodies))[:bodies_out]
    return [(p,) + source_frames(present[p], frames_out)[:2] for p in order]


def select_only(bodies, frames_out, bodies_out=2):
    """The kept bodies placed into ``frames_out`` frames, zeros behind frame T (read_xyz + gendata): (3, frames_out, V, M)."""
    t, _, v, _ = bodies.shape
    out = np.zeros((3, frames_out, v, bodies_out), dtype=np.float32)
    for m, p in enumerate(order_bodies(energies(bodies))[:bodies_out]):
        out[:, :t, :, m] = bodies[:, p].transpose(2, 0, 1)
    return out


def select_bodies(bodies, frames_out=None, bodies_out=2):
    """One clip (T, P, V, 3) fp32 -> (3, frames_out, V, bodies_out) fp32, sections (a)-(d) of the definition."""
    t, _, v, _ = bodies.shape
    frames_out = t if frames_out is None else frames_out
    present = null_flags(bodies)
    out = np.zeros((3, frames_out, v, bodies_out), dtype=np.float32)
    for m, p in enumerate(order_bodies(energies(bodies))[:bodies_out]):
        src = source_frames(present[p], frames_out)[2]
        if src is not None:
            out[:, :, :, m] = bodies[src, p].transpose(2, 0, 1)
    return out


def select_bodies_clip(bodies, frames_out=None, bodies_out=2):
    """(N, T, P, V, 3) -> (N, 3, frames_out, V, bodies_out)."""
    return np.stack([select_bodies(b, frames_out, bodies_out) for b in bodies])
