"""The rings of a ``CoStGcn`` slab, described ONCE ("The ring inventory"): ``SlabRings._rings()`` yields one
``Ring`` per ring.  Reset (co_reset.py), move (co_migrate.py), priming (co_prime.py) and the model's bytes / snapshot / clean
(continual.py) read it and name no ring; the native job structs are built here from an entry.  The per-stream arrays of the
input pre-passes come from the stage protocol (input_stage.py) and pass through here as one-slot rings when they move."""
from typing import NamedTuple, Optional

import torch

from . import native

XIN0, POOL = "xin0", "pool"     # the names in records, test data and tools; nothing in the package compares them


def block_ring_names(n_blocks):
    """[(post-GCN ring, output ring)] of blocks 0 .. n_blocks - 1; the clip tensors of the same frames go by the same names."""
    return [(f"y{i}", f"out{i}") for i in range(n_blocks)]


class Ring(NamedTuple):
    name: str
    kind: int                       # native.SCRUB_BLOCK_RING [depth][rows][P]: stream n owns seg floats of every row;
    #                                 native.SCRUB_POOL_RING [depth][N][seg]: stream n owns row n of every slot
    rows: int                       # rows of a slot one stream has a segment in
    seg: int                        # 32-bit words of a segment
    window: Optional[int]           # newest slots a future launch can still read; None: state, but in no record
    level: Optional[int]            # producer level L: the ring has received e(L) frames and is live once age >= D(L)
    source: Optional[str]           # the clip tensor whose frame j is frame j of the ring
    tensor: Optional[torch.Tensor] = None   # [depth][rows or N][row floats], on a bound slab
    counter: Optional[int] = None   # index in ``_ctr`` of the count of frames the ring has received


def ring_window(count: int, depth: int, window: int):
    """(newest, window) as ``csk_move_job`` takes them, for a ring of ``depth`` slots that has received ``count`` frames:
    the slot of frame count - 1 and how many newest slots move."""
    if not 0 <= window <= depth:
        raise ValueError(f"a window of {window} slots in a ring of {depth}")
    return (count - 1) % depth, window


def window_slots(newest: int, depth: int, window: int):
    """The slots a job (newest, window) covers in a ring of ``depth`` slots, OLDEST first: the order of the packed record
    (the arithmetic of csk_co_move_streams_f32)."""
    return [(newest + 1 - window + i) % depth for i in range(window)]


def array_ring(entry, tensor):
    """A per-stream array of a pre-pass (one ``windows()`` entry and its ``state()`` tensor) as a ring of one slot and one row
    of 32-bit words, the way the move entry takes it."""
    name, rows, seg, window = entry
    return Ring(name, native.SCRUB_BLOCK_RING, rows, seg, window, None, None, tensor.view(torch.int32).view(1, 1, -1))


# The job structs name a ring of either kind by its tensor: [depth][rows][row_floats] (include/cskel.h).
def scrub_job(ring, first, count):
    """``csk_scrub_job`` for the slots of frames ``first .. first + count - 1`` (frame numbers, taken modulo the depth)."""
    depth, rows, row_floats = ring.tensor.shape
    return native.ScrubJob(ring.tensor.data_ptr(), row_floats, depth, rows, first % depth, min(count, depth), ring.seg, ring.kind)


def move_job(ring, count, offset):
    """``csk_move_job`` for the window of a ring that has received ``count`` frames, at ``offset`` in the record."""
    depth, rows, row_floats = ring.tensor.shape
    newest, window = ring_window(count, depth, ring.window)
    return native.MoveJob(ring.tensor.data_ptr(), row_floats, offset, depth, rows, newest, window, ring.seg, ring.kind)


class SlabRings:
    """Base class of ``CoStGcn``: the inventory.  Its state is ``_bound_rings``, the entries of the bound slab, made once by
    ``_bind`` next to the tensors they name (exports and scrubs are launch-bound: they do not describe the slab again)."""

    def _rings(self):
        """The inventory: of the bound slab, else from the blocks alone (tensors None)."""
        return self._bound_rings if self._n is not None else self._describe_rings(False)

    def _describe_rings(self, bound):
        """[Ring] in slab order, which is record order (every saved ``StreamState`` depends on it); windows, levels and counters
        as DESIGN.md section 3 derives them: (k - 1) / 2 of an input ring (the residual lag of ``engine_advance``), k - 1 of a
        post-GCN ring, none of the last output ring; ``_ctr`` is {frames, features, (received, emitted) per block}."""
        c, _, v, m = self.input_shape
        mv, blks = m * v, self._blocks
        block, lags = native.SCRUB_BLOCK_RING, [(blk.kernel_size - 1) // 2 for blk in blks] + [None]
        out = [Ring(XIN0, block, c, mv, lags[0], 0, XIN0, self._xin0 if bound else None, 0)]
        for i, (blk, (y_name, out_name)) in enumerate(zip(blks, block_ring_names(len(blks)))):
            y, o = (blk._state.y, blk._state.out) if bound else (None, None)
            out.append(Ring(y_name, block, blk.out_channels, mv, blk.kernel_size - 1, i, y_name, y, 2 + 2 * i))
            out.append(Ring(out_name, block, blk.out_channels, mv, lags[i + 1], i + 1, out_name, o, 3 + 2 * i))
        out.append(Ring(POOL, native.SCRUB_POOL_RING, 1, blks[-1].out_channels, self.pool_size, len(blks), out_name,
                        self._pool_ring if bound else None, 1))
        return out

    def _record_rings(self):
        """The rings a record holds: those with a window."""
        return [ring for ring in self._rings() if ring.window is not None]
