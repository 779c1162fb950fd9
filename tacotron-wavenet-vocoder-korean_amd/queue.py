"""Utterance queue: the static schedule that puts a list of utterances of any lengths on a fixed set of stream slots.

The vocoder's step time does not depend on the batch (a stream is latency-bound), so a batch costs its longest member and a slot
whose utterance has ended idles until the batch is done.  The reference never pads (generate.py:151-155 vocodes one mel of its own
length per run); here a slot takes the next utterance at the next CHUNK boundary instead: generation runs in launches of
`chunk_frames` mel frames for all slots, and between two launches a slot that has finished is reset (twv_wavenet_reset_streams) and
handed the next utterance.  This module is the host-side planner: pure Python / numpy, no device.

Table layout (what twv_wavenet_queue_stage / _collect read, include/twv_amd.h): int32 (n_chunks, n_slots, 4) =
{utterance index or -1 for an idle slot, first frame of the piece, valid frames, 1 where the utterance starts in this chunk}."""
import heapq
from collections import namedtuple

import numpy as np

UTT, FIRST, VALID, START = 0, 1, 2, 3
ORDERS = ("longest_first", "fifo")


# table: int32 (makespan, n_slots, 4), utterance indices are those of the input list; makespan: chunks; inverse[i] = position of
# utterance i in `order` (the permutation back to input order); order: the sequence in which the utterances were dealt out
Plan = namedtuple("Plan", "table makespan inverse order")


def plan(lengths_in_frames, n_slots, chunk_frames, order="longest_first"):
    """Greedy list scheduling: the next utterance in `order` ("longest_first": by decreasing length, ties in input order; "fifo":
    input order) goes to the slot that frees first, ties to the lowest slot; it occupies that slot for ceil(len / chunk_frames)
    consecutive chunks from that chunk boundary on.  Every piece but an utterance's last is chunk_frames long.  Any such greedy
    order meets the list-scheduling bound makespan <= sum(c_i) / m + (1 - 1/m) * max(c_i) in chunks."""
    lengths = [int(v) for v in lengths_in_frames]
    if any(v < 1 for v in lengths):
        raise ValueError("every utterance needs at least one frame: %r" % (lengths,))
    n_slots, chunk_frames = int(n_slots), int(chunk_frames)
    if n_slots < 1:
        raise ValueError("n_slots must be >= 1")
    if chunk_frames < 1:
        raise ValueError("chunk_frames must be >= 1")
    if order not in ORDERS:
        raise ValueError("order must be one of %r" % (ORDERS,))
    n = len(lengths)
    seq = sorted(range(n), key=lambda i: (-lengths[i], i)) if order == "longest_first" else list(range(n))
    free = [(0, s) for s in range(n_slots)]                  # (chunk at which the slot frees, slot): a heap, so ties go to the lowest slot
    heapq.heapify(free)
    placed = []
    for i in seq:
        at, s = heapq.heappop(free)
        c = -(-lengths[i] // chunk_frames)
        placed.append((i, s, at, c))
        heapq.heappush(free, (at + c, s))
    makespan = max([at + c for _, _, at, c in placed] or [0])
    table = np.zeros((makespan, n_slots, 4), np.int32)
    table[:, :, UTT] = -1
    for i, s, at, c in placed:
        for k in range(c):
            first = k * chunk_frames
            table[at + k, s] = (i, first, min(chunk_frames, lengths[i] - first), 1 if k == 0 else 0)
    inverse = np.empty(n, np.int64)
    inverse[np.asarray(seq, np.int64)] = np.arange(n)
    return Plan(table, int(makespan), inverse, np.asarray(seq, np.int64))


def padded_makespan_frames(lengths_in_frames, n_slots):
    """what FIFO batches of n_slots through one-length `generate` calls cost, in frames: the sum of every batch's longest member"""
    lengths = [int(v) for v in lengths_in_frames]
    return sum(max(lengths[i:i + n_slots]) for i in range(0, len(lengths), n_slots))
