"""The utterance queue's host planner (twvk_amd.queue.plan) and the C-ABI entries it drives, without a GPU.

The sweep takes seeded length lists (n = 1..40 utterances of 1..50 frames) over slots {1, 3, 8, 32}, chunk_frames {1, 2, 8, 64} and
both orders, and checks the schedule's defining properties on the table itself: every frame of every utterance exactly once, in
order, in one slot, in consecutive chunks; full pieces but the last; the start (= reset) flag on the first piece only; no slot
with two utterances in a chunk; the list-scheduling bound on the makespan."""
import os
import subprocess

import numpy as np
import pytest

import twvk_amd  # noqa: F401
from twvk_amd import queue as Q

SLOTS = (1, 3, 8, 32)
CHUNKS = (1, 2, 8, 64)


def _length_lists():
    rng = np.random.RandomState(0)
    return [rng.randint(1, 51, size=n).tolist() for n in range(1, 41)]


def _pieces(table):
    """{utterance: [(chunk, slot, first, valid, start), ...] in chunk order}; a (chunk, slot) cell holds one row, so no slot can hold
    two utterances in one chunk by construction of the table -- what is checked is that no utterance is lost by such a collision"""
    got = {}
    for c in range(table.shape[0]):
        for s in range(table.shape[1]):
            u, first, valid, start = (int(v) for v in table[c, s])
            if u < 0:
                assert (first, valid, start) == (0, 0, 0), "an idle cell carries no piece"
                continue
            got.setdefault(u, []).append((c, s, first, valid, start))
    return got


def _check_plan(lengths, m, k, order):
    p = Q.plan(lengths, m, k, order)
    table, makespan, inverse = p.table, p.makespan, p.inverse
    assert tuple(p) == (table, makespan, inverse, p.order) and isinstance(makespan, int)
    assert table.dtype == np.int32 and table.shape == (makespan, m, 4)
    pieces = _pieces(table)
    assert sorted(pieces) == list(range(len(lengths))), "every utterance is scheduled"
    busy_until = {}
    for u, ps in pieces.items():
        c_u = -(-lengths[u] // k)
        assert len(ps) == c_u
        chunks = [q[0] for q in ps]
        assert chunks == list(range(chunks[0], chunks[0] + c_u)), "consecutive chunks"
        assert len({q[1] for q in ps}) == 1, "one slot"
        covered = 0
        for i, (c, s, first, valid, start) in enumerate(ps):
            assert first == covered, "frames in order, each exactly once"
            assert valid == (k if i < c_u - 1 else lengths[u] - first) and 1 <= valid <= k, "every piece but the last is a full chunk"
            assert start == (1 if i == 0 else 0), "the start flag sits on the first piece only"
            covered += valid
        assert covered == lengths[u]
        busy_until.setdefault(ps[0][1], []).append((chunks[0], chunks[-1], u))
    for s, spans in busy_until.items():                      # an utterance's span in a slot overlaps no other's
        spans.sort()
        for a, b in zip(spans, spans[1:]):
            assert a[1] < b[0], "slot %d holds utterances %d and %d in one chunk" % (s, a[2], b[2])
    c = [-(-v // k) for v in lengths]
    assert makespan == max(q[-1][0] for q in pieces.values()) + 1, "no empty chunk at the end"
    assert makespan <= int(np.floor(sum(c) / m + (1 - 1 / m) * max(c) + 1e-9)), (makespan, sum(c), m, max(c))
    # the permutation back to input order
    assert sorted(p.order.tolist()) == list(range(len(lengths)))
    assert [int(p.order[int(inverse[i])]) for i in range(len(lengths))] == list(range(len(lengths)))
    if order == "fifo":
        assert p.order.tolist() == list(range(len(lengths)))
    else:
        dealt = [lengths[i] for i in p.order]
        assert dealt == sorted(lengths, reverse=True)
    # the greedy rule itself: in dealing order, an utterance starts at the earliest boundary at which any slot is free, lowest slot first
    free = [0] * m
    for u in p.order:
        at = min(free)
        s = free.index(at)
        assert (pieces[int(u)][0][0], pieces[int(u)][0][1]) == (at, s)
        free[s] = at + -(-lengths[int(u)] // k)
    return p


@pytest.mark.parametrize("order", Q.ORDERS)
@pytest.mark.parametrize("m", SLOTS)
def test_plan_sweep(m, order):
    for lengths in _length_lists():
        for k in CHUNKS:
            _check_plan(lengths, m, k, order)


@pytest.mark.parametrize("order", Q.ORDERS)
def test_equal_lengths_fill_the_slots_exactly(order):
    for m in SLOTS:
        for k in CHUNKS:
            for length in (1, 7, 64, 65):
                for rounds in (1, 2, 5):
                    p = _check_plan([length] * (m * rounds), m, k, order)
                    assert p.makespan == rounds * -(-length // k)
                    assert (p.table[:, :, Q.UTT] >= 0).all(), "no idle cell"


@pytest.mark.parametrize("order", Q.ORDERS)
def test_fewer_utterances_than_slots_leave_idle_slots(order):
    p = _check_plan([5, 3], 8, 2, order)
    assert p.makespan == 3
    used = {int(s) for s in np.argwhere(p.table[:, :, Q.UTT] >= 0)[:, 1]}
    assert len(used) == 2
    for s in set(range(8)) - used:
        assert (p.table[:, s, Q.UTT] == -1).all()
    assert (p.table[2, :, Q.UTT] >= 0).sum() == 1, "the shorter utterance's slot idles in the last chunk"


def test_a_known_schedule():
    # 3 slots, chunk 2: lengths -> chunks [1, 2, 1, 2, 1, 1, 1, 2], 11 in all.  fifo leaves the last long utterance alone at the end
    # (5 chunks), longest-first packs the 11 into ceil(11 / 3) = 4
    lengths = [1, 3, 2, 4, 1, 1, 2, 3]
    f = Q.plan(lengths, 3, 2, "fifo")
    g = Q.plan(lengths, 3, 2, "longest_first")
    assert f.makespan == 5 and g.makespan == 4
    assert g.order.tolist() == [3, 1, 7, 2, 6, 0, 4, 5]
    assert f.table[:, :, Q.UTT].tolist() == [[0, 1, 2], [3, 1, 4], [3, 5, 6], [7, -1, -1], [7, -1, -1]]
    assert g.table[:, :, Q.UTT].tolist() == [[3, 1, 7], [3, 1, 7], [2, 6, 0], [4, 5, -1]]
    assert f.table[1, 0].tolist() == [3, 0, 2, 1] and f.table[2, 0].tolist() == [3, 2, 2, 0] and f.table[1, 1].tolist() == [1, 2, 1, 0]
    assert Q.padded_makespan_frames(lengths, 3) == 3 + 4 + 3


def test_value_errors():
    with pytest.raises(ValueError):
        Q.plan([3, 0, 2], 2, 1)
    with pytest.raises(ValueError):
        Q.plan([3, 2], 0, 1)
    with pytest.raises(ValueError):
        Q.plan([3, 2], 2, 0)
    with pytest.raises(ValueError):
        Q.plan([3, 2], 2, 1, order="shortest_first")


def test_library_exports_the_queue_entries():
    from twvk_amd import _lib
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in ("twv_wavenet_reset_streams", "twv_wavenet_queue_stage", "twv_wavenet_queue_collect"):
        assert (" T " + name + "\n") in syms, name
        assert name in _lib.EXPORTS
    with open(os.path.join(os.path.dirname(_lib._HERE), "include", "twv_amd.h")) as fh:
        header = fh.read()
    for name in ("twv_wavenet_reset_streams", "twv_wavenet_queue_stage", "twv_wavenet_queue_collect"):
        assert ("int %s(" % name) in header
