"""Batched Tick on the GPU (etick_batch_device, include/ewal.h): `node.Tick()`
(raft/node.go:237-238, 262-269), that is `tickElection` at a follower or a
candidate and `tickHeartbeat` at a leader (raft/raft.go:287-307, 590-595,
608-617), for many raft groups at once -- the timer that starts every other
step.  The groups are raftlead's elead_group records (read only) with
raftvote's evote_state, whose `elapsed` it keeps; the msgHup come back as
evote_msg rows that `raftvote.vote_batch_device` takes as they lie, the msgBeat
as elead_local rows for `raftprop.local_batch_device`."""
import ctypes as C

import numpy as np

from ._lib import lib, check
from .raftlead import GROUP_WORDS, _up
from .raftvote import VSTATE_WORDS, MSG_IN_WORDS
from .raftprop import LOCAL_WORDS
from .raftmsg import _ptr

RESULT_WORDS = 4    # etick_result, 32 B (word 0: status | action << 32)
ACTIONS = ("", "idle", "held", "hup", "beat", "not_promotable", "panicked")
IDLE, HELD, HUP, BEAT, NOT_PROMOTABLE, PANICKED = range(1, 7)
_M = (1 << 64) - 1


def draw(seed, id, term, elapsed):
    """etick_draw: the library's stand-in for the process-wide rand.Int() --
    63 bits from the seed, the node's id and term and the incremented elapsed."""
    x = (seed ^ id * 0x9E3779B97F4A7C15 ^ term * 0xBF58476D1CE4E5B9 ^ elapsed * 0x94D049BB133111EB) & _M
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & _M
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & _M
    x ^= x >> 31
    return x >> 1


def results_from(raw, n):
    """etick_result rows (bytes) as dicts."""
    out = []
    for r in np.frombuffer(raw, dtype=np.uint64, count=n * RESULT_WORDS).reshape(n, RESULT_WORDS):
        w0 = int(r[0])
        out.append(dict(status=w0 & 0xFFFFFFFF, action=w0 >> 32, elapsed=int(r[1]), out_pos=int(r[2]), draw=int(r[3])))
    return out


def tick_batch_device(ctx, d_groups, d_vstate, G, d_sel, n, election, heartbeat, d_draws, seed, d_res, d_hups=None,
                      hups_cap=0, d_beats=None, beats_cap=0):
    """etick_batch_device over device arrays (elead_group[G], evote_state[G], n
    group numbers or None for every group in order, n draws or None for
    etick_draw(seed, ...), etick_result[n], evote_msg[hups_cap] and
    elead_local[beats_cap], or None for both: the peek).  Returns (n_hups,
    n_beats)."""
    nh, nb = C.c_uint64(0), C.c_uint64(0)
    check(lib.etick_batch_device(ctx.handle, _ptr(d_groups), _ptr(d_vstate), G, _ptr(d_sel), n, election, heartbeat,
                                 _ptr(d_draws), seed, _ptr(d_res), _ptr(d_hups), hups_cap, _ptr(d_beats), beats_cap,
                                 C.byref(nh), C.byref(nb)))
    return nh.value, nb.value


def tick_batch(ctx, grows, vrows, election, heartbeat, sel=None, draws=None, seed=0, peek=False):
    """Host convenience over packed rows: grows (G, 32) uint64 elead_group rows
    (raftlead.pack_groups), vrows (G, 8) uint64 evote_state rows
    (raftvote.pack_vstate), sel a list of group numbers (None: every group in
    order), draws one value per selection (None: etick_draw(seed, ...)).
    Uploads, peeks for the sizes, calls (unless peek), downloads.  Returns
    (results as dicts, new vstate rows, msgHup rows (n_hups, 8), msgBeat rows
    (n_beats, 6), n_hups, n_beats)."""
    grows = np.ascontiguousarray(grows, dtype=np.uint64).reshape(-1, GROUP_WORDS)
    vrows = np.ascontiguousarray(vrows, dtype=np.uint64).reshape(-1, VSTATE_WORDS)
    G = len(grows)
    n = G if sel is None else len(sel)
    hups, beats = np.zeros((0, MSG_IN_WORDS), np.uint64), np.zeros((0, LOCAL_WORDS), np.uint64)
    if n == 0:
        return [], vrows.copy(), hups, beats, 0, 0
    bufs = [_up(ctx, grows), _up(ctx, vrows), _up(ctx, np.array(sel, dtype=np.uint64)) if sel is not None else None,
            _up(ctx, np.array(draws, dtype=np.uint64)) if draws is not None else None, ctx.alloc(n * 32 + 64)]
    try:
        args = (ctx, bufs[0], bufs[1], G, bufs[2], n, election, heartbeat, bufs[3], seed, bufs[4])
        nh, nb = tick_batch_device(*args)
        if not peek:
            bufs += [ctx.alloc(nh * 64 + 64), ctx.alloc(nb * 48 + 64)]
            nh, nb = tick_batch_device(*args, bufs[5], nh, bufs[6], nb)
            if nh:
                hups = np.frombuffer(bufs[5].download(nh * 64), dtype=np.uint64).reshape(nh, MSG_IN_WORDS).copy()
            if nb:
                beats = np.frombuffer(bufs[6].download(nb * 48), dtype=np.uint64).reshape(nb, LOCAL_WORDS).copy()
        res = results_from(bufs[4].download(n * 32), n)
        v2 = np.frombuffer(bufs[1].download(vrows.nbytes), dtype=np.uint64).reshape(-1, VSTATE_WORDS).copy()
    finally:
        for b in bufs:
            if b is not None:
                b.free()
    return res, v2, hups, beats, nh, nb
