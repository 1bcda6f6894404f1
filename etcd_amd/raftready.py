"""Batched Ready on the GPU (eready_batch_device, include/ewal.h): `newReady`
(raft/node.go:332-348), node.run's accept branch (:239-255) and the record
order of `Storage.Save` (wal/wal.go:281-288) for many raft groups at once --
the joint between the step calls (raftlog / raftlead / raftprop / raftvote) and
the write side.  The groups are raftlead's elead_group records with raftprop's
state records, raftvote's evote_state and one more side record (eready_state);
per group a Ready comes back, and the ewal_save_rec records that
`ewal_save_device` takes directly."""
import ctypes as C

import numpy as np

from ._lib import lib, check, READY_SOFT, READY_HARD, READY_SNAP, READY_UPDATES  # noqa: F401
from .raftlead import GROUP_WORDS, ENTRY_WORDS, _u64, _up, pack_snaps  # noqa: F401
from .raftprop import STATE_WORDS, pack_logs, pack_state, unpack_state  # noqa: F401
from .raftvote import VSTATE_WORDS, pack_vstate
from .raftmsg import _ptr

RSTATE_WORDS = 8    # eready_state, 64 B
RESULT_WORDS = 12   # eready_result, 96 B (word 0: status | flags << 32, word 11: state | pad << 32)
SAVE_WORDS = 7      # ewal_save_rec, 56 B (word 0: kind | etype << 32, word 6: data_nil | pad << 32)
SAVE_ENTRY, SAVE_STATE, SAVE_CUT = 2, 3, 4
_RSTATE_KEYS = ("hs_term", "hs_vote", "hs_commit", "lead", "state", "snapi", "applied", "soft_dirty")
_STATES = {"follower": 0, "candidate": 1, "leader": 2}


def pack_rstate(rstate):
    """eready_state rows: one dict (hs_term, hs_vote, hs_commit, lead, state --
    0 / 1 / 2 or its name --, snapi, applied, soft_dirty) per group."""
    return _u64([[_STATES.get(s.get(k), s.get(k, 0)) if k == "state" else int(s.get(k, 0)) for k in _RSTATE_KEYS]
                 for s in rstate], RSTATE_WORDS)


def unpack_rstate(rows):
    return [dict(zip(_RSTATE_KEYS, (int(x) for x in r)))
            for r in np.asarray(rows, dtype=np.uint64).reshape(-1, RSTATE_WORDS)]


def results_from(raw, n):
    """eready_result rows (bytes) as dicts."""
    out = []
    for r in np.frombuffer(raw, dtype=np.uint64, count=n * RESULT_WORDS).reshape(n, RESULT_WORDS):
        w = [int(x) for x in r]
        out.append(dict(status=w[0] & 0xFFFFFFFF, flags=w[0] >> 32, term=w[1], vote=w[2], commit=w[3],
                        ents_first=w[4], n_ents=w[5], committed_first=w[6], n_committed=w[7], save_first=w[8],
                        n_save=w[9], lead=w[10], state=w[11] & 0xFFFFFFFF))
    return out


def saves_from(raw, n):
    """ewal_save_rec rows (bytes) as dicts."""
    out = []
    for r in np.frombuffer(raw, dtype=np.uint64, count=n * SAVE_WORDS).reshape(n, SAVE_WORDS):
        w = [int(x) for x in r]
        out.append(dict(kind=w[0] & 0xFFFFFFFF, etype=w[0] >> 32, a=w[1], b=w[2], c=w[3], data_off=w[4],
                        data_len=w[5], data_nil=w[6] & 0xFFFFFFFF))
    return out


def ready_batch_device(ctx, d_groups, d_pstate, d_vstate, d_rstate, G, d_snaps, d_ents, n_ents_total, d_sel, n, d_res,
                       d_save=None, save_cap=0):
    """eready_batch_device over device arrays (elead_group[G],
    elead_prop_state[G], evote_state[G], eready_state[G], elead_snap[G] or
    None, ewal_entry[n_ents_total], n group numbers or None for every group in
    order, eready_result[n], ewal_save_rec[save_cap] or None for the peek).
    Returns (n_save, n_ready)."""
    ns, nr = C.c_uint64(0), C.c_uint64(0)
    check(lib.eready_batch_device(ctx.handle, _ptr(d_groups), _ptr(d_pstate), _ptr(d_vstate), _ptr(d_rstate), G,
                                  _ptr(d_snaps), _ptr(d_ents), n_ents_total, _ptr(d_sel), n, _ptr(d_res),
                                  _ptr(d_save), save_cap, C.byref(ns), C.byref(nr)))
    return ns.value, nr.value


def ready_batch(ctx, groups, logs, state, vstate, rstate, snaps=None, sel=None, peek=False):
    """Host convenience: groups and logs as raftlead.pack_groups takes them,
    state as raftprop.pack_state, vstate as raftvote.pack_vstate, rstate as
    pack_rstate, snaps as raftlead.pack_snaps, sel a list of group numbers
    (None: every group in order).  Packs, uploads, peeks for the size, calls
    (unless peek), downloads.  Returns (results, save records, new state, new
    rstate, n_ready) -- lists of dicts."""
    G = len(groups)
    n = G if sel is None else len(sel)
    grows, erows = pack_logs(groups, logs, state)
    srows, vrows, rrows = pack_state(state), pack_vstate(vstate), pack_rstate(rstate)
    if n == 0:
        return [], [], unpack_state(srows), unpack_rstate(rrows), 0
    bufs = [_up(ctx, grows), _up(ctx, srows), _up(ctx, vrows), _up(ctx, rrows),
            _up(ctx, pack_snaps(snaps)) if snaps is not None else None, _up(ctx, erows),
            _up(ctx, np.array(sel, dtype=np.uint64)) if sel is not None else None, ctx.alloc(n * 96 + 64)]
    try:
        args = (ctx, bufs[0], bufs[1], bufs[2], bufs[3], G, bufs[4], bufs[5], len(erows), bufs[6], n, bufs[7])
        total, n_ready = ready_batch_device(*args)
        saves = []
        if not peek:
            bufs.append(ctx.alloc(total * 56 + 64))
            total, n_ready = ready_batch_device(*args, bufs[8], total)
            saves = saves_from(bufs[8].download(total * 56), total) if total else []
        res = results_from(bufs[7].download(n * 96), n)
        s2 = np.frombuffer(bufs[1].download(srows.nbytes), dtype=np.uint64).reshape(-1, STATE_WORDS)
        r2 = np.frombuffer(bufs[3].download(rrows.nbytes), dtype=np.uint64).reshape(-1, RSTATE_WORDS)
    finally:
        for b in bufs:
            if b is not None:
                b.free()
    return res, saves, unpack_state(s2), unpack_rstate(r2), n_ready
