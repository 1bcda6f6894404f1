"""Batched log compaction on the GPU (ecompact_batch_device, include/ewal.h):
`node.Compact` (raft/node.go:226-227, 325-330) -- raft.compact
(raft/raft.go:522-531) with raftLog.snap and raftLog.compact (raft/log.go:
156-179) and, for a request "at applied, when due", raftLog.shouldCompact
(:181-183) -- for at most one request per raft group.  The groups are the
records every other step uses (raftlead's elead_group, raftprop's state record,
raftready's eready_state); the survivors of a compaction slide to the base of
the group's window, so the room comes back, and d_snaps[g] -- what the leader
ships as msgSnap and what `snap.save_packed` writes -- is produced here."""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import lib, check
from .raftlead import GROUP_WORDS, ENTRY_WORDS, SNAP_WORDS, _u64, _up
from .raftprop import STATE_WORDS
from .raftready import RSTATE_WORDS
from .raftmsg import _ptr

REQ_WORDS = 12      # ecompact_req, 96 B
RESULT_WORDS = 8    # ecompact_result, 64 B (word 0: status | action << 32)
AT_APPLIED = L.COMPACT_AT_APPLIED
PEEK = L.COMPACT_PEEK
ACTIONS = ("not_stepped", "not_due", "compacted", "panicked")
_REQ_KEYS = ("group", "flags", "index", "threshold", "data_off", "data_len", "nodes_off", "n_nodes", "removed_off",
             "n_removed")
_RES_KEYS = ("index", "term", "n_left", "shift", "src_first", "dst_first", "unstable")


def pack_reqs(reqs):
    """ecompact_req rows of request dicts: group, flags (or at_applied=True),
    index, threshold, data_off, data_len, nodes_off, n_nodes, removed_off,
    n_removed."""
    rows = []
    for r in reqs:
        w = [int(r.get(k, 0)) for k in _REQ_KEYS]
        if r.get("at_applied"):
            w[1] |= AT_APPLIED
        rows.append(w + [0, 0])
    return _u64(rows, REQ_WORDS)


def results_from(raw, n):
    """ecompact_result rows (bytes) as dicts."""
    out = []
    for r in np.frombuffer(raw, dtype=np.uint64, count=n * RESULT_WORDS).reshape(n, RESULT_WORDS):
        w = [int(x) for x in r]
        d = dict(status=w[0] & 0xFFFFFFFF, action=w[0] >> 32)
        d.update(zip(_RES_KEYS, w[1:]))
        out.append(d)
    return out


def snap_save_recs(snap_rows, groups=None):
    """The esnap_save_rec rows (a ctypes array, what esnap_save_packed_device
    takes) of the elead_snap rows of the given groups (None: every row): the
    snapshot a compaction left in d_snaps.  The Nodes / RemovedNodes ranges stay
    as they are: the host array that goes with them is the caller's copy of
    d_u64; XXX_unrecognized is nil."""
    rows = np.asarray(snap_rows, dtype=np.uint64).reshape(-1, SNAP_WORDS)
    sel = range(len(rows)) if groups is None else list(groups)
    recs = (L.SnapSaveRec * max(len(sel), 1))()
    for rec, g in zip(recs, sel):
        (rec.index, rec.term, rec.data_off, rec.data_len, rec.nodes_off, rec.n_nodes, rec.removed_off,
         rec.n_removed) = (int(x) for x in rows[g])
    return recs


def compact_batch_device(ctx, d_groups, d_pstate, d_rstate, G, d_snaps, d_ents, n_ents_total, data_len_total, n_u64,
                         d_reqs, n, d_res, flags=0):
    """ecompact_batch_device over device arrays (elead_group[G],
    elead_prop_state[G], eready_state[G], elead_snap[G], ewal_entry[n_ents_total],
    ecompact_req[n], ecompact_result[n]); flags = PEEK fills d_res and modifies
    nothing else.  Returns (n_compacted, n_moved)."""
    nc, nm = C.c_uint64(0), C.c_uint64(0)
    check(lib.ecompact_batch_device(ctx.handle, _ptr(d_groups), _ptr(d_pstate), _ptr(d_rstate), G, _ptr(d_snaps),
                                    _ptr(d_ents), n_ents_total, data_len_total, n_u64, _ptr(d_reqs), n, _ptr(d_res),
                                    flags, C.byref(nc), C.byref(nm)))
    return nc.value, nm.value


def _rows(a, width):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1, width))


def compact_batch(ctx, grows, srows, rrows, snaprows, erows, reqs, data_len_total=0, n_u64=0, peek=False):
    """Host convenience over packed rows: grows / srows / rrows / snaprows as
    raftprop.pack_logs, pack_state, raftready.pack_rstate and
    raftlead.pack_snaps give them, erows every window's entries, reqs
    ecompact_req rows or dicts; data_len_total and n_u64 bound the requests'
    ranges.  Uploads, calls, downloads.  Returns a dict: res (list of dicts),
    res_rows, groups, pstate, rstate, snaps, ents (row arrays), n_compacted,
    n_moved."""
    if len(reqs) and isinstance(reqs[0], dict):
        reqs = pack_reqs(reqs)
    inrows = _rows(reqs, REQ_WORDS)
    n, G = len(inrows), len(grows)
    grows, srows, rrows = _rows(grows, GROUP_WORDS), _rows(srows, STATE_WORDS), _rows(rrows, RSTATE_WORDS)
    snaprows, erows = _rows(snaprows, SNAP_WORDS), _rows(erows, ENTRY_WORDS)
    out = dict(res=[], res_rows=np.zeros((0, RESULT_WORDS), dtype=np.uint64), groups=grows, pstate=srows, rstate=rrows,
               snaps=snaprows, ents=erows, n_compacted=0, n_moved=0)
    if n == 0:
        return out
    names = ("groups", "pstate", "rstate", "snaps", "ents")
    host = (grows, srows, rrows, snaprows, erows)
    bufs = [_up(ctx, h) for h in host] + [_up(ctx, inrows), ctx.alloc(n * 64 + 64)]
    try:
        nc, nm = compact_batch_device(ctx, bufs[0], bufs[1], bufs[2], G, bufs[3], bufs[4], len(erows), data_len_total,
                                      n_u64, bufs[5], n, bufs[6], PEEK if peek else 0)
        raw = bufs[6].download(n * 64)
        out["res"] = results_from(raw, n)
        out["res_rows"] = np.frombuffer(raw, dtype=np.uint64).reshape(n, RESULT_WORDS).copy()
        for name, h, b in zip(names, host, bufs):
            if h.size:
                out[name] = np.frombuffer(b.download(h.nbytes), dtype=np.uint64).reshape(h.shape).copy()
        out.update(n_compacted=nc, n_moved=nm)
    finally:
        for b in bufs:
            b.free()
    return out
