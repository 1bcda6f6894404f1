"""Batched follower step on the GPU (efollow_step_batch_device, include/ewal.h):
`raft.Step` for msgApp and msgSnap (raft/raft.go:372-408) -- the term switch,
the follower's and the candidate's cases, handleAppendEntries with
raftLog.maybeAppend, handleSnapshot with raft.restore -- for runs of messages
per raft group.  The groups are the records the leader-side calls use
(raftlead's elead_group, raftprop's state record, raftvote's evote_state,
raftready's eready_state), so a follower's appended entries reach
`raftready.ready_batch_device` and the WAL like a leader's; the msgAppResp
come back as emsg_out records for `raftlead.lead_step_batch_device`'s caller or
`raftmsg.encode_messages_device`."""
import ctypes as C

import numpy as np

from ._lib import lib, check
from .raftlead import (GROUP_WORDS, ENTRY_WORDS, MSG_WORDS, SNAP_WORDS, MSG_APP, MSG_SNAP, _u64, _up,  # noqa: F401
                       messages_from, pack_snaps, unpack_groups)
from .raftprop import STATE_WORDS
from .raftvote import VSTATE_WORDS
from .raftready import RSTATE_WORDS
from .raftmsg import _ptr

MSG_IN_WORDS = 12   # efollow_msg, 96 B
RESULT_WORDS = 12   # efollow_result, 96 B (word 0: status | action << 32, word 10: state | flags << 32)
MSG_APP_RESP = 4    # raft.msgAppResp
ACTIONS = ("not_stepped", "ignored", "no_case", "appended", "rejected", "restored", "snap_stale", "deferred",
           "panicked")
FLAG_TERM_SWITCH, FLAG_CONCEDED = 1, 2
_KINDS = {"app": MSG_APP, "snap": MSG_SNAP}
_MSG_KEYS = ("group", "kind", "from_", "term", "index", "log_term", "commit", "ents_first", "n_ents", "data_delta",
             "snap")
_RES_KEYS = ("msg_first", "n_msgs", "conflict", "app_first", "n_app", "dst_first", "last_index", "committed", "term")


def pack_msgs(msgs):
    """efollow_msg rows of message dicts: group, kind ("app" / "snap" or 3 /
    7), from_, term, index, log_term, commit, ents_first, n_ents, data_delta,
    snap."""
    return _u64([[_KINDS.get(m.get(k), m.get(k, MSG_APP)) if k == "kind" else int(m.get(k, 0)) for k in _MSG_KEYS] +
                 [0] for m in msgs], MSG_IN_WORDS)


def results_from(raw, n):
    """efollow_result rows (bytes) as dicts."""
    out = []
    for r in np.frombuffer(raw, dtype=np.uint64, count=n * RESULT_WORDS).reshape(n, RESULT_WORDS):
        w = [int(x) for x in r]
        d = dict(status=w[0] & 0xFFFFFFFF, action=w[0] >> 32, state=w[10] & 0xFFFFFFFF, flags=w[10] >> 32)
        d.update(zip(_RES_KEYS, w[1:10]))
        out.append(d)
    return out


def msgs_from_out(rows, groups, data_delta=0, snap_base=0):
    """The leader-side calls' emsg_out rows ((n, 18) uint64, or their bytes) as
    the follower step's input.  groups[i] is the group that steps message i (the
    replica `to` names; the caller's routing), or None to drop it.  Messages
    that are neither msgApp nor msgSnap are dropped.  The rows are ordered by
    group, stably, as the call wants them.  Returns (efollow_msg rows, elead_snap
    rows of the msgSnap messages -- message.snap indexes them from snap_base on
    --, the input positions in output order)."""
    rows = np.frombuffer(rows, dtype=np.uint64).reshape(-1, MSG_WORDS) if isinstance(rows, (bytes, bytearray)) \
        else np.asarray(rows, dtype=np.uint64).reshape(-1, MSG_WORDS)
    keep = [i for i in range(len(rows)) if groups[i] is not None and int(rows[i, 0]) in (MSG_APP, MSG_SNAP)]
    keep.sort(key=lambda i: groups[i])
    out = np.zeros((len(keep), MSG_IN_WORDS), dtype=np.uint64)
    snaps = []
    for j, i in enumerate(keep):
        w = rows[i]
        # emsg_out: type, to, from, term, log_term, index, commit, ents_first, n_ents, snapshot[8], reject
        out[j, :9] = [groups[i], w[0], w[2], w[3], w[5], w[4], w[6], w[7], w[8]]
        if int(w[0]) == MSG_SNAP:
            out[j, 10] = snap_base + len(snaps)
            snaps.append(w[9:17].copy())
        else:
            out[j, 9] = np.uint64(data_delta)
    return out, _u64(snaps, SNAP_WORDS) if snaps else np.zeros((0, SNAP_WORDS), dtype=np.uint64), keep


def follow_batch_device(ctx, d_groups, d_pstate, d_vstate, d_rstate, G, d_snaps, d_ents, n_ents_total, d_src,
                        n_src_total, d_in_snaps, n_in_snaps, d_u64, n_u64, d_in, n, d_res, d_msgs=None, msgs_cap=0):
    """efollow_step_batch_device over device arrays (elead_group[G],
    elead_prop_state[G], evote_state[G], eready_state[G] or None, elead_snap[G]
    or None, ewal_entry[n_ents_total], the source ewal_entry[n_src_total] --
    d_ents itself is allowed --, elead_snap[n_in_snaps], uint64[n_u64],
    efollow_msg[n], efollow_result[n], emsg_out[msgs_cap] or None for the size
    query).  Returns (n_msgs, n_appended, n_restored)."""
    nm, na, nr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    check(lib.efollow_step_batch_device(ctx.handle, _ptr(d_groups), _ptr(d_pstate), _ptr(d_vstate), _ptr(d_rstate), G,
                                        _ptr(d_snaps), _ptr(d_ents), n_ents_total, _ptr(d_src), n_src_total,
                                        _ptr(d_in_snaps), n_in_snaps, _ptr(d_u64), n_u64, _ptr(d_in), n, _ptr(d_res),
                                        _ptr(d_msgs), msgs_cap, C.byref(nm), C.byref(na), C.byref(nr)))
    return nm.value, na.value, nr.value


def _rows(a, width):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1, width))


def follow_batch(ctx, grows, srows, vrows, rrows, snaprows, erows, msgs_in, src=None, in_snaps=None, u64=None,
                 size_query=False):
    """Host convenience over packed rows: grows / srows / vrows / rrows /
    snaprows as raftprop.pack_logs, pack_state, raftvote.pack_vstate,
    raftready.pack_rstate and raftlead.pack_snaps give them (rrows and snaprows
    may be None), erows every window's entries, msgs_in efollow_msg rows or
    dicts, src the source entry rows (None: the messages name ranges of erows
    itself), in_snaps elead_snap rows, u64 the Nodes values.  Uploads, asks for
    the size, calls (unless size_query), downloads.  Returns a dict: res (list
    of dicts), res_rows, msgs (dicts), msg_rows, groups, pstate, vstate,
    rstate, snaps, ents (row arrays, None where none was given), n_msgs,
    n_appended, n_restored."""
    if len(msgs_in) and isinstance(msgs_in[0], dict):
        msgs_in = pack_msgs(msgs_in)
    inrows = _rows(msgs_in, MSG_IN_WORDS)
    n, G = len(inrows), len(grows)
    grows, srows, vrows = _rows(grows, GROUP_WORDS), _rows(srows, STATE_WORDS), _rows(vrows, VSTATE_WORDS)
    erows = _rows(erows, ENTRY_WORDS)
    rrows = None if rrows is None else _rows(rrows, RSTATE_WORDS)
    snaprows = None if snaprows is None else _rows(snaprows, SNAP_WORDS)
    in_snaps = _rows(in_snaps if in_snaps is not None else [], SNAP_WORDS)
    u64 = np.ascontiguousarray(np.asarray(u64 if u64 is not None else [], dtype=np.uint64))
    srcrows = None if src is None else _rows(src, ENTRY_WORDS)
    out = dict(res=[], res_rows=np.zeros((0, RESULT_WORDS), dtype=np.uint64), msgs=[],
               msg_rows=np.zeros((0, MSG_WORDS), dtype=np.uint64), groups=grows, pstate=srows, vstate=vrows,
               rstate=rrows, snaps=snaprows, ents=erows, n_msgs=0, n_appended=0, n_restored=0)
    if n == 0:
        return out
    names = ("groups", "pstate", "vstate", "rstate", "snaps", "ents")
    host = (grows, srows, vrows, rrows, snaprows, erows)
    bufs = [None if h is None else _up(ctx, h) for h in host]
    bufs += [None if srcrows is None else _up(ctx, srcrows), _up(ctx, in_snaps), _up(ctx, u64), _up(ctx, inrows),
             ctx.alloc(n * 96 + 64)]
    try:
        d_src, n_src = (bufs[5], len(erows)) if srcrows is None else (bufs[6], len(srcrows))
        args = (ctx, bufs[0], bufs[1], bufs[2], bufs[3], G, bufs[4], bufs[5], len(erows), d_src, n_src, bufs[7],
                len(in_snaps), bufs[8], len(u64), bufs[9], n, bufs[10])
        total, na, nr = follow_batch_device(*args)
        if not size_query:
            bufs.append(ctx.alloc(total * 144 + 64))
            total, na, nr = follow_batch_device(*args, bufs[11], total)
            raw = bufs[11].download(total * 144) if total else b""
            out["msg_rows"] = np.frombuffer(raw, dtype=np.uint64).reshape(-1, MSG_WORDS).copy()
            out["msgs"] = messages_from(raw, total) if total else []
        raw = bufs[10].download(n * 96)
        out["res"] = results_from(raw, n)
        out["res_rows"] = np.frombuffer(raw, dtype=np.uint64).reshape(n, RESULT_WORDS).copy()
        for name, h, b in zip(names, host, bufs):
            if h is not None and h.size:
                out[name] = np.frombuffer(b.download(h.nbytes), dtype=np.uint64).reshape(h.shape).copy()
        out.update(n_msgs=total, n_appended=na, n_restored=nr)
    finally:
        for b in bufs:
            if b is not None:
                b.free()
    return out
