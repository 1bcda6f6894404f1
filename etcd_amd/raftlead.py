"""Batched leader msgAppResp step on the GPU (elead_step_batch_device,
include/ewal.h): `stepLeader`'s msgAppResp case (raft/raft.go:456-466) --
progress.update / maybeDecrTo, raft.maybeCommit, sendAppend / bcastAppend --
for runs of responses per raft group, over leader logs kept as ewal_entry
ranges of one device array.  The next fan-out comes back as emsg_out records
that `raftmsg.encode_messages_device` takes directly."""
import ctypes as C

import numpy as np

from ._lib import lib, check
from .raftmsg import _ptr

GROUP_WORDS = 32   # elead_group, 256 B
SNAP_WORDS = 8     # elead_snap, 64 B
RESP_WORDS = 6     # elead_resp, 48 B (word 4: reject | pad << 32)
RESULT_WORDS = 6   # elead_result, 48 B (word 0: status | action << 32)
MSG_WORDS = 18     # emsg_out, 144 B (word 17: reject | pad << 32)
ENTRY_WORDS = 5    # ewal_entry, 40 B (word 4: type | data_nil << 32)
MAX_PEERS = 7
MSG_APP, MSG_SNAP = 3, 7   # raft.msgApp, raft.msgSnap
ACTIONS = ("not_stepped", "ignored", "step_down", "stale", "probe", "updated", "committed", "panicked")

_U64 = (1 << 64) - 1
_SNAP_KEYS = ("index", "term", "data_off", "data_len", "nodes_off", "n_nodes", "removed_off", "n_removed")


def _u64(rows, width):
    return np.array(rows, dtype=np.uint64).reshape(len(rows), width)


def pack_groups(groups, logs):
    """elead_group rows and the ewal_entry rows of the leaders' logs.  A group
    is a dict: id, term, committed, log_offset and prs, a list of (peer id,
    match, next) in slot order (n_peers = len(prs), or the explicit n_peers);
    logs[g][k] is the term of raftLog.ents[k] of group g (at raft index
    log_offset + k), or a dict with term / index / type.  Group g's entries
    start where group g-1's end.  Returns ((G, 32) uint64, (n_ents, 5) uint64)."""
    rows = np.zeros((len(groups), GROUP_WORDS), dtype=np.uint64)
    ents = []
    for g, (grp, log) in enumerate(zip(groups, logs)):
        prs = list(grp.get("prs") or ())
        if len(prs) > MAX_PEERS:
            raise ValueError("elead_group holds at most %d peers" % MAX_PEERS)
        off = grp.get("log_offset", 0)
        row = [grp.get("id", 0), grp.get("term", 0), grp.get("committed", 0), off, len(log), len(ents),
               grp.get("n_peers", len(prs))] + [0] * 25
        for k, (pid, match, nxt) in enumerate(prs):
            row[7 + k], row[14 + k], row[21 + k] = pid, match, nxt
        rows[g] = np.array(row, dtype=np.uint64)
        for k, e in enumerate(log):
            e = e if isinstance(e, dict) else dict(term=e, index=(off + k) & _U64)
            ents.append([e.get("term", 0), e.get("index", 0), 0, 0, (e.get("type", 0) & 0xFFFFFFFF) | (1 << 32)])
    return rows, _u64(ents, ENTRY_WORDS)


def unpack_groups(rows):
    """The per-group dicts (id, term, committed, log_offset, nlog, ents_first,
    n_peers, prs) of elead_group rows."""
    out = []
    for r in np.asarray(rows, dtype=np.uint64).reshape(-1, GROUP_WORDS):
        w = [int(x) for x in r]
        out.append(dict(id=w[0], term=w[1], committed=w[2], log_offset=w[3], nlog=w[4], ents_first=w[5],
                        n_peers=w[6], prs=[(w[7 + k], w[14 + k], w[21 + k]) for k in range(min(w[6], MAX_PEERS))]))
    return out


def pack_snaps(snaps):
    """elead_snap rows: one dict (index, term, data_off, data_len, nodes_off,
    n_nodes, removed_off, n_removed; all optional) or None per group."""
    return _u64([[(s or {}).get(k, 0) for k in _SNAP_KEYS] for s in snaps], SNAP_WORDS)


def pack_resps(resps):
    """elead_resp rows of response dicts: group, from_, term, index, reject."""
    return _u64([[r.get("group", 0), r.get("from_", 0), r.get("term", 0), r.get("index", 0),
                  1 if r.get("reject") else 0, 0] for r in resps], RESP_WORDS)


def results_from(raw, n):
    """elead_result rows (bytes) as dicts."""
    out = []
    for r in np.frombuffer(raw, dtype=np.uint64, count=n * RESULT_WORDS).reshape(n, RESULT_WORDS):
        w0 = int(r[0])
        out.append(dict(status=w0 & 0xFFFFFFFF, action=w0 >> 32, msg_first=int(r[1]), n_msgs=int(r[2]),
                        committed=int(r[3]), match=int(r[4]), next=int(r[5])))
    return out


def messages_from(raw, n):
    """emsg_out rows (bytes) as dicts: the fields of raftmsg.pack_messages'
    input, the entries as their (ents_first, n_ents) range of the leader's
    array and the snapshot as its eight words."""
    out = []
    for r in np.frombuffer(raw, dtype=np.uint64, count=n * MSG_WORDS).reshape(n, MSG_WORDS):
        w = [int(x) for x in r]
        out.append(dict(type=w[0], to=w[1], from_=w[2], term=w[3], log_term=w[4], index=w[5], commit=w[6],
                        ents_first=w[7], n_ents=w[8], snap=dict(zip(_SNAP_KEYS, w[9:17])),
                        reject=bool(w[17] & 0xFFFFFFFF)))
    return out


def lead_step_batch_device(ctx, d_groups, G, d_snaps, d_ents, n_ents_total, d_resps, n, d_res, d_msgs=None,
                           msgs_cap=0):
    """elead_step_batch_device over device arrays (elead_group[G], elead_snap[G]
    or None, ewal_entry[n_ents_total], elead_resp[n], elead_result[n],
    emsg_out[msgs_cap] or None for the size query).  Returns (n_msgs,
    n_committed)."""
    nm, nc = C.c_uint64(0), C.c_uint64(0)
    check(lib.elead_step_batch_device(ctx.handle, _ptr(d_groups), G, _ptr(d_snaps), _ptr(d_ents), n_ents_total,
                                      _ptr(d_resps), n, _ptr(d_res), _ptr(d_msgs), msgs_cap, C.byref(nm),
                                      C.byref(nc)))
    return nm.value, nc.value


def _up(ctx, arr):
    raw = arr.tobytes()
    d = ctx.alloc(len(raw) + 64)
    if raw:
        d.upload(raw)
    return d


def lead_step_batch(ctx, groups, ents, resps, snaps=None):
    """Host convenience: groups as pack_groups takes them, ents their logs,
    resps as pack_resps takes them, snaps as pack_snaps.  Packs, uploads, asks
    for the size, calls, downloads.  Returns (results, new groups as
    unpack_groups gives them, messages) -- lists of dicts."""
    n, G = len(resps), len(groups)
    grows, erows = pack_groups(groups, ents)
    if n == 0:
        return [], unpack_groups(grows), []
    bufs = [_up(ctx, grows), _up(ctx, pack_snaps(snaps)) if snaps is not None else None, _up(ctx, erows),
            _up(ctx, pack_resps(resps)), ctx.alloc(n * 48 + 64)]
    try:
        args = (ctx, bufs[0], G, bufs[1], bufs[2], len(erows), bufs[3], n, bufs[4])
        total, _ = lead_step_batch_device(*args)
        bufs.append(ctx.alloc(total * 144 + 64))
        lead_step_batch_device(*args, bufs[5], total)
        res = results_from(bufs[4].download(n * 48), n)
        msgs = messages_from(bufs[5].download(total * 144), total) if total else []
        g2 = np.frombuffer(bufs[0].download(grows.nbytes), dtype=np.uint64).reshape(-1, GROUP_WORDS)
    finally:
        for b in bufs:
            if b is not None:
                b.free()
    return res, unpack_groups(g2), msgs
