"""Batched leader msgProp / msgBeat step on the GPU (elead_local_batch_device,
include/ewal.h): `stepLeader`'s msgProp and msgBeat cases
(raft/raft.go:441-455) -- appendEntry, progress.update, maybeCommit,
bcastAppend, bcastHeartbeat -- for runs of local messages per raft group.  The
leaders are raftlead's elead_group records and their logs ewal_entry ranges of
one device array, which this call grows; the round's first fan-out comes back
as emsg_out records that `raftmsg.encode_messages_device` takes directly."""
import ctypes as C

import numpy as np

from ._lib import lib, check
from .raftlead import (GROUP_WORDS, ENTRY_WORDS, _u64, _up, messages_from, pack_groups, pack_snaps,  # noqa: F401
                       unpack_groups)
from .raftmsg import _ptr

STATE_WORDS = 4    # elead_prop_state, 32 B
LOCAL_WORDS = 6    # elead_local, 48 B (word 2: etype | data_nil << 32)
RESULT_WORDS = 6   # elead_local_result, 48 B (word 0: status | action << 32)
MSG_BEAT, MSG_PROP = 1, 2          # raft.msgBeat, raft.msgProp
ENTRY_NORMAL, ENTRY_CONF_CHANGE = 0, 1
ACTIONS = ("not_stepped", "beat", "appended", "dropped", "panicked")


def pack_state(state):
    """elead_prop_state rows: one dict (ents_cap, unstable, pending_conf) per group."""
    return _u64([[s.get("ents_cap", 0), s.get("unstable", 0), 1 if s.get("pending_conf") else 0, 0] for s in state],
                STATE_WORDS)


def unpack_state(rows):
    return [dict(ents_cap=int(r[0]), unstable=int(r[1]), pending_conf=int(r[2]))
            for r in np.asarray(rows, dtype=np.uint64).reshape(-1, STATE_WORDS)]


def pack_locals(locals_):
    """elead_local rows of local-message dicts: group, kind ("beat" / "prop" or
    1 / 2), and for a proposal etype, data_off, data_len, data_nil."""
    rows = []
    for m in locals_:
        kind = {"beat": MSG_BEAT, "prop": MSG_PROP}.get(m.get("kind"), m.get("kind", MSG_PROP))
        rows.append([m.get("group", 0), kind, (m.get("etype", 0) & 0xFFFFFFFF) | ((1 if m.get("data_nil") else 0) << 32),
                     m.get("data_off", 0), m.get("data_len", 0), 0])
    return _u64(rows, LOCAL_WORDS)


def pack_logs(groups, logs, state):
    """pack_groups with room to grow: group g's window starts where group
    g-1's ends and is state[g]["ents_cap"] entries long.  Returns (group rows,
    entry rows of every window, free slots zero)."""
    rows, _ = pack_groups(groups, logs)
    caps = [s.get("ents_cap", 0) for s in state]
    ents = np.zeros((sum(caps), ENTRY_WORDS), dtype=np.uint64)
    first = 0
    for g, (log, cap) in enumerate(zip(logs, caps)):
        if len(log) > cap:
            raise ValueError("group %d: ents_cap %d is below its %d entries" % (g, cap, len(log)))
        _, e = pack_groups([groups[g]], [log])
        ents[first:first + len(log)] = e
        rows[g, 5] = np.uint64(first)
        first += cap
    return rows, ents


def results_from(raw, n):
    """elead_local_result rows (bytes) as dicts."""
    out = []
    for r in np.frombuffer(raw, dtype=np.uint64, count=n * RESULT_WORDS).reshape(n, RESULT_WORDS):
        w0 = int(r[0])
        out.append(dict(status=w0 & 0xFFFFFFFF, action=w0 >> 32, msg_first=int(r[1]), n_msgs=int(r[2]),
                        index=int(r[3]), ent_pos=int(r[4]), committed=int(r[5])))
    return out


def local_batch_device(ctx, d_groups, d_state, G, d_snaps, d_ents, n_ents_total, data_len_total, d_locals, n, d_res,
                       d_msgs=None, msgs_cap=0):
    """elead_local_batch_device over device arrays (elead_group[G],
    elead_prop_state[G], elead_snap[G] or None, ewal_entry[n_ents_total],
    elead_local[n], elead_local_result[n], emsg_out[msgs_cap] or None for the
    size query).  Returns (n_msgs, n_appended)."""
    nm, na = C.c_uint64(0), C.c_uint64(0)
    check(lib.elead_local_batch_device(ctx.handle, _ptr(d_groups), _ptr(d_state), G, _ptr(d_snaps), _ptr(d_ents),
                                       n_ents_total, data_len_total, _ptr(d_locals), n, _ptr(d_res), _ptr(d_msgs),
                                       msgs_cap, C.byref(nm), C.byref(na)))
    return nm.value, na.value


def local_batch(ctx, groups, logs, state, locals_, data=b"", snaps=None):
    """Host convenience: groups and logs as raftlead.pack_groups takes them,
    state as pack_state, locals_ as pack_locals, data the bytes the proposals'
    (data_off, data_len) index, snaps as raftlead.pack_snaps.  Packs, uploads,
    asks for the size, calls, downloads.  Returns (results, new groups as
    unpack_groups gives them, new state, entry rows (n_ents, 5) uint64,
    messages) -- the results, groups, state and messages as lists of dicts."""
    n, G = len(locals_), len(groups)
    grows, erows = pack_logs(groups, logs, state)
    srows = pack_state(state)
    if n == 0:
        return [], unpack_groups(grows), unpack_state(srows), erows, []
    bufs = [_up(ctx, grows), _up(ctx, srows), _up(ctx, pack_snaps(snaps)) if snaps is not None else None,
            _up(ctx, erows), _up(ctx, pack_locals(locals_)), ctx.alloc(n * 48 + 64)]
    try:
        args = (ctx, bufs[0], bufs[1], G, bufs[2], bufs[3], len(erows), len(data), bufs[4], n, bufs[5])
        total, _ = local_batch_device(*args)
        bufs.append(ctx.alloc(total * 144 + 64))
        local_batch_device(*args, bufs[6], total)
        res = results_from(bufs[5].download(n * 48), n)
        msgs = messages_from(bufs[6].download(total * 144), total) if total else []
        g2 = np.frombuffer(bufs[0].download(grows.nbytes), dtype=np.uint64).reshape(-1, GROUP_WORDS)
        s2 = np.frombuffer(bufs[1].download(srows.nbytes), dtype=np.uint64).reshape(-1, STATE_WORDS)
        e2 = np.frombuffer(bufs[3].download(erows.nbytes), dtype=np.uint64).reshape(-1, ENTRY_WORDS) if len(erows) \
            else erows
    finally:
        for b in bufs:
            if b is not None:
                b.free()
    return res, unpack_groups(g2), unpack_state(s2), e2.copy(), msgs
