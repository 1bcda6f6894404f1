"""Batched follower append on the GPU (elog_append_batch_device, include/ewal.h):
`raft.handleAppendEntries` (raft/raft.go:410-416) with `raftLog.maybeAppend`
(raft/log.go:49-84) for one msgApp per raft group, over logs kept as windows
of entry terms in one device array, and the msgAppResp batch as emsg_out
records that `raftmsg.encode_messages_device` takes directly."""
import ctypes as C

import numpy as np

from ._lib import lib, check
from .raftmsg import _ptr

GROUP_WORDS = 8    # elog_group, 64 B
APP_WORDS = 8      # elog_app, 64 B
RESULT_WORDS = 6   # elog_app_result, 48 B (word 0: status | accepted << 32)
RESP_WORDS = 18    # emsg_out, 144 B (word 17: reject | pad << 32)
ENTRY_WORDS = 5    # ewal_entry, 40 B (word 4: type | data_nil << 32)
MSG_APP_RESP = 4   # raft.msgAppResp
# messages of more entries than this take the wave-per-message kernel (0: an older A/B build, EWAL_LIB_PATH)
LANE_MAX = lib.elog_lane_max_entries() if hasattr(lib, "elog_lane_max_entries") else 0

_U64 = (1 << 64) - 1


def _u64(rows, width):
    return np.array(rows, dtype=np.uint64).reshape(len(rows), width)


def pack_groups(ids, term, committed, unstable, log_offset, logs, capacity=2.0, room=0, fill=0, caps=None):
    """elog_group rows and the d_terms array for per-group term lists `logs`
    (logs[g][k] is the term of raftLog.ents[k] of group g, at raft index
    log_offset[g] + k).  Group g's window starts where group g-1's ends and
    holds max(ceil(capacity * len(logs[g])), len(logs[g]) + room) entries
    (or caps[g] when given); the words no log owns are `fill`.
    Returns ((G, 8) uint64, (n_terms,) uint64)."""
    G = len(logs)
    rows = np.zeros((G, GROUP_WORDS), dtype=np.uint64)
    if caps is None:
        caps = [max(int(np.ceil(capacity * len(t))), len(t) + room) for t in logs]
    terms = np.full(max(sum(caps), 1), fill, dtype=np.uint64)
    off = 0
    for g, t in enumerate(logs):
        rows[g] = np.array([ids[g], term[g], committed[g], unstable[g], log_offset[g], len(t), off, caps[g]],
                           dtype=np.uint64)
        if len(t):
            terms[off:off + len(t)] = np.array(t, dtype=np.uint64)
        off += caps[g]
    return rows, terms


def unpack_groups(rows, terms):
    """The per-group dicts (id, term, committed, unstable, log_offset, terms)
    of elog_group rows and their d_terms array."""
    out = []
    for r in np.asarray(rows, dtype=np.uint64).reshape(-1, GROUP_WORDS):
        i, tm, c, u, lo, nlog, toff, _ = (int(x) for x in r)
        out.append(dict(id=i, term=tm, committed=c, unstable=u, log_offset=lo,
                        terms=[int(x) for x in terms[toff:toff + nlog]]))
    return out


def pack_apps(apps):
    """elog_app rows and the ewal_entry rows of their entries.  An app is a
    dict: group, from_, index, log_term, commit and either ents (a list of
    terms, or of dicts with term / index / type) or an explicit
    (ents_first, n_ents) range `ents_at` into entries another app packed (a
    leader's fan-out shares one range)."""
    rows, ents = [], []
    for a in apps:
        if "ents_at" in a:
            first, cnt = a["ents_at"]
        else:
            es = a.get("ents") or ()
            first, cnt = len(ents), len(es)
            for k, e in enumerate(es):
                e = e if isinstance(e, dict) else dict(term=e, index=(a.get("index", 0) + 1 + k) & _U64)
                ents.append([e.get("term", 0), e.get("index", 0), 0, 0,
                             (e.get("type", 0) & 0xFFFFFFFF) | (1 << 32)])   # Data nil
        rows.append([a.get("group", 0), a.get("from_", 0), a.get("index", 0), a.get("log_term", 0),
                     a.get("commit", 0), first, cnt, 0])
    return _u64(rows, APP_WORDS), _u64(ents, ENTRY_WORDS)


def results_from(raw, n):
    """elog_app_result rows (bytes) as dicts."""
    out = []
    for r in np.frombuffer(raw, dtype=np.uint64, count=n * RESULT_WORDS).reshape(n, RESULT_WORDS):
        w0 = int(r[0])
        out.append(dict(status=w0 & 0xFFFFFFFF, accepted=w0 >> 32, conflict=int(r[1]), app_first=int(r[2]),
                        n_app=int(r[3]), last_index=int(r[4]), committed=int(r[5])))
    return out


def responses_from(raw, n):
    """emsg_out rows (bytes) as dicts; None for 144 zero bytes (a message Go
    panicked on sends nothing)."""
    out = []
    for r in np.frombuffer(raw, dtype=np.uint64, count=n * RESP_WORDS).reshape(n, RESP_WORDS):
        if not r.any():
            out.append(None)
            continue
        d = dict(type=int(r[0]), to=int(r[1]), from_=int(r[2]), term=int(r[3]), log_term=int(r[4]),
                 index=int(r[5]), commit=int(r[6]), reject=bool(int(r[17]) & 0xFFFFFFFF))
        d["rest"] = [int(x) for x in r[7:17]]   # entries and snapshot words: all 0
        out.append(d)
    return out


def append_batch_device(ctx, d_groups, G, d_terms, n_terms, d_apps, n, d_ents, n_ents_total, d_res, d_resp=None):
    """elog_append_batch_device over device arrays (elog_group[G], uint64[n_terms],
    elog_app[n], ewal_entry[n_ents_total], elog_app_result[n], emsg_out[n] or
    None).  Returns (n_accepted, n_appended)."""
    acc, app = C.c_uint64(0), C.c_uint64(0)
    check(lib.elog_append_batch_device(ctx.handle, _ptr(d_groups), G, _ptr(d_terms), n_terms, _ptr(d_apps), n,
                                       _ptr(d_ents), n_ents_total, _ptr(d_res), _ptr(d_resp), C.byref(acc),
                                       C.byref(app)))
    return acc.value, app.value


def _up(ctx, arr):
    raw = arr.tobytes()
    d = ctx.alloc(len(raw) + 64)
    if raw:
        d.upload(raw)
    return d


def append_batch(ctx, groups, logs, apps, capacity=2.0):
    """Host convenience: groups are dicts (id, term, committed, unstable,
    log_offset), logs their term lists, apps as pack_apps takes them.  Packs,
    uploads, calls, downloads.  Returns (results, new groups with their logs
    as unpack_groups gives them, responses) -- lists of dicts."""
    n = len(apps)
    need = [0] * len(logs)
    arows, erows = pack_apps(apps)
    for r in arows:
        if int(r[0]) < len(need):
            need[int(r[0])] = max(need[int(r[0])], int(r[6]))
    grows, terms = pack_groups(*([g.get(k, 0) for g in groups] for k in ("id", "term", "committed", "unstable",
                                                                        "log_offset")),
                               logs, capacity=capacity, room=max(need, default=0))
    if n == 0:
        return [], unpack_groups(grows, terms), []
    bufs = [_up(ctx, grows), _up(ctx, terms), _up(ctx, arows), _up(ctx, erows), ctx.alloc(n * 48 + 64),
            ctx.alloc(n * 144 + 64)]
    try:
        append_batch_device(ctx, bufs[0], len(groups), bufs[1], len(terms), bufs[2], n, bufs[3], len(erows),
                            bufs[4], bufs[5])
        res = results_from(bufs[4].download(n * 48), n)
        resp = responses_from(bufs[5].download(n * 144), n)
        g2 = np.frombuffer(bufs[0].download(grows.nbytes), dtype=np.uint64).reshape(-1, GROUP_WORDS)
        t2 = np.frombuffer(bufs[1].download(terms.nbytes), dtype=np.uint64)
    finally:
        for b in bufs:
            b.free()
    return res, unpack_groups(g2, t2), resp
