"""Batched membership on the GPU (include/ewal.h): `node.ApplyConfChange` with
`raft.addNode` / `removeNode` (raft/node.go:228-236, raft/raft.go:426-435), the
removed[] / msgDenied lines at the head of `raft.Step` (raft.go:376-387), the
removed half of `raft.restore` (:549-552) and the server loop's
EntryConfChange arm with `ConfChange.Unmarshal` (etcdserver/server.go:265-286,
raft/raftpb/raft.pb.go:705-813), for many raft groups at once.  Three calls on
the records the step calls share plus the econf_state side record:
`conf_batch_device` applies requests, `scan_committed_device` turns a Ready's
committed entries into requests, `gate_batch_device` filters any step call's
input array by removed[m.From]."""
import ctypes as C

import numpy as np

from ._lib import lib, check, CONF_FROM_SELF, CONF_MAX_REMOVED
from .raftlead import GROUP_WORDS, SNAP_WORDS, MSG_WORDS, ENTRY_WORDS, messages_from
from .raftprop import STATE_WORDS
from .raftvote import VSTATE_WORDS
from .raftready import RSTATE_WORDS, RESULT_WORDS as READY_WORDS
from .raftmsg import _ptr, _varint

CSTATE_WORDS = 16    # econf_state, 128 B
REQ_WORDS = 4        # econf_req, 32 B
RESULT_WORDS = 6     # econf_result, 48 B (word 0: status | action << 32)
APPLIED_WORDS = 4    # econf_applied, 32 B
SCAN_WORDS = 6       # econf_scan_result, 48 B (word 0: status | detail << 32)
GATE_WORDS = 4       # econf_gate_result, 32 B (word 0: status | action << 32)
ADD, REMOVE, DENIED, RELOAD = 1, 2, 3, 4
ACTIONS = ("not_stepped", "added", "removed", "denied_back", "stopped", "reloaded", "panicked")
NOT_STEPPED, ADDED, REMOVED, DENIED_BACK, STOPPED, RELOADED, PANICKED = range(7)
GATE_ACTIONS = ("", "pass", "denied", "dropped")
G_PASS, G_DENIED, G_DROPPED = 1, 2, 3
FROM_SELF = CONF_FROM_SELF
MSG_DENIED = 8       # raft.msgDenied


def pack_cstate(removed):
    """econf_state rows: one list of removed ids (insertion order) per group."""
    rows = np.zeros((len(removed), CSTATE_WORDS), dtype=np.uint64)
    for g, ids in enumerate(removed):
        ids = list(ids)
        if len(ids) > CONF_MAX_REMOVED:
            raise ValueError("econf_state holds at most %d removed ids" % CONF_MAX_REMOVED)
        rows[g, 0] = len(ids)
        for k, v in enumerate(ids):
            rows[g, 1 + k] = v
    return rows


def unpack_cstate(rows):
    """The per-group lists of removed ids of econf_state rows."""
    out = []
    for r in np.asarray(rows, dtype=np.uint64).reshape(-1, CSTATE_WORDS):
        out.append([int(x) for x in r[1:1 + min(int(r[0]), CONF_MAX_REMOVED)]])
    return out


def removed_u64(cstate_rows):
    """The RemovedNodes ranges `ecompact_req` wants: (u64 values, [(removed_off,
    n_removed) per group]) of econf_state rows, group after group."""
    vals, ranges = [], []
    for ids in unpack_cstate(cstate_rows):
        ranges.append((len(vals), len(ids)))
        vals += ids
    return np.array(vals, dtype=np.uint64), ranges


def pack_reqs(reqs):
    """econf_req rows of request dicts (group, kind, node) or 3-tuples."""
    rows = np.zeros((len(reqs), REQ_WORDS), dtype=np.uint64)
    for k, r in enumerate(reqs):
        if isinstance(r, dict):
            r = (r.get("group", 0), r.get("kind", 0), r.get("node", 0))
        rows[k, :3] = np.array(r, dtype=np.uint64)
    return rows


def conf_change_marshal(id=0, type_=0, node=0, context=b""):
    """ConfChange.MarshalTo (raft/raftpb/raft.pb.go:1108-1130): every field is
    written, field 4 included."""
    return (b"\x08" + _varint(id) + b"\x10" + _varint(type_ & 0xFFFFFFFFFFFFFFFF) + b"\x18" + _varint(node) +
            b"\x22" + _varint(len(context)) + bytes(context))


def results_from(raw, n):
    """econf_result rows (bytes) as dicts."""
    out = []
    for r in np.frombuffer(raw, dtype=np.uint64, count=n * RESULT_WORDS).reshape(n, RESULT_WORDS):
        w0 = int(r[0])
        out.append(dict(status=w0 & 0xFFFFFFFF, action=w0 >> 32, msg_first=int(r[1]), n_msgs=int(r[2]),
                        n_peers=int(r[3]), n_removed=int(r[4])))
    return out


def scan_results_from(raw, n):
    """econf_scan_result rows (bytes) as dicts."""
    out = []
    for r in np.frombuffer(raw, dtype=np.uint64, count=n * SCAN_WORDS).reshape(n, SCAN_WORDS):
        w0 = int(r[0])
        out.append(dict(status=w0 & 0xFFFFFFFF, detail=w0 >> 32, req_first=int(r[1]), n_reqs=int(r[2]),
                        bad_pos=int(r[3]), n_scanned=int(r[4])))
    return out


def gate_results_from(raw, n):
    """econf_gate_result rows (bytes) as dicts."""
    out = []
    for r in np.frombuffer(raw, dtype=np.uint64, count=n * GATE_WORDS).reshape(n, GATE_WORDS):
        w0 = int(r[0])
        out.append(dict(status=w0 & 0xFFFFFFFF, action=w0 >> 32, pass_pos=int(r[1]), msg_pos=int(r[2])))
    return out


def conf_batch_device(ctx, d_groups, d_pstate, d_vstate, d_rstate, d_cstate, G, d_snaps, d_u64, n_u64, d_reqs, n,
                      d_res, d_msgs=None, msgs_cap=0):
    """econf_batch_device over device arrays (elead_group[G], elead_prop_state[G],
    evote_state[G], eready_state[G], econf_state[G], elead_snap[G] or None,
    uint64[n_u64], econf_req[n], econf_result[n], emsg_out[msgs_cap] or None for
    the size query).  Returns (n_msgs, n_changed)."""
    nm, nc = C.c_uint64(0), C.c_uint64(0)
    check(lib.econf_batch_device(ctx.handle, _ptr(d_groups), _ptr(d_pstate), _ptr(d_vstate), _ptr(d_rstate),
                                 _ptr(d_cstate), G, _ptr(d_snaps), _ptr(d_u64), n_u64, _ptr(d_reqs), n, _ptr(d_res),
                                 _ptr(d_msgs), msgs_cap, C.byref(nm), C.byref(nc)))
    return nm.value, nc.value


def scan_committed_device(ctx, d_ready, d_sel, n, G, d_ents, n_ents_total, d_data, data_len_total, d_scan,
                          d_reqs=None, d_applied=None, reqs_cap=0):
    """econf_scan_committed_device over device arrays (eready_result[n], the
    selection given to eready_batch_device or None, ewal_entry[n_ents_total],
    the entries' data, econf_scan_result[n], econf_req[reqs_cap] with
    econf_applied[reqs_cap], or None for both: the size query).  Returns
    (n_reqs, n_entries)."""
    nr, ne = C.c_uint64(0), C.c_uint64(0)
    check(lib.econf_scan_committed_device(ctx.handle, _ptr(d_ready), _ptr(d_sel), n, G, _ptr(d_ents), n_ents_total,
                                          _ptr(d_data), data_len_total, _ptr(d_scan), _ptr(d_reqs), _ptr(d_applied),
                                          reqs_cap, C.byref(nr), C.byref(ne)))
    return nr.value, ne.value


def gate_batch_device(ctx, d_groups, d_cstate, G, d_recs, n, rec_bytes, from_word, d_res, d_pass=None, pass_cap=0,
                      d_msgs=None, msgs_cap=0):
    """econf_gate_batch_device over device arrays (elead_group[G],
    econf_state[G], n records of rec_bytes, econf_gate_result[n], the copies
    and emsg_out[msgs_cap], or None for both: the size query).  Returns
    (n_pass, n_msgs)."""
    np_, nm = C.c_uint64(0), C.c_uint64(0)
    check(lib.econf_gate_batch_device(ctx.handle, _ptr(d_groups), _ptr(d_cstate), G, _ptr(d_recs), n, rec_bytes,
                                      from_word, _ptr(d_res), _ptr(d_pass), pass_cap, _ptr(d_msgs), msgs_cap,
                                      C.byref(np_), C.byref(nm)))
    return np_.value, nm.value


def _rows(a, width):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1, width))


def _up(ctx, arr):
    raw = arr.tobytes()
    d = ctx.alloc(len(raw) + 64)
    if raw:
        d.upload(raw)
    return d


def _free(bufs):
    for b in bufs:
        if b is not None:
            b.free()


def conf_batch(ctx, grows, srows, vrows, rrows, crows, reqs, snaprows=None, u64=None, size_query=False):
    """Host convenience over packed rows (raftprop.pack_logs, pack_state,
    raftvote.pack_vstate, raftready.pack_rstate, pack_cstate; reqs econf_req
    rows, dicts or tuples).  Uploads, asks for the size, calls (unless
    size_query), downloads.  Returns a dict: res, res_rows, msgs, msg_rows,
    groups, pstate, vstate, rstate, cstate, n_msgs, n_changed."""
    reqs = _rows(reqs, REQ_WORDS) if isinstance(reqs, np.ndarray) else pack_reqs(reqs)
    host = [_rows(grows, GROUP_WORDS), _rows(srows, STATE_WORDS), _rows(vrows, VSTATE_WORDS),
            _rows(rrows, RSTATE_WORDS), _rows(crows, CSTATE_WORDS)]
    names = ("groups", "pstate", "vstate", "rstate", "cstate")
    n, G = len(reqs), len(host[0])
    snaprows = None if snaprows is None else _rows(snaprows, SNAP_WORDS)
    u64 = np.ascontiguousarray(np.asarray(u64 if u64 is not None else [], dtype=np.uint64))
    out = dict(zip(names, host), res=[], res_rows=np.zeros((0, RESULT_WORDS), np.uint64), msgs=[],
               msg_rows=np.zeros((0, MSG_WORDS), np.uint64), n_msgs=0, n_changed=0)
    if n == 0:
        return out
    bufs = [_up(ctx, h) for h in host]
    bufs += [None if snaprows is None else _up(ctx, snaprows), _up(ctx, u64), _up(ctx, reqs),
             ctx.alloc(n * 48 + 64)]
    try:
        args = (ctx, bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], G, bufs[5], bufs[6], len(u64), bufs[7], n, bufs[8])
        total, nc = conf_batch_device(*args)
        if not size_query:
            bufs.append(ctx.alloc(total * 144 + 64))
            total, nc = conf_batch_device(*args, bufs[9], total)
            raw = bufs[9].download(total * 144) if total else b""
            out["msg_rows"] = np.frombuffer(raw, dtype=np.uint64).reshape(-1, MSG_WORDS).copy()
            out["msgs"] = messages_from(raw, total) if total else []
        raw = bufs[8].download(n * 48)
        out["res"] = results_from(raw, n)
        out["res_rows"] = np.frombuffer(raw, dtype=np.uint64).reshape(n, RESULT_WORDS).copy()
        for name, h, b in zip(names, host, bufs):
            if h.size:
                out[name] = np.frombuffer(b.download(h.nbytes), dtype=np.uint64).reshape(h.shape).copy()
        out.update(n_msgs=total, n_changed=nc)
    finally:
        _free(bufs)
    return out


def scan_committed(ctx, ready_rows, erows, data=b"", sel=None, G=None, size_query=False):
    """Host convenience: ready_rows eready_result rows (n, 12), erows every
    entry row, data the entries' bytes, sel the selection the Ready call got
    (None: group i, G = n).  Returns a dict: scan (dicts), scan_rows, req_rows
    (n_reqs, 4), applied_rows (n_reqs, 4), n_reqs, n_entries."""
    ready_rows = _rows(ready_rows, READY_WORDS)
    erows = _rows(erows, ENTRY_WORDS)
    n = len(ready_rows)
    G = n if G is None else G
    out = dict(scan=[], scan_rows=np.zeros((0, SCAN_WORDS), np.uint64), req_rows=np.zeros((0, REQ_WORDS), np.uint64),
               applied_rows=np.zeros((0, APPLIED_WORDS), np.uint64), n_reqs=0, n_entries=0)
    if n == 0:
        return out
    data = bytes(data)
    bufs = [_up(ctx, ready_rows), None if sel is None else _up(ctx, np.array(sel, dtype=np.uint64)), _up(ctx, erows),
            _up(ctx, np.frombuffer(data, dtype=np.uint8)), ctx.alloc(n * 48 + 64)]
    try:
        args = (ctx, bufs[0], bufs[1], n, G, bufs[2], len(erows), bufs[3], len(data), bufs[4])
        nr, ne = scan_committed_device(*args)
        if not size_query:
            bufs += [ctx.alloc(nr * 32 + 64), ctx.alloc(nr * 32 + 64)]
            nr, ne = scan_committed_device(*args, bufs[5], bufs[6], nr)
            if nr:
                out["req_rows"] = np.frombuffer(bufs[5].download(nr * 32), dtype=np.uint64).reshape(nr, 4).copy()
                out["applied_rows"] = np.frombuffer(bufs[6].download(nr * 32), dtype=np.uint64).reshape(nr, 4).copy()
        raw = bufs[4].download(n * 48)
        out["scan"] = scan_results_from(raw, n)
        out["scan_rows"] = np.frombuffer(raw, dtype=np.uint64).reshape(n, SCAN_WORDS).copy()
        out.update(n_reqs=nr, n_entries=ne)
    finally:
        _free(bufs)
    return out


def gate_batch(ctx, grows, crows, recs, from_word, size_query=False):
    """Host convenience: recs an (n, W) uint64 array of any step call's input
    rows (W = 6, 8 or 12), from_word the word holding m.From or FROM_SELF.
    Returns a dict: res (dicts), res_rows, pass_rows (n_pass, W), msgs, msg_rows,
    n_pass, n_msgs."""
    recs = np.ascontiguousarray(np.asarray(recs, dtype=np.uint64))
    n, W = recs.shape
    grows, crows = _rows(grows, GROUP_WORDS), _rows(crows, CSTATE_WORDS)
    out = dict(res=[], res_rows=np.zeros((0, GATE_WORDS), np.uint64), pass_rows=np.zeros((0, W), np.uint64), msgs=[],
               msg_rows=np.zeros((0, MSG_WORDS), np.uint64), n_pass=0, n_msgs=0)
    if n == 0:
        return out
    bufs = [_up(ctx, grows), _up(ctx, crows), _up(ctx, recs), ctx.alloc(n * 32 + 64)]
    try:
        args = (ctx, bufs[0], bufs[1], len(grows), bufs[2], n, W * 8, from_word, bufs[3])
        npass, nm = gate_batch_device(*args)
        if not size_query:
            bufs += [ctx.alloc(npass * W * 8 + 64), ctx.alloc(nm * 144 + 64)]
            npass, nm = gate_batch_device(*args, bufs[4], npass, bufs[5], nm)
            if npass:
                out["pass_rows"] = np.frombuffer(bufs[4].download(npass * W * 8), dtype=np.uint64).reshape(npass, W).copy()
            raw = bufs[5].download(nm * 144) if nm else b""
            out["msg_rows"] = np.frombuffer(raw, dtype=np.uint64).reshape(-1, MSG_WORDS).copy()
            out["msgs"] = messages_from(raw, nm) if nm else []
        raw = bufs[3].download(n * 32)
        out["res"] = gate_results_from(raw, n)
        out["res_rows"] = np.frombuffer(raw, dtype=np.uint64).reshape(n, GATE_WORDS).copy()
        out.update(n_pass=npass, n_msgs=nm)
    finally:
        _free(bufs)
    return out
