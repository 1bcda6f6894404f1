"""Batched `raft.StartNode` / `raft.RestartNode` on the GPU (include/ewal.h,
raft/node.go:125-161): builds a group's five records, its snapshot row and its
window of entries from a batch replay's result (kind 1) or from a list of peers
(kind 2).  `node_batch_device` is the call over device arrays, `node_batch` the
host convenience over numpy rows; `entries_device` and `reqs_from_batch` hand a
`ewal_readall_batch_device` result to it without the entries leaving HBM."""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import lib, check
from .raftlead import GROUP_WORDS, SNAP_WORDS, ENTRY_WORDS
from .raftprop import STATE_WORDS
from .raftvote import VSTATE_WORDS
from .raftready import RSTATE_WORDS
from .raftconf import CSTATE_WORDS
from .raftmsg import _ptr

REQ_WORDS = 16       # enode_req, 128 B
PEER_WORDS = 4       # enode_peer, 32 B
RESULT_WORDS = 6     # enode_result, 48 B (word 0: status | action << 32)
KIND_NONE, KIND_RESTART, KIND_START = 0, 1, 2
ACTIONS = ("none", "restarted", "restarted_snap", "started", "panicked")
NONE, RESTARTED, RESTARTED_SNAP, STARTED, PANICKED = range(5)
NO_SNAP = L.NODE_NO_SNAP
REQ_FIELDS = ("group", "kind", "id", "ents_first", "ents_cap", "src_first", "n_src", "data_delta", "hs_term", "hs_vote",
              "hs_commit", "snap")


def pack_reqs(reqs):
    """enode_req rows of request dicts (REQ_FIELDS; snap defaults to NO_SNAP)."""
    rows = np.zeros((len(reqs), REQ_WORDS), dtype=np.uint64)
    for k, r in enumerate(reqs):
        for j, name in enumerate(REQ_FIELDS):
            rows[k, j] = np.uint64(r.get(name, NO_SNAP if name == "snap" else 0))
    return rows


def pack_peers(peers):
    """(enode_peer rows, the Context bytes) of a list of (id, context) pairs."""
    rows = np.zeros((len(peers), PEER_WORDS), dtype=np.uint64)
    ctx = bytearray()
    for k, (id_, context) in enumerate(peers):
        context = bytes(context or b"")
        rows[k, :3] = np.array([id_, len(ctx), len(context)], dtype=np.uint64)
        ctx += context
    return rows, bytes(ctx)


def results_from(raw, n):
    """enode_result rows (bytes) as dicts."""
    out = []
    for r in np.frombuffer(raw, dtype=np.uint64, count=n * RESULT_WORDS).reshape(n, RESULT_WORDS):
        w0 = int(r[0])
        out.append(dict(status=w0 & 0xFFFFFFFF, action=w0 >> 32, nlog=int(r[1]), committed=int(r[2]),
                        log_offset=int(r[3]), n_peers=int(r[4]), data_first=int(r[5])))
    return out


def node_batch_device(ctx, d_groups, d_pstate, d_vstate, d_rstate, d_cstate, d_snaps, G, d_ents, n_ents_total, d_src,
                      n_src_total, d_in_snaps, n_in_snaps, d_u64, n_u64, d_peers, n_peers_total, d_ctx, ctx_len,
                      d_reqs, n, d_res, d_data=None, data_base=0, data_cap=0):
    """enode_batch_device over device arrays (the five record arrays and
    elead_snap[G], the windows' ewal_entry array, the source entries, the input
    snapshots with their uint64 ranges, the peers with their Context bytes,
    enode_req[n], enode_result[n], and d_data[data_cap] or None for the size
    query).  A source may be a DeviceBuffer, an integer address (what
    entries_device returns) or None.  Returns (n_data, n_copied, n_built)."""
    nd, nc, nb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    src = C.c_void_p(d_src) if isinstance(d_src, int) else _ptr(d_src)
    check(lib.enode_batch_device(ctx.handle, _ptr(d_groups), _ptr(d_pstate), _ptr(d_vstate), _ptr(d_rstate),
                                 _ptr(d_cstate), _ptr(d_snaps), G, _ptr(d_ents), n_ents_total, src, n_src_total,
                                 _ptr(d_in_snaps), n_in_snaps, _ptr(d_u64), n_u64, _ptr(d_peers), n_peers_total,
                                 _ptr(d_ctx), ctx_len, _ptr(d_data), data_base, data_cap, _ptr(d_reqs), n, _ptr(d_res),
                                 C.byref(nd), C.byref(nc), C.byref(nb)))
    return nd.value, nc.value, nb.value


def entries_device(ctx):
    """ewal_batch_entries_device: (address, n_total) of the ctx-owned device
    array holding the last batch replay's entries; valid until the next pipeline
    call on ctx."""
    p, n = C.c_void_p(), C.c_uint64(0)
    check(lib.ewal_batch_entries_device(ctx.handle, C.byref(p), C.byref(n)))
    return p.value or 0, n.value


def readall_batch_raw(dbuf, lens, ris):
    """ewal_readall_batch_device returning the raw ewal_result array, as
    reqs_from_batch takes it."""
    ns = len(lens)
    out = (L.Result * max(ns, 1))()
    rc = lib.ewal_readall_batch_device(dbuf.ctx.handle, dbuf.ptr, ns, (C.c_uint64 * max(ns, 1))(*lens),
                                       (C.c_uint64 * max(ns, 1))(*ris), out)
    if rc < 0:
        check(rc)
    return out


def reqs_from_batch(ctx, results, shard_off, rows=None):
    """enode_reqs_from_batch: enode_req rows (n_shards, 16) of a raw ewal_result
    array (readall_batch_raw) and the shards' places in the data buffer.  rows:
    an array to fill in place (id, ents_first, ents_cap and snap are kept);
    a fresh one has them 0 but snap, which is NO_SNAP."""
    ns = len(shard_off)
    if rows is None:
        rows = np.zeros((ns, REQ_WORDS), dtype=np.uint64)
        rows[:, 11] = np.uint64(NO_SNAP)
    assert rows.shape == (ns, REQ_WORDS) and rows.dtype == np.uint64 and rows.flags["C_CONTIGUOUS"]
    check(lib.enode_reqs_from_batch(ctx.handle, C.cast(results, C.c_void_p), ns, (C.c_uint64 * max(ns, 1))(*shard_off),
                                    rows.ctypes.data_as(C.c_void_p)))
    return rows


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


def node_batch(ctx, grows, srows, vrows, rrows, crows, snaprows, erows, reqs, src=None, in_snaps=None, u64=None,
               peers=None, ctx_bytes=b"", data=b"", data_base=0, data_cap=None, size_query=False):
    """Host convenience over packed rows: the six group arrays and every entry
    row as the call finds them, reqs (enode_req rows or dicts), the source
    entry rows, the input snapshot rows with their uint64 values, enode_peer
    rows with their Context bytes, and `data`, the content d_data has before
    the call (data_cap: its capacity, default what the call needs).  Uploads,
    asks for the size, calls (unless size_query), downloads.  Returns a dict:
    res, res_rows, groups, pstate, vstate, rstate, cstate, snaps, ents, data,
    n_data, n_copied, n_built."""
    reqs = _rows(reqs, REQ_WORDS) if isinstance(reqs, np.ndarray) else pack_reqs(reqs)
    host = [_rows(grows, GROUP_WORDS), _rows(srows, STATE_WORDS), _rows(vrows, VSTATE_WORDS),
            _rows(rrows, RSTATE_WORDS), _rows(crows, CSTATE_WORDS), _rows(snaprows, SNAP_WORDS),
            _rows(erows, ENTRY_WORDS)]
    names = ("groups", "pstate", "vstate", "rstate", "cstate", "snaps", "ents")
    n, G = len(reqs), len(host[0])
    src = _rows(src if src is not None else [], ENTRY_WORDS)
    in_snaps = _rows(in_snaps if in_snaps is not None else [], SNAP_WORDS)
    u64 = np.ascontiguousarray(np.asarray(u64 if u64 is not None else [], dtype=np.uint64))
    peers = _rows(peers if peers is not None else [], PEER_WORDS)
    ctx_bytes, data = bytes(ctx_bytes), bytes(data)
    out = dict(zip(names, host), res=[], res_rows=np.zeros((0, RESULT_WORDS), np.uint64), data=data, n_data=0,
               n_copied=0, n_built=0)
    if n == 0:
        return out
    bufs = [_up(ctx, h) for h in host]
    bufs += [_up(ctx, src), _up(ctx, in_snaps), _up(ctx, u64), _up(ctx, peers),
             _up(ctx, np.frombuffer(ctx_bytes, dtype=np.uint8)), _up(ctx, reqs), ctx.alloc(n * 48 + 64)]
    try:
        args = (ctx, bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], bufs[5], G, bufs[6], len(host[6]), bufs[7], len(src),
                bufs[8], len(in_snaps), bufs[9], len(u64), bufs[10], len(peers), bufs[11], len(ctx_bytes), bufs[12], n,
                bufs[13])
        nd, nc, nb = node_batch_device(*args)
        if not size_query:
            cap = nd if data_cap is None else data_cap
            size = max(cap, len(data))
            bufs.append(ctx.alloc(size + 64))
            if data:
                bufs[14].upload(data)
            nd, nc, nb = node_batch_device(*args, bufs[14], data_base, cap)
            out["data"] = bufs[14].download(size) if size else b""
        raw = bufs[13].download(n * 48)
        out["res"] = results_from(raw, n)
        out["res_rows"] = np.frombuffer(raw, dtype=np.uint64).reshape(n, RESULT_WORDS).copy()
        for name, h, b in zip(names, host, bufs):
            if h.size:
                out[name] = np.frombuffer(b.download(h.nbytes), dtype=np.uint64).reshape(h.shape).copy()
        out.update(n_data=nd, n_copied=nc, n_built=nb)
    finally:
        _free(bufs)
    return out
