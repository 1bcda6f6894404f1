"""raftpb.Message on the GPU: the /raft ingress decode (emsg_decode_batch_device)
and the egress encode (emsg_encode_batch_device).

Mirrors `(*raftpb.Message).Unmarshal` (raft/raftpb/raft.pb.go:407-617), the
call etcdhttp's serveRaft makes for every POST /raft body
(etcdserver/etcdhttp/http.go:119-146), batched over many bodies.  Results are
dicts shaped like the oracle's `message_unmarshal` (tests compare them).

The encode mirrors `(*raftpb.Message).Marshal` (raft.pb.go:1000-1068), the call
`send` makes per outgoing message (etcdserver/cluster_store.go:118-144),
batched over messages whose Entries and Snapshot.Data stay in HBM."""
import ctypes as C

from . import _lib as L
from ._lib import lib, check


def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def entry_marshal(type_=0, term=0, index=0, data=None):
    """raftpb.Entry.MarshalTo (raft/raftpb/raft.pb.go:921-943): field 4 always written."""
    d = data or b""
    return b"".join([b"\x08", _varint(type_ & 0xFFFFFFFFFFFFFFFF), b"\x10", _varint(term), b"\x18", _varint(index),
                     b"\x22", _varint(len(d)), d])


def message_marshal(type_=0, to=0, from_=0, term=0, log_term=0, index=0, entries=(), commit=0, snapshot=b"",
                    reject=False):
    """raftpb.Message.MarshalTo (raft/raftpb/raft.pb.go:1010-1068); entries are
    marshalled Entry bodies, snapshot a marshalled raftpb.Snapshot."""
    parts = [b"\x08", _varint(type_), b"\x10", _varint(to), b"\x18", _varint(from_), b"\x20", _varint(term),
             b"\x28", _varint(log_term), b"\x30", _varint(index)]
    for e in entries:
        parts += [b"\x3a", _varint(len(e)), e]
    parts += [b"\x40", _varint(commit), b"\x4a", _varint(len(snapshot)), snapshot, b"\x50",
              b"\x01" if reject else b"\x00"]
    return b"".join(parts)


def _fetch(copy, handle, desc, total):
    arr = (desc * max(total, 1))()
    if total:
        k = copy(handle, 0, arr, total)
        check(0 if k >= 0 else int(k))
    return arr


def decode_messages(ctx, bodies):
    """Decode message bodies (bytes each): one dict per body, with every
    XXX_unrecognized, split bytes field and the Snapshot's Nodes /
    RemovedNodes assembled from the message's segments (include/ewal.h)."""
    n = len(bodies)
    if n == 0:
        return []
    blob = b"".join(bytes(b) for b in bodies)
    offs, pos = [], 0
    for b in bodies:
        offs.append(pos)
        pos += len(b)
    d = ctx.alloc(len(blob) + 64)
    try:
        if blob:
            d.upload(blob)
        out = (L.MessageDesc * n)()
        tot = C.c_uint64(0)
        check(lib.emsg_decode_batch_device(ctx.handle, d.ptr, len(blob), (C.c_uint64 * n)(*offs),
                                           (C.c_uint64 * n)(*[len(b) for b in bodies]), n, out, C.byref(tot)))
        ents = _fetch(lib.emsg_copy_entries, ctx.handle, L.EntryDesc, tot.value)
        nseg = out[n - 1].segs_first + out[n - 1].n_segs
        segs = _fetch(lib.emsg_copy_segments, ctx.handle, L.SegmentDesc, nseg)
    finally:
        d.free()
    res = []
    for m in out:
        bykind = {}
        for g in segs[m.segs_first:m.segs_first + m.n_segs]:
            bykind.setdefault((g.kind, g.ent), []).append(g)

        def cat(kind, ent=-1):
            gs = bykind.get((kind, ent))
            return b"".join(blob[g.off:g.off + g.len] for g in gs) if gs else None

        es = []
        for j, e in enumerate(ents[m.ents_first:m.ents_first + m.n_ents]):
            ei = j   # segments name the entry by its index within the message
            data = (cat(L.SEG_ENTRY_DATA, ei) if e.data_nil == 2 else
                    None if e.data_nil else blob[e.data_off:e.data_off + e.data_len])
            ur = cat(L.SEG_ENTRY_UNREC, ei)
            es.append(dict(type=e.type, term=e.term, index=e.index, data=data, unrec=ur,
                           unrec_len=len(ur) if ur else 0))
        sd = (cat(L.SEG_SNAP_DATA) if m.snap_data_off == -2 else
              None if m.snap_data_off < 0 else blob[m.snap_data_off:m.snap_data_off + m.snap_data_len])
        su = cat(L.SEG_SNAP_UNREC)
        res.append(dict(status=m.status, type=m.type, to=m.to, from_=m.from_, term=m.term, log_term=m.log_term,
                        index=m.index, commit=m.commit, reject=bool(m.reject), ents=es, unrec_len=m.unrec_len,
                        unrec=cat(L.SEG_UNREC),
                        snap=dict(data=sd, index=m.snap_index, term=m.snap_term, n_nodes=m.snap_n_nodes,
                                  n_removed=m.snap_n_removed, unrec=su, unrec_len=len(su) if su else 0,
                                  nodes=[g.off for g in bykind.get((L.SEG_SNAP_NODE, -1), [])],
                                  removed=[g.off for g in bykind.get((L.SEG_SNAP_REMOVED, -1), [])])))
    return res


# bytes of the output one wave of the encode's body kernel owns (0: an older A/B build, EWAL_LIB_PATH)
ENCODE_TILE = lib.emsg_encode_tile_bytes() if hasattr(lib, "emsg_encode_tile_bytes") else 0


def _ptr(d):
    """A device pointer argument: None, a DeviceBuffer, a c_void_p or an int."""
    if d is None:
        return None
    if hasattr(d, "ptr"):
        d = d.ptr
    return d if isinstance(d, C.c_void_p) else C.c_void_p(d)


def encode_messages_device(ctx, d_data, data_len, d_msgs, n, d_ents, n_ents, d_u64, n_u64, d_out, cap):
    """emsg_encode_batch_device over device arrays (emsg_out[n], ewal_entry[n_ents],
    uint64[n_u64]; Data ranges index d_data[0, data_len)): message i is
    d_out[offs[i], offs[i] + lens[i]).  Returns (offs, lens, total); with
    d_out=None it is the size query and nothing is written."""
    enc = (L.Encoded * max(n, 1))()
    total = C.c_uint64(0)
    check(lib.emsg_encode_batch_device(ctx.handle, _ptr(d_data), data_len, _ptr(d_msgs), n, _ptr(d_ents), n_ents,
                                       _ptr(d_u64), n_u64, _ptr(d_out), cap, enc, C.byref(total)))
    return [e.off for e in enc[:n]], [e.len for e in enc[:n]], total.value


def pack_messages(msgs):
    """Host arrays for a list of message dicts shaped like decode_messages'
    results (type, to, from_, term, log_term, index, commit, reject, ents:
    [type, term, index, data], snap: data, index, term, nodes, removed; all
    optional): (data blob, emsg_out[], ewal_entry[], uint64[]) and their
    counts n_ents, n_u64."""
    blob, u64, ents = bytearray(), [], []
    out = (L.OutMsg * max(len(msgs), 1))()
    for o, m in zip(out, msgs):
        o.type, o.to, o.from_, o.term = m.get("type", 0), m.get("to", 0), m.get("from_", 0), m.get("term", 0)
        o.log_term, o.index, o.commit = m.get("log_term", 0), m.get("index", 0), m.get("commit", 0)
        o.reject = 1 if m.get("reject") else 0
        es = m.get("ents") or ()
        o.ents_first, o.n_ents = len(ents), len(es)
        for e in es:
            d = e.get("data")
            ents.append((e.get("term", 0), e.get("index", 0), len(blob) if d else 0, len(d) if d else 0,
                         e.get("type", 0), 1 if d is None else 0))
            blob += d or b""
        sn = m.get("snap") or {}
        d = sn.get("data") or b""
        o.snap_index, o.snap_term = sn.get("index", 0), sn.get("term", 0)
        o.snap_data_off, o.snap_data_len = (len(blob) if d else 0), len(d)
        blob += d
        nodes, removed = list(sn.get("nodes") or ()), list(sn.get("removed") or ())
        o.snap_nodes_off, o.snap_n_nodes = len(u64), len(nodes)
        u64 += nodes
        o.snap_removed_off, o.snap_n_removed = len(u64), len(removed)
        u64 += removed
    earr = (L.EntryDesc * max(len(ents), 1))()
    for a, (term, index, off, ln, type_, nil) in zip(earr, ents):
        a.term, a.index, a.data_off, a.data_len, a.type, a.data_nil = term, index, off, ln, type_, nil
    return bytes(blob), out, earr, len(ents), (C.c_uint64 * max(len(u64), 1))(*u64), len(u64)


def encode_size(msgs):
    """emsg_encode_size: the summed Message.Size() of the message dicts (host only)."""
    _, out, earr, ne, u64, nu = pack_messages(msgs)
    return lib.emsg_encode_size(out, len(msgs), earr, ne, u64, nu)


def _up(ctx, raw):
    d = ctx.alloc(len(raw) + 64)
    if raw:
        d.upload(raw)
    return d


def encode_messages(ctx, msgs):
    """Marshal message dicts (host bytes) on the GPU: uploads the payload and
    the descriptors, encodes, downloads; one `bytes` per message."""
    n = len(msgs)
    if n == 0:
        return []
    blob, out, earr, ne, u64, nu = pack_messages(msgs)
    bufs = [_up(ctx, blob), _up(ctx, C.string_at(out, n * C.sizeof(L.OutMsg))),
            _up(ctx, C.string_at(earr, ne * C.sizeof(L.EntryDesc))), _up(ctx, C.string_at(u64, nu * 8))]
    try:
        args = (ctx, bufs[0], len(blob), bufs[1], n, bufs[2], ne, bufs[3], nu)
        _, _, total = encode_messages_device(*args, None, 0)
        bufs.append(ctx.alloc(total + 64))
        offs, lens, total = encode_messages_device(*args, bufs[4], total)
        raw = bufs[4].download(total)
    finally:
        for b in bufs:
            b.free()
    return [raw[o:o + k] for o, k in zip(offs, lens)]
