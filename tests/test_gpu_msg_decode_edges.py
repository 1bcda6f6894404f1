"""Edge-lattice parity of emsg_decode_batch_device: the bodies of
tests/msg_decode_cases.py, one batch per family, each compared with the
oracle's raftpb.Message.Unmarshal (tests/test_msg_decode_host.py holds the
oracle against a second reference over the same bodies, and asserts that
every body sent here has a small proven bound on proto.Skip's loops).

What is compared, per body:
  Go returns nil, ErrUnexpectedEOF or ErrWrongType, and the groups nest
    within the device walker's stack: the status and every value Go leaves
    in the struct, as tests/test_gpu_raftmsg.py compares them;
  Go panics or never returns: the status (Go hands the caller no value);
  Go returns nil and the groups nest deeper: EWAL_UNSUPPORTED_ENCODING;
  EWAL_UNSUPPORTED_ENCODING anywhere else is a mismatch.
The boundary counts pushes on pb_skip's frame stack: PB_SKIP_DEPTH pushes
(PB_SKIP_DEPTH + 1 start-group tags nested) are exact, one more is 48.
"""
import ctypes as C
import functools
import itertools

import pytest

import msg_decode_cases as K
import pb_model as P
from oracle import oracle as O
from etcd_amd import _lib as L
from etcd_amd._lib import lib

pytestmark = pytest.mark.gpu

SKIP_ITER_CAP = 4096   # as tests/test_msg_decode_host.py asserts it
MSG_KEYS = ("type", "to", "from_", "term", "log_term", "index", "commit", "reject", "unrec", "unrec_len")
ENT_KEYS = ("type", "term", "index", "data", "unrec")
SNAP_KEYS = ("data", "index", "term", "n_nodes", "n_removed", "unrec", "nodes", "removed")
RAW_KEYS = ("status", "reject", "type", "to", "from_", "term", "log_term", "index", "commit", "n_ents", "snap_index",
            "snap_term", "snap_data_len", "snap_n_nodes", "snap_n_removed", "unrec_len", "n_segs")


@functools.lru_cache(maxsize=None)
def expected(body):
    """("full", oracle dict) | ("status", status) | ("unsup", None)"""
    m = P.message_unmarshal(body)
    assert m["skip_iters"] <= SKIP_ITER_CAP
    o = O.message_unmarshal(body)
    if o["status"] in (O.PANIC_BOUNDS, O.NONTERMINATING):
        return "status", o["status"]
    if m["pushes"] > K.MAX_PUSHES:
        assert o["status"] == O.OK
        return "unsup", None
    return "full", o


def device_bodies(fam):
    return [(n, b) for n, b in K.family(fam) if P.message_unmarshal(b)["skip_iters"] <= SKIP_ITER_CAP] \
        if fam == "g" else K.family(fam)


def differs(g, body):
    """None, or what the device's result g has different from what is expected for body."""
    kind, o = expected(body)
    if kind == "status":
        return None if g["status"] == o else "status %d, expected %d" % (g["status"], o)
    if kind == "unsup":
        return None if g["status"] == L.UNSUPPORTED_ENCODING else "status %d, expected 48" % g["status"]
    if g["status"] != o["status"]:
        return "status %d, expected %d" % (g["status"], o["status"])
    for k in MSG_KEYS:
        if g[k] != o[k]:
            return k
    if len(g["ents"]) != len(o["ents"]):
        return "len(ents)"
    for i, (x, y) in enumerate(zip(g["ents"], o["ents"])):
        for k in ENT_KEYS:
            if x[k] != y[k]:
                return "ents[%d].%s" % (i, k)
    for k in SNAP_KEYS:
        if g["snap"][k] != o["snap"][k]:
            return "snap." + k
    return None


def decode_at(ctx, blob, offs, lens, only=None):
    """emsg_decode_batch_device over blob at (offs, lens): (dicts, the raw
    emsg_message array, *n_entries).  The dicts are etcd_amd.raftmsg.
    decode_messages' (None for an index outside `only`, when that is given)."""
    n = len(offs)
    d = ctx.alloc(len(blob) + 64)
    try:
        if blob:
            d.upload(blob)
        out = (L.MessageDesc * n)()
        tot = C.c_uint64(0)
        rc = lib.emsg_decode_batch_device(ctx.handle, d.ptr, len(blob), (C.c_uint64 * n)(*offs),
                                          (C.c_uint64 * n)(*lens), n, out, C.byref(tot))
        assert rc == L.OK, rc
        ents = (L.EntryDesc * max(tot.value, 1))()
        assert lib.emsg_copy_entries(ctx.handle, 0, ents, tot.value) == tot.value
        nseg = out[n - 1].segs_first + out[n - 1].n_segs
        segs = (L.SegmentDesc * max(nseg, 1))()
        assert lib.emsg_copy_segments(ctx.handle, 0, segs, nseg) == nseg
    finally:
        d.free()
    res = []
    for i, m in enumerate(out):
        if only is not None and i not in only:
            res.append(None)
            continue
        bykind = {}
        for g in segs[m.segs_first:m.segs_first + m.n_segs]:
            bykind.setdefault((g.kind, g.ent), []).append(g)

        def cat(kind, ent=-1):
            gs = bykind.get((kind, ent))
            return b"".join(blob[g.off:g.off + g.len] for g in gs) if gs else None

        es = []
        for j, e in enumerate(ents[m.ents_first:m.ents_first + m.n_ents]):
            data = (cat(L.SEG_ENTRY_DATA, j) if e.data_nil == 2 else
                    None if e.data_nil else blob[e.data_off:e.data_off + e.data_len])
            es.append(dict(type=e.type, term=e.term, index=e.index, data=data, unrec=cat(L.SEG_ENTRY_UNREC, j)))
        sd = (cat(L.SEG_SNAP_DATA) if m.snap_data_off == -2 else
              None if m.snap_data_off < 0 else blob[m.snap_data_off:m.snap_data_off + m.snap_data_len])
        res.append(dict(status=m.status, type=m.type, to=m.to, from_=m.from_, term=m.term, log_term=m.log_term,
                        index=m.index, commit=m.commit, reject=bool(m.reject), ents=es, unrec_len=m.unrec_len,
                        unrec=cat(L.SEG_UNREC),
                        snap=dict(data=sd, index=m.snap_index, term=m.snap_term, n_nodes=m.snap_n_nodes,
                                  n_removed=m.snap_n_removed, unrec=cat(L.SEG_SNAP_UNREC),
                                  nodes=[g.off for g in bykind.get((L.SEG_SNAP_NODE, -1), [])],
                                  removed=[g.off for g in bykind.get((L.SEG_SNAP_REMOVED, -1), [])])))
    return res, out, tot.value


def decode(ctx, bodies, only=None):
    offs = list(itertools.accumulate([0] + [len(b) for b in bodies[:-1]]))
    return decode_at(ctx, b"".join(bodies), offs, [len(b) for b in bodies], only)


def report(cases, got):
    bad = [(name, why, body.hex()) for (name, body), g in zip(cases, got) if g is not None
           for why in [differs(g, body)] if why]
    assert not bad, "%d of %d bodies differ; the first: %r" % (len(bad), len(cases), bad[:5])


@pytest.mark.parametrize("fam", list(K.FAMILIES))
def test_family(ctx, fam):
    cases = device_bodies(fam)
    assert len(cases) * 100 >= 99 * len(K.family(fam))
    got, _, _ = decode(ctx, [b for _, b in cases])
    report(cases, got)
    if fam == "f":   # the boundary is met from both sides, at every level
        st = {name: g["status"] for (name, _), g in zip(cases, got)}
        for lv in K.LEVELS:
            assert st["f/%s.nest%d" % (lv, K.MAX_NESTED_STARTS)] == L.OK
            assert st["f/%s.siblings" % lv] == L.OK
            assert st["f/%s.nest%d" % (lv, K.MAX_NESTED_STARTS + 1)] == L.UNSUPPORTED_ENCODING
            assert st["f/%s.back11" % lv] == st["f/%s.back12" % lv] == L.NONTERMINATING
            assert st["f/%s.back-over-group" % lv] == L.NONTERMINATING


def test_no_over_read(ctx):
    """A prefix of S decodes the same whether zeros or S's own continuation lie behind it."""
    cases = K.prefixes()
    alone, _, _ = decode(ctx, [b for _, b in cases])
    inside, _, _ = decode_at(ctx, K.S, [0] * len(cases), [len(b) for _, b in cases])
    report(cases, inside)
    assert alone == inside
    # and from an odd offset, with S's head before the body and its tail behind it
    blob = K.S[-7:] + K.S + K.S[:9]
    shifted, _, _ = decode_at(ctx, blob, [7] * len(cases), [len(b) for _, b in cases])
    assert shifted == alone


def structured():
    seen, out = set(), []
    for f in K.STRUCTURED:
        for name, b in K.family(f):
            if b not in seen:
                seen.add(b)
                out.append((name, b))
    return out


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_batch_sizes_around_one_block(ctx, n):
    pool = structured()
    cases = [pool[(k * 37 + n) % len(pool)] for k in range(n)]
    got, out, total = decode(ctx, [b for _, b in cases])
    report(cases, got)
    check_placement(out, total)


def check_placement(out, total):
    ents = segs = 0
    for i, m in enumerate(out):
        assert (m.ents_first, m.segs_first) == (ents, segs), i
        ents += m.n_ents
        segs += m.n_segs
    assert total == ents
    return ents, segs


def test_large_batch_then_small_on_the_same_ctx(ctx):
    """70 001 bodies: both exclusive scans run over many scan tiles with uneven
    counts per message.  Each distinct body is compared in full once; its
    repeats must give the same position-independent words."""
    pool = structured()
    n = 70001
    assert len(pool) < n
    cases = [pool[k % len(pool)] for k in range(n)]
    got, out, total = decode(ctx, [b for _, b in cases], only=set(range(len(pool))))
    ents, segs = check_placement(out, total)
    assert ents > n and segs > n // 4
    report(cases, got)
    raw = [tuple(getattr(m, k) for k in RAW_KEYS) for m in out]
    bad = [k for k in range(len(pool), n) if raw[k] != raw[k % len(pool)]]
    assert not bad, (len(bad), bad[:5])
    small = [("S", K.S), ("empty", b""), ("group", K.put("msg", K.group()))]
    got, out, total = decode(ctx, [b for _, b in small])
    check_placement(out, total)
    report(small, got)
    assert total == 4 and [m.n_segs for m in out] == [4, 0, 5]   # nothing of the large batch is left behind


# ---- the host half of the call ---------------------------------------------
def filled(n):
    out = (L.MessageDesc * n)()
    C.memset(out, 0xA5, C.sizeof(out))
    return out


def u64s(vals):
    return (C.c_uint64 * max(len(vals), 1))(*vals)


def test_empty_batches(ctx):
    d = ctx.alloc(256)
    try:
        d.upload(K.S)
        tot = C.c_uint64(77)
        assert lib.emsg_decode_batch_device(ctx.handle, d.ptr, len(K.S), None, None, 0, None, C.byref(tot)) == L.OK
        assert tot.value == 0
        assert lib.emsg_decode_batch_device(ctx.handle, d.ptr, len(K.S), None, None, 0, None, None) == L.OK
        assert lib.emsg_decode_batch_device(ctx.handle, None, 0, None, None, 0, None, None) == L.OK
        # no buffer at all, and every body empty
        out = filled(3)
        assert lib.emsg_decode_batch_device(ctx.handle, None, 0, u64s([0] * 3), u64s([0] * 3), 3, out,
                                            C.byref(tot)) == L.OK
        assert tot.value == 0
        for m in out:
            assert (m.status, m.n_ents, m.n_segs, m.unrec_len, m.snap_data_off) == (L.OK, 0, 0, 0, -1)
        assert lib.emsg_copy_entries(ctx.handle, 0, None, 0) == 0
        assert lib.emsg_copy_entries(ctx.handle, 1, None, 0) == L.E_INVAL
        assert lib.emsg_copy_segments(ctx.handle, 0, None, 0) == 0
        assert lib.emsg_copy_segments(ctx.handle, 1, None, 0) == L.E_INVAL
    finally:
        d.free()


@pytest.mark.parametrize("pos", [0, 2, 4])
@pytest.mark.parametrize("what", ["one-past", "wraps", "len-2^62", "null-buf"])
def test_bad_ranges_leave_out_alone(ctx, what, pos):
    n, ls = 5, len(K.S)
    d = ctx.alloc(ls * n + 64)
    try:
        d.upload(K.S * n)
        buf_len = ls * n
        offs, lens = [k * ls for k in range(n)], [ls] * n
        ptr = d.ptr
        if what == "one-past":
            offs[pos], lens[pos] = buf_len - ls + 1, ls
        elif what == "wraps":
            offs[pos], lens[pos] = (1 << 64) - 8, 16
        elif what == "len-2^62":
            offs[pos], lens[pos] = 0, 1 << 62
        else:
            ptr = None
        out = filled(n)
        tot = C.c_uint64(77)
        rc = lib.emsg_decode_batch_device(ctx.handle, ptr, buf_len, u64s(offs), u64s(lens), n, out, C.byref(tot))
        assert rc == L.E_INVAL
        assert C.string_at(out, C.sizeof(out)) == b"\xa5" * C.sizeof(out)
        for args in ((None, u64s(lens), out), (u64s(offs), None, out), (u64s(offs), u64s(lens), None)):
            assert lib.emsg_decode_batch_device(ctx.handle, d.ptr, buf_len, args[0], args[1], n, args[2],
                                                None) == L.E_INVAL
        assert lib.emsg_decode_batch_device(None, d.ptr, buf_len, u64s(offs), u64s(lens), n, out, None) == L.E_INVAL
        assert C.string_at(out, C.sizeof(out)) == b"\xa5" * C.sizeof(out)
        # the boundary's other side: a body that ends exactly at buf_len is decoded
        offs, lens = [k * ls for k in range(n)], [ls] * n
        rc = lib.emsg_decode_batch_device(ctx.handle, d.ptr, buf_len, u64s(offs), u64s(lens), n, out, C.byref(tot))
        assert rc == L.OK and tot.value == 2 * n and all(m.status == L.OK for m in out)
    finally:
        d.free()


@pytest.mark.parametrize("which", ["entries", "segments"])
def test_copy_windows(ctx, which):
    pool = structured()
    bodies = [K.S] * 3 + [b for _, b in pool[:200]]
    _, out, total = decode(ctx, bodies)
    if which == "entries":
        copy, desc = lib.emsg_copy_entries, L.EntryDesc
    else:
        copy, desc, total = lib.emsg_copy_segments, L.SegmentDesc, out[len(out) - 1].segs_first + out[len(out) - 1].n_segs
    assert total > 40
    size = C.sizeof(desc)
    whole = (desc * total)()
    assert copy(ctx.handle, 0, whole, total) == total
    whole = C.string_at(whole, total * size)
    assert whole != b"\xa5" * len(whole)
    mid = total // 2
    for first in (0, mid, total):
        left = total - first
        for cap in (0, 1, left - 1, left, left + 5):
            if cap < 0:
                continue
            arr = (desc * (left + 6))()
            C.memset(arr, 0xA5, C.sizeof(arr))
            k = min(cap, left)
            assert copy(ctx.handle, first, arr, cap) == k, (first, cap)
            raw = C.string_at(arr, C.sizeof(arr))
            assert raw[:k * size] == whole[first * size:(first + k) * size]
            assert raw[k * size:] == b"\xa5" * (len(raw) - k * size)     # nothing past the window is written
        assert copy(ctx.handle, first, None, 0) == 0
        assert copy(ctx.handle, first, None, 1) == L.E_INVAL
    arr = (desc * 2)()
    assert copy(ctx.handle, total + 1, arr, 1) == L.E_INVAL
    assert copy(ctx.handle, total + 1, arr, 0) == L.E_INVAL
    assert copy(None, 0, arr, 1) == L.E_INVAL
