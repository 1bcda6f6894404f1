"""GPU parity tests of the batched StartNode / RestartNode (enode_batch_device)
against node_cases' restatement: bit-exact for the five records, d_snaps, every
window slot, d_data, d_res and the counters.  The lattice, the reference's
tables (the Ready through the real eready_batch_device), random mixes at 1, 65
and 257 requests scattered over 300 groups with canary groups and canary slots,
the size query, exact NOMEM, every INVAL class leaving every array untouched, a
repeated call, a caller's stream, and ewal_batch_entries_device."""
import ctypes as C

import numpy as np
import pytest

from etcd_amd import _lib as L
from etcd_amd import raftnode as RN
from etcd_amd import wal as W
from etcd_amd.raftmsg import _ptr

import cluster_cases as CL
import node_cases as N

pytestmark = pytest.mark.gpu
M64 = N.M64


def raw_call(ctx, c, with_data=True, G=None, n=None):
    """enode_batch_device without the wrappers: (status, (n_data, n_copied,
    n_built), every array as the call left it, d_data, the result rows)."""
    up = RN._up
    host = [np.ascontiguousarray(c[k]) for k in N.ARRAY_KEYS]
    bufs = [up(ctx, h) for h in host]
    bufs += [up(ctx, c["src"]), up(ctx, c["in_snaps"]), up(ctx, c["u64"]), up(ctx, c["peers"]),
             up(ctx, np.frombuffer(c["ctx"], dtype=np.uint8)), up(ctx, c["reqs"]), ctx.alloc(c["n"] * 48 + 64),
             up(ctx, np.frombuffer(c["data"], dtype=np.uint8))]
    canary = b"\xa5" * (c["n"] * 48)
    if canary:
        bufs[13].upload(canary)
    counters = [C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)]
    try:
        st = L.lib.enode_batch_device(
            ctx.handle, *[_ptr(b) for b in bufs[:6]], c["G"] if G is None else G, _ptr(bufs[6]), c["n_ents_total"],
            _ptr(bufs[7]), len(c["src"]), _ptr(bufs[8]), len(c["in_snaps"]), _ptr(bufs[9]), len(c["u64"]),
            _ptr(bufs[10]), len(c["peers"]), _ptr(bufs[11]), len(c["ctx"]), _ptr(bufs[14]) if with_data else None,
            c["data_base"], c["data_cap"], _ptr(bufs[12]), c["n"] if n is None else n, _ptr(bufs[13]),
            *[C.byref(x) for x in counters])
        arrays = {k: np.frombuffer(b.download(h.nbytes), dtype=np.uint64).reshape(h.shape).copy() if h.size else h
                  for k, h, b in zip(N.ARRAY_KEYS, host, bufs)}
        data = bufs[14].download(len(c["data"])) if c["data"] else b""
        res = bufs[13].download(c["n"] * 48) if c["n"] else b""
    finally:
        RN._free(bufs)
    return st, tuple(x.value for x in counters), arrays, data, res, canary


def assert_untouched(ctx, c, status, **kw):
    st, counters, arrays, data, res, canary = raw_call(ctx, c, **kw)
    assert st == status, (st, status)
    assert counters == (0, 0, 0)
    for k in N.ARRAY_KEYS:
        assert np.array_equal(arrays[k], c[k]), k
    assert data == c["data"] and res == canary


@pytest.mark.parametrize("name,c", N.lattice_calls(), ids=[name for name, _ in N.lattice_calls()])
def test_lattice(ctx, name, c):
    N.check_call(ctx, c)


def _ready(ctx, arrays):
    """One eready_batch_device over every group of the arrays, against the model's newReady."""
    a = dict(arrays, sel=None)
    want = CL.ready_call(a)
    got = CL.DeviceBackend(ctx).ready(a)
    for k in ("res_rows", "save_rows", "pstate", "rstate"):
        assert np.array_equal(got[k], want[k]), k
    return want


def test_node_restart_table(ctx):
    """TestNodeRestart: one Ready with the committed entries 1..commit, no
    HardState and no entries to save; then nothing."""
    t = N.load_kats()["TestNodeRestart"]
    ents = [N.entry_row(e["term"], e["index"], e["type"], 4 if e["data"] else 0, len(e["data"] or ""),
                        0 if e["data"] else 1) for e in t["entries"]]
    st = t["st"]
    c = N.call_of([N.restart(id=t["id"], ents=ents, st=(st["term"], st["vote"], st["commit"]))], G=1)
    got, _ = N.check_call(ctx, c)
    arrays = {k: got[k] for k in CL.ARRAYS}
    rd = _ready(ctx, arrays)
    r = [int(v) for v in rd["res_rows"][0]]
    first = int(c["reqs"][0, 3])
    assert r[0] >> 32 == CL.R_UPDATES and r[1:4] == [0, 0, 0] and r[4:6] == [0, 0]
    assert r[6:8] == [first + 1, len(t["want"]["committed"])] and rd["n_save"] == 0
    row = [int(v) for v in arrays["ents"][first + 1]]
    assert row[:2] == [t["want"]["committed"][0]["term"], t["want"]["committed"][0]["index"]]
    arrays.update(pstate=rd["pstate"], rstate=rd["rstate"])
    rd2 = _ready(ctx, arrays)
    assert rd2["n_ready"] == 0


def test_node_start_table(ctx):
    """TestNode's StartNode(1, [{ID: 1}]): the ConfChange bytes and the first
    Ready's shape before the campaign (the two Readys themselves are played by
    the host test on the restatements)."""
    t = N.load_kats()["TestNode"]
    c = N.call_of([N.start(id=t["id"], peers=[(p["id"], p["context"] or b"") for p in t["peers"]])], G=1, data_fill=3)
    got, _ = N.check_call(ctx, c)
    cc = bytes.fromhex(t["ccdata_hex"])
    assert got["data"][:len(cc)] == cc and got["n_data"] == len(cc)
    first = int(c["reqs"][0, 3])
    assert [int(v) for v in got["ents"][first + 1]] == [1, 1, c["data_base"], len(cc), 1]
    rd = _ready(ctx, {k: got[k] for k in CL.ARRAYS})
    r = [int(v) for v in rd["res_rows"][0]]
    assert r[1:4] == [0, 0, 0]                       # no HardState: the seeding
    assert r[4:6] == [first, 2] and r[6:8] == [first + 1, 1]


def test_restore_table(ctx):
    t = N.load_kats()["TestRestore"]
    s = t["snapshot"]
    c = N.call_of([N.restart(id=t["id"], ents=(), st=(s["term"], 0, s["index"]),
                             snap=N.snapshot(s["index"], s["term"], s["nodes"], s["removed"]))], G=1)
    got, _ = N.check_call(ctx, c)
    g = [int(v) for v in got["groups"][0]]
    assert g[3] == t["last_index"] and g[6] == len(t["prs"])
    for k, (id_, (match, nxt)) in enumerate(sorted((int(i), v) for i, v in t["prs"].items())):
        assert (g[7 + k], g[14 + k], g[21 + k]) == (id_, match, nxt)
    assert [int(v) for v in got["cstate"][0, :3]] == [len(t["removed"])] + t["removed"]
    assert [int(v) for v in got["snaps"][0, :2]] == [s["index"], s["term"]]


@pytest.mark.parametrize("n", [1, 65, 257])
def test_random_mix(ctx, n):
    c = N.random_call(n, n, 300)
    got, want = N.check_call(ctx, c)
    if n > 1:
        acts = N.mix_of(want["outcomes"])
        assert all(acts), acts


def test_size_query_without_start_requests(ctx):
    c = N.call_of([N.restart(id=1, ents=N.E3, st=(1, 0, 1)), N.none()], G=4, groups=[3, 1], data_cap=0)
    N.check_call(ctx, c)


def test_exact_nomem(ctx):
    for spec in (N.restart(id=1, ents=N.E3, cap=3), N.start(id=1, peers=[(1, b""), (2, b"")], cap=3)):
        N.check_call(ctx, N.call_of([spec], G=2))
        tight = dict(spec, cap=2)
        c = N.call_of([tight], G=2)
        assert N.validate(c) == N.E_NOMEM
        assert_untouched(ctx, c, L.E_NOMEM)
    c = N.call_of([N.start(id=1, peers=[(1, b"abc"), (300, b"")])], G=1)
    need = c["data_cap"]
    N.check_call(ctx, c)
    c = N.call_of([N.start(id=1, peers=[(1, b"abc"), (300, b"")])], G=1, data_cap=need - 1)
    assert N.validate(c) == N.E_NOMEM
    assert_untouched(ctx, c, L.E_NOMEM)
    # the size query does not look at data_cap
    st, counters, _, _, _, _ = raw_call(ctx, c, with_data=False)
    assert st == L.OK and counters == (need, 0, 1)


@pytest.mark.parametrize("name,c", N.inval_calls(), ids=[name for name, _ in N.inval_calls()])
def test_inval_leaves_everything_untouched(ctx, name, c):
    assert N.validate(c) == N.E_INVAL
    assert_untouched(ctx, c, L.E_INVAL)
    assert_untouched(ctx, c, L.E_INVAL, with_data=False)


def test_inval_wins_over_nomem_and_host_checks(ctx):
    c = N.call_of([N.restart(id=1, ents=N.E3, cap=2), N.start(id=2, group=0)], G=2)
    assert N.validate(c) == N.E_INVAL
    assert_untouched(ctx, c, L.E_INVAL)
    ok = N.call_of([N.restart(id=1, ents=N.E3)], G=1)
    assert_untouched(ctx, ok, L.E_INVAL, G=N.INT_MAX)
    assert_untouched(ctx, ok, L.E_INVAL, n=N.INT_MAX)
    st, counters, arrays, _, _, _ = raw_call(ctx, ok, n=0)
    assert st == L.OK and counters == (0, 0, 0) and all(np.array_equal(arrays[k], ok[k]) for k in N.ARRAY_KEYS)


def test_repeated_call_and_stream(ctx):
    """The same call twice gives the same bytes (the second on rows the first
    built: their previous content is not read), also on a caller's stream."""
    import torch
    c = N.random_call(5, 65, 300)
    got, want = N.check_call(ctx, c)
    again = N.copy_call(c)
    for k in N.ARRAY_KEYS:
        again[k] = got[k]
    again["data"] = got["data"]
    N.assert_parity(again, N.run_device(ctx, again), N.expected(again))
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    try:
        N.check_call(ctx, c)
    finally:
        ctx.set_stream(0)


def test_batch_entries_device(ctx):
    """ewal_batch_entries_device points at the bytes ewal_batch_copy_entries
    returns, and enode_reqs_from_batch names each shard's range of them."""
    shards = [W.synth_wal(1 << 14, 16, 128, seed=s)[0] for s in (3, 4, 5)]
    blob = b"".join(bytes(x) for x in shards)
    d = ctx.alloc(len(blob) + 64)
    try:
        d.upload(blob)
        res = RN.readall_batch_raw(d, [len(x) for x in shards], [1] * len(shards))
        ptr, total = RN.entries_device(ctx)
        offs = np.cumsum([0] + [len(x) for x in shards[:-1]]).tolist()
        reqs = RN.reqs_from_batch(ctx, res, offs)
        assert ptr and total == max(int(reqs[s, 5]) + int(reqs[s, 6]) for s in range(len(shards)))   # the ranges may have gaps
        for s in range(len(shards)):
            n = int(res[s].n_ents)
            assert res[s].status == L.OK and n > 0 and int(reqs[s, 6]) == n
            host = (L.EntryDesc * n)()
            assert L.lib.ewal_batch_copy_entries(ctx.handle, s, host, n) == n
            raw = (C.c_char * (n * 40))()
            L.check(L.lib.ewal_download(ctx.handle, raw, C.c_void_p(ptr + int(reqs[s, 5]) * 40), n * 40))
            assert raw.raw == bytes(host)
    finally:
        d.free()


def _wal(seed, with_state=True, n=6):
    """A small WAL by the oracle's encoder: the head, n entries from index 1, a HardState."""
    from oracle import oracle as O
    enc = O.WalEncoder(0)
    enc.save_crc(0)
    enc.encode(1, b"meta")
    for i in range(1, n + 1):
        enc.save_entry(i % 2, seed, i, b"d%d-%d" % (seed, i))
    if with_state:
        enc.save_state(seed, seed + 1, n - 1)
    return enc.getvalue()


def test_reqs_from_batch_field_by_field(ctx):
    """enode_reqs_from_batch over a batch with a good shard, a shard without a
    state record, a shard whose ReadAll fails and another good one: every field
    it owns against res[s], the fields it leaves to the caller untouched, pad
    zeroed, the mismatch and the superseded batch refused."""
    bad = bytearray(_wal(9))
    bad[len(bad) // 2] ^= 0x40
    shards = [_wal(3), _wal(5, with_state=False, n=3), bytes(bad), _wal(7, n=4)]
    blob = b"".join(shards)
    lens = [len(x) for x in shards]
    offs = np.cumsum([0] + lens[:-1]).tolist()
    SENT = 0xA5A5A5A5A5A5A5A5
    d = ctx.alloc(len(blob) + 64)
    try:
        d.upload(blob)
        res = RN.readall_batch_raw(d, lens, [1] * 4)
        assert [res[s].status == L.OK for s in range(4)] == [True, True, False, True]
        assert [int(res[s].has_state) for s in (0, 1, 3)] == [1, 0, 1]
        rows = np.full((4, N.REQ_WORDS), SENT, dtype=np.uint64)
        assert RN.reqs_from_batch(ctx, res, offs, rows) is rows
        ptr, total = RN.entries_device(ctx)
        for s in range(4):
            r, w = res[s], [int(v) for v in rows[s]]
            ok = r.status == L.OK and r.n_unrec == 0
            st = (r.state_term, r.state_vote, r.state_commit) if r.has_state else (0, 0, 0)
            assert w[0] == s and w[1] == (1 if ok else 0), s                 # group, kind
            assert w[2:5] == [SENT] * 3 and w[11] == SENT, s                  # id, ents_first, ents_cap, snap: the caller's
            assert w[7] == offs[s] and tuple(w[8:11]) == st and w[12:16] == [0] * 4, s   # data_delta, hs_*, pad
            if ok:
                assert w[6] == r.n_ents and w[5] + w[6] <= total, s
                host = (L.EntryDesc * w[6])()
                assert L.lib.ewal_batch_copy_entries(ctx.handle, s, host, w[6]) == w[6]
                raw = (C.c_char * (w[6] * 40))()
                L.check(L.lib.ewal_download(ctx.handle, raw, C.c_void_p(ptr + w[5] * 40), w[6] * 40))
                assert raw.raw == bytes(host)
                assert [(e.term, e.index) for e in host] == [((3, 5, 9, 7)[s], i + 1) for i in range(w[6])]
        assert tuple(int(v) for v in rows[0, 8:11]) == (3, 4, 5) and tuple(int(v) for v in rows[1, 8:11]) == (0, 0, 0)
        assert tuple(int(v) for v in rows[3, 8:11]) == (7, 8, 3) and int(rows[2, 1]) == 0
        # n_shards is not the batch's
        keep = rows.copy()
        for n_bad in (3, 5):
            assert L.lib.enode_reqs_from_batch(ctx.handle, C.cast(res, C.c_void_p), n_bad, (C.c_uint64 * 5)(*offs, 0),
                                               rows.ctypes.data_as(C.c_void_p)) == L.E_INVAL
        assert np.array_equal(rows, keep)
        # a single ReadAll supersedes the batch: its ranges are refused, not reported stale
        assert W.readall_device(d, lens[0], 1).status == L.OK
        p, n = C.c_void_p(), C.c_uint64(0)
        assert L.lib.ewal_batch_entries_device(ctx.handle, C.byref(p), C.byref(n)) == L.E_INVAL
        assert L.lib.enode_reqs_from_batch(ctx.handle, C.cast(res, C.c_void_p), 4, (C.c_uint64 * 4)(*offs),
                                           rows.ctypes.data_as(C.c_void_p)) == L.E_INVAL
        assert np.array_equal(rows, keep)
    finally:
        d.free()
