"""GPU parity of the batched log compaction (ecompact_batch_device) with the
restatement in compact_cases.py: bit for bit over every output array, every
group record, d_snaps and all of d_ents (the windows' free slots hold canaries),
then the chains that run on one set of device arrays with nothing forged:
TestNodeCompact, TestSlowNodeRestore with the real compaction, a full window's
room regained, and the compaction's snapshot written as a snap file."""
import ctypes as C

import numpy as np
import pytest

from etcd_amd import _lib as L
from etcd_amd import raftcompact as RC
from etcd_amd import raftlead as R
from etcd_amd import raftprop as P
from etcd_amd import raftready as RD
from etcd_amd import snap as S

import compact_cases as K
import follow_cases as FK
import test_gpu_follow as TF

pytestmark = pytest.mark.gpu

M64 = FK.M64
NAMES = ("res", "groups", "pstate", "rstate", "snaps", "ents", "reqs")
ONE = [(1, 0, 1)]


class Dev:
    """One call's arrays on the device."""

    def __init__(self, ctx, a):
        self.ctx, self.a = ctx, a
        n = len(a["reqs"])
        self.fill_res = np.frombuffer(b"\xa5" * (n * 64), dtype=np.uint64).reshape(n, K.OW)
        self.host = (self.fill_res, a["groups"], a["pstate"], a["rstate"], a["snaps"], a["ents"], a["reqs"])
        self.bufs = [R._up(ctx, h) for h in self.host]

    def call(self, flags=0, **kw):
        nc, nm = C.c_uint64(99), C.c_uint64(99)
        b, a = self.bufs, self.a
        k = dict(G=len(a["groups"]), ne=len(a["ents"]), nd=a["data_len"], nu=a["n_u64"], n=len(a["reqs"]),
                 groups=b[1].ptr, pstate=b[2].ptr, rstate=b[3].ptr, snaps=b[4].ptr, ents=b[5].ptr, reqs=b[6].ptr,
                 res=b[0].ptr)
        k.update(kw)
        rc = L.lib.ecompact_batch_device(self.ctx.handle, k["groups"], k["pstate"], k["rstate"], k["G"], k["snaps"],
                                         k["ents"], k["ne"], k["nd"], k["nu"], k["reqs"], k["n"], k["res"], flags,
                                         C.byref(nc), C.byref(nm))
        return rc, nc.value, nm.value

    def state(self):
        return tuple(np.frombuffer(b.download(h.nbytes), dtype=np.uint64).reshape(h.shape) if h.nbytes else h
                     for b, h in zip(self.bufs, self.host))

    def free(self):
        for b in self.bufs:
            b.free()


def same(got, want):
    for name, g, w in zip(NAMES, got, want):
        if not np.array_equal(g, w):
            at = tuple(int(x) for x in np.argwhere(g != w)[0])
            raise AssertionError("%s differs at %r: got %#x, want %#x" % (name, at, int(g[at]), int(w[at])))


def want_of(a, x, emit=True):
    if emit:
        return (x["res_rows"], x["groups"], x["pstate"], a["rstate"], x["snaps"], x["ents"], a["reqs"])
    return (x["res_rows"], a["groups"], a["pstate"], a["rstate"], a["snaps"], a["ents"], a["reqs"])


def check(ctx, a):
    """The peek fills d_res and the counters, agrees with the real call and
    modifies nothing; the real call equals the restatement.  Returns the
    restatement's dict."""
    assert K.validate(a) == K.OK
    x = K.expected(a)
    counts = (x["n_compacted"], x["n_moved"])
    dv = Dev(ctx, a)
    try:
        assert dv.call(flags=RC.PEEK) == (L.OK,) + counts
        same(dv.state(), want_of(a, x, emit=False))
        assert dv.call() == (L.OK,) + counts
        got = dv.state()
    finally:
        dv.free()
    same(got, want_of(a, x))
    return x


def check_fails(ctx, a, want_rc, **kw):
    """The call fails with want_rc and leaves every array as it was, the counters 0."""
    dv = Dev(ctx, a)
    try:
        before = dv.state()
        got = dv.call(**kw)
        after = dv.state()
    finally:
        dv.free()
    assert got == (want_rc, 0, 0)
    same(after, before)


def acts(x):
    return [(o["status"], o["action"]) for o in x["outcomes"]]


def test_table_compaction(ctx):
    """TestCompaction: the successive compactions 300 / 500 / 800 / 900 as
    successive calls on what the previous call left, the three panics."""
    a, rounds = K.compaction_play()
    for rnd in rounds:
        a = K.after(a, a, [K.req(g, index) for g, index, _ in rnd])
        x = check(ctx, a)
        for (g, _, wleft), o in zip(rnd, x["outcomes"]):
            assert (o["action"] == K.PANICKED) if wleft < 0 else (o["action"], o["n_left"]) == (K.COMPACTED, wleft)
        a = K.after(a, x, [])


def test_table_side_effects_and_compact(ctx):
    a, t = K.side_effects_call()
    x = check(ctx, a)
    o = x["outcomes"][0]
    assert (o["n_left"], o["shift"], o["unstable"], o["cls"]) == (501, 500, 501, K.MOVE_OVERLAP)
    a, rows, _, _ = K.compact_table_call()
    x = check(ctx, a)
    assert acts(x) == [(0, K.COMPACTED), (0, K.COMPACTED), (K.PANIC_COMPACT_APPLIED, K.PANICKED)]


def test_side_effects_ready_sees_the_unstable_tail(ctx):
    """TestCompactionSideEffects through the library: after compact(500) Ready's
    rd.Entries are the 500 entries from Index 501 on, at the window's base + 1."""
    a, t = K.side_effects_call()
    sc_v = np.zeros((1, FK.VW), dtype=np.uint64)
    d = [R._up(ctx, a[k]) for k in ("groups", "pstate", "rstate", "snaps", "ents", "reqs")] + [R._up(ctx, sc_v)]
    d_res, d_rres = ctx.alloc(64 + 64), ctx.alloc(96 + 64)
    try:
        assert RC.compact_batch_device(ctx, d[0], d[1], d[2], 1, d[3], d[4], len(a["ents"]), 0, 0, d[5], 1, d_res) == \
            (1, 501)
        RD.ready_batch_device(ctx, d[0], d[1], d[6], d[2], 1, d[3], d[4], len(a["ents"]), None, 1, d_rres)
        r = RD.results_from(d_rres.download(96), 1)[0]
        assert r["status"] == L.OK and r["flags"] & L.READY_SNAP
        assert (r["ents_first"], r["n_ents"]) == (1, t["wunstable_len"])
        ents = np.frombuffer(d[4].download(a["ents"].nbytes), dtype=np.uint64).reshape(a["ents"].shape)
        assert int(ents[r["ents_first"], 1]) == t["wunstable_first_index"]
        # the append afterwards: a proposal lands right behind the slid log, in the room the compaction gave back
        d += [R._up(ctx, P.pack_locals([dict(group=0, kind="prop", data_nil=1)])), ctx.alloc(48 + 64), ctx.alloc(144 + 64)]
        assert P.local_batch_device(ctx, d[0], d[1], 1, d[3], d[4], len(a["ents"]), 0, d[7], 1, d[8], d[9], 0) == (0, 1)
        r = P.results_from(d[8].download(48), 1)[0]
        assert (r["status"], r["action"]) == (L.OK, L.LEAD_L_APPENDED)
        assert (r["index"], r["ent_pos"]) == (t["wlastIndex_after_append"], 501)
    finally:
        for b in d + [d_res, d_rres]:
            b.free()


def test_provide_snap(ctx):
    """TestProvideSnap with the compaction on the device: a leader compacted at
    the table's index holds a log that starts there and a snapshot with that
    Term; the test forces the peer's next to the offset, as Go's does, and the
    rejected probe makes elead_step_batch_device ship exactly d_snaps[g]."""
    s = K.load_kats()["TestProvideSnap"]
    idx, term = s["snapshot"]["index"], s["snapshot"]["term"]
    sc = FK.Scenario()
    sc.add_group([term] * 3, [(1, idx + 1, idx + 2), (2, 0, idx + 2)], term=term, log_offset=idx - 1, committed=idx + 1,
                 applied=idx + 1, state=FK.LEADER)
    a = K.call_of(sc, [K.req(0, idx, nodes=(0, len(s["snapshot"]["nodes"])))], 0, 2)
    a["ents"][a["ents"] == np.uint64(FK.CANARY)] = 0
    x = K.expected(a)
    d = [R._up(ctx, a[k]) for k in ("groups", "pstate", "rstate", "snaps", "ents", "reqs")]
    d += [ctx.alloc(64 + 64), ctx.alloc(48 + 64), ctx.alloc(144 + 64)]
    try:
        assert RC.compact_batch_device(ctx, d[0], d[1], d[2], 1, d[3], d[4], len(a["ents"]), 0, 2, d[5], 1, d[6]) == (1, 2)
        g = np.frombuffer(d[0].download(a["groups"].nbytes), dtype=np.uint64).reshape(a["groups"].shape).copy()
        assert np.array_equal(g, x["groups"]) and int(g[0, 3]) == idx
        g[0, 22] = g[0, 3]                                   # sm.prs[2].next = sm.raftLog.offset
        d[0].upload(g.tobytes())
        d.append(R._up(ctx, R.pack_resps([dict(group=0, from_=2, index=idx - 1, reject=True)])))
        args = (ctx, d[0], 1, d[3], d[4], len(a["ents"]), d[9], 1, d[7])
        assert R.lead_step_batch_device(*args)[0] == 1
        assert R.lead_step_batch_device(*args, d[8], 1)[0] == 1
        m = np.frombuffer(d[8].download(144), dtype=np.uint64)
        assert int(m[0]) == s["wtype"] and [int(v) for v in m[9:17]] == [idx, term, 0, 0, 0, 2, 0, 0]
        assert np.array_equal(m[9:17], x["snaps"][0])
    finally:
        for b in d:
            b.free()


def test_random(ctx):
    a = K.random_scenario(11, 5000, 4000, idle_every=9)
    x = check(ctx, a)
    n_acts, stats, cls = K.mix_of(x["outcomes"])
    assert all(v >= 4000 * 0.02 for v in n_acts[1:] + stats), (n_acts, stats)
    assert all(c >= n_acts[K.COMPACTED] * 0.10 for c in cls), cls


def shape_group(sc, n_left, shift, room=1, salt=0):
    """A group that keeps n_left entries and drops shift: every entry distinct."""
    nlog = n_left + shift
    log = [FK.entry(2 + (k + salt) % 5, 500 + k, 7 * k, k % 11, k % 2, 0) for k in range(nlog)]
    g = sc.add_group(log, ONE, log_offset=500, committed=500 + nlog - 1, applied=500 + nlog - 1, room=room)
    return g, K.req(g, 500 + shift, data=(g % 50, 3), nodes=(g % 4, 2))


def test_move_shapes(ctx):
    """n_left x shift on both sides of the overlap boundary, the requests
    lying across the descriptors' workgroup seam (request 256)."""
    sc, reqs = FK.Scenario(), []
    for k in range(230):
        reqs.append(shape_group(sc, 1, k % 3, salt=k)[1])
    for n_left in (1, 2, 63, 64, 65, 255, 256, 257, 513):
        for shift in (0, 1, n_left - 1, n_left, n_left + 1, 1000):
            reqs.append(shape_group(sc, n_left, shift, salt=n_left + shift)[1])
    assert len(reqs) > 256
    x = check(ctx, K.call_of(sc, reqs, 100, 8))
    assert all(a == (0, K.COMPACTED) for a in acts(x))
    assert all(c > 10 for c in K.mix_of(x["outcomes"])[2])


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_requests_across_wave_and_workgroup_seams(ctx, n):
    a = K.random_scenario(100 + n, n + 3, n)
    check(ctx, a)


def test_n_is_one_and_zero(ctx):
    sc = FK.Scenario()
    _, q = shape_group(sc, 3, 2)
    a = K.call_of(sc, [q], 100, 8)
    x = check(ctx, a)
    assert acts(x) == [(0, K.COMPACTED)] and x["n_moved"] == 3
    dv = Dev(ctx, a)
    try:
        before = dv.state()
        assert dv.call(n=0) == (L.OK, 0, 0)
        same(dv.state(), before)
    finally:
        dv.free()


def test_one_long_group_next_to_one_entry_groups(ctx):
    """One group keeps 4 097 entries with shift 1 (overlapping: 17 workgroups
    of the move pass for one descriptor) next to 1 000 one-entry groups; the last
    window ends exactly at n_ents_total."""
    sc, reqs = FK.Scenario(), []
    for k in range(500):
        reqs.append(shape_group(sc, 1, 1, salt=k)[1])
    reqs.append(shape_group(sc, 4097, 1)[1])
    for k in range(499):
        reqs.append(shape_group(sc, 1, 1, salt=k)[1])
    reqs.append(shape_group(sc, 1, 1, room=0)[1])
    a = K.call_of(sc, reqs, 100, 8)
    g = a["groups"][-1]
    assert int(g[5]) + int(a["pstate"][-1][0]) == len(a["ents"])
    x = check(ctx, a)
    assert x["n_moved"] == 4097 + 1000 and K.mix_of(x["outcomes"])[2] == [0, 1000, 1]


def test_single_class_calls_and_a_smaller_second_call(ctx):
    """Only the disjoint class, only the overlapping class, then a smaller
    overlapping call on the same ctx: the staging buffer is reused and nothing
    stale of the larger call reaches a window."""
    for shapes, want in (([(3, 3), (2, 9), (1, 1)] * 40, [0, 120, 0]), ([(300, 7), (9, 8), (2, 1)] * 40, [0, 0, 120]),
                         ([(5, 2), (2, 1)], [0, 0, 2])):
        sc, reqs = FK.Scenario(), []
        for k, (n_left, shift) in enumerate(shapes):
            reqs.append(shape_group(sc, n_left, shift, salt=k)[1])
        x = check(ctx, K.call_of(sc, reqs, 100, 8))
        assert K.mix_of(x["outcomes"])[2] == want


def test_a_panicking_group_between_two_compacting_ones(ctx):
    sc = FK.Scenario()
    _, q0 = shape_group(sc, 5, 3)
    g1 = sc.add_group([1] * 6, ONE, log_offset=10, committed=15, applied=12, room=2)
    _, q2 = shape_group(sc, 2, 7, salt=1)
    x = check(ctx, K.call_of(sc, [q0, K.req(g1, 13, data=(1, 1)), q2], 100, 8))
    assert acts(x) == [(0, K.COMPACTED), (K.PANIC_COMPACT_APPLIED, K.PANICKED), (0, K.COMPACTED)]


def _inval_cases():
    def word(name, row, col, val):
        def f(a):
            a[name][row, col] = np.uint64(val & M64)
        return f
    return [("group >= G", word("reqs", 0, 0, 3)), ("a group named twice", word("reqs", 1, 0, 0)),
            ("flags bit 1", word("reqs", 0, 1, 2)), ("flags bit 63", word("reqs", 1, 1, 1 << 63)),
            ("pad0", word("reqs", 0, 10, 1)), ("pad1", word("reqs", 1, 11, 1)),
            ("AT_APPLIED with an index", word("reqs", 0, 1, 1)), ("Data outside", word("reqs", 0, 5, 91)),
            ("Data wraps", word("reqs", 0, 4, M64)), ("Nodes outside", word("reqs", 0, 7, 9)),
            ("Nodes wrap", word("reqs", 0, 6, M64 - 3)), ("Removed outside", word("reqs", 0, 8, 11)),
            ("Removed wrap", word("reqs", 1, 9, M64)), ("group reserved", word("groups", 0, 31, 1)),
            ("state reserved", word("pstate", 2, 3, 1)), ("pending_conf > 1", word("pstate", 2, 2, 2)),
            ("nlog > ents_cap", word("groups", 2, 4, 99)), ("the window wraps", word("groups", 2, 5, M64)),
            ("the window ends outside", word("pstate", 2, 0, 1 << 40)), ("two equal peer ids", word("groups", 0, 8, 1))]


def test_whole_call_failures(ctx):
    """Every EWAL_E_INVAL class, on the device and on the host: every array is
    as it was and the counters are 0."""
    def call():
        sc = FK.Scenario()
        for _ in range(3):
            sc.add_group([1, 1, 1], [(1, 0, 1), (2, 0, 1)], committed=2, applied=2)
        return K.call_of(sc, [K.req(0, 1, data=(10, 90), nodes=(2, 8), removed=(10, 0)), K.req(2, 2)], 100, 10)
    check(ctx, call())
    for name, edit in _inval_cases():
        a = call()
        edit(a)
        assert K.validate(a) == K.E_INVAL, name
        check_fails(ctx, a, L.E_INVAL)
    a = call()
    check_fails(ctx, a, L.E_INVAL, groups=None)
    check_fails(ctx, a, L.E_INVAL, rstate=None)
    check_fails(ctx, a, L.E_INVAL, snaps=None)
    check_fails(ctx, a, L.E_INVAL, res=None)
    check_fails(ctx, a, L.E_INVAL, reqs=None)
    check_fails(ctx, a, L.E_INVAL, ents=None)
    check_fails(ctx, a, L.E_INVAL, n=0x7fffffff)
    check_fails(ctx, a, L.E_INVAL, G=0x7fffffff)
    dv = Dev(ctx, a)
    try:
        before = dv.state()
        assert dv.call(flags=2) == (L.E_INVAL, 0, 0) and dv.call(flags=3) == (L.E_INVAL, 0, 0)
        assert dv.call(groups=dv.bufs[1].ptr.value + 8) == (L.E_INVAL, 0, 0)
        assert dv.call(ents=dv.bufs[5].ptr.value + 4) == (L.E_INVAL, 0, 0)
        same(dv.state(), before)
    finally:
        dv.free()


def test_host_convenience_and_repeat_calls(ctx):
    a = K.random_scenario(5, 40, 30)
    x = K.expected(a)
    for _ in range(2):
        out = RC.compact_batch(ctx, a["groups"], a["pstate"], a["rstate"], a["snaps"], a["ents"], a["reqs"],
                               a["data_len"], a["n_u64"])
        assert (out["n_compacted"], out["n_moved"]) == (x["n_compacted"], x["n_moved"])
        for k in ("res_rows", "groups", "pstate", "snaps", "ents"):
            assert np.array_equal(out[k], x[k]), k
        assert [(r["status"], r["action"]) for r in out["res"]] == acts(x)
    out = RC.compact_batch(ctx, a["groups"], a["pstate"], a["rstate"], a["snaps"], a["ents"], a["reqs"], a["data_len"],
                           a["n_u64"], peek=True)
    assert np.array_equal(out["res_rows"], x["res_rows"]) and np.array_equal(out["ents"], a["ents"])


# ---- chains on one set of device arrays ---------------------------------------------------

def ready_all(cl, accept=True):
    """eready_batch_device over every group; returns the results."""
    G = cl.G
    d_res = cl.alloc(G * 96)
    rargs = (cl.ctx, cl.d["groups"], cl.d["pstate"], cl.d["vstate"], cl.d["rstate"], G, cl.d["snaps"], cl.d["ents"],
             cl.ne, None, G, d_res)
    n_save, _ = RD.ready_batch_device(*rargs)
    if accept:
        d_save = cl.alloc((n_save + 1) * 56)
        RD.ready_batch_device(*rargs, d_save, n_save)
    return RD.results_from(d_res.download(G * 96), G)


def compact(cl, reqs, n_u64=0, peek=False):
    """ecompact_batch_device on the cluster's arrays, checked against the restatement; returns its dict."""
    a = dict(cl.arrays(), reqs=np.array(reqs, dtype=np.uint64).reshape(-1, K.QW), data_len=len(cl.data), n_u64=n_u64)
    assert K.validate(a) == K.OK
    x = K.expected(a)
    n = len(reqs)
    d_in, d_res = cl.up(a["reqs"]), cl.alloc(n * 64)
    got = RC.compact_batch_device(cl.ctx, cl.d["groups"], cl.d["pstate"], cl.d["rstate"], cl.G, cl.d["snaps"],
                                  cl.d["ents"], cl.ne, len(cl.data), n_u64, d_in, n, d_res, RC.PEEK if peek else 0)
    assert got == (x["n_compacted"], x["n_moved"])
    assert np.array_equal(np.frombuffer(d_res.download(n * 64), dtype=np.uint64).reshape(n, K.OW), x["res_rows"])
    after = cl.arrays()
    for k in ("groups", "pstate", "rstate", "snaps", "ents"):
        assert np.array_equal(after[k], a[k] if peek else x[k]), k
    return x


def test_node_compact_chain(ctx):
    """TestNodeCompact on the device: Campaign, Propose("foo"), Ready; Compact(2,
    [1], "a snapshot"); the next Ready carries exactly that snapshot, the one
    after it has no update; log_offset is 2."""
    t = K.load_kats()["TestNodeCompact"]
    w = t["snapshot"]
    cl = TF.Cluster(ctx, 1, 1)
    try:
        cl.vote([dict(group=0, kind="hup", from_=1)])
        assert int(cl.get("vstate")[0, 0]) == FK.LEADER
        cl.propose([0], [t["proposal"].encode()])
        r = ready_all(cl)[0]
        assert r["status"] == L.OK and r["flags"] & L.READY_UPDATES and r["commit"] == 2 and not r["flags"] & L.READY_SNAP
        data = w["data"].encode()
        off = len(cl.data)
        cl.data += data
        cl.d["data"].free()
        cl.d["data"] = R._up(ctx, np.frombuffer(cl.data + b"\0" * (-len(cl.data) % 8 + 8), dtype=np.uint64))
        x = compact(cl, [K.req(0, w["index"], data=(off, len(data)), nodes=(0, len(w["nodes"])))], n_u64=1)
        assert acts(x) == [(0, K.COMPACTED)]
        snap = [w["index"], w["term"], off, len(data), 0, 1, 0, 0]
        assert [int(v) for v in cl.get("snaps")[0]] == snap
        r = ready_all(cl)[0]
        assert r["status"] == L.OK and r["flags"] & L.READY_SNAP and r["flags"] & L.READY_UPDATES
        assert cl.data[snap[2]:snap[2] + snap[3]] == data and int(cl.get("rstate")[0, 5]) == w["index"]
        r = ready_all(cl)[0]
        assert r["status"] == L.OK and r["flags"] == 0
        assert int(cl.get("groups")[0, 3]) == t["woffset"]
    finally:
        cl.free()


class RoomyCluster(TF.Cluster):
    """TF.Cluster's empty cluster with the windows the forged restore play has:
    11 slots for the nodes that will hold the leader's log, 9 for the slow one."""

    def __init__(self, ctx, nodes, clusters, slow):
        self.ctx, self.nodes, self.G = ctx, nodes, nodes * clusters
        sc = FK.Scenario()
        for c in range(clusters):
            for id_ in range(1, nodes + 1):
                sc.add_group([0], [(p, 0, 1) for p in range(1, nodes + 1)], gid=id_, term=0,
                             room=8 if id_ == slow else 10)
        a = sc.pack()
        a["ents"][a["ents"] == np.uint64(FK.CANARY)] = 0
        self.shape = {k: a[k].shape for k in ("groups", "pstate", "vstate", "rstate", "snaps", "ents")}
        self.ne = len(a["ents"])
        self.data = b""
        self.d = {k: R._up(ctx, a[k]) for k in self.shape}
        self.d["data"] = R._up(ctx, np.zeros(1, dtype=np.uint64))
        self.extra = []

    def propose_nil(self, leaders, k):
        """k proposals with nil Data per leader; returns the LAST msgApp per (leader, peer) -- it carries every
        entry from Progress.next on; the earlier ones are lost, as the network may -- and the msgSnap rows."""
        locs = [dict(group=g, kind="prop", data_nil=1) for g in leaders for _ in range(k)]
        d_loc, d_res = self.up(P.pack_locals(locs)), self.alloc(len(locs) * 48)
        args = (self.ctx, self.d["groups"], self.d["pstate"], self.G, self.d["snaps"], self.d["ents"], self.ne,
                len(self.data), d_loc, len(locs), d_res)
        total, napp = P.local_batch_device(*args)
        assert napp == len(locs)
        d_out = self.alloc(total * 144)
        P.local_batch_device(*args, d_out, total)
        res = P.results_from(d_res.download(len(locs) * 48), len(locs))
        assert all(r["status"] == L.OK for r in res)
        rows = np.frombuffer(d_out.download(total * 144), dtype=np.uint64).reshape(total, FK.MW).copy()
        senders = [m["group"] for m, r in zip(locs, res) for _ in range(r["n_msgs"])]
        last = {}
        for i, (r, s) in enumerate(zip(rows, senders)):
            last[(s, int(r[1]))] = i
        keep = sorted(last.values())
        return rows[keep], [senders[i] for i in keep]


def without(rows, senders, to):
    keep = [i for i, r in enumerate(rows) if int(r[1]) != to]
    return rows[keep], [senders[i] for i in keep]


@pytest.mark.parametrize("nodes", [3, 5])
def test_slow_node_restore_chain_with_the_real_compaction(ctx, nodes):
    """TestSlowNodeRestore with nothing forged: the election, 101 proposals in
    rounds (append, replicate to the nodes that are not isolated, commit, Ready,
    compact at applied so the 11-slot windows never fill), the last compaction at
    100 under applied == 102; the leader's records then equal the state
    test_gpu_follow.py forges for this play.  Then the play itself, as Go runs it:
    the network recovers, one proposal makes the leader ship its snapshot (the
    slow node's Progress.next is below the offset), the follower step restores
    from it, the next proposal is appended and committed everywhere."""
    clusters, slow = 3, nodes
    cl = RoomyCluster(ctx, nodes, clusters, slow)
    try:
        leaders = [c * nodes for c in range(clusters)]
        live = [g for g in range(cl.G) if g % nodes != slow - 1]

        def replicate(rows, senders):
            rows, senders = without(rows, senders, slow)
            x, _ = cl.follow(rows, senders)
            assert all(a == (0, FK.APPENDED) for a in TF.acts(x))
            _, rows, senders, _ = cl.lead_step(x)
            rows, senders = without(rows, senders, slow)
            if len(rows):
                cl.follow(rows, senders)
            res = ready_all(cl)
            assert all(res[g]["status"] == L.OK for g in live)

        rows, senders = cl.elect(leaders)
        replicate(rows, senders)
        for rnd in range(26):                                # 4 a round: a re-sent suffix still fits the window
            rows, senders = cl.propose_nil(leaders, 4 if rnd < 25 else 1)
            replicate(rows, senders)
            if rnd < 24:                                     # shouldCompact with a threshold of 3, at applied
                x = compact(cl, [K.req(g, at_applied=True, threshold=3, nodes=(0, nodes)) for g in live], n_u64=nodes)
                assert all(a == (0, K.COMPACTED) for a in acts(x)), rnd
        g = cl.get("groups")
        assert all([int(v) for v in g[k, 2:5]] == [102, 97, 6] for k in live)
        assert int(cl.get("rstate")[leaders[0], 6]) == 102   # applied
        # a peek at a threshold nobody reaches, then the compaction at 100
        x = compact(cl, [K.req(k, at_applied=True, threshold=K.DEFAULT_COMPACT_THRESHOLD) for k in live], peek=True)
        assert all(a == (0, K.NOT_DUE) for a in acts(x))
        x = compact(cl, [K.req(k, 100, nodes=(0, nodes)) for k in live], n_u64=nodes)
        assert all((o["n_left"], o["shift"], o["term"], o["cls"]) == (3, 3, 1, K.MOVE_DISJOINT) for o in x["outcomes"])
        # the forged state of test_gpu_follow.py::test_slow_node_restore_chain, with its progress edits
        snap = [100, 1, 0, 0, 0, nodes, 0, 0]
        forged = TF.Cluster(ctx, nodes, clusters, leader_log=[1, 1, 1], offset=100, snaps=snap, slow=slow)
        try:
            f = forged.arrays()
        finally:
            forged.free()
        real = cl.arrays()
        for ld in leaders:
            for p in range(1, nodes):
                f["groups"][ld, 14 + p], f["groups"][ld, 21 + p] = (102, 103) if p + 1 != slow else (0, 101)
            # the forged play probes the slow node at 100 by hand; the real leader never heard from it: next is 1
            assert int(real["groups"][ld, 21 + slow - 1]) == 1
            f["groups"][ld, 21 + slow - 1] = 1
            assert np.array_equal(real["groups"][ld], f["groups"][ld])
            assert np.array_equal(real["pstate"][ld], f["pstate"][ld])
            assert np.array_equal(real["snaps"][ld], f["snaps"][ld])
            first = int(real["groups"][ld, 5])
            assert np.array_equal(real["ents"][first:first + 3], f["ents"][first:first + 3])
            # Ready's own words: the compaction left them alone, the next Ready reports the snapshot
            assert [int(v) for v in real["rstate"][ld, 5:7]] == [97, 102]
        res = ready_all(cl)
        assert all(res[k]["flags"] & L.READY_SNAP for k in live)
        assert all(int(v) == 100 for v in cl.get("rstate")[live, 5])
        # nt.recover(); "trigger a snapshot"
        u64 = np.arange(1, nodes + 1, dtype=np.uint64)
        rows, senders = cl.propose_nil(leaders, 1)
        to_slow = [r for r in rows if int(r[1]) == slow]
        assert len(to_slow) == clusters and all(int(r[0]) == 7 and [int(v) for v in r[9:17]] == snap for r in to_slow)
        x, stepped = cl.follow(rows, senders, u64=u64)
        outs = dict(zip(stepped, TF.acts(x)))
        assert all(outs[ld + slow - 1] == (0, FK.RESTORED) for ld in leaders)
        sn, g = cl.get("snaps"), cl.get("groups")
        for ld in leaders:
            fo = ld + slow - 1
            assert np.array_equal(sn[fo], sn[ld])                                   # follower.snap == lead.snap
            assert [int(v) for v in g[fo][2:5]] == [100, 100, 1] and int(g[fo][6]) == nodes
        res, rows, senders, _ = cl.lead_step(x)
        if len(rows):
            cl.follow(rows, senders, u64=u64)
        # "trigger a commit"
        rows, senders = cl.propose_nil(leaders, 1)
        x, stepped = cl.follow(rows, senders, u64=u64)
        slow_outs = [o for o, s in zip(x["outcomes"], stepped) if s % nodes == slow - 1]
        assert all((o["status"], o["action"]) == (0, FK.APPENDED) and o["last_index"] == 104 for o in slow_outs)
        res, rows, senders, _ = cl.lead_step(x)
        cl.follow(rows, senders, u64=u64)
        g = cl.get("groups")
        for ld in leaders:
            assert int(g[ld + slow - 1, 2]) == int(g[ld, 2]) == 104                  # committed
    finally:
        cl.free()


def test_room_regained(ctx):
    """A leader whose window is full gets EWAL_E_NOMEM from
    elead_local_batch_device; after compacting at applied the same proposals
    succeed."""
    sc = FK.Scenario()
    for k in range(3):
        sc.add_group([1] * 6, [(1, 5, 6)], term=1, committed=5, applied=5, room=0, state=FK.LEADER)
    a = sc.pack()
    a["ents"][a["ents"] == np.uint64(FK.CANARY)] = 0
    G, ne = 3, len(a["ents"])
    d = {k: R._up(ctx, a[k]) for k in ("groups", "pstate", "rstate", "snaps", "ents")}
    locs = P.pack_locals([dict(group=g, kind="prop", data_nil=1) for g in range(G) for _ in range(2)])
    d_loc, d_lres = R._up(ctx, locs), ctx.alloc(len(locs) * 48 + 64)
    reqs = np.array([K.req(g, at_applied=True, threshold=0) for g in range(G)], dtype=np.uint64)
    d_req, d_res = R._up(ctx, reqs), ctx.alloc(G * 64 + 64)
    try:
        largs = (ctx.handle, d["groups"].ptr, d["pstate"].ptr, G, d["snaps"].ptr, d["ents"].ptr, ne, 0, d_loc.ptr,
                 len(locs), d_lres.ptr, None, 0)
        nm, na = C.c_uint64(9), C.c_uint64(9)
        assert L.lib.elead_local_batch_device(*largs, C.byref(nm), C.byref(na)) == L.E_NOMEM
        assert RC.compact_batch_device(ctx, d["groups"], d["pstate"], d["rstate"], G, d["snaps"], d["ents"], ne, 0, 0,
                                       d_req, G, d_res) == (3, 3)
        assert L.lib.elead_local_batch_device(*largs, C.byref(nm), C.byref(na)) == L.OK and na.value == 6
        d_out = ctx.alloc(max(nm.value, 1) * 144 + 64)
        try:
            assert P.local_batch_device(ctx, d["groups"], d["pstate"], G, d["snaps"], d["ents"], ne, 0, d_loc, len(locs),
                                        d_lres, d_out, nm.value) == (nm.value, 6)
        finally:
            d_out.free()
        g = np.frombuffer(d["groups"].download(a["groups"].nbytes), dtype=np.uint64).reshape(a["groups"].shape)
        assert all([int(v) for v in g[k, 3:5]] == [5, 3] for k in range(G))
        res = P.results_from(d_lres.download(len(locs) * 48), len(locs))
        assert [r["index"] for r in res] == [6, 7] * G and all(r["action"] == L.LEAD_L_APPENDED for r in res)
    finally:
        for b in list(d.values()) + [d_loc, d_lres, d_req, d_res]:
            b.free()


def test_compact_to_file(ctx):
    """The compaction's d_snaps rows through snap_save_recs into
    esnap_save_packed_device; esnap_verify_packed and esnap_copy_snapshot give
    back the same index, term, nodes, removed and Data."""
    a, rows, data, u64 = K.compact_table_call()
    x = K.expected(a)
    d = {k: R._up(ctx, a[k]) for k in ("groups", "pstate", "rstate", "snaps", "ents", "reqs")}
    pad = data + b"\0" * (-len(data) % 16 + 16)
    d_data, d_res, d_out = R._up(ctx, np.frombuffer(pad, dtype=np.uint64)), ctx.alloc(3 * 64 + 64), ctx.alloc(4096)
    try:
        assert RC.compact_batch_device(ctx, d["groups"], d["pstate"], d["rstate"], 3, d["snaps"], d["ents"],
                                       len(a["ents"]), len(data), len(u64), d["reqs"], 3, d_res) == (2, x["n_moved"])
        snaps = np.frombuffer(d["snaps"].download(a["snaps"].nbytes), dtype=np.uint64).reshape(a["snaps"].shape)
        assert np.array_equal(snaps, x["snaps"])
        done = [g for g, r in enumerate(RC.results_from(d_res.download(3 * 64), 3)) if r["action"] == L.COMPACT_COMPACTED]
        assert done == [0, 1]
        recs = RC.snap_save_recs(snaps, done)
        h_u64 = (C.c_uint64 * len(u64))(*u64)
        out = (L.SnapSaved * len(done))()
        L.check(L.lib.esnap_save_packed_device(ctx.handle, d_data.ptr, len(data), recs, len(done), h_u64, b"",
                                               L.CASTAGNOLI, d_out.ptr, 4096, out))
        offs, lens = [o.off for o in out], [o.len for o in out]
        st, stored, computed = S.verify_packed(d_out, 4096, offs, lens)
        assert st == [L.OK] * 2 and stored == computed == [o.crc for o in out]
        for i, g in enumerate(done):
            s = S.snapshot(ctx, i)
            row = rows[g]
            assert (s["index"], s["term"]) == (row["compacti"], 1)
            assert s["nodes"] == row["nodes"] and s["removed"] == row["removed"] and s["data"] == row["snapd"].encode()
    finally:
        for b in list(d.values()) + [d_data, d_res, d_out]:
            b.free()
