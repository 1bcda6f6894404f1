"""GPU parity of the batched leader msgProp / msgBeat step
(elead_local_batch_device) with the restatement of stepLeader's msgProp and
msgBeat cases in lead_prop_cases.py (raft/raft.go:441-455 and what they call).
Every call compares d_res, the complete d_groups, d_state and d_ents arrays and
the complete d_msgs array byte for byte; d_res starts as 0xA5 bytes, d_msgs and
the free slots of d_ents as a canary in every word (d_msgs SLACK records longer
than the call may fill), so a failing call must leave all five as they were
and a successful one the canary after its last message and entry."""
import collections
import ctypes as C

import numpy as np
import pytest

from etcd_amd import _lib as L
from etcd_amd import raftlead as R
from etcd_amd import raftlog as RL
from etcd_amd import raftmsg as M
from etcd_amd import raftprop as P
from etcd_amd import wal as W

import lead_prop_cases as K
import lead_step_cases as KL
import log_append_cases as KA

pytestmark = pytest.mark.gpu

U64 = K.M64
SLACK = 3
NAMES = ("d_res", "d_groups", "d_state", "d_ents", "d_msgs")


class Dev:
    """One call's arrays on the device."""

    def __init__(self, ctx, arrays, cap, data_len_total=1 << 20):
        self.ctx = ctx
        self.grows, self.strows, self.srows, self.erows, self.lrows = arrays
        self.G, self.ne, self.n, self.cap = len(self.grows), len(self.erows), len(self.lrows), cap
        self.dl = data_len_total
        self.fill_res = np.frombuffer(b"\xa5" * (self.n * 48), dtype=np.uint64).reshape(self.n, P.RESULT_WORDS)
        self.fill_msgs = np.full((cap + SLACK, R.MSG_WORDS), K.CANARY, dtype=np.uint64)
        self.bufs = [R._up(ctx, a) if a is not None else None
                     for a in (self.grows, self.strows, self.srows, self.erows, self.lrows, self.fill_res,
                               self.fill_msgs)]

    def call(self, G=None, n=None, ne=None, cap=None, msgs=True, snaps=True, dl=None):
        nm, na = C.c_uint64(99), C.c_uint64(99)
        b = self.bufs
        rc = L.lib.elead_local_batch_device(self.ctx.handle, b[0].ptr, b[1].ptr, self.G if G is None else G,
                                            b[2].ptr if snaps and b[2] else None, b[3].ptr,
                                            self.ne if ne is None else ne, self.dl if dl is None else dl, b[4].ptr,
                                            self.n if n is None else n, b[5].ptr, b[6].ptr if msgs else None,
                                            self.cap if cap is None else cap, C.byref(nm), C.byref(na))
        return rc, nm.value, na.value

    def state(self):
        b = self.bufs

        def get(buf, like):
            return np.frombuffer(buf.download(like.nbytes), dtype=np.uint64).reshape(like.shape) if like.nbytes else like
        return (get(b[5], self.fill_res), get(b[0], self.grows), get(b[1], self.strows), get(b[3], self.erows),
                get(b[6], self.fill_msgs))

    def free(self):
        for b in self.bufs:
            if b is not None:
                b.free()


def same(got, want):
    for name, g, w in zip(NAMES, got, want):
        if not np.array_equal(g, w):
            at = tuple(int(x) for x in np.argwhere(g != w)[0])
            raise AssertionError("%s differs at %r: got %#x, want %#x" % (name, at, int(g[at]), int(w[at])))


def want_of(sc):
    """expected() with the message array as the device holds it: the canary after the last message."""
    res, grows, strows, erows, msgs = sc.expected()
    full = np.full((len(msgs) + SLACK, R.MSG_WORDS), K.CANARY, dtype=np.uint64)
    full[:len(msgs)] = msgs
    return res, grows, strows, erows, full


def check(ctx, sc, snaps=True):
    """The call on sc with msgs_cap == the exact total equals the restatement; returns the outcomes."""
    want = want_of(sc)
    dv = Dev(ctx, sc.pack(), sc.n_msgs, sc.data_len_total)
    try:
        rc, nm, na = dv.call(snaps=snaps)
        got = dv.state()
    finally:
        dv.free()
    assert rc == L.OK
    same(got, want)
    assert (nm, na) == (sc.n_msgs, sc.n_appended)
    return sc.outcomes


def check_fails(ctx, arrays, want_rc, cap=8192, **kw):
    """The call fails with want_rc and leaves all five arrays as they were."""
    dv = Dev(ctx, arrays, 8192)
    try:
        before = dv.state()
        rc, nm, na = dv.call(cap=cap, **kw)
        after = dv.state()
    finally:
        dv.free()
    assert (rc, nm, na) == (want_rc, 0, 0)
    same(after, before)


def test_kats(ctx):
    sc, named = K.kat_scenario()
    outs = check(ctx, sc)
    K.check_kats(sc, named)
    assert len(outs) == 8 and [o["action"] for o in outs[:3]] == [K.APPENDED, K.APPENDED, K.DROPPED]


def test_kats_between_idle_groups(ctx):
    sc, named = K.kat_scenario(idle=50)
    assert len(sc.groups) == 56 and len(sc.locals) == 8
    check(ctx, sc)


def test_lattice(ctx):
    sc = K.lattice_scenario()
    outs = check(ctx, sc)
    acts = collections.Counter(o["action"] for o in outs)
    stats = collections.Counter(o["status"] for o in outs)
    assert len(sc.groups) == 292 and all(acts[a] for a in range(5)), acts
    assert all(stats[s] for s in (K.PANIC_NIL_PROGRESS, K.PANIC_NEED_SNAPSHOT, K.PANIC_FIRST_ENTRY, K.UNSUPPORTED)), stats
    # the whole call again without d_snaps: every needSnapshot panics
    sc2 = K.lattice_scenario()
    sc2.with_snaps = False
    outs2 = check(ctx, sc2)
    assert sum(o["status"] == K.PANIC_NEED_SNAPSHOT for o in outs2) > stats[K.PANIC_NEED_SNAPSHOT]


def test_edges(ctx):
    """The nil-slice appends, a wrapped lastIndex, update(2^64 - 1), term 0, an empty log."""
    sc = K.Scenario()
    off = U64 - 1
    sc.add_run(sc.add_group([], [(1, 0, 1), (2, 0, 6)], gid=1, term=3, log_offset=5, unstable=9), "PBP")
    sc.add_run(sc.add_group([], [(1, 0, 1), (2, 0, 1)], gid=1, term=3), "PP")
    sc.add_run(sc.add_group([1, 1, 1], [(1, 0, 1), (2, 0, U64)], gid=1, term=3, log_offset=off, unstable=U64), "PPCB")
    sc.add_run(sc.add_group([1], [(1, 0, 1)], gid=1, term=3, log_offset=off, room=3), "PPP")
    sc.add_run(sc.add_group([0, 0], [(1, 1, 2), (2, 1, 2), (3, 0, 9)], gid=1, term=0, committed=0), "PCP")
    sc.add_run(sc.add_group([0, 1, 1], [(1, 2, 3), (2, 0, 3), (3, 0, 0)], gid=1, term=1, unstable=7), "BCP")
    sc.add_run(sc.add_group([1, 1], [(1, 1, 2), (2, 0, 3)], gid=1, term=4), "PP")
    outs = check(ctx, sc)
    assert [o["index"] for o in outs[:5]] == [5, 0, 6, 0, 1]
    assert [(o["status"], o["action"]) for o in outs[-5:-2]] == [(0, K.BEAT), (K.PANIC_FIRST_ENTRY, K.PANICKED),
                                                                  (0, K.NOT_STEPPED)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_boundary_shapes(ctx, n):
    sc = K.boundary_scenario(n)
    check(ctx, sc)
    assert len(sc.locals) == n
    if n == 1025:
        # message totals on both sides of the same seams: cut the call after each prefix
        firsts = [o["msg_first"] for o in sc.outcomes]
        for seam in (64, 256, 1024):
            below = max(k for k, f in enumerate(firsts) if f < seam)
            above = min(k for k, f in enumerate(firsts) if f > seam)
            totals = []
            for k in sorted({below, above} | {k for k, f in enumerate(firsts) if f == seam}):
                cut = K.Scenario()
                cut.groups, cut.logs, cut.snaps, cut.state, cut.locals = sc.groups, sc.logs, sc.snaps, sc.state, \
                    sc.locals[:k]
                check(ctx, cut)
                totals.append(cut.n_msgs)
            assert totals[0] < seam < totals[-1] and totals[-1] - totals[0] <= 4, (seam, totals)


def test_long_runs(ctx):
    """A run of 300 (longer than a workgroup) and one of 70 that starts at lane 60."""
    sc = K.long_scenario([300])
    outs = check(ctx, sc)
    assert sum(o["action"] == K.APPENDED for o in outs) > 200 and sum(o["action"] == K.DROPPED for o in outs) > 10
    sc = K.long_scenario([70, 300, 70], lead_in=60)
    check(ctx, sc)
    assert [i for _, i in sc.runs[60:]] == [60, 130, 430]


def test_many_workgroups(ctx):
    """256 * 256 + 300 records: each thread of the two scans owns more than one workgroup, and the last run
    crosses a workgroup seam."""
    sc = K.wide_scenario(256 * 256, 300)
    outs = check(ctx, sc)
    assert len(outs) == 256 * 256 + 300 and outs[-1]["index"] == 2 + 300


@pytest.mark.parametrize("seed", [1, 2])
def test_random(ctx, seed):
    sc = K.random_scenario(seed)
    outs = check(ctx, sc)
    acts = collections.Counter(o["action"] for o in outs)
    assert all(acts[a] >= 300 for a in (K.BEAT, K.APPENDED, K.DROPPED)) and acts[K.PANICKED] >= 30, acts


def test_size_query(ctx):
    sc = K.random_scenario(3, G=800, n=1500)
    want = want_of(sc)
    dv = Dev(ctx, sc.pack(), sc.n_msgs)
    try:
        before = dv.state()
        rc, nm, na = dv.call(msgs=False, cap=0)
        after = dv.state()
        assert (rc, nm, na) == (L.OK, sc.n_msgs, sc.n_appended)
        same(after, (want[0],) + before[1:])               # d_res filled, everything else untouched
        assert dv.call() == (rc, nm, na)
        same(dv.state(), want)                             # the real call gives the same d_res
    finally:
        dv.free()


def test_nomem_is_exact(ctx):
    sc = K.random_scenario(4, G=400, n=700)
    sc.expected()
    assert sc.n_msgs > 64
    check_fails(ctx, sc.pack(), L.E_NOMEM, cap=sc.n_msgs - 1)
    check_fails(ctx, sc.pack(), L.E_NOMEM, cap=0)
    check(ctx, sc)                                         # msgs_cap == the total: the canary after it intact
    # the room for entries: nlog + the run's proposals (a dropped one counts), exactly
    for what, room, ok in (("PCP", 3, True), ("PCP", 2, False), ("BCC", 2, True), ("BCC", 1, False), ("B", 0, True)):
        one = K.Scenario()
        for _ in range(70):
            one.add_run(one.add_group([1, 2], THREE, term=2, room=4, pending_conf=1), "P")
        one.add_run(one.add_group([1, 2], THREE, term=2, room=room, pending_conf=1), what)
        one.add_run(one.add_group([1, 2], THREE, term=2, room=4), "P")
        if ok:
            check(ctx, one)
        else:
            check_fails(ctx, one.pack(), L.E_NOMEM)
            dv = Dev(ctx, one.pack(), 0)                   # ... for the size query too
            try:
                assert dv.call(msgs=False) == (L.E_NOMEM, 0, 0)
            finally:
                dv.free()


THREE = [(1, 2, 3), (2, 0, 3), (3, 0, 2)]


def _thousand():
    sc = K.Scenario()
    for g in range(1000):
        sc.add_group([1, 2, 2], [(1, g + 2, g + 3), (2, 0, g + 3), (3, 0, g + 2)], term=2, committed=g, log_offset=g,
                     room=2)
        sc.add_run(g, "PB" if g % 3 == 0 else "C")
    return sc


def test_whole_call_failures(ctx):
    sc = _thousand()
    check(ctx, sc)
    n, ne = len(sc.locals), 5000

    def broken(edit):
        arrays = sc.pack()
        edit(*arrays)
        return arrays

    def setter(which, at, value):
        return lambda *a: a[which].__setitem__(at, np.uint64(value))
    GR, ST, EN, LO = 0, 1, 3, 4
    # group == G, as a record's word and as the G argument
    check_fails(ctx, broken(setter(LO, (500, 0), 1000)), L.E_INVAL)
    check_fails(ctx, sc.pack(), L.E_INVAL, G=999)
    # a group's records not adjacent
    check_fails(ctx, broken(setter(LO, (n - 1, 0), 0)), L.E_INVAL)
    check_fails(ctx, broken(lambda *a: a[LO].__setitem__((300, 0), a[LO][100, 0])), L.E_INVAL)
    # kind not 1 or 2; data_nil not 0 or 1
    check_fails(ctx, broken(setter(LO, (77, 1), 0)), L.E_INVAL)
    check_fails(ctx, broken(setter(LO, (77, 1), 3)), L.E_INVAL)
    check_fails(ctx, broken(setter(LO, (640, 2), 2 << 32)), L.E_INVAL)
    check_fails(ctx, broken(setter(LO, (640, 2), U64)), L.E_INVAL)
    # a proposal's Data range outside data_len_total, or wrapping (record 0 is a proposal)
    check_fails(ctx, sc.pack(), L.E_INVAL, dl=2)
    check_fails(ctx, broken(setter(LO, (0, 3), (1 << 20) - 2)), L.E_INVAL)
    check_fails(ctx, broken(setter(LO, (0, 3), U64)), L.E_INVAL)
    check_fails(ctx, broken(setter(LO, (0, 4), U64)), L.E_INVAL)
    # the entry window one past n_ents_total; one that wraps; nlog > ents_cap
    check_fails(ctx, sc.pack(), L.E_INVAL, ne=ne - 1)
    check_fails(ctx, broken(setter(GR, (998, 5), ne - 4)), L.E_INVAL)
    check_fails(ctx, broken(setter(GR, (7, 5), U64 - 1)), L.E_INVAL)
    check_fails(ctx, broken(setter(ST, (7, 0), U64)), L.E_INVAL)
    check_fails(ctx, broken(setter(ST, (7, 0), 2)), L.E_INVAL)
    check_fails(ctx, broken(setter(GR, (7, 4), U64)), L.E_INVAL)
    # two equal peer ids within n_peers
    check_fails(ctx, broken(lambda *a: a[GR].__setitem__((640, 9), a[GR][640, 7])), L.E_INVAL)
    # reserved != 0 in the group or the state record; pending_conf > 1
    check_fails(ctx, broken(setter(GR, (999, 31), 1)), L.E_INVAL)
    check_fails(ctx, broken(setter(GR, (0, 28), 1 << 63)), L.E_INVAL)
    check_fails(ctx, broken(setter(ST, (3, 3), 1)), L.E_INVAL)
    check_fails(ctx, broken(setter(ST, (3, 2), 2)), L.E_INVAL)
    # INVAL wins over NOMEM (of the messages, and of the entries)
    check_fails(ctx, broken(setter(GR, (999, 31), 1)), L.E_INVAL, cap=0)

    def both(*a):
        a[ST][0, 0] = np.uint64(3)          # group 0: nlog 3 + 1 proposal > 3
        a[GR][999, 31] = np.uint64(1)
    check_fails(ctx, broken(both), L.E_INVAL)
    check_fails(ctx, broken(setter(ST, (0, 0), 3)), L.E_NOMEM)
    # the host's own checks
    check_fails(ctx, sc.pack(), L.E_INVAL, n=(1 << 31) - 1)
    check_fails(ctx, sc.pack(), L.E_INVAL, G=(1 << 31) - 1)
    check(ctx, sc)


def test_idle_groups_may_hold_anything(ctx):
    sc = _thousand()
    idle = K.Scenario()
    idle.groups, idle.logs, idle.snaps, idle.state = sc.groups, sc.logs, sc.snaps, sc.state
    idle.locals = [m for m in sc.locals if m["group"] != 5]
    want = want_of(idle)
    arrays = idle.pack()
    arrays[0][5, 28:] = np.uint64(7)
    arrays[0][5, 5] = np.uint64(U64)
    arrays[0][5, 8] = arrays[0][5, 7]
    arrays[1][5] = np.uint64(U64)
    want[1][5] = arrays[0][5]
    want[2][5] = arrays[1][5]
    dv = Dev(ctx, arrays, idle.n_msgs)
    try:
        assert dv.call() == (L.OK, idle.n_msgs, idle.n_appended)
        same(dv.state(), want)
    finally:
        dv.free()
    dup = K.Scenario()
    dup.add_run(dup.add_group([1, 2, 2], [(1, 2, 3), (2, 0, 3), (2, 0, 2)], term=2, n_peers=2), "P")
    check(ctx, dup)


def test_empty_call(ctx):
    sc, _ = K.kat_scenario()
    check_fails(ctx, sc.pack(), L.OK, n=0)
    nm, na = C.c_uint64(5), C.c_uint64(5)
    assert L.lib.elead_local_batch_device(ctx.handle, None, None, 0, None, None, 0, 0, None, 0, None, None, 0,
                                          C.byref(nm), C.byref(na)) == L.OK
    assert (nm.value, na.value) == (0, 0)
    assert P.local_batch(ctx, [dict(id=1, term=2, prs=[(1, 0, 1)])], [[0, 1]], [dict(ents_cap=2)], [])[0] == []
    # a call whose records send nothing at all
    quiet = K.Scenario()
    quiet.add_run(quiet.add_group([0, 1, 1], [(1, 2, 3)], gid=1, term=1, pending_conf=1), "BCPB")
    check(ctx, quiet)
    assert quiet.n_msgs == 0 and quiet.n_appended == 1


def test_repeat_calls_and_set_stream(ctx):
    import torch
    big, small = K.random_scenario(5, G=1000, n=2000), K.kat_scenario(idle=3)[0]
    check(ctx, big)
    check(ctx, small)
    check(ctx, K.random_scenario(6, G=1000, n=2000))      # the same shape on a fresh scenario: no state is kept
    check(ctx, big)
    c2 = W.Context(0)
    stream = torch.cuda.Stream()
    try:
        check(c2, small)
        c2.set_stream(stream.cuda_stream)
        check(c2, big)
        assert L.lib.ewal_last_device_ms(c2.handle) > 0
        check(c2, small)
    finally:
        c2.close()
    del stream


def _proposal_round(rng, n_groups=60):
    """n_groups three-node leaders with 1-3 proposals each over random payloads; every window is exactly as
    long as its log becomes (emsg_encode_batch_device checks every entry of d_ents, so no canary may stay)."""
    sc = K.Scenario()
    data = bytes(rng.integers(0, 256, 4096, dtype=np.uint8))
    sc.data_len_total = len(data)
    for g in range(n_groups):
        nlog = int(rng.integers(2, 8))
        terms = [0] + [1] * (nlog - 2) + [2]
        last = nlog - 1
        props = int(rng.integers(1, 4))
        sc.add_group(terms, [(1, last, last + 1), (2, last, last + 1), (3, 0, int(rng.integers(1, nlog + 1)))], gid=1,
                     term=2, committed=0, room=props)
        for _ in range(props):
            ln = int(rng.integers(0, 40))
            sc.add_prop(g, etype=0, data_off=int(rng.integers(0, len(data) - ln)), data_len=ln)
    return sc, data


def test_fan_out_goes_straight_to_the_encoder(ctx):
    """d_msgs with the grown d_ents and d_data feeds emsg_encode_batch_device unchanged; decoded again, the
    entries carry the proposals' terms, indexes and Data bytes."""
    sc, data = _proposal_round(np.random.default_rng(8))
    _, _, _, erows, msgs = sc.expected()
    dv = Dev(ctx, sc.pack(), sc.n_msgs, len(data))
    dd = M._up(ctx, data)
    out = None
    try:
        assert dv.call() == (L.OK, sc.n_msgs, sc.n_appended)
        args = (ctx, dd, len(data), dv.bufs[6], sc.n_msgs, dv.bufs[3], dv.ne, None, 0)
        offs, lens, total = M.encode_messages_device(*args, None, 0)
        out = ctx.alloc(total + 64)
        assert M.encode_messages_device(*args, out, total) == (offs, lens, total)
        raw = out.download(total)
    finally:
        dv.free()
        dd.free()
        if out:
            out.free()
    back = M.decode_messages(ctx, [raw[o:o + k] for o, k in zip(offs, lens)])
    carried = 0
    for d, m, row in zip(back, sc.messages, msgs):
        assert d["status"] == L.OK
        assert (d["type"], d["to"], d["from_"], d["term"], d["log_term"], d["index"], d["commit"], d["reject"]) == \
            (K.MSG_APP, m["to"], 1, 2, m["log_term"], m["index"], m["commit"], False)
        first, cnt = int(row[7]), int(row[8])
        assert len(d["ents"]) == cnt
        for e, w in zip(d["ents"], erows[first:first + cnt]):
            nil = int(w[4]) >> 32
            assert (e["term"], e["index"]) == (int(w[0]), int(w[1]))
            assert (e["data"] or b"") == (b"" if nil else data[int(w[2]):int(w[2]) + int(w[3])])
            carried += int(w[3]) > 0
    # every proposal rides in its own broadcast's message to peer 2 (whose next was the old lastIndex + 1)
    assert carried > 0 and sc.n_appended == len(sc.locals)
    for o, m in zip(sc.outcomes, sc.locals):
        d = back[o["msg_first"]]
        assert d["to"] == 2 and o["n_msgs"] == 2
        e = [x for x in d["ents"] if x["index"] == o["index"]]
        assert len(e) == 1 and e[0]["term"] == 2 and e[0]["type"] == 0
        assert (e[0]["data"] or b"") == data[m["data_off"]:m["data_off"] + m["data_len"]]
        assert (e[0]["data"] is None) == (m["data_len"] == 0)


def test_appended_entries_go_straight_to_the_wal(ctx):
    """One group's appended entries d_ents[ent_pos, + k) through ewal_encode_entries_device: the frames equal
    the host writer's (ewal_encoder_save_entry) for the same entries."""
    sc, data = _proposal_round(np.random.default_rng(9), n_groups=5)
    sc.expected()
    g = max(range(5), key=lambda x: sum(m["group"] == x for m in sc.locals))
    recs = [(o, m) for o, m in zip(sc.outcomes, sc.locals) if m["group"] == g]
    k = len(recs)
    pos = recs[0][0]["ent_pos"]
    assert k >= 2 and [o["ent_pos"] for o, _ in recs] == list(range(pos, pos + k))
    enc = W.Encoder(prev_crc=77)
    for o, m in recs:
        enc.save_entry(0, 2, o["index"], None if m["data_nil"] else data[m["data_off"]:m["data_off"] + m["data_len"]])
    want, want_crc = enc.getvalue(), enc.crc
    dv = Dev(ctx, sc.pack(), sc.n_msgs, len(data))
    dd = M._up(ctx, data)
    out = ctx.alloc(len(want) + 256)
    try:
        assert dv.call() == (L.OK, sc.n_msgs, sc.n_appended)
        out_len, crc = C.c_uint64(), C.c_uint32()
        rc = L.lib.ewal_encode_entries_device(ctx.handle, dd.ptr, len(data), C.c_void_p(dv.bufs[3].ptr.value + pos * 40),
                                              k, 77, out.ptr, len(want) + 192, C.byref(out_len), C.byref(crc))
        assert rc == L.OK
        got = out.download(out_len.value)
    finally:
        dv.free()
        dd.free()
        out.free()
    assert got == want and crc.value == want_crc


def test_full_round_on_three_nodes(ctx):
    """60 leaders take 1-3 proposals -> their msgApp records as elog_app rows over the leader's own d_ents ->
    elog_append_batch_device on two followers per group -> its d_resp as elead_resp ->
    elead_step_batch_device: every group ends with committed == the last proposed index."""
    rng = np.random.default_rng(12)
    sc = K.Scenario()
    flogs = []
    for g in range(60):
        nlog = int(rng.integers(3, 8))
        terms = [0] + [1] * (nlog - 2) + [2]
        last = nlog - 1
        have = [int(rng.integers(1, nlog + 1)) for _ in range(2)]          # each follower holds a prefix
        flogs.append([terms[:h] for h in have])
        sc.add_group(terms, [(1, last, last + 1), (2, 0, have[0]), (3, 0, have[1])], gid=1, term=2, committed=0, room=3)
        sc.add_run(g, "P" * int(rng.integers(1, 4)))
    want = want_of(sc)
    last_run = {}                                                          # group -> its last proposal's record
    for i, m in enumerate(sc.locals):
        last_run[m["group"]] = i
    # the leader's call; its arrays stay on the device
    dv = Dev(ctx, sc.pack(), sc.n_msgs)
    fol = KA.Scenario()
    lead = KL.Scenario(snaps=False)
    bufs = []
    try:
        assert dv.call() == (L.OK, sc.n_msgs, sc.n_appended)
        got = dv.state()
        same(got, want)
        res, grows, strows, erows, msgs = got
        # the followers: one elog_group per (group, follower), the msgApp of the group's LAST proposal (it
        # carries every entry from the follower's next on)
        for g in range(60):
            o = sc.outcomes[last_run[g]]
            for f in (0, 1):
                row = msgs[o["msg_first"] + f]
                assert int(row[0]) == K.MSG_APP and int(row[1]) == 2 + f
                flog = flogs[g][f]
                fg = fol.add_group(flog, committed=0, unstable=len(flog), gid=2 + f, term=2, room=8)
                first, cnt = int(row[7]), int(row[8])
                fol.add_app(fg, int(row[5]), int(row[4]), commit=int(row[6]), ents_at=(first, cnt), from_=1)
        own_pack = fol.pack
        fol.pack = lambda: own_pack()[:3] + (erows,)                       # Entries = the leader's own d_ents ranges
        fgrows, fterms, farows, _ = fol.pack()
        want_fol = fol.expected()
        n = len(farows)
        bufs = [RL._up(ctx, fgrows), RL._up(ctx, fterms), RL._up(ctx, farows), ctx.alloc(n * 48 + 64),
                ctx.alloc(n * 144 + 64)]
        RL.append_batch_device(ctx, bufs[0], len(fgrows), bufs[1], len(fterms), bufs[2], n, dv.bufs[3], dv.ne, bufs[3],
                               bufs[4])
        resp = RL.responses_from(bufs[4].download(n * 144), n)
        fres = np.frombuffer(bufs[3].download(n * 48), dtype=np.uint64).reshape(n, 6)
        assert np.array_equal(fres, want_fol[0])
        assert all(not r["reject"] for r in resp)
        # the leader's msgAppResp step on the groups as the first call left them
        for g in range(60):
            w = [int(x) for x in grows[g]]
            lead.add_group([int(erows[w[5] + k, 0]) for k in range(w[4])],
                           [(w[7 + k], w[14 + k], w[21 + k]) for k in range(3)], gid=w[0], term=w[1], committed=w[2])
        for i, r in enumerate(resp):
            assert r["to"] == 1 and r["type"] == 4
            lead.add_resp(i // 2, r["from_"], r["index"], reject=r["reject"], term=r["term"])
        lres, lgrows, lmsgs = lead.expected()
        lrows = R.pack_resps(lead.resps)
        bufs += [R._up(ctx, lrows), ctx.alloc(len(lrows) * 48 + 64), ctx.alloc(lead.n_msgs * 144 + 64)]
        nm, nc = R.lead_step_batch_device(ctx, dv.bufs[0], 60, None, dv.bufs[3], dv.ne, bufs[5], len(lrows), bufs[6],
                                          bufs[7], lead.n_msgs)
        assert (nm, nc) == (lead.n_msgs, lead.n_committed)
        gres = np.frombuffer(bufs[6].download(len(lrows) * 48), dtype=np.uint64).reshape(-1, 6)
        ggrows = np.frombuffer(dv.bufs[0].download(grows.nbytes), dtype=np.uint64).reshape(-1, 32)
        gmsgs = np.frombuffer(bufs[7].download(lead.n_msgs * 144), dtype=np.uint64).reshape(-1, 18)
    finally:
        dv.free()
        for b in bufs:
            b.free()
    # the step's checker packs its logs densely: move its ents_first words to the windows of this round
    dense = lead.pack()[0][:, 5]
    for i, o in enumerate(lead.outcomes):
        for row in lmsgs[o["msg_first"]:o["msg_first"] + o["n_msgs"]]:
            if int(row[8]):
                row[7] = row[7] - dense[i // 2] + ggrows[i // 2, 5]
    assert np.array_equal(gres, lres) and np.array_equal(gmsgs, lmsgs)
    lgrows[:, 5] = ggrows[:, 5]
    assert np.array_equal(ggrows, lgrows)
    for g in range(60):
        assert int(ggrows[g, 2]) == sc.outcomes[last_run[g]]["index"], g
