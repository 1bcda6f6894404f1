"""GPU parity of the batched election step (evote_step_batch_device) with the
restatement of raft.Step for msgHup, msgVote and msgVoteResp in
vote_step_cases.py (raft/raft.go:372-408 and what it calls).  Every call
compares d_res, the complete d_groups, d_pstate, d_vstate and d_ents arrays and
the complete d_msgs array byte for byte; d_res starts as 0xA5 bytes, d_msgs and
the free slots of d_ents as a canary in every word (d_msgs SLACK records longer
than the call may fill), so a failing call must leave all six as they were and
a successful one the canary after its last message and entry."""
import collections
import ctypes as C

import numpy as np
import pytest

from etcd_amd import _lib as L
from etcd_amd import raftlead as R
from etcd_amd import raftlog as RL
from etcd_amd import raftmsg as M
from etcd_amd import raftvote as V
from etcd_amd import wal as W

import vote_step_cases as K
import lead_step_cases as KL
import log_append_cases as KA

pytestmark = pytest.mark.gpu

U64 = K.M64
SLACK = 3
NAMES = ("d_res", "d_groups", "d_pstate", "d_vstate", "d_ents", "d_msgs")


class Dev:
    """One call's arrays on the device."""

    def __init__(self, ctx, arrays, cap):
        self.ctx = ctx
        self.grows, self.strows, self.vrows, self.srows, self.erows, self.mrows = arrays
        self.G, self.ne, self.n, self.cap = len(self.grows), len(self.erows), len(self.mrows), cap
        self.fill_res = np.frombuffer(b"\xa5" * (self.n * 48), dtype=np.uint64).reshape(self.n, V.RESULT_WORDS)
        self.fill_msgs = np.full((cap + SLACK, R.MSG_WORDS), K.CANARY, dtype=np.uint64)
        self.bufs = [R._up(ctx, a) if a is not None else None
                     for a in (self.grows, self.strows, self.vrows, self.srows, self.erows, self.mrows, self.fill_res,
                               self.fill_msgs)]

    def call(self, G=None, n=None, ne=None, cap=None, msgs=True, snaps=True):
        nm, nw = C.c_uint64(99), C.c_uint64(99)
        b = self.bufs
        rc = L.lib.evote_step_batch_device(self.ctx.handle, b[0].ptr, b[1].ptr, b[2].ptr, self.G if G is None else G,
                                           b[3].ptr if snaps and b[3] else None, b[4].ptr,
                                           self.ne if ne is None else ne, b[5].ptr, self.n if n is None else n,
                                           b[6].ptr, b[7].ptr if msgs else None, self.cap if cap is None else cap,
                                           C.byref(nm), C.byref(nw))
        return rc, nm.value, nw.value

    def state(self):
        b = self.bufs

        def get(buf, like):
            return np.frombuffer(buf.download(like.nbytes), dtype=np.uint64).reshape(like.shape) if like.nbytes else like
        return (get(b[6], self.fill_res), get(b[0], self.grows), get(b[1], self.strows), get(b[2], self.vrows),
                get(b[4], self.erows), get(b[7], self.fill_msgs))

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
    res, grows, strows, vrows, erows, msgs = sc.expected()
    full = np.full((len(msgs) + SLACK, R.MSG_WORDS), K.CANARY, dtype=np.uint64)
    full[:len(msgs)] = msgs
    return res, grows, strows, vrows, erows, full


def check(ctx, sc, snaps=True):
    """The call on sc with msgs_cap == the exact total equals the restatement; returns the outcomes."""
    want = want_of(sc)
    dv = Dev(ctx, sc.pack(), sc.n_msgs)
    try:
        rc, nm, nw = dv.call(snaps=snaps)
        got = dv.state()
    finally:
        dv.free()
    assert rc == L.OK
    same(got, want)
    assert (nm, nw) == (sc.n_msgs, sc.n_won)
    return sc.outcomes


def check_fails(ctx, arrays, want_rc, cap=8192, **kw):
    """The call fails with want_rc and leaves all six arrays as they were."""
    dv = Dev(ctx, arrays, 8192)
    try:
        before = dv.state()
        rc, nm, nw = dv.call(cap=cap, **kw)
        after = dv.state()
    finally:
        dv.free()
    assert (rc, nm, nw) == (want_rc, 0, 0)
    same(after, before)


def test_kats(ctx):
    sc, named = K.kat_scenario()
    outs = check(ctx, sc)
    K.check_kats(sc, named)
    assert len(named) == 31 and len(outs) == 34


def test_kats_between_idle_groups(ctx):
    """Three garbage groups (non-zero reserved words included) before every table row: untouched."""
    sc, named = K.kat_scenario(idle=3)
    assert len(sc.groups) == 4 * 31 and len(sc.garbage) == 3 * 31
    check(ctx, sc)
    K.check_kats(sc, named)


def gpu_call(ctx):
    """play_election's `call` on the device: the arrays the call left and its messages, byte for byte the restatement's."""
    def call(sc):
        want = want_of(sc)
        dv = Dev(ctx, sc.pack(), sc.n_msgs)
        try:
            assert dv.call() == (L.OK, sc.n_msgs, sc.n_won)
            got = dv.state()
        finally:
            dv.free()
        same(got, want)
        msgs = R.messages_from(got[5].tobytes(), sc.n_msgs)
        assert [m["to"] for m in msgs] == [m["to"] for m in sc.messages]
        return got[1:5], [dict(m, group=s["group"]) for m, s in zip(msgs, sc.messages)]
    return call


def test_leader_election_rows(ctx):
    rows = K.load_kats()["TestLeaderElection"]["rows"]
    got = K.play_election(rows, gpu_call(ctx))[0]
    assert got == [(row["wstate"], row["wterm"]) for row in rows]


def test_lattice(ctx):
    sc = K.lattice_scenario()
    outs = check(ctx, sc)
    acts = collections.Counter(o["action"] for o in outs)
    assert len(sc.groups) == 1377 and all(acts[a] for a in range(1, 10)), acts


def _edges():
    sc = K.Scenario()
    three = [(1, 0, 3), (2, 0, 3), (3, 0, 3)]
    cc = dict(term=1, type=1)

    def run(log, prs, msgs, **kw):
        kw.setdefault("room", 4)                                          # a run's msgHup and msgVoteResp records
        g = sc.add_group(log, prs, **kw)
        for m in msgs:
            sc.add_msg(g, **m)
    vote = lambda f, **kw: dict(kind=K.MSG_VOTE, from_=f, **kw)            # noqa: E731
    resp = lambda f, **kw: dict(kind=K.MSG_VOTE_RESP, from_=f, **kw)      # noqa: E731
    hup = dict(kind=K.MSG_HUP)
    run([], three, [vote(2, term=1)], gid=1, log_offset=5, vote=3)
    run([], three, [vote(2, term=1), vote(2, term=1)], gid=1, log_offset=5)
    run([], three, [vote(2, term=9)], gid=1, log_offset=5, vote=3, state=K.LEADER)
    run([], three, [vote(2, term=1)], gid=1)
    run([], three, [hup], gid=1)
    run([1, 1, 1], three, [vote(2, term=1)], gid=1, log_offset=U64 - 1)
    run([1, 1, 1], three, [hup, resp(2, term=2)], gid=1, log_offset=U64 - 1,
        snap=dict(index=U64 - 1, term=1, data_off=1, data_len=2, nodes_off=3, n_nodes=4, removed_off=5, n_removed=6))
    run([1, 1, 1], three, [resp(2, term=1)], gid=1, state=K.CANDIDATE, voted=1, granted=1, log_offset=U64 - 1)
    run([0], [(1, 0, 1)], [resp(1, reject=True), resp(1)], gid=1, state=K.CANDIDATE)
    run([0], [(1, 0, 1), (2, 0, 1)], [resp(2), resp(1)], gid=1, state=K.CANDIDATE)
    run([0], [(1, 0, 1), (2, 0, 1)], [resp(2, reject=True), resp(1, reject=True)], gid=1, state=K.CANDIDATE)
    run([0], three, [hup, resp(2, term=2, reject=True), resp(2, term=2), resp(3, term=2)], gid=1)
    run([0], three, [resp(3, term=7)], gid=1, state=K.CANDIDATE, voted=1, granted=1)
    run([0, 1], three, [vote(2, term=7, index=1, log_term=1)], gid=1, state=K.LEADER, vote=3, lead=1)
    run([0], [(1, 0, 1)], [hup, hup, hup], gid=1, term=0)
    run([0], [(1, 0, 1)], [hup, vote(9, term=5, index=1), vote(9, term=6, log_term=1), hup], gid=1, term=0)
    run([0], three, [hup], gid=9)
    run([0], three, [resp(2), resp(3)], gid=9, state=K.CANDIDATE)
    run([0], three, [resp(8)], gid=1, state=K.CANDIDATE)
    run([1, 1], three, [resp(2)], gid=1, state=K.CANDIDATE, voted=1, granted=1, log_offset=5, committed=4)
    run([0, cc, 1], three, [resp(2)], gid=1, state=K.CANDIDATE, voted=1, granted=1)
    run([0, cc, cc], three, [resp(2)], gid=1, state=K.CANDIDATE, voted=1, granted=1, pending_conf=1)
    run([0], three, [vote(2, term=3), vote(2), resp(2, term=3)], gid=1, term=4, state=K.LEADER)
    return sc


def test_edges(ctx):
    """The short circuit, empty and wrapped logs, the poll's order, duplicates, the quirk, two wins in a run,
    becomeLeader's scan, a panic in the winner's broadcast (test_vote_step_host.py says what each must give)."""
    sc = _edges()
    outs = check(ctx, sc)
    stats = collections.Counter(o["status"] for o in outs)
    assert set(stats) == set(K.STATUSES), stats
    assert any(m["type"] == K.MSG_SNAP for m in sc.messages)
    # the whole call again without d_snaps: the msgSnap becomes a panic
    sc2 = _edges()
    sc2.with_snaps = False
    outs2 = check(ctx, sc2, snaps=False)
    assert sum(o["status"] == K.PANIC_NEED_SNAPSHOT for o in outs2) == stats[K.PANIC_NEED_SNAPSHOT] + 1


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_boundary_shapes(ctx, n):
    sc = K.boundary_scenario(n)
    check(ctx, sc)
    assert len(sc.msgs) == n


def test_long_runs(ctx):
    """A run of 300 records (longer than a workgroup: 150 wins, each entry read back by the next msgVote), alone
    and starting at lane 60."""
    sc = K.long_scenario(300)
    outs = check(ctx, sc)
    assert sum(o["action"] == K.WON for o in outs) == 150
    sc = K.long_scenario(300, lead_in=60)
    check(ctx, sc)
    assert sc.runs[-1] == (60, 60)


def test_many_workgroups(ctx):
    """17 workgroups of run heads, every lane a head."""
    sc = K.wide_scenario(16 * 256 + 3)
    outs = check(ctx, sc)
    acts = collections.Counter(o["action"] for o in outs)
    assert acts == {K.CAMPAIGNED: 1367, K.GRANTED: 1366, K.WON: 1366}, acts


@pytest.mark.parametrize("seed", [1, 2])
def test_random(ctx, seed):
    sc = K.random_scenario(seed)
    outs = check(ctx, sc)
    acts = collections.Counter(o["action"] for o in outs)
    stats = collections.Counter(o["status"] for o in outs)
    assert all(acts[a] >= 20 for a in range(10)) and all(stats[s] >= 20 for s in K.STATUSES), (acts, stats)


def test_size_query(ctx):
    sc = K.random_scenario(3, runs=800)
    want = want_of(sc)
    dv = Dev(ctx, sc.pack(), sc.n_msgs)
    try:
        before = dv.state()
        rc, nm, nw = dv.call(msgs=False, cap=0)
        after = dv.state()
        assert (rc, nm, nw) == (L.OK, sc.n_msgs, sc.n_won)
        same(after, (want[0],) + before[1:])               # d_res filled, everything else untouched
        assert dv.call() == (rc, nm, nw)
        same(dv.state(), want)                             # the real call gives the same d_res
    finally:
        dv.free()


THREE = [(1, 0, 3), (2, 0, 3), (3, 0, 3)]


def test_nomem_is_exact(ctx):
    sc = K.random_scenario(4, runs=400)
    sc.expected()
    assert sc.n_msgs > 64
    check_fails(ctx, sc.pack(), L.E_NOMEM, cap=sc.n_msgs - 1)
    check_fails(ctx, sc.pack(), L.E_NOMEM, cap=0)
    check(ctx, sc)                                         # msgs_cap == the total: the canary after it intact
    # the room for entries: nlog + the run's msgHup and msgVoteResp records (whatever they do), exactly
    hup, vote, resp = dict(kind=K.MSG_HUP), dict(kind=K.MSG_VOTE, from_=2, term=1), dict(kind=K.MSG_VOTE_RESP, from_=2)
    for run, room, ok in (([hup, resp, vote], 2, True), ([hup, resp, vote], 1, False), ([vote, vote], 0, True),
                          ([resp], 0, False), ([resp], 1, True)):
        one = K.Scenario()
        for _ in range(70):
            one.add_hup(one.add_group([0, 1], THREE, room=1))
        g = one.add_group([0, 1], THREE, room=room)
        for m in run:
            one.add_msg(g, **m)
        one.add_hup(one.add_group([0, 1], THREE, room=1))
        if ok:
            check(ctx, one)
        else:
            check_fails(ctx, one.pack(), L.E_NOMEM)
            dv = Dev(ctx, one.pack(), 0)                   # ... for the size query too
            try:
                assert dv.call(msgs=False) == (L.E_NOMEM, 0, 0)
            finally:
                dv.free()


def _thousand():
    sc = K.Scenario()
    for g in range(1000):
        sc.add_group([1, 2, 2], [(1, 0, g + 3), (2, 0, g + 3), (3, 0, g + 3)], term=2, committed=g, log_offset=g,
                     state=K.CANDIDATE if g % 3 else K.FOLLOWER, vote=1 if g % 3 else 0, voted=g % 3 and 1,
                     granted=g % 3 and 1)
        if g % 3:
            sc.add_msg(g, K.MSG_VOTE_RESP, from_=2, term=2, reject=g % 3 == 2)
            sc.add_msg(g, K.MSG_VOTE_RESP, from_=3, term=2)
        else:
            sc.add_hup(g)
    return sc


def test_whole_call_failures(ctx):
    sc = _thousand()
    check(ctx, sc)
    n, ne = len(sc.msgs), 5000

    def broken(edit):
        arrays = sc.pack()
        edit(*arrays)
        return arrays

    def setter(which, at, value):
        return lambda *a: a[which].__setitem__(at, np.uint64(value))
    GR, ST, VS, EN, MS = 0, 1, 2, 4, 5
    # group == G, as a record's word and as the G argument
    check_fails(ctx, broken(setter(MS, (500, 0), 1000)), L.E_INVAL)
    check_fails(ctx, sc.pack(), L.E_INVAL, G=999)
    # a group's records not adjacent
    check_fails(ctx, broken(setter(MS, (n - 1, 0), 0)), L.E_INVAL)
    check_fails(ctx, broken(lambda *a: a[MS].__setitem__((300, 0), a[MS][100, 0])), L.E_INVAL)
    # kind not 0, 5 or 6; reject not 0 or 1; padding not 0
    for kind in (1, 2, 4, 7, U64):
        check_fails(ctx, broken(setter(MS, (77, 1), kind)), L.E_INVAL)
    check_fails(ctx, broken(setter(MS, (640, 6), 2)), L.E_INVAL)
    check_fails(ctx, broken(setter(MS, (640, 6), 0xFFFFFFFF)), L.E_INVAL)
    check_fails(ctx, broken(setter(MS, (640, 6), 1 << 32)), L.E_INVAL)
    check_fails(ctx, broken(setter(MS, (641, 7), 1)), L.E_INVAL)
    # evote_state: state > 2; bits at or above n_peers; granted outside voted; reserved words
    check_fails(ctx, broken(setter(VS, (7, 0), 3)), L.E_INVAL)
    check_fails(ctx, broken(setter(VS, (7, 4), 9)), L.E_INVAL)
    check_fails(ctx, broken(setter(VS, (7, 5), 1 << 63)), L.E_INVAL)
    check_fails(ctx, broken(setter(VS, (9, 5), 1)), L.E_INVAL)            # group 9 is a follower: voted is 0
    check_fails(ctx, broken(setter(VS, (7, 6), 1)), L.E_INVAL)
    check_fails(ctx, broken(setter(VS, (999, 7), 1 << 40)), L.E_INVAL)
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
    check_fails(ctx, broken(setter(VS, (999, 7), 1)), L.E_INVAL, cap=0)

    def both(*a):
        a[ST][0, 0] = np.uint64(3)          # group 0: nlog 3 + 1 msgHup > 3
        a[GR][999, 31] = np.uint64(1)
    check_fails(ctx, broken(both), L.E_INVAL)
    check_fails(ctx, broken(setter(ST, (0, 0), 3)), L.E_NOMEM)
    # the host's own checks
    check_fails(ctx, sc.pack(), L.E_INVAL, n=(1 << 31) - 1)
    check_fails(ctx, sc.pack(), L.E_INVAL, G=(1 << 31) - 1)
    check(ctx, sc)


def test_empty_call(ctx):
    sc, _ = K.kat_scenario()
    check_fails(ctx, sc.pack(), L.OK, n=0)
    nm, nw = C.c_uint64(5), C.c_uint64(5)
    assert L.lib.evote_step_batch_device(ctx.handle, None, None, None, 0, None, None, 0, None, 0, None, None, 0,
                                         C.byref(nm), C.byref(nw)) == L.OK
    assert (nm.value, nw.value) == (0, 0)
    assert V.vote_batch(ctx, [dict(id=1, term=2, prs=[(1, 0, 1)])], [[0, 1]], [dict(ents_cap=2)], [dict()], [])[0] == []
    # a call whose records send nothing at all
    quiet = K.Scenario()
    g = quiet.add_group([0], [(1, 0, 1)], gid=1, term=0)
    quiet.add_hup(g)
    quiet.add_msg(g, K.MSG_VOTE_RESP, from_=1)
    check(ctx, quiet)
    assert quiet.n_msgs == 0 and quiet.n_won == 1


def test_host_convenience(ctx):
    res, groups, state, vstate, ents, msgs = V.vote_batch(
        ctx, [dict(id=1, term=0, prs=[(1, 0, 1), (2, 0, 1), (3, 0, 1)])], [[0]], [dict(ents_cap=3, unstable=1)],
        [dict()], [dict(group=0, kind="hup"), dict(group=0, kind="vote_resp", from_=3, term=1)])
    assert [V.ACTIONS[r["action"]] for r in res] == ["campaigned", "won"]
    assert (groups[0]["term"], groups[0]["nlog"], vstate[0]["state"], vstate[0]["lead"]) == (1, 2, V.LEADER, 1)
    assert [m["type"] for m in msgs] == [5, 5, 3, 3] and [int(x) for x in ents[1]] == [1, 1, 0, 0, 1 << 32]


def test_repeat_calls_and_set_stream(ctx):
    import torch
    big, small = K.random_scenario(5, runs=1000), K.kat_scenario(idle=1)[0]
    check(ctx, big)
    check(ctx, small)
    check(ctx, K.random_scenario(6, runs=1000))            # the same shape on a fresh scenario: no state is kept
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


@pytest.mark.parametrize("nodes", [3, 5])
def test_full_election_on_the_device(ctx, nodes):
    """40 clusters, one group per node: msgHup at node 1 -> its msgVote through emsg_encode_batch_device and
    emsg_decode_batch_device -> the voters -> their msgVoteResp at the candidate -> WON, whose broadcast goes
    through elog_append_batch_device on the followers and their answers through elead_step_batch_device: every
    leader ends with its empty entry committed."""
    clusters = 40
    rng = np.random.default_rng(nodes)
    rows = []
    for c in range(clusters):
        k = int(rng.integers(1, 5))
        # every follower holds the candidate's log, but in odd clusters the last one is an entry short: it
        # grants all the same, rejects the winner's msgApp, and the quorum commits without it
        rows.append(dict(peers=[[1] * k] * (nodes - 1) + [[1] * (k - c % 2)]))
    base = gpu_call(ctx)
    wire = []

    def call(sc):
        arrays, msgs = base(sc)
        if not wire:
            # the first call's fan-out over the wire: encode on the device, decode on the device
            _, _, _, _, erows, mrows = sc.expected()
            erows = np.where(erows == np.uint64(K.CANARY), np.uint64(0), erows)   # the encoder checks every entry
            bufs = [R._up(ctx, mrows), R._up(ctx, erows), None]
            try:
                args = (ctx, None, 0, bufs[0], len(mrows), bufs[1], len(erows), None, 0)
                offs, lens, total = M.encode_messages_device(*args, None, 0)
                bufs[2] = ctx.alloc(total + 64)
                assert M.encode_messages_device(*args, bufs[2], total) == (offs, lens, total)
                raw = bufs[2].download(total)
            finally:
                for b in bufs:
                    if b is not None:
                        b.free()
            back = M.decode_messages(ctx, [raw[o:o + k] for o, k in zip(offs, lens)])
            assert len(back) == len(msgs) == clusters * (nodes - 1)
            for d, m in zip(back, msgs):
                assert d["status"] == L.OK and not d["ents"]
                for key in ("type", "to", "from_", "term", "log_term", "index", "reject"):
                    assert d[key] == m[key], key
            wire.append(len(back))
            msgs = [dict(d, group=m["group"]) for d, m in zip(back, msgs)]
        return arrays, msgs
    states, sc, arrays, msgs = K.play_election(rows, call)
    assert wire and states == [(K.LEADER, 1)] * clusters
    grows, strows, vrows, erows = arrays
    # the winners' broadcast at the followers: one elog_group per (cluster, follower)
    fol = KA.Scenario()
    lead = KL.Scenario(snaps=False)
    heads = sorted(set(sc.cluster))
    won = [o for o in sc.outcomes if o["action"] == K.WON]
    assert len(won) == clusters and all(o["n_msgs"] == nodes - 1 for o in won)
    mrows = sc.expected()[5]
    for c, (g, o) in enumerate(zip(heads, won)):
        w = [int(x) for x in grows[g]]
        assert (w[1], w[4]) == (1, len(rows[c]["peers"][0]) + 2) and int(vrows[g, 0]) == K.LEADER
        for f in range(nodes - 1):
            row = mrows[o["msg_first"] + f]
            assert (int(row[0]), int(row[1]), int(row[8])) == (K.MSG_APP, 2 + f, 1)
            flog = [0] + rows[c]["peers"][1 + f]
            fg = fol.add_group(flog, committed=0, unstable=len(flog), gid=2 + f, term=1, room=8)
            fol.add_app(fg, int(row[5]), int(row[4]), commit=int(row[6]), ents_at=(int(row[7]), 1), from_=1)
    own_pack = fol.pack
    fol.pack = lambda: own_pack()[:3] + (erows,)                           # Entries = the leaders' own d_ents ranges
    fgrows, fterms, farows, _ = fol.pack()
    want_fol = fol.expected()
    n = len(farows)
    bufs = [R._up(ctx, grows), R._up(ctx, erows), RL._up(ctx, fgrows), RL._up(ctx, fterms), RL._up(ctx, farows),
            ctx.alloc(n * 48 + 64), ctx.alloc(n * 144 + 64)]
    try:
        RL.append_batch_device(ctx, bufs[2], len(fgrows), bufs[3], len(fterms), bufs[4], n, bufs[1], len(erows), bufs[5],
                               bufs[6])
        resp = RL.responses_from(bufs[6].download(n * 144), n)
        fres = np.frombuffer(bufs[5].download(n * 48), dtype=np.uint64).reshape(n, 6)
        assert np.array_equal(fres, want_fol[0])
        # a follower whose log is as long as the leader's was accepts at once; the others reject (the leader
        # probes them next round).  Their answers at the leaders, on the groups as the election left them:
        lrows = R.pack_resps([dict(group=heads[i // (nodes - 1)], from_=r["from_"], term=r["term"], index=r["index"],
                                   reject=r["reject"]) for i, r in enumerate(resp)])
        bufs += [R._up(ctx, lrows), ctx.alloc(n * 48 + 64)]
        total, _ = R.lead_step_batch_device(ctx, bufs[0], len(grows), None, bufs[1], len(erows), bufs[7], n, bufs[8])
        bufs.append(ctx.alloc(total * 144 + 64))
        nm, nc = R.lead_step_batch_device(ctx, bufs[0], len(grows), None, bufs[1], len(erows), bufs[7], n, bufs[8],
                                          bufs[9], total)
        after = np.frombuffer(bufs[0].download(grows.nbytes), dtype=np.uint64).reshape(-1, 32)
    finally:
        for b in bufs:
            b.free()
    assert sum(r["reject"] for r in resp) == clusters // 2 and nm == total
    for c, g in enumerate(heads):
        assert int(after[g, 2]) == int(after[g, 4]) - 1 == len(rows[c]["peers"][0]) + 1, c     # the empty entry's index
    assert nc == clusters
