"""GPU parity tests of the batched follower step (efollow_step_batch_device):
bit for bit against the restatement in follow_cases.py, over every output
array, every group record and every input array (canaries in the free window
slots, between the messages' source entries, in unnamed groups and in d_msgs
past *n_msgs).  There is no inline-copy threshold in this implementation (every
appended entry goes through the copy pass), so the entry counts below are the
copy pass's wave and workgroup edges."""
import ctypes as C
import random

import numpy as np
import pytest

from etcd_amd import _lib as L
from etcd_amd import raftfollow as F
from etcd_amd import raftlead as R
from etcd_amd import raftlog as RL
from etcd_amd import raftmsg as RM
from etcd_amd import raftprop as P
from etcd_amd import raftready as RD
from etcd_amd import raftvote as V
from etcd_amd import wal as W

import follow_cases as K

pytestmark = pytest.mark.gpu

M64 = K.M64
SLACK = 3
NAMES = ("res", "out", "groups", "pstate", "vstate", "rstate", "snaps", "ents", "src", "in_snaps", "u64", "msgs")
THREE = [(1, 0, 1), (2, 0, 1), (3, 0, 1)]


class Dev:
    """One call's arrays on the device."""

    def __init__(self, ctx, a, cap):
        self.ctx, self.a, self.cap = ctx, a, cap
        n = len(a["msgs"])
        self.fill_res = np.frombuffer(b"\xa5" * (n * 96), dtype=np.uint64).reshape(n, K.OW)
        self.fill_out = np.full((cap + SLACK, K.MW), K.CANARY, dtype=np.uint64)
        self.host = (self.fill_res, self.fill_out, a["groups"], a["pstate"], a["vstate"], a["rstate"], a["snaps"],
                     a["ents"], a["src"], a["in_snaps"], a["u64"], a["msgs"])
        self.bufs = [R._up(ctx, h) if h is not None else None for h in self.host]

    def call(self, out=True, **kw):
        nm, na, nr = C.c_uint64(99), C.c_uint64(99), C.c_uint64(99)
        b, a = self.bufs, self.a
        src = b[7] if a["src"] is None else b[8]
        p = lambda x: x.ptr if x is not None else None   # noqa: E731
        k = dict(G=len(a["groups"]), ne=len(a["ents"]), ns=len(a["ents"] if a["src"] is None else a["src"]),
                 nin=len(a["in_snaps"]), nu=len(a["u64"]), n=len(a["msgs"]), cap=self.cap, groups=p(b[2]),
                 rstate=p(b[5]), snaps=p(b[6]), res=p(b[0]))
        k.update(kw)
        rc = L.lib.efollow_step_batch_device(self.ctx.handle, k["groups"], p(b[3]), p(b[4]), k["rstate"], k["G"],
                                             k["snaps"], p(b[7]), k["ne"], p(src), k["ns"], p(b[9]), k["nin"], p(b[10]),
                                             k["nu"], p(b[11]), k["n"], k["res"], p(b[1]) if out else None, k["cap"],
                                             C.byref(nm), C.byref(na), C.byref(nr))
        return rc, nm.value, na.value, nr.value

    def state(self):
        def get(buf, like):
            if like is None or not like.nbytes:
                return like
            return np.frombuffer(buf.download(like.nbytes), dtype=np.uint64).reshape(like.shape)
        return tuple(get(b, h) for b, h in zip(self.bufs, self.host))

    def free(self):
        for b in self.bufs:
            if b is not None:
                b.free()


def same(got, want):
    for name, g, w in zip(NAMES, got, want):
        if g is None and w is None:
            continue
        if not np.array_equal(g, w):
            at = tuple(int(x) for x in np.argwhere(g != w)[0])
            raise AssertionError("%s differs at %r: got %#x, want %#x" % (name, at, int(g[at]), int(w[at])))


def want_of(a, x, emit=True):
    full = np.full((x["n_msgs"] + SLACK, K.MW), K.CANARY, dtype=np.uint64)
    if emit:
        full[:x["n_msgs"]] = x["msg_rows"]
        return (x["res_rows"], full, x["groups"], x["pstate"], x["vstate"], x["rstate"], x["snaps"], x["ents"],
                a["src"], a["in_snaps"], a["u64"], a["msgs"])
    return (x["res_rows"], full, a["groups"], a["pstate"], a["vstate"], a["rstate"], a["snaps"], a["ents"], a["src"],
            a["in_snaps"], a["u64"], a["msgs"])


def check(ctx, a):
    """The size query fills d_res and the counters, agrees with the real call
    and modifies nothing; the real call with msgs_cap == the exact total equals
    the restatement.  Returns the restatement's dict."""
    assert K.validate(a) == K.OK
    x = K.expected(a)
    counts = (x["n_msgs"], x["n_appended"], x["n_restored"])
    dv = Dev(ctx, a, x["n_msgs"])
    try:
        assert dv.call(out=False) == (L.OK,) + counts
        same(dv.state(), want_of(a, x, emit=False))
        assert dv.call() == (L.OK,) + counts
        got = dv.state()
    finally:
        dv.free()
    same(got, want_of(a, x))
    return x


def check_fails(ctx, a, want_rc, cap=8192, **kw):
    """The call fails with want_rc and leaves every array as it was, the counters 0."""
    dv = Dev(ctx, a, cap)
    try:
        before = dv.state()
        got = dv.call(**kw)
        after = dv.state()
    finally:
        dv.free()
    assert got == (want_rc, 0, 0, 0)
    same(after, before)


def acts(x):
    return [(o["status"], o["action"]) for o in x["outcomes"]]


def test_kats(ctx):
    sc, named = K.kat_scenario()
    a = sc.pack()
    K.check_kats(sc, named, a, check(ctx, a))


def test_kats_between_idle_groups(ctx):
    sc, named = K.kat_scenario(idle=2)
    a = sc.pack()
    K.check_kats(sc, named, a, check(ctx, a))


@pytest.mark.parametrize("seed", [1, 2])
def test_random(ctx, seed):
    """A few thousand records; a data_delta that wraps every rebased data_off; garbage groups in between."""
    sc = K.random_scenario(seed, 1300, idle_every=9, data_delta=M64 - 4)
    x = check(ctx, sc.pack())
    assert len(x["outcomes"]) > 3000
    seen = {o["action"] for o in x["outcomes"]}
    assert seen == set(range(9)) and {o["status"] for o in x["outcomes"]} == set(K.STATUSES)


def test_random_source_is_d_ents(ctx):
    sc = K.random_scenario(3, 700, same_array=True)
    a = sc.pack()
    assert a["src"] is None
    x = check(ctx, a)
    assert x["n_appended"] > 200 and x["n_restored"] > 50


def test_n_is_one(ctx):
    for add in (lambda sc, g: sc.add_app(g, from_=2, term=1, ents=[1]),
                lambda sc, g: sc.add_app(g, from_=2, term=1),
                lambda sc, g: sc.add_snap(g, from_=2, term=1, index=4, snap_term=1, nodes=[1, 2])):
        sc = K.Scenario()
        add(sc, sc.add_group([0], THREE, gid=1, term=1))
        x = check(ctx, sc.pack())
        assert x["n_msgs"] == 1


def boundary_scenario(n):
    """n records: single-record runs, and a six-record run that starts three
    records before every wave and workgroup seam (63|64, 255|256, 1023|1024):
    an append, two heartbeats on the grown log, then entries, a snapshot and a
    heartbeat that wait.  The last record heads a run of its own."""
    sc = K.Scenario()
    i = 0
    while i < n:
        seam = next((s for s in (64, 256, 1024) if i == s - 3 and n >= s + 4), None)
        g = sc.add_group([0, 1], THREE, gid=1 + i % 3, term=1, room=3, elapsed=i % 5)
        if seam:
            sc.add_app(g, from_=2, term=1, index=1, log_term=1, ents=[1, 1])
            sc.add_app(g, from_=2, term=1, index=3, log_term=1, commit=3)
            sc.add_app(g, from_=2, term=1, index=2, log_term=1, commit=2)
            sc.add_app(g, from_=2, term=1, index=3, log_term=1, ents=[1])
            sc.add_snap(g, from_=2, term=1, index=9, snap_term=1, nodes=[1, 2, 3])
            sc.add_app(g, from_=2, term=1, index=3, log_term=1)
            i += 6
        else:
            sc.add_app(g, from_=2, term=1 + i % 2, index=1, log_term=1, commit=i % 3, ents=[1] * (i % 2))
            i += 1
    return sc


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 1030])
def test_runs_across_wave_and_workgroup_seams(ctx, n):
    sc = boundary_scenario(n)
    assert abs(len(sc.msgs) - n) < 6 and sc.msgs[-1][0] != sc.msgs[-2][0]      # a run head as the last record
    x = check(ctx, sc.pack())
    if n > 70:
        assert [o["action"] for o in x["outcomes"][61:67]] == [K.APPENDED] * 3 + [K.DEFERRED] * 3
        assert x["outcomes"][62]["committed"] == 3


def test_entry_counts(ctx):
    """n_ents 0, 1, 2, 63, 64, 65, 255, 256, 257 and 513, with and without a
    matching prefix (the suffix starts inside the message), so the copy pass's
    lanes cross wave and workgroup edges at every alignment."""
    sc = K.Scenario()
    for ne in (0, 1, 2, 63, 64, 65, 255, 256, 257, 513):
        for keep in (0, 1, 5):
            log = [0] + [1] * keep + [1]                   # `keep` entries match, the next one conflicts (term 1 vs 2)
            g = sc.add_group(log, THREE, gid=1, term=2, room=ne + 2)
            ents = [K.entry(1 if k < keep else 2, k + 1, 8 * k, 8, 0, k % 3) for k in range(ne)]
            sc.add_app(g, from_=2, term=2, index=0, log_term=0, commit=ne, ents=ents, data_delta=1000)
    x = check(ctx, sc.pack())
    assert x["n_appended"] == sum(max(ne - keep, 0) for ne in (0, 1, 2, 63, 64, 65, 255, 256, 257, 513)
                                  for keep in (0, 1, 5))


def test_one_long_message_next_to_heartbeats(ctx):
    sc = K.Scenario()
    for k in range(500):
        sc.add_app(sc.add_group([0, 1], THREE, gid=2, term=1, room=0), from_=1, term=1, index=1, log_term=1, commit=1)
    g = sc.add_group([0, 1], THREE, gid=2, term=1, room=4097)
    sc.add_app(g, from_=1, term=1, index=1, log_term=1, commit=4000,
               ents=[K.entry(1, 2 + k, 16 * k, 16, 0, 0) for k in range(4097)], data_delta=1 << 40)
    for k in range(500):
        sc.add_app(sc.add_group([0, 1], THREE, gid=3, term=1, room=0), from_=1, term=1, index=1, log_term=1, commit=1)
    x = check(ctx, sc.pack())
    assert (x["n_msgs"], x["n_appended"]) == (1001, 4097) and x["outcomes"][500]["last_index"] == 4098


def test_source_is_d_ents_with_a_wrapping_delta(ctx):
    sc = K.Scenario(same_array=True)
    g = sc.add_group([0], THREE, gid=2, term=1, room=5)
    h = sc.add_group([0], THREE, gid=3, term=1, room=5)
    ents = [K.entry(1, 1, 3, 9, 0, 0), K.entry(1, 2, 0, 0, 0, 1), K.entry(1, 3, 7, 1, 1, 2)]
    sc.add_app(g, from_=1, term=1, ents=ents, data_delta=M64 - 1)
    sc.add_app(h, from_=1, term=1, ents=ents, data_delta=M64)
    x = check(ctx, sc.pack())
    assert [int(e[2]) for e in x["ents"][1:4]] == [1, 0, 7] and [int(e[2]) for e in x["ents"][7:10]] == [2, 0, 7]


def test_a_panic_in_the_middle_of_a_run_rolls_back_that_record_only(ctx):
    sc = K.Scenario()
    g = sc.add_group([0, 1, 1], THREE, gid=1, term=2, committed=2, room=3, elapsed=7)
    sc.add_app(g, from_=2, term=2, index=2, log_term=1, commit=2)                  # stepped: lead, elapsed
    sc.add_app(g, from_=3, term=5, index=0, log_term=0, ents=[3])                  # conflicts with committed entry 1
    sc.add_app(g, from_=2, term=2, index=2, log_term=1)
    h = sc.add_group([0], THREE, gid=1, term=1, room=2)
    sc.add_app(h, from_=2, term=1, ents=[1])
    a = sc.pack()
    x = check(ctx, a)
    assert acts(x)[:3] == [(0, K.APPENDED), (K.PANIC_COMMITTED_CONFLICT, K.PANICKED), (0, K.NOT_STEPPED)]
    assert [int(v) for v in x["vstate"][g][:4]] == [0, 0, 2, 0] and int(x["groups"][g][1]) == 2   # not term 5
    assert x["outcomes"][1]["term"] == 2 and x["n_msgs"] == 2 and acts(x)[3] == (0, K.APPENDED)


def _failing():
    sc = K.Scenario()
    rng = random.Random(5)
    sc.add_idle(rng)
    g = sc.add_group([0, 1], THREE, gid=1, term=1, room=1)
    h = sc.add_group([0], THREE, gid=1, term=1, room=1)
    sc.add_app(g, from_=2, term=1, index=1, log_term=1, ents=[1])
    sc.add_snap(h, from_=2, term=1, index=3, snap_term=1, nodes=[1, 2])
    for k in range(300):                                   # more than one workgroup
        sc.add_app(sc.add_group([0], THREE, gid=1, term=1, room=1), from_=2, term=1, ents=[1])
    return sc.pack(), g, h


def test_whole_call_failures(ctx):
    def word(name, i, j, v):
        def f(a):
            a[name][i, j] = np.uint64(v)
        return f

    base, g, h = _failing()
    G, n = len(base["groups"]), len(base["msgs"])
    inval = [word("msgs", 0, 0, G), word("msgs", 0, 1, 4), word("msgs", 0, 11, 1), word("msgs", 0, 7, len(base["src"])),
             word("msgs", 0, 8, M64), word("msgs", 1, 10, 1), word("in_snaps", 0, 5, 3), word("in_snaps", 0, 4, M64),
             word("groups", g, 28, 1), word("groups", g, 8, 1), word("pstate", g, 3, 1), word("pstate", g, 2, 2),
             word("pstate", h, 0, 1 << 40), word("vstate", g, 0, 3), word("vstate", g, 4, 8), word("vstate", g, 5, 1),
             word("vstate", h, 7, 1), word("groups", g, 4, 4), word("msgs", n - 1, 0, g), word("msgs", 300, 1, 0),
             word("msgs", 257, 8, M64 - 1)]
    for k, edit in enumerate(inval):
        a = {key: (v.copy() if v is not None else None) for key, v in base.items()}
        edit(a)
        assert K.validate(a) == K.E_INVAL, k
        check_fails(ctx, a, L.E_INVAL)
    for key in ("rstate", "snaps"):                        # a msgSnap needs both
        check_fails(ctx, base, L.E_INVAL, **{key: None})
    nomem = [word("msgs", 0, 8, 2), lambda a: (word("groups", h, 4, 0)(a), word("pstate", h, 0, 0)(a))]
    for k, edit in enumerate(nomem):
        a = {key: (v.copy() if v is not None else None) for key, v in base.items()}
        edit(a)
        assert K.validate(a) == K.E_NOMEM, k
        check_fails(ctx, a, L.E_NOMEM)
        word("msgs", 5, 11, 1)(a)                          # INVAL wins
        check_fails(ctx, a, L.E_INVAL)
    check_fails(ctx, base, L.E_NOMEM, cap=n - 1)           # one message too many for d_msgs
    # host checks: misaligned records, counts out of range
    dv = Dev(ctx, base, 8192)
    try:
        before = dv.state()
        assert dv.call(groups=C.c_void_p(dv.bufs[2].ptr.value + 8))[0] == L.E_INVAL
        assert dv.call(res=C.c_void_p(dv.bufs[0].ptr.value + 8))[0] == L.E_INVAL
        assert dv.call(n=0x7fffffff)[0] == L.E_INVAL and dv.call(G=0x7fffffff)[0] == L.E_INVAL
        assert dv.call(n=0) == (L.OK, 0, 0, 0)
        same(dv.state(), before)
    finally:
        dv.free()


def test_host_convenience_and_repeat_calls(ctx):
    sc = K.random_scenario(4, 60)
    a = sc.pack()
    x = K.expected(a)
    for _ in range(2):
        r = F.follow_batch(ctx, a["groups"], a["pstate"], a["vstate"], a["rstate"], a["snaps"], a["ents"], a["msgs"],
                           src=a["src"], in_snaps=a["in_snaps"], u64=a["u64"])
        for key in ("res_rows", "msg_rows", "groups", "pstate", "vstate", "rstate", "snaps", "ents"):
            assert np.array_equal(r[key], x[key]), key
        assert (r["n_msgs"], r["n_appended"], r["n_restored"]) == (x["n_msgs"], x["n_appended"], x["n_restored"])
        assert [(o["status"], o["action"]) for o in r["res"]] == acts(x)
        assert [(m["type"], m["to"], m["index"], m["reject"]) for m in r["msgs"]] == \
            [(4, m["to"], m["index"], m["reject"]) for m in x["messages"]]
    q = F.follow_batch(ctx, a["groups"], a["pstate"], a["vstate"], a["rstate"], a["snaps"], a["ents"], a["msgs"],
                       src=a["src"], in_snaps=a["in_snaps"], u64=a["u64"], size_query=True)
    assert np.array_equal(q["res_rows"], x["res_rows"]) and np.array_equal(q["groups"], a["groups"])


def test_same_answers_as_the_terms_only_append(ctx):
    """The second yardstick: one same-term msgApp per follower group gives what
    elog_append_batch_device gives on the equivalent elog_group / d_terms state."""
    sc = K.Scenario()
    groups, logs, apps = [], [], []
    j = 0
    while len(groups) < 1500:
        grp, msgs = K.draw(9, j)
        j += 1
        m = next((m for m in msgs if m["kind"] == K.MSG_APP), None)
        if m is None or grp["n_peers"] > 7:
            continue
        grp.update(state=K.FOLLOWER, voted=0, granted=0)
        g = sc.add_group(**grp)
        sc.add_app(g, from_=m["from_"], term=grp["term"], index=m["index"], log_term=m["log_term"], commit=m["commit"],
                   ents=m["ents"])
        groups.append(dict(id=grp["gid"], term=grp["term"], committed=grp["committed"], unstable=grp["unstable"],
                           log_offset=grp["log_offset"]))
        logs.append(grp["log"])
        apps.append(dict(group=g, from_=m["from_"], index=m["index"], log_term=m["log_term"], commit=m["commit"],
                         ents=m["ents"]))
    x = check(ctx, sc.pack())
    res, g2, resp = RL.append_batch(ctx, groups, logs, apps, capacity=1.0 + 8)
    assert {o["status"] for o in x["outcomes"]} == {K.OK, K.PANIC_BOUNDS, K.PANIC_COMMITTED_CONFLICT}
    for o, r, m, g, e in zip(x["outcomes"], res, resp, g2, x["groups"]):
        assert o["status"] == r["status"]
        assert (o["action"] == K.APPENDED) == bool(r["accepted"])
        assert (o["conflict"], o["n_app"], o["last_index"], o["committed"]) == \
            (r["conflict"], r["n_app"], r["last_index"], r["committed"])
        assert [int(t[0]) for t in x["ents"][int(e[5]):int(e[5]) + int(e[4])]] == g["terms"]
    sent = iter(x["messages"])
    for o, m in zip(x["outcomes"], resp):
        if o["status"] != K.OK:
            assert m is None
            continue
        s = next(sent)
        assert (m["type"], m["to"], m["from_"], m["term"], m["index"], m["reject"], m["log_term"], m["commit"]) == \
            (s["type"], s["to"], s["from_"], s["term"], s["index"], s["reject"], 0, 0)


# ---- chains: the calls of a replication round in one set of arrays ------------------------

class Cluster:
    """`nodes` replicas of `clusters` raft groups, one group record per
    replica (cluster c's node id is group c * nodes + id - 1).  Without a
    leader_log every node is as RestartNode leaves an empty one -- a follower
    of term 0 with the dummy entry, no vote, no leader, node.run's empty prev
    states -- and elect() runs the election on the device.  With a leader_log
    at an offset the compacted state is forged (see __init__)."""

    def __init__(self, ctx, nodes, clusters, leader_log=None, offset=0, snaps=None, slow=None, data=b""):
        """leader_log at offset, with snaps: node 1 is the leader of term 1 over that compacted log; slow is the
        one node that has nothing of it (log [0]); the others hold the leader's log, all of it committed and
        applied."""
        self.ctx, self.nodes, self.G = ctx, nodes, nodes * clusters
        sc = K.Scenario()
        for c in range(clusters):
            for id_ in range(1, nodes + 1):
                if leader_log is None:
                    sc.add_group([0], [(p, 0, 1) for p in range(1, nodes + 1)], gid=id_, term=0, room=8)
                    continue
                lead = id_ == 1
                has = lead or id_ != slow
                log = leader_log if has else [0]
                off = offset if has else 0
                last = off + len(log) - 1
                done = last if has else off                              # committed and applied
                prs = [(p, last if (lead and p == 1) else 0, last + 1 if (lead and p == 1) else off + 1)
                       for p in range(1, nodes + 1)]
                sc.add_group(log, prs, gid=id_, term=1, log_offset=off, committed=done, room=8,
                             state=K.LEADER if lead else K.FOLLOWER, vote=1, lead=1 if lead else 0,
                             unstable=(done + 1) if has else 1, applied=done, snap=snaps if lead else None,
                             rstate={0: 1, 1: 1, 2: done, 3: 0, 4: 0, 5: off})
        a = sc.pack()
        a["ents"][a["ents"] == np.uint64(K.CANARY)] = 0     # emsg_encode_batch_device checks every entry it is given
        self.shape = {k: a[k].shape for k in ("groups", "pstate", "vstate", "rstate", "snaps", "ents")}
        self.ne = len(a["ents"])
        self.data = data
        self.d = {k: R._up(ctx, a[k]) for k in self.shape}
        self.d["data"] = R._up(ctx, np.frombuffer(data + b"\0" * (-len(data) % 8 + 8), dtype=np.uint64))
        self.extra = []

    def free(self):
        for b in list(self.d.values()) + self.extra:
            b.free()

    def get(self, name):
        shape = self.shape[name]
        return np.frombuffer(self.d[name].download(int(np.prod(shape)) * 8), dtype=np.uint64).reshape(shape).copy()

    def arrays(self):
        return {k: self.get(k) for k in self.shape}

    def alloc(self, nbytes):
        b = self.ctx.alloc(nbytes + 64)
        self.extra.append(b)
        return b

    def up(self, arr):
        b = R._up(self.ctx, arr)
        self.extra.append(b)
        return b

    def group_of(self, sender_group, to):
        return sender_group - sender_group % self.nodes + to - 1

    def vote(self, msgs):
        """evote_step_batch_device over election message dicts (raftvote.pack_msgs), ordered by group.
        Returns (results, emsg_out rows, the sender group of each row)."""
        msgs = sorted(msgs, key=lambda m: m["group"])
        n = len(msgs)
        d_in, d_res = self.up(V.pack_msgs(msgs)), self.alloc(n * 48)
        args = (self.ctx, self.d["groups"], self.d["pstate"], self.d["vstate"], self.G, self.d["snaps"], self.d["ents"],
                self.ne, d_in, n, d_res)
        total, _ = V.vote_batch_device(*args)
        d_out = self.alloc(total * 144)
        V.vote_batch_device(*args, d_out, total)
        res = V.results_from(d_res.download(n * 48), n)
        assert all(r["status"] == L.OK for r in res)
        rows = np.frombuffer(d_out.download(total * 144), dtype=np.uint64).reshape(total, K.MW).copy()
        senders = [m["group"] for m, r in zip(msgs, res) for _ in range(r["n_msgs"])]
        return res, rows, senders

    def elect(self, leaders):
        """The election of node 1 of every cluster on the device: msgHup, the msgVote at the voters, the
        msgVoteResp at the candidates.  Returns the winners' first broadcast (emsg_out rows, senders)."""
        res, rows, senders = self.vote([dict(group=g, kind="hup", from_=1) for g in leaders])
        assert [r["action"] for r in res] == [L.VOTE_CAMPAIGNED] * len(leaders)
        assert len(rows) == len(leaders) * (self.nodes - 1) and all(int(r[0]) == 5 for r in rows)
        res, rows, senders = self.vote([dict(group=self.group_of(s, int(r[1])), kind=5, from_=int(r[2]), term=int(r[3]),
                                             index=int(r[5]), log_term=int(r[4])) for r, s in zip(rows, senders)])
        assert [r["action"] for r in res] == [L.VOTE_GRANTED] * len(rows) and all(int(r[0]) == 6 for r in rows)
        res, rows, senders = self.vote([dict(group=self.group_of(s, int(r[1])), kind=6, from_=int(r[2]), term=int(r[3]),
                                             reject=bool(int(r[17]) & 1)) for r, s in zip(rows, senders)])
        assert sum(r["action"] == L.VOTE_WON for r in res) == len(leaders) and sorted(set(senders)) == sorted(leaders)
        return rows, senders

    def propose(self, leaders, payloads):
        """One msgProp per leader group; returns (emsg_out rows, the sender group of each)."""
        locs, off = [], len(self.data)
        for g, p in zip(leaders, payloads):
            locs.append(dict(group=g, kind="prop", data_off=off, data_len=len(p)))
            off += len(p)
        self.data += b"".join(payloads)
        self.d["data"].free()
        self.d["data"] = R._up(self.ctx, np.frombuffer(self.data + b"\0" * (-len(self.data) % 8 + 8), dtype=np.uint64))
        d_loc, d_res = self.up(P.pack_locals(locs)), self.alloc(len(locs) * 48)
        args = (self.ctx, self.d["groups"], self.d["pstate"], self.G, self.d["snaps"], self.d["ents"], self.ne,
                len(self.data), d_loc, len(locs), d_res)
        total, napp = P.local_batch_device(*args)
        assert napp == len(locs)
        d_out = self.alloc(total * 144)
        P.local_batch_device(*args, d_out, total)
        res = P.results_from(d_res.download(len(locs) * 48), len(locs))
        rows = np.frombuffer(d_out.download(total * 144), dtype=np.uint64).reshape(total, K.MW).copy()
        senders = [g for g, r in zip(leaders, res) for _ in range(r["n_msgs"])]
        return rows, senders

    def follow(self, rows, senders, in_snaps=None, u64=None):
        """The follower step over leader-side emsg_out rows, d_src = d_ents, checked against the restatement.
        Returns (the restatement's dict, the stepped groups in record order)."""
        groups = [self.group_of(s, int(r[1])) for r, s in zip(rows, senders)]
        inrows, snaps, order = F.msgs_from_out(rows, groups)
        if in_snaps is not None:
            snaps = in_snaps
        u64 = np.zeros(0, dtype=np.uint64) if u64 is None else u64
        a = dict(self.arrays(), src=None, in_snaps=snaps, u64=u64, msgs=inrows)
        assert K.validate(a) == K.OK
        x = K.expected(a)
        n = len(inrows)
        d_in, d_sn, d_u, d_res = self.up(inrows), self.up(snaps), self.up(u64), self.alloc(n * 96)
        args = (self.ctx, self.d["groups"], self.d["pstate"], self.d["vstate"], self.d["rstate"], self.G,
                self.d["snaps"], self.d["ents"], self.ne, self.d["ents"], self.ne, d_sn, len(snaps), d_u, len(u64),
                d_in, n, d_res)
        total, na, nr = F.follow_batch_device(*args)
        d_out = self.alloc(total * 144)
        assert F.follow_batch_device(*args, d_out, total) == (x["n_msgs"], x["n_appended"], x["n_restored"])
        got = self.arrays()
        for k in self.shape:
            assert np.array_equal(got[k], x[k]), k
        assert np.array_equal(np.frombuffer(d_res.download(n * 96), dtype=np.uint64).reshape(n, K.OW), x["res_rows"])
        out = np.frombuffer(d_out.download(total * 144), dtype=np.uint64).reshape(total, K.MW)
        assert np.array_equal(out, x["msg_rows"])
        return x, [groups[i] for i in order]

    def lead_step(self, x):
        """The followers' msgAppResp at their leaders; returns (results, emsg_out rows, the sender group of each)."""
        resps = sorted((self.group_of(m["group"], m["to"]), k, m) for k, m in enumerate(x["messages"]))
        rrows = R.pack_resps([dict(group=g, from_=m["from_"], term=m["term"], index=m["index"], reject=m["reject"])
                              for g, _, m in resps])
        n = len(rrows)
        d_in, d_res = self.up(rrows), self.alloc(n * 48)
        args = (self.ctx, self.d["groups"], self.G, self.d["snaps"], self.d["ents"], self.ne, d_in, n, d_res)
        total, _ = R.lead_step_batch_device(*args)
        d_out = self.alloc(total * 144)
        R.lead_step_batch_device(*args, d_out, total)
        res = R.results_from(d_res.download(n * 48), n)
        rows = np.frombuffer(d_out.download(total * 144), dtype=np.uint64).reshape(total, K.MW).copy()
        senders = [g for (g, _, _), r in zip(resps, res) for _ in range(r["n_msgs"])]
        return res, rows, senders, d_out


@pytest.mark.parametrize("nodes", [3, 5])
def test_replication_chain(ctx, nodes):
    """On one set of arrays, from nodes as RestartNode leaves them: the
    election (evote_step_batch_device); the winners' first broadcast through
    msgs_from_out to every follower; the leaders propose and the fan-out's
    msgApp -- which re-send the election entry the followers already hold --
    reach the followers; their msgAppResp commit at the leaders; the next
    broadcast carries the commit; Ready, ewal_save_device and
    ewal_readall_device then find the leader's entries in every follower's WAL."""
    clusters = 6
    cl = Cluster(ctx, nodes, clusters)
    try:
        leaders = [c * nodes for c in range(clusters)]
        rows, senders = cl.elect(leaders)
        v = cl.get("vstate")
        # the followers voted for node 1 and know no leader yet; becomeLeader's reset cleared the winner's own Vote
        assert all([int(x) for x in v[k, :3]] == ([K.LEADER, 0, 1] if k % nodes == 0 else [K.FOLLOWER, 1, 0])
                   for k in range(cl.G))
        g = cl.get("groups")
        assert all(int(g[k, 1]) == 1 and int(g[k, 4]) == (2 if k % nodes == 0 else 1) for k in range(cl.G))
        # becomeLeader's entry: index 0, one entry each, nothing committed yet
        assert len(rows) == clusters * (nodes - 1) and all(int(r[0]) == 3 and int(r[8]) == 1 for r in rows)
        x, stepped = cl.follow(rows, senders)
        assert acts(x) == [(0, K.APPENDED)] * len(rows) and all(o["n_app"] == 1 for o in x["outcomes"])
        v = cl.get("vstate")
        assert all(int(v[k, 2]) == 1 for k in range(cl.G))     # lead, everywhere
        # their acknowledgements are lost; the leaders propose with next still at 1
        payloads = [b"proposal of cluster %d;" % c for c in range(clusters)]
        rows, senders = cl.propose(leaders, payloads)
        assert len(rows) == clusters * (nodes - 1) and all(int(r[0]) == 3 and int(r[8]) == 2 for r in rows)
        x, stepped = cl.follow(rows, senders)
        assert acts(x) == [(0, K.APPENDED)] * len(rows)
        assert all((o["conflict"], o["n_app"], o["last_index"]) == (2, 1, 2) for o in x["outcomes"])
        res, rows, senders, _ = cl.lead_step(x)
        assert sum(r["action"] == L.LEAD_COMMITTED for r in res) == clusters
        g = cl.get("groups")
        assert all(int(g[ld, 2]) == 2 for ld in leaders)
        x, stepped = cl.follow(rows, senders)
        assert all(a == (0, K.APPENDED) for a in acts(x)) and x["n_appended"] == 0
        g = cl.get("groups")
        assert sorted(stepped) == [k for k in range(cl.G) if k % nodes]
        assert all(int(g[k, 2]) == int(g[k - k % nodes, 2]) == 2 for k in range(cl.G))   # followers' committed
        # Ready over every group, then each follower's WAL
        G = cl.G
        d_res = cl.alloc(G * 96)
        rargs = (ctx, cl.d["groups"], cl.d["pstate"], cl.d["vstate"], cl.d["rstate"], G, cl.d["snaps"], cl.d["ents"],
                 cl.ne, None, G, d_res)
        n_save, n_ready = RD.ready_batch_device(*rargs)
        d_save = cl.alloc((n_save + 1) * 56)
        assert RD.ready_batch_device(*rargs, d_save, n_save) == (n_save, n_ready)
        res = RD.results_from(d_res.download(G * 96), G)
        saves = np.frombuffer(d_save.download(n_save * 56), dtype=np.uint64).reshape(n_save, 7)
        ents = cl.get("ents")
        cut = np.array([[RD.SAVE_CUT, 0, 0, 0, 0, 0, 1]], dtype=np.uint64)
        dout = cl.alloc(1 << 16)
        for k in range(G):
            if k % nodes == 0:
                continue
            r, ld = res[k], k - k % nodes
            assert r["status"] == L.OK and r["flags"] & L.READY_HARD and r["n_ents"] == 2
            assert (r["term"], r["vote"], r["commit"]) == (1, 1, 2)
            recs = np.concatenate([cut, saves[r["save_first"]:r["save_first"] + r["n_save"]]])
            drec = cl.up(recs)
            out_len, crc = C.c_uint64(), C.c_uint32()
            L.check(L.lib.ewal_save_device(ctx.handle, cl.d["data"].ptr, len(cl.data), drec.ptr, len(recs), 0, dout.ptr,
                                           1 << 16, C.byref(out_len), C.byref(crc), None))
            raw = dout.download(out_len.value)
            back = W.readall_device(dout, out_len.value, 1, host_view=memoryview(raw), with_ents=True)
            assert back.status == L.OK and back.last_crc == crc.value
            lead_ents = ents[int(g[ld, 5]) + 1:int(g[ld, 5]) + 3]
            assert [(e.Term, e.Index, e.Type, bytes(e.Data or b"")) for e in back.ents] == \
                [(int(e[0]), int(e[1]), int(e[4]) & 0xFFFFFFFF, cl.data[int(e[2]):int(e[2]) + int(e[3])])
                 for e in lead_ents]
            assert bytes(back.ents[1].Data) == payloads[k // nodes]
    finally:
        cl.free()


@pytest.mark.parametrize("nodes", [3, 5])
def test_slow_node_restore_chain(ctx, nodes):
    """TestSlowNodeRestore's assertions on the device.  The leader's
    compaction is forged: its log starts at offset 100 under a snapshot of
    index 100.  The slow node's rejection makes the leader probe and send a
    msgSnap; it goes through Marshal and Unmarshal on the device, then the
    follower step restores from it."""
    clusters = 4
    slow = nodes                                             # the last node never heard of anything
    u64 = np.array(list(range(1, nodes + 1)), dtype=np.uint64)
    snap = [100, 1, 0, 0, 0, nodes, 0, 0]
    cl = Cluster(ctx, nodes, clusters, leader_log=[1, 1, 1], offset=100, snaps=snap, slow=slow)
    try:
        G = cl.G
        g0 = cl.get("groups")
        for c in range(clusters):                           # the others are up to date; the slow node is probed at 100
            for p in range(1, nodes):
                g0[c * nodes, 14 + p], g0[c * nodes, 21 + p] = (102, 103) if p + 1 != slow else (0, 101)
        cl.d["groups"].upload(g0.tobytes())
        leaders = [c * nodes for c in range(clusters)]
        # the leader's msgApp at next - 1 == 100 reaches the slow node: rejected
        probe = np.zeros((clusters, K.MW), dtype=np.uint64)
        for c in range(clusters):
            probe[c, :9] = [3, slow, 1, 1, 1, 100, 102, 0, 0]
        x, stepped = cl.follow(probe, leaders)
        assert acts(x) == [(0, K.REJECTED)] * clusters and stepped == [ld + slow - 1 for ld in leaders]
        res, rows, senders, d_out = cl.lead_step(x)
        assert [r["action"] for r in res] == [L.LEAD_PROBE] * clusters
        assert all(int(r[0]) == 7 and [int(v) for v in r[9:17]] == snap for r in rows)
        # Marshal on the device, Unmarshal on the device
        d_u = cl.up(u64)
        eargs = (ctx, cl.d["data"], len(cl.data), d_out, len(rows), cl.d["ents"], cl.ne, d_u, len(u64))
        _, _, total = RM.encode_messages_device(*eargs, None, 0)
        d_wire = cl.alloc(total)
        offs, lens, total = RM.encode_messages_device(*eargs, d_wire, total)
        wire = d_wire.download(total)
        back = RM.decode_messages(ctx, [wire[o:o + n] for o, n in zip(offs, lens)])
        assert all(m["status"] == L.OK and m["type"] == 7 for m in back)
        in_u64, in_snaps, msgs = [], [], np.zeros((clusters, K.MW), dtype=np.uint64)
        for k, m in enumerate(back):
            s = m["snap"]
            in_snaps.append([s["index"], s["term"], 0, 0, len(in_u64), len(s["nodes"]), 0, 0])
            in_u64 += s["nodes"]
            msgs[k, :7] = [m["type"], m["to"], m["from_"], m["term"], m["log_term"], m["index"], m["commit"]]
            msgs[k, 9:17] = in_snaps[-1]
        x, stepped = cl.follow(msgs, senders, in_snaps=np.array(in_snaps, dtype=np.uint64),
                               u64=np.array(in_u64, dtype=np.uint64))
        assert acts(x) == [(0, K.RESTORED)] * clusters
        sn, g = cl.get("snaps"), cl.get("groups")
        for ld in leaders:
            f = ld + slow - 1
            assert [int(v) for v in sn[f][:2]] == [int(v) for v in sn[ld][:2]] == [100, 1]       # follower.snap == lead.snap
            assert [int(v) for v in in_u64[int(sn[f][4]):int(sn[f][4]) + int(sn[f][5])]] == list(range(1, nodes + 1))
            assert [int(v) for v in g[f][2:5]] == [100, 100, 1] and int(g[f][6]) == nodes
        # Ready on the restored followers: the snapshot, and nil rd.Entries
        sel = np.array([ld + slow - 1 for ld in leaders], dtype=np.uint64)
        d_sel, d_res = cl.up(sel), cl.alloc(len(sel) * 96)
        RD.ready_batch_device(ctx, cl.d["groups"], cl.d["pstate"], cl.d["vstate"], cl.d["rstate"], G, cl.d["snaps"],
                              cl.d["ents"], cl.ne, d_sel, len(sel), d_res)
        for r in RD.results_from(d_res.download(len(sel) * 96), len(sel)):
            assert r["status"] == L.OK and r["flags"] & L.READY_SNAP and (r["ents_first"], r["n_ents"]) == (0, 0)
        # the follower's response moves the leader's progress; its broadcast brings the rest of the log
        res, rows, senders, _ = cl.lead_step(x)
        assert all((r["match"], r["next"]) == (100, 101) for r in res)
        if len(rows):
            x, _ = cl.follow(rows, senders)
        # one more proposal: accepted by the restored follower; after the acknowledgements it commits everywhere
        rows, senders = cl.propose(leaders, [b"after the snapshot %d;" % c for c in range(clusters)])
        x, stepped = cl.follow(rows, senders)
        slow_outs = [o for o, s in zip(x["outcomes"], stepped) if s % nodes == slow - 1]
        assert all((o["status"], o["action"]) == (0, K.APPENDED) and o["last_index"] == 103 for o in slow_outs)
        res, rows, senders, _ = cl.lead_step(x)
        x, _ = cl.follow(rows, senders)
        g = cl.get("groups")
        for ld in leaders:
            assert int(g[ld + slow - 1, 2]) == int(g[ld, 2]) == 103                              # committed
    finally:
        cl.free()
