"""The checker of the batched log compaction (ecompact_batch_device): a
restatement of node.Compact (raft/node.go:226-227, 325-330), that is
raft.compact (raft/raft.go:522-531) with raftLog.term, raftLog.snap,
raftLog.compact, raftLog.shouldCompact and isOutOfAppliedBounds (raft/log.go:
119-124, 156-183, 219-224), written from the Go text on Python ints masked to
64 bits and on a log that really is a list of entries (Go's reslice is Python's
slice: no positions, no move classes), pinned by the reference's own tables
(tests/golden/raft_compact_kats.json).  It works on the call's packed rows, so
what it returns is compared word for word.  at, slice, isOutOfBounds and
lastIndex are follow_cases.Log's, the group builder is follow_cases.Scenario:
neither is restated here.  The scenario builders and the generator are shared
by the host and GPU tests."""
import json
import os

import numpy as np

import follow_cases as K
from follow_cases import M64, Panic, SplitMix, _fold, _w

OK, PANIC_BOUNDS, PANIC_COMPACT_APPLIED, PANIC_COMPACT_BOUNDS, UNSUPPORTED = 0, 33, 45, 46, 48
E_INVAL = -1                       # the call's own verdict (validate); the library's code is the tests' to map
STATUSES = (OK, PANIC_BOUNDS, PANIC_COMPACT_APPLIED, PANIC_COMPACT_BOUNDS, UNSUPPORTED)
NOT_STEPPED, NOT_DUE, COMPACTED, PANICKED = range(4)
AT_APPLIED = 1
MOVE_NONE, MOVE_DISJOINT, MOVE_OVERLAP = range(3)
CANARY = K.CANARY
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raft_compact_kats.json")
GW, SW, RW, NW, EW, QW, OW = 32, 4, 8, 8, 5, 12, 8   # words per record
DEFAULT_COMPACT_THRESHOLD = 10000                     # raft/log.go:10-12


class Log(K.Log):
    """follow_cases.Log with the compaction's functions."""

    def term(self, i):   # log.go:119-124
        e = self.at(i)
        if e is not None:
            return e[0]
        return 0

    def compact(self, i):   # log.go:161-169
        if self.is_out_of_applied_bounds(i):
            raise Panic(PANIC_COMPACT_BOUNDS)
        self.ents = self.slice(i, (self.last_index() + 1) & M64)
        self.unstable = max((i + 1) & M64, self.unstable)
        self.offset = i
        return len(self.ents)

    def snap(self, d, index, term, nodes, removed):   # log.go:171-179; the three slices as (off, len) ranges
        self.snapshot = [index, term, d[0], d[1], nodes[0], nodes[1], removed[0], removed[1]]

    def should_compact(self, threshold):   # log.go:181-183
        return ((self.applied - self.offset) & M64) > threshold

    def is_out_of_applied_bounds(self, i):   # log.go:219-224
        return i < self.offset or i > self.applied


def raft_compact(log, index, nodes, d, removed):   # raft.go:522-531; removed: r.removedNodes(), the caller's
    if index > log.applied:
        raise Panic(PANIC_COMPACT_APPLIED)
    log.snap(d, index, log.term(index), nodes, removed)
    log.compact(index)


def request(log, q):
    """One ecompact_req (its 12 words) on the log.  Returns (status, action);
    after a panic, or where Go's slice came out nil, the log is not to be used."""
    index = q[2]
    if q[1] & AT_APPLIED:
        if not log.should_compact(q[3]):
            return OK, NOT_DUE
        index = log.applied   # EtcdServer.snapshot, etcdserver/server.go:562-571
    try:
        raft_compact(log, index, (q[6], q[7]), (q[4], q[5]), (q[8], q[9]))
    except Panic as p:
        return p.status, PANICKED
    if not log.ents:
        return UNSUPPORTED, PANICKED   # Go is left with a zero-length log: reported, never guessed
    return OK, COMPACTED


# ---- one call on packed rows ---------------------------------------------------

def validate(a):
    """The device's checks before anything is modified: OK or E_INVAL."""
    G = len(a["groups"])
    seen = set()
    for q in a["reqs"]:
        q = _w(q)
        g = q[0]
        if g >= G or g in seen or (q[1] & ~AT_APPLIED) or q[10] or q[11] or ((q[1] & AT_APPLIED) and q[2] != 0):
            return E_INVAL
        seen.add(g)
        for off, ln, total in ((q[4], q[5], a["data_len"]), (q[6], q[7], a["n_u64"]), (q[8], q[9], a["n_u64"])):
            if ln > total or off > total - ln:
                return E_INVAL
        w, s = _w(a["groups"][g]), _w(a["pstate"][g])
        cap, nlog, npeers = s[0], w[4], w[6]
        if any(w[28:32]) or s[3] != 0 or s[2] > 1 or cap > len(a["ents"]) or w[5] > len(a["ents"]) - cap or nlog > cap:
            return E_INVAL
        if any(w[7 + j] == w[7 + k] for j in range(min(npeers, K.PEERS)) for k in range(j)):
            return E_INVAL
    return OK


def move_class(n_left, shift):
    if shift == 0 or n_left == 0:
        return MOVE_NONE
    return MOVE_DISJOINT if shift >= n_left else MOVE_OVERLAP


def expected(a):
    """What a successful call leaves: res_rows, groups, pstate, snaps, ents,
    n_compacted, n_moved and outcomes (per request dicts, with the move class).
    rstate is never written.  A peek leaves the inputs and gives the same
    res_rows and counters."""
    grows, srows, snaprows, erows = a["groups"].copy(), a["pstate"].copy(), a["snaps"].copy(), a["ents"].copy()
    n = len(a["reqs"])
    res = np.zeros((n, OW), dtype=np.uint64)
    outcomes, n_compacted, n_moved = [], 0, 0
    for i in range(n):
        q = _w(a["reqs"][i])
        g = q[0]
        w, s, rd = _w(grows[g]), _w(srows[g]), _w(a["rstate"][g])
        efirst, off0, nlog0 = w[5], w[3], w[4]
        log = Log([_w(e) for e in erows[efirst:efirst + nlog0]], off0, w[2], s[1], rd[6])
        status, action = request(log, q)
        o = dict(status=status, action=action, group=g, index=0, term=0, n_left=0, shift=0, src_first=0, dst_first=0,
                 unstable=0, cls=MOVE_NONE)
        if action == COMPACTED:
            shift = (log.offset - off0) & M64
            o.update(index=log.snapshot[0], term=log.snapshot[1], n_left=len(log.ents), shift=shift,
                     src_first=efirst + shift, dst_first=efirst, unstable=log.unstable,
                     cls=move_class(len(log.ents), shift))
            grows[g, 3:5] = np.array([log.offset, len(log.ents)], dtype=np.uint64)
            srows[g, 1] = np.uint64(log.unstable)
            snaprows[g] = np.array(log.snapshot, dtype=np.uint64)
            for k, e in enumerate(log.ents):           # the window slides: the room comes back
                erows[efirst + k] = np.array(e, dtype=np.uint64)
            n_compacted += 1
            n_moved += len(log.ents) if shift else 0
        outcomes.append(o)
        res[i] = np.array([status | (action << 32), o["index"], o["term"], o["n_left"], o["shift"], o["src_first"],
                           o["dst_first"], o["unstable"]], dtype=np.uint64)
    return dict(res_rows=res, groups=grows, pstate=srows, rstate=a["rstate"], snaps=snaprows, ents=erows,
                n_compacted=n_compacted, n_moved=n_moved, outcomes=outcomes)


# ---- scenario builder ------------------------------------------------------------

def req(group, index=0, at_applied=False, threshold=0, data=(0, 0), nodes=(0, 0), removed=(0, 0), flags=0):
    return [group, flags | (AT_APPLIED if at_applied else 0), index, threshold, data[0], data[1], nodes[0], nodes[1],
            removed[0], removed[1], 0, 0]


def call_of(sc, reqs, data_len=0, n_u64=0):
    """The call's arrays (a dict of uint64 row arrays) of a follow_cases.Scenario's
    groups and the request rows."""
    p = sc.pack()
    return dict(groups=p["groups"], pstate=p["pstate"], rstate=p["rstate"], snaps=p["snaps"], ents=p["ents"],
                reqs=np.array(reqs, dtype=np.uint64).reshape(-1, QW), data_len=data_len, n_u64=n_u64)


def after(a, x, reqs):
    """The next call on what the call a left (x: expected's or the device's arrays)."""
    return dict(a, groups=x["groups"], pstate=x["pstate"], snaps=x["snaps"], ents=x["ents"],
                reqs=np.array(reqs, dtype=np.uint64).reshape(-1, QW))


# ---- the reference's tables ---------------------------------------------------------

def load_kats():
    with open(KATS) as f:
        return json.load(f)


def compaction_play():
    """TestCompaction: one group per row, the successive compactions as
    successive calls.  Returns (the first call's arrays without requests, rounds):
    round j is [(group, index, wleft)] of the rows that get there."""
    sc = K.Scenario()
    rows = load_kats()["TestCompaction"]
    for t in rows:
        # newLog's dummy entry and lastIndex appended Entry{}; maybeCommit(applied, 0); resetNextEnts
        sc.add_group([0] * (t["lastIndex"] + 1), [(1, 0, 1)], committed=t["applied"], applied=t["applied"], unstable=0,
                     room=3)
    rounds = []
    for j in range(max(len(t["compact"]) for t in rows)):
        rounds.append([(g, t["compact"][j], t["wleft"][j]) for g, t in enumerate(rows)
                       if j < len(t["compact"]) and -1 not in t["wleft"][:j]])
    return call_of(sc, []), rounds


def side_effects_call():
    """TestCompactionSideEffects: (the call's arrays, the table)."""
    t = load_kats()["TestCompactionSideEffects"]
    n = t["lastIndex"]
    sc = K.Scenario()
    log = [K.entry(0)] + [K.entry(i + 1, i + 1) for i in range(n)]
    sc.add_group(log, [(1, 0, 1)], term=n, committed=n, applied=n, unstable=0, room=4)
    return call_of(sc, [req(0, t["compact"])]), t


def compact_table_call():
    """TestCompact: one group per row.  Returns (the call's arrays, the rows,
    the data bytes, the u64 values)."""
    t = load_kats()["TestCompact"]
    sc = K.Scenario()
    data, u64, reqs = b"", [], []
    for g, row in enumerate(t["rows"]):
        sc.add_group(t["log_terms"], [(1, 0, 1)], committed=t["committed"], applied=t["applied"], state=K.LEADER, room=2)
        d = row["snapd"].encode()
        nodes, removed = (len(u64), len(row["nodes"])), (len(u64) + len(row["nodes"]), len(row["removed"]))
        u64 += row["nodes"] + row["removed"]
        reqs.append(req(g, row["compacti"], data=(len(data), len(d)), nodes=nodes, removed=removed))
        data += d
    return call_of(sc, reqs, len(data), len(u64)), t["rows"], data, u64


def check_tables():
    """The restatement on every table of raft_compact_kats.json that needs no
    other call (TestNodeCompact and TestProvideSnap's Ready and msgSnap halves
    are the GPU tests'); raises AssertionError."""
    a, rounds = compaction_play()
    for rnd in rounds:
        a = after(a, a, [req(g, index) for g, index, _ in rnd])
        assert validate(a) == OK
        x = expected(a)
        for (g, index, wleft), o in zip(rnd, x["outcomes"]):
            if wleft < 0:
                assert o["action"] == PANICKED and o["status"] in (PANIC_COMPACT_APPLIED, PANIC_COMPACT_BOUNDS), (g, o)
            else:
                assert (o["action"], o["n_left"], int(x["groups"][g][4])) == (COMPACTED, wleft, wleft), (g, o)
        a = after(a, x, [])
    a, t = side_effects_call()
    x = expected(a)
    w, s = _w(x["groups"][0]), _w(x["pstate"][0])
    assert x["outcomes"][0]["action"] == COMPACTED and K.last_index_of(w) == t["wlastIndex"]
    log = Log([_w(e) for e in x["ents"][w[5]:w[5] + w[4]]], w[3], w[2], s[1], 0)
    assert all(log.term(i) == i and log.match_term(i, i) for i in range(log.offset, log.last_index() + 1))
    unstable = log.slice(log.unstable, log.last_index() + 1)
    assert len(unstable) == t["wunstable_len"] and unstable[0][1] == t["wunstable_first_index"]
    log.append(log.last_index(), [K.entry(log.last_index() + 1)])
    assert log.last_index() == t["wlastIndex_after_append"] and len(log.slice(log.last_index(), log.last_index() + 1)) == 1
    a, rows, data, u64 = compact_table_call()
    x = expected(a)
    for g, (row, o) in enumerate(zip(rows, x["outcomes"])):
        assert (o["action"] == PANICKED) == row["wpanic"], (g, o)
        if row["wpanic"]:
            assert o["status"] == PANIC_COMPACT_APPLIED and not x["snaps"][g].any()
            continue
        sn = _w(x["snaps"][g])
        assert int(x["groups"][g][3]) == sn[0] == row["compacti"] and sn[1] == 1
        assert data[sn[2]:sn[2] + sn[3]].decode() == row["snapd"]
        assert u64[sn[4]:sn[4] + sn[5]] == row["nodes"] and u64[sn[6]:sn[6] + sn[7]] == row["removed"]
    return True


# ---- the generator the host program restates draw for draw ------------------------------

OFF_TABLE = (0, 0, 5, 1000, M64 - 7, 0)
NLOG_TABLE = (0, 1, 2, 3, 6, 9, 20, 70)
ROOM = 4
DATA_LEN, N_U64 = 200, 16


def draw(seed, run):
    """One random request on its group: (group kwargs for Scenario.add_group, request kwargs)."""
    r = SplitMix(seed, run)
    off = OFF_TABLE[r.rnd(6)]
    nlog = NLOG_TABLE[r.rnd(8)]
    t = 1 + r.rnd(3)
    terms = []
    for _ in range(nlog):
        t += 1 if r.rnd(3) == 0 else 0
        terms.append(t)
    last = (off + nlog - 1) & M64
    amode = r.rnd(8)
    if amode == 0:
        applied = (off - 1 - r.rnd(2)) & M64
    elif amode == 1:
        applied = (last + 1 + r.rnd(3)) & M64
    else:
        applied = (off + r.rnd(nlog + 1)) & M64
    unstable = (off + r.rnd(nlog + 3)) & M64
    grp = dict(log=terms, prs=[(1, 0, 1)], term=t, committed=applied, log_offset=off, room=ROOM, unstable=unstable,
               applied=applied, state=K.LEADER)
    at = r.rnd(3) == 0
    index = threshold = 0
    if at:
        tmode = r.rnd(4)
        threshold = (0, (applied - off) & M64, (applied - off - 1) & M64, DEFAULT_COMPACT_THRESHOLD)[tmode]
    else:
        imode = r.rnd(8)
        index = ((applied + 1) & M64, (off - 1) & M64, off, applied)[imode] if imode < 4 else (off + r.rnd(nlog + 1)) & M64
    data = (r.rnd(100), r.rnd(50))
    nodes = (r.rnd(8), r.rnd(4))
    removed = (r.rnd(8), r.rnd(3))
    return grp, dict(index=index, at_applied=at, threshold=threshold, data=data, nodes=nodes, removed=removed)


def random_scenario(seed, groups, named, idle_every=0):
    """`groups` drawn groups; the first `named` of a seeded shuffle get their
    drawn request, in shuffled order (so requests and groups are not aligned).
    idle_every: a garbage group that no request names before every such group."""
    import random
    sc = K.Scenario()
    rng = random.Random(seed)
    drawn = []
    for j in range(groups):
        if idle_every and j % idle_every == 0:
            sc.add_idle(rng)
        grp, q = draw(seed, j)
        drawn.append((sc.add_group(**grp), q))
    rng.shuffle(drawn)
    return call_of(sc, [req(g, **q) for g, q in drawn[:named]], DATA_LEN, N_U64)


def mix_of(outcomes):
    """(per-action counts, per-status counts, per-move-class counts of the compacted ones)."""
    acts, stats, cls = [0] * 4, {s: 0 for s in STATUSES}, [0] * 3
    for o in outcomes:
        acts[o["action"]] += 1
        stats[o["status"]] += 1
        if o["action"] == COMPACTED:
            cls[o["cls"]] += 1
    return acts, [stats[s] for s in STATUSES], cls


def digest(seed, runs):
    """(digest, per-action counts, per-status counts, per-class counts) of the
    host program tests/host/compact_forms.cpp, from the restatement alone."""
    h = 0xCBF29CE484222325
    outs = []
    for j in range(runs):
        sc = K.Scenario()
        grp, q = draw(seed, j)
        g = sc.add_group(**grp)
        x = expected(call_of(sc, [req(g, **q)], DATA_LEN, N_U64))
        o = x["outcomes"][0]
        outs.append(o)
        for v in (o["status"], o["action"], o["index"], o["term"], o["n_left"], o["shift"], o["unstable"], o["cls"]):
            h = _fold(h, v)
        gw = _w(x["groups"][g])
        for v in gw[3:5] + [int(x["pstate"][g][1])] + _w(x["snaps"][g]):
            h = _fold(h, v)
        for e in x["ents"][gw[5]:gw[5] + int(x["pstate"][g][0])]:     # the log and the window's free slots
            h = _fold(h, int(e[0]))
    return (h,) + mix_of(outs)
