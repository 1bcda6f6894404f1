"""The checker of the batched follower step (efollow_step_batch_device): a
restatement of raft.Step's term switch (raft/raft.go:393-405), the msgApp and
msgSnap cases of stepFollower (:504-510) and stepCandidate (:476-481),
handleAppendEntries (:410-416), handleSnapshot (:418-424), raft.restore
(:535-554), reset / becomeFollower (:260-273, :309-315) and, from raft/log.go,
maybeAppend, findConflict, append, matchTerm, at, slice, isOutOfBounds,
lastIndex and restore, written from the Go text on Python ints masked to 64
bits and on a log that really is a list of entries (no overlay, no positions
arithmetic: Go's slices as Python's), pinned by the reference's own tables
(tests/golden/raft_follow_kats.json).  It works on the call's packed rows, so
what it returns is compared word for word; the scenario builders and
generators are shared by the host and GPU tests."""
import json
import os

import numpy as np

M64 = (1 << 64) - 1
OK, PANIC_BOUNDS, PANIC_COMMITTED_CONFLICT, UNSUPPORTED = 0, 33, 38, 48
E_INVAL, E_NOMEM = -1, -2          # the call's own verdicts (validate); the library's codes are the tests' to map
STATUSES = (OK, PANIC_BOUNDS, PANIC_COMMITTED_CONFLICT, UNSUPPORTED)
(NOT_STEPPED, IGNORED, NO_CASE, APPENDED, REJECTED, RESTORED, SNAP_STALE, DEFERRED, PANICKED) = range(9)
MSG_APP, MSG_SNAP, MSG_APP_RESP = 3, 7, 4
FOLLOWER, CANDIDATE, LEADER = 0, 1, 2
NONE = 0
PEERS, MAX_NODES = 7, 64
CANARY = 0xC0FFEE00DEADBEEF
NIL_ENTRY_WORD = 1 << 32           # type 0, data_nil 1
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raft_follow_kats.json")
GW, SW, VW, RW, NW, EW, IW, OW, MW = 32, 4, 8, 8, 8, 5, 12, 12, 18   # words per record


class Panic(Exception):
    def __init__(self, status):
        super().__init__(status)
        self.status = status


class Log:
    """raftLog: ents a list of 5-word entries [term, index, data_off, data_len, type | data_nil << 32]."""

    def __init__(self, ents, offset, committed, unstable, applied):
        self.ents, self.offset, self.committed, self.unstable, self.applied = ents, offset, committed, unstable, applied
        self.snapshot = None
        self.ci, self.app_k, self.n_app, self.dst_pos = 0, 0, 0, 0   # instrumentation of the last maybeAppend

    def maybe_append(self, index, log_term, committed, ents):   # log.go:49-69
        lastnewi = (index + len(ents)) & M64
        if self.match_term(index, log_term):
            frm = (index + 1) & M64
            ci = self.find_conflict(frm, ents)
            if ci == 0:
                pass
            elif ci <= self.committed:
                raise Panic(PANIC_COMMITTED_CONFLICT)
            else:
                k = (ci - frm) & M64
                if k > len(ents):
                    raise Panic(PANIC_BOUNDS)
                self.append((ci - 1) & M64, ents[k:])
                self.ci, self.app_k, self.n_app = ci, k, len(ents) - k
                self.dst_pos = len(self.ents) - self.n_app
            tocommit = min(committed, lastnewi)
            if self.committed < tocommit:
                self.committed = tocommit
            return True
        return False

    def append(self, after, ents):   # log.go:71-75
        self.ents = self.slice(self.offset, (after + 1) & M64) + [list(e) for e in ents]
        self.unstable = min(self.unstable, (after + 1) & M64)
        return self.last_index()

    def find_conflict(self, frm, ents):   # log.go:77-84
        for i, ne in enumerate(ents):
            oe = self.at((frm + i) & M64)
            if oe is None or oe[0] != ne[0]:
                return (frm + i) & M64
        return 0

    def last_index(self):   # log.go:115-117
        return (len(self.ents) - 1 + self.offset) & M64

    def match_term(self, i, term):   # log.go:141-146
        e = self.at(i)
        if e is not None:
            return e[0] == term
        return False

    def restore(self, s):   # log.go:185-192; s: the eight elead_snap words
        self.ents = [[s[1], 0, 0, 0, NIL_ENTRY_WORD]]
        self.unstable = (s[0] + 1) & M64
        self.committed = s[0]
        self.applied = s[0]
        self.offset = s[0]
        self.snapshot = list(s)

    def at(self, i):   # log.go:194-199
        if self.is_out_of_bounds(i):
            return None
        k = (i - self.offset) & M64
        if k >= len(self.ents):
            raise Panic(PANIC_BOUNDS)   # Go indexes past ents
        return self.ents[k]

    def slice(self, lo, hi):   # log.go:202-210
        if lo >= hi:
            return []
        if self.is_out_of_bounds(lo) or self.is_out_of_bounds((hi - 1) & M64):
            return []
        a, b = (lo - self.offset) & M64, (hi - self.offset) & M64
        if a > b or b > len(self.ents):
            raise Panic(PANIC_BOUNDS)
        return self.ents[a:b]

    def is_out_of_bounds(self, i):   # log.go:212-217
        return i < self.offset or i > self.last_index()


class Raft:
    """raft with what a msgApp or a msgSnap touches.  prs is the record's seven
    slots (pid, match, next) with n_peers saying how many are keys; votes is
    keyed by peer id."""

    def __init__(self, id_, term, log, n_peers, pid, match, nxt, pending_conf, state, vote, lead, elapsed, votes,
                 soft_dirty):
        self.id, self.term, self.log, self.np = id_, term, log, n_peers
        self.pid, self.match, self.next = list(pid), list(match), list(nxt)
        self.pending_conf, self.state, self.vote, self.lead, self.elapsed = pending_conf, state, vote, lead, elapsed
        self.votes, self.soft_dirty = dict(votes), soft_dirty
        self.msgs, self.restored_from = [], None

    def send(self, to, index, reject=False):   # raft.go:190-199
        self.msgs.append(dict(type=MSG_APP_RESP, to=to, from_=self.id, term=self.term, index=index, reject=reject))

    def reset(self, term):   # raft.go:260-273
        self.term = term
        self.lead = NONE
        self.vote = NONE
        self.elapsed = 0
        self.votes = {}
        for k in range(min(self.np, PEERS)):
            self.match[k], self.next[k] = 0, (self.log.last_index() + 1) & M64
            if self.pid[k] == self.id:
                self.match[k] = self.log.last_index()
        self.pending_conf = 0

    def become_follower(self, term, lead):   # raft.go:309-315
        self.reset(term)
        self.lead = lead
        self.state = FOLLOWER

    def handle_append_entries(self, m):   # raft.go:410-416
        if self.log.maybe_append(m["index"], m["log_term"], m["commit"], m["ents"]):
            self.send(m["from_"], self.log.last_index())
            return APPENDED
        self.send(m["from_"], m["index"], True)
        return REJECTED

    def handle_snapshot(self, m):   # raft.go:418-424
        if self.restore(m["snapshot"], m["nodes"]):
            self.restored_from = m["snap"]
            self.send(m["from_"], self.log.last_index())
            return RESTORED
        self.send(m["from_"], self.log.committed)
        return SNAP_STALE

    def restore(self, s, nodes):   # raft.go:535-554
        if s[0] <= self.log.committed:
            return False
        # the library's limits: reported, never guessed
        distinct = list(dict.fromkeys(nodes))
        if len(nodes) > MAX_NODES or len(distinct) > PEERS or self.votes:
            raise Panic(UNSUPPORTED)
        self.log.restore(s)
        before = (self.np, self.pid[:len(distinct)])
        self.pid, self.match, self.next = [0] * PEERS, [0] * PEERS, [0] * PEERS
        for k, n in enumerate(distinct):   # r.prs = make(map); setProgress per node, in slot order
            last = self.log.last_index()
            self.pid[k], self.match[k], self.next[k] = n, (last if n == self.id else 0), (last + 1) & M64
        self.np = len(distinct)
        if (self.np, self.pid[:self.np]) != before:
            self.soft_dirty = 1
        return True

    def Step(self, m):   # raft.go:372-408 with stepFollower / stepCandidate / stepLeader; returns (action, flags)
        flags = 0
        if m["term"] == 0:
            pass
        elif m["term"] > self.term:
            self.become_follower(m["term"], m["from_"])
            flags |= 1
        elif m["term"] < self.term:
            return IGNORED, 0
        if self.state == LEADER:
            return NO_CASE, flags
        if self.state == CANDIDATE:
            if m["kind"] == MSG_APP:
                self.become_follower(self.term, m["from_"])
                return self.handle_append_entries(m), flags | 2
            self.become_follower(m["term"], m["from_"])
            return self.handle_snapshot(m), flags | 2
        self.elapsed = 0
        if m["kind"] == MSG_APP:
            self.lead = m["from_"]
            return self.handle_append_entries(m), flags
        return self.handle_snapshot(m), flags

    def saved(self):
        lg = self.log
        return ([list(e) for e in lg.ents], lg.offset, lg.committed, lg.unstable, lg.applied, lg.snapshot, self.term,
                self.np, list(self.pid), list(self.match), list(self.next), self.pending_conf, self.state, self.vote,
                self.lead, self.elapsed, dict(self.votes), self.soft_dirty, self.restored_from)

    def put_back(self, b):
        lg = self.log
        (lg.ents, lg.offset, lg.committed, lg.unstable, lg.applied, lg.snapshot, self.term, self.np, self.pid,
         self.match, self.next, self.pending_conf, self.state, self.vote, self.lead, self.elapsed, self.votes,
         self.soft_dirty, self.restored_from) = b


def step(r, m):
    """One message on r.  Returns (status, action, flags, messages, log
    instrumentation); a panic leaves r as it was and sends nothing."""
    before = r.saved()
    r.msgs = []
    r.log.ci = r.log.app_k = r.log.n_app = r.log.dst_pos = 0
    try:
        action, flags = r.Step(m)
    except Panic as p:
        r.put_back(before)
        r.msgs = []
        return p.status, PANICKED, 0, [], (0, 0, 0, 0)
    lg = r.log
    return OK, action, flags, r.msgs, (lg.ci, lg.app_k, lg.n_app, lg.dst_pos)


# ---- one call on packed rows ---------------------------------------------------

def _w(row):
    return [int(x) for x in row]


def validate(a):
    """The device's checks before anything is modified: OK, E_INVAL or E_NOMEM."""
    G, n = len(a["groups"]), len(a["msgs"])
    src = a["ents"] if a["src"] is None else a["src"]
    inval = nomem = False
    seen, prev, of = set(), None, {}
    for i in range(n):
        m = _w(a["msgs"][i])
        g = m[0]
        of.setdefault(g, []).append(m)
        bad = g >= G or m[11] != 0 or m[1] not in (MSG_APP, MSG_SNAP) or m[8] > len(src) or m[7] > len(src) - m[8]
        if not bad and m[1] == MSG_SNAP:
            bad = a["rstate"] is None or a["snaps"] is None or m[10] >= len(a["in_snaps"])
            if not bad:
                s = _w(a["in_snaps"][m[10]])
                bad = s[5] > len(a["u64"]) or s[4] > len(a["u64"]) - s[5]
        inval |= bad
        if g != prev:
            inval |= g in seen
            seen.add(g)
            prev = g
    for g in seen:
        if g >= G:
            continue
        w, s, v = _w(a["groups"][g]), _w(a["pstate"][g]), _w(a["vstate"][g])
        cap, nlog, npeers = s[0], w[4], w[6]
        bad = any(w[28:32]) or s[3] != 0 or s[2] > 1 or cap > len(a["ents"]) or w[5] > len(a["ents"]) - cap or nlog > cap
        bad |= any(w[7 + j] == w[7 + k] for j in range(min(npeers, PEERS)) for k in range(j))
        mask = (1 << min(npeers, PEERS)) - 1
        bad |= any(v[6:8]) or v[0] > 2 or ((v[4] | v[5]) & ~mask) != 0 or (v[5] & ~v[4]) != 0
        inval |= bad
        for m in of[g]:
            nomem |= (m[1] == MSG_APP and nlog <= cap and m[8] > cap - nlog) or (m[1] == MSG_SNAP and cap == 0)
    return E_INVAL if inval else E_NOMEM if nomem else OK


def expected(a):
    """What a successful call leaves: a dict like raftfollow.follow_batch's
    (res_rows, msg_rows, groups, pstate, vstate, rstate, snaps, ents, n_msgs,
    n_appended, n_restored) plus outcomes (per record dicts) and messages."""
    grows, srows, vrows = a["groups"].copy(), a["pstate"].copy(), a["vstate"].copy()
    rrows = None if a["rstate"] is None else a["rstate"].copy()
    snaprows = None if a["snaps"] is None else a["snaps"].copy()
    erows = a["ents"].copy()
    src = a["ents"] if a["src"] is None else a["src"]     # the source as the call found it
    n = len(a["msgs"])
    res = np.zeros((n, OW), dtype=np.uint64)
    rows, outcomes, messages = [], [], []
    n_appended = n_restored = 0
    i = 0
    while i < n:
        g = int(a["msgs"][i][0])
        w, s, v = _w(grows[g]), _w(srows[g]), _w(vrows[g])
        rd = _w(rrows[g]) if rrows is not None else [0] * RW
        efirst = w[5]
        log = Log([_w(e) for e in erows[efirst:efirst + w[4]]], w[3], w[2], s[1], rd[6])
        slots = min(w[6], PEERS)
        votes = {w[7 + k]: bool(v[5] >> k & 1) for k in range(slots) if v[4] >> k & 1}
        r = Raft(w[0], w[1], log, w[6], w[7:14], w[14:21], w[21:28], s[2], v[0], v[1], v[2], v[3], votes, rd[7])
        stopped = deferring = grown = False
        writes = []
        while i < n and int(a["msgs"][i][0]) == g:
            m = _w(a["msgs"][i])
            ents = [_w(e) for e in src[m[7]:m[7] + m[8]]]
            for e in ents:
                if e[4] >> 32 == 0:
                    e[2] = (e[2] + m[9]) & M64
            msg = dict(kind=m[1], from_=m[2], term=m[3], index=m[4], log_term=m[5], commit=m[6], ents=ents, snap=m[10])
            if m[1] == MSG_SNAP:
                sn = _w(a["in_snaps"][m[10]])
                msg.update(snapshot=sn, nodes=[int(x) for x in a["u64"][sn[4]:sn[4] + sn[5]]])
            flags, msgs, ins = 0, [], (0, 0, 0, 0)
            if stopped:
                status, action = OK, NOT_STEPPED
            elif w[6] > PEERS:
                status, action = UNSUPPORTED, PANICKED
            elif deferring or (grown and (m[8] > 0 or m[1] == MSG_SNAP)):
                status, action, deferring = OK, DEFERRED, True
            else:
                status, action, flags, msgs, ins = step(r, msg)
            stopped = stopped or status != OK
            ci, app_k, n_app, dst_pos = ins
            if n_app:
                grown = True
                writes.append((efirst + dst_pos, [list(e) for e in r.log.ents[dst_pos:dst_pos + n_app]]))
                n_appended += n_app
            if action == RESTORED:
                grown = True
                writes.append((efirst, [list(r.log.ents[0])]))
                n_restored += 1
            o = dict(status=status, action=action, msg_first=len(rows), n_msgs=len(msgs), conflict=ci,
                     app_first=m[7] + app_k if n_app else 0, n_app=n_app, dst_first=efirst + dst_pos if n_app else 0,
                     last_index=r.log.last_index(), committed=r.log.committed, term=r.term, state=r.state, flags=flags,
                     group=g)
            outcomes.append(o)
            res[i] = np.array([status | (action << 32), o["msg_first"], o["n_msgs"], ci, o["app_first"], n_app,
                               o["dst_first"], o["last_index"], o["committed"], r.term, r.state | (flags << 32), 0],
                              dtype=np.uint64)
            for x in msgs:
                rows.append([x["type"], x["to"], x["from_"], x["term"], 0, x["index"]] + [0] * 11 + [int(x["reject"])])
                messages.append(dict(x, group=g))
            i += 1
        if w[6] > PEERS:
            continue
        lg = r.log
        grows[g, 1:5] = np.array([r.term, lg.committed, lg.offset, len(lg.ents)], dtype=np.uint64)
        grows[g, 6] = np.uint64(r.np)
        grows[g, 7:28] = np.array(r.pid + r.match + r.next, dtype=np.uint64)
        srows[g, 1:3] = np.array([lg.unstable, r.pending_conf], dtype=np.uint64)
        voted = granted = 0
        for k in range(min(r.np, PEERS)):
            if r.pid[k] in r.votes:
                voted |= 1 << k
                granted |= (1 << k) if r.votes[r.pid[k]] else 0
        vrows[g, :6] = np.array([r.state, r.vote, r.lead, r.elapsed, voted, granted], dtype=np.uint64)
        if r.restored_from is not None:
            rrows[g, 6:8] = np.array([lg.applied, r.soft_dirty], dtype=np.uint64)
            snaprows[g] = np.array(lg.snapshot, dtype=np.uint64)
        for first, ents in writes:
            for k, e in enumerate(ents):
                erows[first + k] = np.array(e, dtype=np.uint64)
    return dict(res_rows=res, msg_rows=np.array(rows, dtype=np.uint64).reshape(len(rows), MW), groups=grows,
                pstate=srows, vstate=vrows, rstate=rrows, snaps=snaprows, ents=erows, n_msgs=len(rows),
                n_appended=n_appended, n_restored=n_restored, outcomes=outcomes, messages=messages)


# ---- scenario builder ------------------------------------------------------------

def entry(term, index=0, data_off=0, data_len=0, type_=0, data_nil=1):
    return [term & M64, index & M64, data_off & M64, data_len & M64, (type_ & 0xFFFFFFFF) | (data_nil << 32)]


class Scenario:
    """Groups with their windows and side records, a source array and one
    call's messages.  same_array: the messages' entries live in d_ents itself,
    in a region past every window."""

    def __init__(self, same_array=False, rstate=True, snaps=True):
        self.same_array, self.with_rstate, self.with_snaps = same_array, rstate, snaps
        self.g, self.s, self.v, self.r, self.sn, self.windows = [], [], [], [], [], []
        self.src, self.in_snaps, self.u64, self.msgs = [], [], [], []

    def add_group(self, log, prs, gid=None, term=1, committed=0, log_offset=0, n_peers=None, room=2, unstable=None,
                  pending_conf=0, state=FOLLOWER, vote=NONE, lead=NONE, elapsed=0, voted=0, granted=0, applied=0,
                  soft_dirty=0, snap=None, rstate=None):
        """log: terms, or 5-word entries.  prs: (id, match, next) per slot."""
        ents = [e if isinstance(e, list) else entry(e, log_offset + k) for k, e in enumerate(log)]
        row = [gid if gid is not None else (prs[0][0] if prs else 1), term, committed, log_offset, len(ents), 0,
               len(prs) if n_peers is None else n_peers] + [0] * 25
        for k, (p, m, x) in enumerate(prs[:PEERS]):
            row[7 + k], row[14 + k], row[21 + k] = p, m, x
        self.g.append([x & M64 for x in row])
        self.s.append([len(ents) + room, (log_offset + len(ents)) & M64 if unstable is None else unstable,
                       pending_conf, 0])
        self.v.append([state, vote, lead, elapsed, voted, granted, 0, 0])
        rs = [0] * RW
        rs[6], rs[7] = applied, soft_dirty
        for k, x in (rstate or {}).items():
            rs[k] = x
        self.r.append(rs)
        self.sn.append(list(snap) if snap else [0] * NW)
        self.windows.append(ents)
        return len(self.g) - 1

    def add_idle(self, rng):
        """A group that no record names: garbage in every record."""
        g = self.add_group([1], [(1, 0, 1)], room=0)
        self.g[g] = [rng.getrandbits(64) for _ in range(GW)]
        self.g[g][4], self.g[g][5] = 1, 0
        self.s[g] = [1] + [rng.getrandbits(64) for _ in range(SW - 1)]
        self.v[g] = [rng.getrandbits(64) for _ in range(VW)]
        self.r[g] = [rng.getrandbits(64) for _ in range(RW)]
        self.sn[g] = [rng.getrandbits(64) for _ in range(NW)]
        return g

    def add_app(self, group, from_=0, term=0, index=0, log_term=0, commit=0, ents=(), data_delta=0, gap=1):
        """ents: terms or 5-word entries; they go to the source array, `gap` canary entries after them."""
        first = len(self.src)
        for k, e in enumerate(ents):
            self.src.append(e if isinstance(e, list) else entry(e, index + 1 + k))
        self.src += [[CANARY] * EW] * (gap if ents else 0)
        self.msgs.append([group, MSG_APP, from_, term, index, log_term, commit, first if ents else 0, len(ents),
                          data_delta, 0, 0])

    def add_snap(self, group, from_=0, term=0, index=0, snap_term=0, nodes=(), data=(0, 0), removed=()):
        nodes_off = len(self.u64)
        self.u64 += list(nodes)
        removed_off = len(self.u64)
        self.u64 += list(removed)
        self.in_snaps.append([index, snap_term, data[0], data[1], nodes_off, len(nodes), removed_off, len(removed)])
        self.msgs.append([group, MSG_SNAP, from_, term, 0, 0, 0, 0, 0, 0, len(self.in_snaps) - 1, 0])

    def pack(self):
        """The call's arrays as a dict of uint64 row arrays (validate / expected / the GPU tests take it)."""
        g = np.array(self.g, dtype=np.uint64).reshape(-1, GW)
        ents, first = [], 0
        for k, (win, s) in enumerate(zip(self.windows, self.s)):
            g[k, 5] = np.uint64(first)
            ents += [[x & M64 for x in e] for e in win] + [[CANARY] * EW] * (s[0] - len(win))
            first += s[0]
        src = np.array(self.src, dtype=np.uint64).reshape(-1, EW)
        msgs = np.array(self.msgs, dtype=np.uint64).reshape(-1, IW)
        if self.same_array:
            for m in msgs:
                if int(m[8]):
                    m[7] += np.uint64(first)
            ents += [list(e) for e in self.src]
        return dict(groups=g, pstate=np.array(self.s, dtype=np.uint64).reshape(-1, SW),
                    vstate=np.array(self.v, dtype=np.uint64).reshape(-1, VW),
                    rstate=np.array(self.r, dtype=np.uint64).reshape(-1, RW) if self.with_rstate else None,
                    snaps=np.array(self.sn, dtype=np.uint64).reshape(-1, NW) if self.with_snaps else None,
                    ents=np.array(ents, dtype=np.uint64).reshape(-1, EW), src=None if self.same_array else src,
                    in_snaps=np.array(self.in_snaps, dtype=np.uint64).reshape(-1, NW),
                    u64=np.array(self.u64, dtype=np.uint64), msgs=msgs)


# ---- the reference's tables ---------------------------------------------------------

def load_kats():
    with open(KATS) as f:
        return json.load(f)


def kat_scenario(idle=0):
    """The single-node tables of raft_follow_kats.json, one group each,
    interleaved with `idle` garbage groups.  Returns (scenario, [(name, group,
    want dict)])."""
    import random
    k = load_kats()
    sc = Scenario()
    rng = random.Random(12)
    named = []

    def group(*args, **kw):
        for _ in range(idle):
            sc.add_idle(rng)
        return sc.add_group(*args, **kw)

    t = k["TestHandleMsgApp"]
    for j, c in enumerate(t["cases"]):
        g = group(t["log_terms"], [(1, 0, 1)], gid=1, term=t["term"], committed=t["committed"], state=t["state"],
                  room=3)
        # the table calls handleAppendEntries directly, past Step's term switch (rows 7 and 8 carry Term 1 < 2):
        # a local message (Term 0) is how a record gets there
        sc.add_app(g, from_=2, term=0, index=c["index"], log_term=c["log_term"], commit=c["commit"], ents=c["ents"])
        named.append(("TestHandleMsgApp_%d" % j, g, dict(last_index=c["windex"], committed=c["wcommit"],
                                                         reject=c["wreject"])))
    t = k["TestAllServerStepdown"]
    for j, c in enumerate(t["cases"]):
        s, m = c["start"], t["msg"]
        g = group(s["log_terms"], s["prs"], gid=t["id"], term=s["term"], state=s["state"], vote=s["vote"],
                  lead=s["lead"])
        sc.add_app(g, from_=m["from"], term=m["term"], log_term=m["log_term"])
        named.append(("TestAllServerStepdown_%d" % j, g, dict(state=c["wstate"], term=c["wterm"], nlog=c["windex"],
                                                              lead=c["wlead"])))
    t = k["TestStepIgnoreOldTermMsg"]
    g = group([0], [(p, 0, 1) for p in t["peers"]], gid=t["id"], term=t["term"])
    sc.add_app(g, term=t["msg"]["term"])
    named.append(("TestStepIgnoreOldTermMsg", g, dict(action=IGNORED)))
    t = k["TestRestore"]
    s = t["snapshot"]
    g = group([0], [(p, 0, 1) for p in t["peers"]], gid=t["id"], term=0)
    sc.add_snap(g, from_=2, index=s["index"], snap_term=s["term"], nodes=s["nodes"], removed=s["removed"])
    sc.add_snap(g, from_=2, index=s["index"], snap_term=s["term"], nodes=s["nodes"], removed=s["removed"])
    named.append(("TestRestore", g, dict(restore=t, actions=[RESTORED, DEFERRED])))
    g = group([s["term"]], [(p, 0, s["index"] + 1) for p in s["nodes"]], gid=t["id"], term=0, log_offset=s["index"],
              committed=s["index"], applied=s["index"])
    sc.add_snap(g, from_=2, index=s["index"], snap_term=s["term"], nodes=s["nodes"], removed=s["removed"])
    named.append(("TestRestore_second", g, dict(action=SNAP_STALE)))
    t = k["TestRestoreFromSnapMsg"]
    s, m = t["snapshot"], t["msg"]
    g = group([0], [(p, 0, 1) for p in t["peers"]], gid=t["id"], term=0)
    sc.add_snap(g, from_=m["from"], term=m["term"], index=s["index"], snap_term=s["term"], nodes=s["nodes"])
    named.append(("TestRestoreFromSnapMsg", g, dict(snapshot=s, action=RESTORED)))
    t = k["TestCandidateConcede"]
    s = t["start"]
    g = group(s["log_terms"], [(p, 0, 1) for p in t["peers"]], gid=t["id"], term=s["term"], state=s["state"],
              vote=s["vote"], voted=1, granted=1, room=4)
    for m in t["msgs"]:
        sc.add_app(g, from_=m["from"], term=m["term"], index=m["index"], log_term=m["log_term"], commit=m["commit"],
                   ents=m["ents"])
    named.append(("TestCandidateConcede", g, dict(state=t["wstate"], term=t["wterm"], log_terms=t["wlog_terms"],
                                                  committed=t["wcommitted"])))
    t = k["TestLogRestore"]
    g = group([0] + [i + 1 for i in range(t["n_appended"])], [(1, 0, 1), (2, 0, 1)], gid=1, term=0, room=0)
    sc.add_snap(g, from_=2, index=t["index"], snap_term=t["term"], nodes=[1, 2])
    named.append(("TestLogRestore", g, dict(log_restore=t)))
    return sc, named


def check_kats(sc, named, a=None, x=None):
    """The tables' wanted values against the outcomes of expected()."""
    a = a or sc.pack()
    x = x or expected(a)
    assert validate(a) == OK
    first = {}
    for i, o in enumerate(x["outcomes"]):
        first.setdefault(o["group"], i)
    for name, g, w in named:
        i = first[g]
        n = sum(1 for m in sc.msgs if m[0] == g)
        outs = x["outcomes"][i:i + n]
        last = outs[-1]
        msgs = [m for m in x["messages"] if m["group"] == g]
        gw, vw, sw = _w(x["groups"][g]), _w(x["vstate"][g]), _w(x["pstate"][g])
        assert all(o["status"] == OK for o in outs), name
        if "reject" in w:
            assert len(msgs) == 1 and msgs[0]["reject"] == w["reject"] and msgs[0]["type"] == MSG_APP_RESP, name
            assert last["last_index"] == w["last_index"] and last["committed"] == w["committed"] == gw[2], name
        if "action" in w:
            assert last["action"] == w["action"], name
        if "actions" in w:
            assert [o["action"] for o in outs] == w["actions"], name
        if "state" in w:
            assert (vw[0], gw[1]) == (w["state"], w["term"]) == (last["state"], last["term"]), name
        if "nlog" in w:
            assert gw[4] == w["nlog"] and vw[2] == w["lead"], name
        if "log_terms" in w:
            assert [int(e[0]) for e in x["ents"][gw[5]:gw[5] + gw[4]]] == w["log_terms"] and gw[2] == w["committed"], name
        if "restore" in w:
            t = w["restore"]
            assert last_index_of(gw) == t["wlast_index"] and int(x["ents"][gw[5]][0]) == t["wlast_term"], name
            assert sorted(gw[7:7 + gw[6]]) == t["wnodes"], name
            sn = _w(x["snaps"][g])
            assert sn[:2] == [t["snapshot"]["index"], t["snapshot"]["term"]], name
            assert [int(v) for v in a["u64"][sn[4]:sn[4] + sn[5]]] == t["snapshot"]["nodes"], name
            assert [int(v) for v in a["u64"][sn[6]:sn[6] + sn[7]]] == t["snapshot"]["removed"], name
        if "snapshot" in w:
            sn = _w(x["snaps"][g])
            assert sn[:2] == [w["snapshot"]["index"], w["snapshot"]["term"]], name
            assert [int(v) for v in a["u64"][sn[4]:sn[4] + sn[5]]] == w["snapshot"]["nodes"], name
        if "log_restore" in w:
            t = w["log_restore"]
            assert (gw[4], gw[3], gw[2], sw[1]) == (t["wlen"], t["woffset"], t["wcommitted"], t["wunstable"]), name
            assert int(x["rstate"][g][6]) == t["wapplied"] and int(x["ents"][gw[5]][0]) == t["wterm"], name


def last_index_of(gw):
    return (gw[4] - 1 + gw[3]) & M64


# ---- the generator the host program restates draw for draw ------------------------------

class SplitMix:
    def __init__(self, seed, run):
        self.x = (seed * 0x9E3779B97F4A7C15 + run) & M64

    def next(self):
        self.x = (self.x + 0x9E3779B97F4A7C15) & M64
        z = self.x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    def rnd(self, n):
        return self.next() % n


NP_TABLE = (1, 2, 3, 3, 3, 3, 5, 5, 7, 3, 2, 3, 3, 5, 0, 8)
OFF_TABLE = (0, 0, 5, 1000, M64 - 7, 0)
STATE_TABLE = (0, 0, 0, 0, 1, 1, 2, 0)
NE_TABLE = (0, 0, 0, 1, 1, 2, 3, 5)
NN_TABLE = (1, 2, 3, 3, 5, 9, 9, 65)
RG_TABLE = (40, 40, 40, 3, 40, 40, 6, 40)


def draw(seed, run):
    """One random run: (group kwargs for Scenario.add_group, [message dicts])."""
    r = SplitMix(seed, run)
    np_ = NP_TABLE[r.rnd(16)]
    slots = min(np_, PEERS)
    off = OFF_TABLE[r.rnd(6)]
    nlog = r.rnd(8)
    t = 1 + r.rnd(3)
    terms = []
    for _ in range(nlog):
        t += 1 if r.rnd(3) == 0 else 0
        terms.append(t)
    term = t + r.rnd(2)
    committed = (off + (r.rnd(nlog + 1) if r.rnd(2) else 0)) & M64
    pid = [10 + 3 * k + r.rnd(3) for k in range(slots)]
    me = r.rnd(slots) if slots else 0
    gid = pid[me] if slots else 10
    if r.rnd(5) == 0:
        gid = 999
    prs = []
    for k in range(slots):
        match = (off + r.rnd(nlog + 1)) & M64
        prs.append((pid[k], match, (match + 1) & M64))
    state = STATE_TABLE[r.rnd(8)]
    vote = r.rnd(2) * 77
    lead = r.rnd(2) * gid
    elapsed = r.rnd(10)
    voted = granted = 0
    if state == CANDIDATE:
        voted = r.next() & ((1 << slots) - 1)
        granted = voted & r.next()
    elif r.rnd(16) == 0 and slots:
        voted = 1
    unstable = (off + r.rnd(nlog + 3)) & M64
    pending = r.rnd(2)
    applied = r.rnd(4)
    soft_dirty = r.rnd(2)
    grp = dict(log=terms, prs=prs, gid=gid, term=term, committed=committed, log_offset=off, n_peers=np_, room=8,
               unstable=unstable, pending_conf=pending, state=state, vote=vote, lead=lead, elapsed=elapsed, voted=voted,
               granted=granted, applied=applied, soft_dirty=soft_dirty)
    cur = term
    msgs = []
    for _ in range(1 + r.rnd(5)):
        kind = MSG_SNAP if r.rnd(4) == 0 else MSG_APP
        from_ = 55
        if slots:
            if r.rnd(8):
                from_ = pid[r.rnd(slots)]
        rel = r.rnd(8)
        mterm = 0 if rel == 0 else (cur - 1) & M64 if rel == 1 else cur + 2 if rel == 7 else \
            cur + (1 if r.rnd(4) == 0 else 0)
        cur = max(cur, mterm)
        if kind == MSG_APP:
            index = (off + r.rnd(nlog + 2)) & M64
            pos = (index - off) & M64
            mode = r.rnd(4)
            log_term = terms[pos] if mode != 0 and pos < nlog else r.rnd(t + 2)
            ne = NE_TABLE[r.rnd(8)]
            ents = []
            for k in range(ne):
                p = pos + 1 + k
                ents.append(terms[p] if p < nlog and r.rnd(4) else t + r.rnd(2))
            commit = (off + r.rnd(nlog + 4)) & M64
            msgs.append(dict(kind=kind, from_=from_, term=mterm, index=index, log_term=log_term, commit=commit,
                             ents=ents))
        else:
            sindex = (committed + r.rnd(4) - 1) & M64
            sterm = 1 + r.rnd(5)
            j = r.rnd(8)
            nodes = [gid if r.rnd(4) == 0 else 10 + r.rnd(RG_TABLE[j]) for _ in range(NN_TABLE[j])]
            msgs.append(dict(kind=kind, from_=from_, term=mterm, index=sindex, snap_term=sterm, nodes=nodes))
    return grp, msgs


def add_run(sc, grp, msgs, data_delta=0):
    g = sc.add_group(**grp)
    for m in msgs:
        if m["kind"] == MSG_APP:
            sc.add_app(g, from_=m["from_"], term=m["term"], index=m["index"], log_term=m["log_term"],
                       commit=m["commit"], ents=m["ents"], data_delta=data_delta)
        else:
            sc.add_snap(g, from_=m["from_"], term=m["term"], index=m["index"], snap_term=m["snap_term"],
                        nodes=m["nodes"])
    return g


def random_scenario(seed, runs, same_array=False, idle_every=0, data_delta=0):
    import random
    sc = Scenario(same_array=same_array)
    rng = random.Random(seed)
    for j in range(runs):
        if idle_every and j % idle_every == 0:
            sc.add_idle(rng)
        add_run(sc, *draw(seed, j), data_delta=data_delta)
    return sc


def _fold(h, v):
    return ((h ^ (v & M64)) * 0x100000001B3) & M64


def digest(seed, runs):
    """(digest, per-action counts, per-status counts, records) of the host
    program tests/host/follow_forms.cpp, from the restatement alone."""
    h = 0xCBF29CE484222325
    acts, stats, records = [0] * 9, {s: 0 for s in STATUSES}, 0
    for j in range(runs):
        sc = Scenario()
        g = add_run(sc, *draw(seed, j))
        a = sc.pack()
        x = expected(a)
        for o in x["outcomes"]:
            acts[o["action"]] += 1
            stats[o["status"]] += 1
            records += 1
            for v in (o["status"], o["action"], o["flags"], o["n_msgs"], o["conflict"], o["n_app"],
                      o["dst_first"], o["last_index"], o["committed"], o["term"], o["state"]):
                h = _fold(h, v)
        for m in x["messages"]:
            for v in (m["to"], m["from_"], m["term"], m["index"], int(m["reject"])):
                h = _fold(h, v)
        gw = _w(x["groups"][g])
        for v in gw[1:5] + gw[6:28] + _w(x["pstate"][g])[1:3] + _w(x["vstate"][g])[:6] + _w(x["rstate"][g])[6:8]:
            h = _fold(h, v)
        for e in x["ents"][gw[5]:gw[5] + gw[4]]:
            h = _fold(h, int(e[0]))
    return h, acts, [stats[s] for s in STATUSES], records
