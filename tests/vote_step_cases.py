"""The checker of the batched election step (evote_step_batch_device):
lead_prop_cases.Raft extended with raft.Step for msgHup, msgVote and
msgVoteResp (raft/raft.go:372-408), the msgVote cases of the three step
functions (:467-468, :482-483, :511-518), stepCandidate's msgVoteResp case
(:484-492), campaign (:358-370), poll (:177-187), reset (:260-273),
becomeFollower / becomeCandidate / becomeLeader (:309-349) and
raftLog.isUpToDate (raft/log.go:136-139), written from the Go text on Python
ints masked to 64 bits, pinned by the reference's own tables
(tests/golden/raft_vote_kats.json), and the scenario builders and generators
the host and GPU tests share."""
import json
import os
import random

import numpy as np

from etcd_amd import raftlead as R
from etcd_amd import raftprop as P
from etcd_amd import raftvote as V

import lead_step_cases as K
import lead_prop_cases as PC
from lead_step_cases import (M64, OK, PANIC_BOUNDS, PANIC_FIRST_ENTRY, PANIC_NEED_SNAPSHOT,  # noqa: F401
                             PANIC_NIL_PROGRESS, UNSUPPORTED, CANARY, MSG_APP, MSG_SNAP, Panic)

PANIC_LEADER_TO_CANDIDATE, PANIC_NIL_ENTRY, PANIC_DOUBLE_CONF = 42, 43, 44
STATUSES = (OK, PANIC_BOUNDS, PANIC_NIL_PROGRESS, PANIC_NEED_SNAPSHOT, PANIC_FIRST_ENTRY, PANIC_LEADER_TO_CANDIDATE,
            PANIC_NIL_ENTRY, PANIC_DOUBLE_CONF, UNSUPPORTED)     # every status a record of this call can get
NOT_STEPPED, IGNORED, GRANTED, REJECTED, CAMPAIGNED, WON, LOST, POLLED, NO_CASE, PANICKED = range(10)
MSG_HUP, MSG_VOTE, MSG_VOTE_RESP = 0, 5, 6
FOLLOWER, CANDIDATE, LEADER = 0, 1, 2
NONE = 0
CONF_CHANGE = 1
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raft_vote_kats.json")


class Raft(PC.Raft):
    """raft with what an election touches: state, Vote, lead, elapsed, votes,
    and the entries' types (position for position with log.ents)."""

    def __init__(self, id_, term, log, prs, snapshot=None, pending_conf=False, types=None, state=FOLLOWER, vote=NONE,
                 lead=NONE, elapsed=0, votes=None):
        super().__init__(id_, term, log, prs, snapshot, pending_conf)
        self.types = list(types) if types is not None else [0] * len(log.ents)
        self.state, self.vote, self.lead, self.elapsed = state, vote, lead, elapsed
        self.votes = dict(votes or {})
        self.appended = None   # (position, term, index) of the entry the last step appended

    def poll(self, id_, v):   # raft.go:177-187
        if id_ not in self.votes:
            self.votes[id_] = v
        return sum(1 for vv in self.votes.values() if vv)

    def reset(self, term):   # raft.go:260-273
        self.term = term
        self.lead = NONE
        self.vote = NONE
        self.elapsed = 0
        self.votes = {}
        for p, pr in self.prs:
            pr.match, pr.next = 0, (self.log.last_index() + 1) & M64
            if p == self.id:
                pr.match = self.log.last_index()
        self.pending_conf = False

    def become_follower(self, term, lead):   # raft.go:309-315
        self.reset(term)
        self.lead = lead
        self.state = FOLLOWER

    def become_candidate(self):   # raft.go:317-327
        if self.state == LEADER:
            raise Panic(PANIC_LEADER_TO_CANDIDATE)
        self.reset((self.term + 1) & M64)
        self.vote = self.id
        self.state = CANDIDATE

    def become_leader(self):   # raft.go:329-349
        assert self.state != FOLLOWER   # "invalid transition [follower -> leader]": Step never gets here
        self.reset(self.term)
        self.lead = self.id
        self.state = LEADER
        got = self.log.entries((self.log.committed + 1) & M64)
        if got is not None:
            for p in range(got[0], got[0] + got[1]):
                if self.types[p] != CONF_CHANGE:
                    continue
                if self.pending_conf:
                    raise Panic(PANIC_DOUBLE_CONF)
                self.pending_conf = True
        index, pos = self.append_entry()
        self.types = [0] if pos == 0 else self.types[:pos] + [0]
        self.appended = (pos, self.term, index)

    def campaign(self):   # raft.go:358-370
        self.become_candidate()
        if self.pr(self.id) is None:
            raise Panic(UNSUPPORTED)   # the library's: the self vote has no slot in the mask
        if self.q() == self.poll(self.id, True):
            self.become_leader()
        for p, _ in self.prs:
            if p == self.id:
                continue
            lasti = self.log.last_index()
            self.send(dict(to=p, type=MSG_VOTE, index=lasti, log_term=self.log.term(lasti), commit=0, ents=None,
                           snap=None))

    def is_up_to_date(self, i, term):   # log.go:136-139
        e = self.log.at(self.log.last_index())
        if e is None:
            raise Panic(PANIC_NIL_ENTRY)
        return term > e or (term == e and i >= self.log.last_index())

    def vote_resp(self, to, reject):
        self.send(dict(to=to, type=MSG_VOTE_RESP, index=0, log_term=0, commit=0, ents=None, snap=None, reject=reject))

    def step_follower(self, m):   # raft.go:511-518
        if m["kind"] == MSG_VOTE:
            if (self.vote == NONE or self.vote == m["from_"]) and self.is_up_to_date(m["index"], m["log_term"]):
                self.elapsed = 0
                self.vote = m["from_"]
                self.vote_resp(m["from_"], False)
                return GRANTED
            self.vote_resp(m["from_"], True)
            return REJECTED
        return NO_CASE

    def step_candidate(self, m):   # raft.go:482-492
        if m["kind"] == MSG_VOTE:
            self.vote_resp(m["from_"], True)
            return REJECTED
        if m["kind"] == MSG_VOTE_RESP:
            if self.pr(m["from_"]) is None:
                raise Panic(UNSUPPORTED)   # the library's: Go would count it, the mask cannot
            gr = self.poll(m["from_"], not m["reject"])
            if self.q() == gr:
                self.become_leader()
                self.bcast_append()
                return WON
            if self.q() == len(self.votes) - gr:
                self.become_follower(self.term, NONE)
                return LOST
            return POLLED
        return NO_CASE

    def step_leader(self, m):   # raft.go:467-468
        if m["kind"] == MSG_VOTE:
            self.vote_resp(m["from_"], True)
            return REJECTED
        return NO_CASE

    def Step(self, m):   # raft.go:372-408; returns (action, flags)
        flags = 0
        if m["kind"] == MSG_HUP:
            self.campaign()
            return (WON if self.state == LEADER else CAMPAIGNED), 0   # m.Term == 0; no step function has the case
        if m["term"] == 0:
            pass
        elif m["term"] > self.term:
            lead = m["from_"]
            if m["kind"] == MSG_VOTE:
                lead = NONE
            self.become_follower(m["term"], lead)
            flags = 1
        elif m["term"] < self.term:
            return IGNORED, 0
        return (self.step_follower, self.step_candidate, self.step_leader)[self.state](m), flags

    def snapshot_of(self):
        return (list(self.log.ents), list(self.types), self.log.committed, self.log.unstable, self.pending_conf,
                self.term, self.state, self.vote, self.lead, self.elapsed, dict(self.votes),
                [(pr.match, pr.next) for _, pr in self.prs])

    def restore(self, b):
        (self.log.ents, self.types, self.log.committed, self.log.unstable, self.pending_conf, self.term, self.state,
         self.vote, self.lead, self.elapsed, self.votes) = b[:11]
        for (_, pr), (m, n) in zip(self.prs, b[11]):
            pr.match, pr.next = m, n


def step(r, m):
    """One election message on r.  Returns (status, action, flags, messages);
    a panic leaves r as it was and sends nothing.  r.appended names the entry
    the step appended, if any."""
    before = r.snapshot_of()
    r.msgs = []
    r.appended = None
    try:
        action, flags = r.Step(m)
    except Panic as p:
        r.restore(before)
        r.msgs = []
        r.appended = None
        return p.status, PANICKED, 0, []
    return OK, action, flags, r.msgs


def masks_of(r):
    """(voted, granted) of r.votes over r's peer slots."""
    voted = granted = 0
    for k, (p, _) in enumerate(r.prs):
        if p in r.votes:
            voted |= 1 << k
            granted |= (1 << k) if r.votes[p] else 0
    return voted, granted


def msg_row(m, ents_first):
    row = K.msg_row(m, ents_first)
    row[17] = 1 if m.get("reject") else 0
    return row


def load_kats():
    with open(KATS) as f:
        return json.load(f)


class Scenario:
    """Groups with their logs, their two state records and one call's election
    messages; packs the device arrays and computes, with the restatement, every
    array the call leaves."""

    def __init__(self, snaps=True):
        self.groups, self.logs, self.snaps, self.state, self.vstate, self.msgs = [], [], [], [], [], []
        self.garbage = {}
        self.with_snaps = snaps

    def add_group(self, log, prs, gid=None, term=1, committed=0, log_offset=0, snap=None, n_peers=None, room=2,
                  unstable=None, pending_conf=0, state=FOLLOWER, vote=NONE, lead=NONE, elapsed=0, voted=0, granted=0):
        """log: a list of terms, or of dicts (term, type)."""
        g = len(self.groups)
        grp = dict(id=gid if gid is not None else prs[0][0], term=term, committed=committed, log_offset=log_offset,
                   prs=[tuple(p) for p in prs])
        if n_peers is not None:
            grp["n_peers"] = n_peers
        self.groups.append(grp)
        self.logs.append([e if isinstance(e, dict) else dict(term=e) for e in log])
        self.snaps.append(snap)
        self.state.append(dict(ents_cap=len(log) + room, pending_conf=pending_conf,
                               unstable=(log_offset + len(log)) & M64 if unstable is None else unstable))
        self.vstate.append(dict(state=state, vote=vote, lead=lead, elapsed=elapsed, voted=voted, granted=granted))
        return g

    def add_idle(self, rng):
        """A group that no record names: garbage in all three records, reserved words included."""
        g = self.add_group([1], [(1, 0, 1)], room=0)
        self.garbage[g] = [rng.getrandbits(64) for _ in range(R.GROUP_WORDS + P.STATE_WORDS + V.VSTATE_WORDS)]
        return g

    def add_msg(self, group, kind, from_=0, term=0, index=0, log_term=0, reject=False):
        self.msgs.append(dict(group=group, kind=kind, from_=from_, term=term, index=index, log_term=log_term,
                              reject=bool(reject)))

    def add_hup(self, group):
        self.add_msg(group, MSG_HUP, from_=self.groups[group]["id"])

    def pack(self):
        """(group rows (G, 32), state rows (G, 4), vote-state rows (G, 8), snap
        rows (G, 8) or None, entry rows with the canary in every free slot,
        message rows (n, 8))."""
        logs = [[dict(term=e["term"], index=(grp.get("log_offset", 0) + k) & M64, type=e.get("type", 0))
                 for k, e in enumerate(log)] for grp, log in zip(self.groups, self.logs)]
        grows, erows = P.pack_logs(self.groups, logs, self.state)
        first = 0
        for log, st in zip(self.logs, self.state):
            erows[first + len(log):first + st["ents_cap"]] = np.uint64(CANARY)
            first += st["ents_cap"]
        strows, vrows = P.pack_state(self.state), V.pack_vstate(self.vstate)
        for g, words in self.garbage.items():
            grows[g] = np.array(words[:32], dtype=np.uint64)
            strows[g] = np.array(words[32:36], dtype=np.uint64)
            vrows[g] = np.array(words[36:], dtype=np.uint64)
        srows = R.pack_snaps(self.snaps) if self.with_snaps else None
        return grows, strows, vrows, srows, erows, V.pack_msgs(self.msgs)

    def raft_of(self, g, grows, strows, vrows):
        w = [int(x) for x in grows[g]]
        v = [int(x) for x in vrows[g]]
        log = K.LeaderLog([e["term"] for e in self.logs[g]], w[3], w[2])
        log.unstable = int(strows[g, 1])
        prs = [(w[7 + k], w[14 + k], w[21 + k]) for k in range(min(w[6], R.MAX_PEERS))]
        votes = {p: bool(v[5] >> k & 1) for k, (p, _, _) in enumerate(prs) if v[4] >> k & 1}
        return Raft(w[0], w[1], log, prs, self.snaps[g] if self.with_snaps else None, pending_conf=int(strows[g, 2]),
                    types=[e.get("type", 0) for e in self.logs[g]], state=v[0], vote=v[1], lead=v[2], elapsed=v[3],
                    votes=votes)

    def expected(self):
        """(results (n, 6), groups (G, 32), state (G, 4), vote state (G, 8),
        entries, messages (n_msgs, 18)) as uint64 arrays: the bytes a
        successful call leaves.  Also sets outcomes, messages (dicts), runs,
        rafts (per run: the restatement's final object), n_msgs, n_won."""
        grows, strows, vrows, _, erows, _ = self.pack()
        n = len(self.msgs)
        res = np.zeros((n, V.RESULT_WORDS), dtype=np.uint64)
        rows, self.outcomes, self.messages, self.runs, self.rafts = [], [], [], [], {}
        i = 0
        while i < n:
            g = self.msgs[i]["group"]
            r = self.raft_of(g, grows, strows, vrows)
            unsupported = int(grows[g, 6]) > R.MAX_PEERS
            efirst = int(grows[g, 5])
            stopped = False
            self.runs.append((g, i))
            while i < n and self.msgs[i]["group"] == g:
                flags, appended = 0, None
                if stopped:
                    status, action, msgs = OK, NOT_STEPPED, []
                elif unsupported:
                    status, action, msgs = UNSUPPORTED, PANICKED, []
                else:
                    status, action, flags, msgs = step(r, self.msgs[i])
                    appended = r.appended
                    if appended is not None:
                        pos, term, index = appended
                        erows[efirst + pos] = np.array([term, index, 0, 0, 1 << 32], dtype=np.uint64)
                stopped = stopped or status != OK
                o = dict(status=status, action=action, msg_first=len(rows), n_msgs=len(msgs), term=r.term, vote=r.vote,
                         state=r.state, flags=flags, appended=appended)
                self.outcomes.append(o)
                res[i] = np.array([status | (action << 32), o["msg_first"], o["n_msgs"], r.term, r.vote,
                                   r.state | (flags << 32)], dtype=np.uint64)
                rows += [msg_row(x, efirst) for x in msgs]
                self.messages += [dict(x, group=g) for x in msgs]
                i += 1
            self.rafts[g] = r
            if not unsupported:
                grows[g, 1], grows[g, 2] = np.uint64(r.term), np.uint64(r.log.committed)
                grows[g, 4] = np.uint64(len(r.log.ents))
                for k, (_, pr) in enumerate(r.prs):
                    grows[g, 14 + k], grows[g, 21 + k] = np.uint64(pr.match), np.uint64(pr.next)
                strows[g, 1], strows[g, 2] = np.uint64(r.log.unstable), np.uint64(int(r.pending_conf))
                voted, granted = masks_of(r)
                vrows[g, :6] = np.array([r.state, r.vote, r.lead, r.elapsed, voted, granted], dtype=np.uint64)
        self.n_msgs = len(rows)
        self.n_won = sum(1 for o in self.outcomes if o["action"] == WON)
        return res, grows, strows, vrows, erows, np.array(rows, dtype=np.uint64).reshape(len(rows), R.MSG_WORDS)


# ---- the reference's tables --------------------------------------------------

def _fresh(peers, id_):
    """newRaft(id, peers): a one-entry log (the dummy), becomeFollower(0, None)."""
    return dict(log=[0], prs=[(p, 0, 1) for p in peers], gid=id_, term=0)


def kat_scenario(idle=0):
    """The single-group tables of raft_vote_kats.json (TestLeaderElection is
    played by play_election), one group each, interleaved with `idle` garbage
    groups that get no record.  Returns (scenario, [(name, group, want)])."""
    k = load_kats()
    sc = Scenario()
    rng = random.Random(11)
    named = []

    def idle_some():
        for _ in range(idle):
            sc.add_idle(rng)

    t = k["TestRecvMsgVote"]
    for j, c in enumerate(t["cases"]):
        idle_some()
        g = sc.add_group(t["log_terms"], [(p, 0, 1) for p in t["peers"]], gid=t["id"], term=0, state=c["state"],
                         vote=c["vote_for"])
        sc.add_msg(g, MSG_VOTE, from_=t["from"], index=c["i"], log_term=c["term"])
        named.append(("TestRecvMsgVote_%d" % j, g, dict(reject=c["wreject"], n_msgs=1)))
    t = k["TestAllServerStepdown"]
    for j, c in enumerate(t["cases"]):
        idle_some()
        s = c["start"]
        g = sc.add_group(s["log_terms"], s["prs"], gid=t["id"], term=s["term"], state=c["state"], vote=s["vote"],
                         lead=s["lead"], voted=s["voted"], granted=s["granted"])
        m = t["msg"]
        sc.add_msg(g, MSG_VOTE, from_=m["from"], term=m["term"], log_term=m["log_term"])
        named.append(("TestAllServerStepdown_%d" % j, g, dict(state=c["wstate"], term=c["wterm"], nlog=c["windex"],
                                                              lead=NONE)))
    for j, c in enumerate(k["TestStateTransition"]["cases"]):
        idle_some()
        g = sc.add_group(**_fresh(c["peers"], 1), state=c["from"])
        sc.add_msg(g, c["kind"], from_=1)
        want = dict(panics=True) if not c["wallow"] else dict(state=c["to"], term=c["wterm"], lead=c["wlead"])
        named.append(("TestStateTransition_%d" % j, g, want))
    idle_some()
    g = sc.add_group(**_fresh([1], 1))
    sc.add_hup(g)
    named.append(("TestSingleNodeCandidate", g, dict(state=LEADER)))
    t = k["TestRecoverPendingConfig"]
    for j, c in enumerate(t["cases"]):
        idle_some()
        g = sc.add_group([dict(term=0)] + [dict(term=0, type=ty) for ty in c["ent_types"]],
                         [(1, len(c["ent_types"]), len(c["ent_types"]) + 1), (2, 0, 1)], gid=1, term=0)
        sc.add_hup(g)
        sc.add_msg(g, MSG_VOTE_RESP, from_=2, term=1)
        want = dict(panics=True, status=PANIC_DOUBLE_CONF) if c["wpanic"] else dict(state=LEADER,
                                                                                     pending_conf=int(c["wpending"]))
        named.append(("TestRecoverPendingConfig_%d" % j, g, want))
    return sc, named


def check_kats(sc, named):
    """The tables' wanted values against the scenario's outcomes."""
    _, grows, strows, vrows, _, _ = sc.expected()
    first = {g: i for g, i in sc.runs}
    for name, g, w in named:
        i = first[g]
        n = sum(1 for m in sc.msgs if m["group"] == g)
        last = sc.outcomes[i + n - 1]
        msgs = [m for m in sc.messages if m["group"] == g]
        if w.get("panics"):
            assert last["action"] == PANICKED and last["status"] == w.get("status", PANIC_LEADER_TO_CANDIDATE), name
            continue
        assert all(o["status"] == OK for o in sc.outcomes[i:i + n]), name
        if "reject" in w:
            assert len(msgs) == w["n_msgs"] and msgs[0]["type"] == MSG_VOTE_RESP, name
            assert bool(msgs[0].get("reject")) == w["reject"], name
        if "state" in w:
            assert int(vrows[g, 0]) == w["state"] == last["state"], name
        if "term" in w:
            assert int(grows[g, 1]) == w["term"] == last["term"], name
        if "lead" in w:
            assert int(vrows[g, 2]) == w["lead"], name
        if "nlog" in w:
            assert int(grows[g, 4]) == w["nlog"], name
        if "pending_conf" in w:
            assert int(strows[g, 2]) == w["pending_conf"], name


def election_scenario(rows, copies=1):
    """The first call of TestLeaderElection rows, each `copies` times: one
    group per node (group = the row's first group + id - 1), node 1's msgHup.
    A nopStepper is a group that is never stepped."""
    sc = Scenario()
    sc.nop, sc.cluster = set(), []
    for row in rows * copies:
        peers = list(range(1, len(row["peers"]) + 1))
        base = len(sc.groups)
        for id_, p in zip(peers, row["peers"]):
            log = [0] if p in (None, "nop") else [0] + list(p)
            # room: the candidate's run is its msgHup, then up to len(peers) - 1 answers
            g = sc.add_group(log, [(q, 0, len(log)) for q in peers], gid=id_, term=0, room=len(peers))
            sc.cluster.append(base)
            if p == "nop":
                sc.nop.add(g)
        sc.add_hup(base)
    return sc


def next_round(sc, arrays, messages):
    """The scenario after a call: the arrays the call left (groups, state,
    vote state, entries) as the new start state, and the call's election
    messages -- dicts with group (the sender's), to, type, from_, term, index,
    log_term, reject -- routed by their `to` within the sender's cluster
    (grouped per receiver, in order; nopStepper peers drop theirs)."""
    grows, strows, vrows, erows = arrays
    nx = Scenario()
    nx.nop, nx.cluster = sc.nop, sc.cluster
    first = 0
    for g in range(len(sc.groups)):
        w = [int(x) for x in grows[g]]
        cap = sc.state[g]["ents_cap"]
        log = [dict(term=int(e[0]), type=int(e[4]) & 0xFFFFFFFF) for e in erows[first:first + w[4]]]
        first += cap
        v = [int(x) for x in vrows[g]]
        nx.add_group(log, [(w[7 + k], w[14 + k], w[21 + k]) for k in range(w[6])], gid=w[0], term=w[1], committed=w[2],
                     log_offset=w[3], room=cap - w[4], unstable=int(strows[g, 1]), pending_conf=int(strows[g, 2]),
                     state=v[0], vote=v[1], lead=v[2], elapsed=v[3], voted=v[4], granted=v[5])
    inbox = {}
    for m in messages:
        to = sc.cluster[m["group"]] + m["to"] - 1
        if to not in sc.nop and m["type"] in (MSG_VOTE, MSG_VOTE_RESP):
            inbox.setdefault(to, []).append(m)
    for to in sorted(inbox):
        for m in inbox[to]:
            nx.add_msg(to, m["type"], from_=m["from_"], term=m["term"], index=m["index"], log_term=m["log_term"],
                       reject=m.get("reject", False))
    return nx


def restated_call(sc):
    res, grows, strows, vrows, erows, _ = sc.expected()
    return (grows, strows, vrows, erows), sc.messages


def play_election(rows, call=restated_call, copies=1):
    """Plays TestLeaderElection rows as three calls -- the msgHup, the msgVote
    at the voters, the msgVoteResp at the candidates -- `call(scenario)` giving
    (the arrays the call left, its messages as next_round takes them).
    Returns (node 1's (state, term) per cluster, the last call's scenario, its
    arrays and messages)."""
    sc = election_scenario(rows, copies)
    for _ in range(3):
        done = sc
        arrays, msgs = call(sc)
        sc = next_round(sc, arrays, msgs)
    heads = sorted(set(sc.cluster))
    return [(sc.vstate[g]["state"], sc.groups[g]["term"]) for g in heads], done, arrays, msgs


# ---- the lattice ---------------------------------------------------------------

def lattice_scenario():
    """state {follower, candidate, leader} x kind {hup, vote, vote_resp} x the
    message's term {0, below, equal, above} x vote {None, from, another} x the
    candidate's log {behind, equal, ahead} x n_peers 0..8: one group and one
    record each.  The record's sender is the second peer; the group is the
    first, or -- n_peers 0 and 8 -- not promotable / unsupported."""
    sc = Scenario()
    log = [1, 2, 2]
    for np_ in range(9):
        for state in (FOLLOWER, CANDIDATE, LEADER):
            for kind in (MSG_HUP, MSG_VOTE, MSG_VOTE_RESP):
                for trel in ("zero", "below", "equal", "above"):
                    if kind == MSG_HUP and trel != "zero":
                        continue
                    for vrel in ("none", "from", "other"):
                        for lrel in ("behind", "equal", "ahead"):
                            if kind != MSG_VOTE and lrel != "equal":
                                continue
                            ids = [10 + k for k in range(min(np_, 7))]
                            from_ = ids[1] if len(ids) > 1 else 99
                            prs = [(p, 0, 3) for p in ids]
                            if np_ == 8:
                                prs = [(10 + k, 0, 3) for k in range(7)]
                            vote = dict(none=NONE, other=77)
                            vote["from"] = from_
                            voted = granted = 0
                            if state == CANDIDATE and ids:
                                voted, granted = (5 if len(ids) >= 3 else 1), 1   # the third peer has rejected
                            g = sc.add_group(log, prs, gid=ids[0] if ids else 10, term=5, committed=1, state=state,
                                             vote=vote[vrel], n_peers=np_ if np_ in (0, 8) else None, voted=voted,
                                             granted=granted, lead=ids[0] if state == LEADER and ids else NONE)
                            mterm = dict(zero=0, below=4, equal=5, above=6)[trel]
                            lt, idx = dict(behind=(1, 9), equal=(2, 2), ahead=(3, 0))[lrel]
                            sc.add_msg(g, kind, from_=from_, term=mterm, index=idx, log_term=lt,
                                       reject=(vrel == "other" and kind == MSG_VOTE_RESP))
    return sc


# ---- the random generator (shared, draw for draw, with tests/host/vote_step_forms.cpp) ----

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


NP_TABLE = (1, 2, 2, 3, 3, 3, 3, 4, 5, 5, 5, 7, 3, 2, 0, 8)
OFF_TABLE = (0, 0, 5, 1000, M64 - 1, M64 - 1)
STATE_TABLE = (FOLLOWER, FOLLOWER, CANDIDATE, CANDIDATE, CANDIDATE, LEADER)
KIND_TABLE = (MSG_HUP, MSG_VOTE, MSG_VOTE, MSG_VOTE_RESP, MSG_VOTE_RESP, MSG_VOTE_RESP)


def random_run(seed, run):
    """One random group and its run of 1-6 records: (group kwargs of
    Scenario.add_group, [message kwargs of Scenario.add_msg])."""
    r = SplitMix(seed, run)
    np_ = NP_TABLE[r.rnd(16)]
    slots = min(np_, 7)
    off = OFF_TABLE[r.rnd(6)]
    nlog = r.rnd(8)
    t = 1 + r.rnd(3)
    log = []
    for _ in range(nlog):
        t += 1 if r.rnd(3) == 0 else 0
        log.append(dict(term=t, type=1 if r.rnd(3) == 0 else 0))
    term = t + r.rnd(2)
    committed = (off + (r.rnd(nlog + 1) if r.rnd(2) else 0)) & M64
    if r.rnd(8) == 0:
        committed = (off - 1) & M64
    ids = [10 + 3 * k + r.rnd(3) for k in range(slots)]
    me = r.rnd(slots) if slots else 0
    gid = ids[me] if slots else 10
    if r.rnd(5) == 0:
        gid = 999
    prs = []
    for k in range(slots):
        match = (off + r.rnd(nlog + 1)) & M64
        roll = r.rnd(10)
        prs.append((ids[k], match, off if roll == 0 else (off - 1) & M64 if roll == 1 else (match + 1) & M64))
    state = STATE_TABLE[r.rnd(6)]
    vote = (NONE, ids[r.rnd(slots)] if slots else NONE, 77)[r.rnd(3)]
    lead = r.rnd(2) * gid
    elapsed = r.rnd(10)
    voted = granted = 0
    if state == CANDIDATE:
        voted = r.next() & ((1 << slots) - 1)
        granted = voted & r.next()
    unstable = (off + r.rnd(nlog + 3)) & M64
    pending = r.rnd(2)
    snap = dict(index=off, term=1, data_off=3, data_len=4, nodes_off=1, n_nodes=2) if r.rnd(2) else None
    group = dict(log=log, prs=prs, gid=gid, term=term, committed=committed, log_offset=off, snap=snap,
                 n_peers=np_ if np_ in (0, 8) else None, room=6, unstable=unstable, pending_conf=pending, state=state,
                 vote=vote, lead=lead, elapsed=elapsed, voted=voted, granted=granted)
    msgs = []
    cur = term   # about where Term stands (panics aside): answers at the running term are the ones that count
    for _ in range(1 + r.rnd(6)):
        kind = KIND_TABLE[r.rnd(6)]
        from_ = ids[r.rnd(slots)] if slots and r.rnd(8) else 55
        rel = r.rnd(8)
        mterm = 0 if rel == 0 else (cur - 1) & M64 if rel == 1 else cur + 2 if rel == 7 else \
            cur + (1 if r.rnd(4) == 0 else 0)
        cur = cur + 1 if kind == MSG_HUP else max(cur, mterm)
        index = (off + r.rnd(nlog + 2)) & M64
        log_term = r.rnd(t + 2)
        reject = r.rnd(4) == 0
        msgs.append(dict(kind=kind, from_=from_, term=mterm, index=index, log_term=log_term, reject=reject))
    return group, msgs


def random_scenario(seed, runs=6000, first=0):
    sc = Scenario()
    for j in range(first, first + runs):
        group, msgs = random_run(seed, j)
        g = sc.add_group(**group)
        for m in msgs:
            sc.add_msg(g, **m)
    return sc


def _fnv(h, v):
    return ((h ^ (v & M64)) * 0x100000001B3) & M64


def digest(seed, runs):
    """The digest tests/host/vote_step_forms.cpp prints for the same seed and
    count: every record's outcome, messages and entry, and every run's final
    records, folded in order."""
    h = 0xCBF29CE484222325
    counts = [0] * 10
    for j in range(runs):
        sc = random_scenario(seed, 1, first=j)
        res, grows, strows, vrows, erows, rows = sc.expected()
        efirst = int(grows[0, 5])
        for i, o in enumerate(sc.outcomes):
            counts[o["action"]] += 1
            for v in (o["status"], o["action"], o["flags"], o["n_msgs"], o["term"], o["vote"], o["state"]) + \
                    (o["appended"] or (M64, M64, M64)):
                h = _fnv(h, v)
            for m in rows[o["msg_first"]:o["msg_first"] + o["n_msgs"]]:
                w = [int(x) for x in m]
                for v in (w[0], w[1], w[5], w[4], w[6], (w[7] - efirst) & M64 if w[8] else 0, w[8], w[17]):
                    h = _fnv(h, v)
        for v in [int(x) for x in grows[0, [1, 2, 4]]] + [int(x) for x in grows[0, 14:28]] + \
                [int(strows[0, 1]), int(strows[0, 2])] + [int(x) for x in vrows[0, :6]]:
            h = _fnv(h, v)
    return h, counts


# ---- shapes ------------------------------------------------------------------------

def boundary_scenario(n, seed=9):
    """n records in runs of 1-4, except that a run of 6 (a five-node election at
    its candidate: a stale answer, then the votes) starts three records before
    the 64th, 256th and 1024th record: a run straddles each wave and workgroup
    seam."""
    rng = random.Random(seed)
    sc = Scenario()
    pos = 0
    five = [(1, 3, 4), (2, 0, 4), (3, 0, 4), (4, 0, 4), (5, 0, 4)]
    while pos < n:
        to_seam = min([b - 3 - pos for b in (64, 256, 1024) if b - 3 >= pos] or [n])
        length = 6 if to_seam == 0 else min(rng.randrange(1, 5), to_seam)
        length = min(length, n - pos)
        off = rng.choice([0, 9])
        g = sc.add_group([1, 1, 2, 2], [(p, m and off + m, off + x) for p, m, x in five], gid=1, term=3,
                         committed=off + 1, log_offset=off, room=6, state=CANDIDATE, vote=1, voted=1, granted=1)
        for k in range(length):
            roll = rng.random()
            if roll < 0.15:
                sc.add_msg(g, MSG_VOTE_RESP, from_=2 + k % 4, term=2)
            elif roll < 0.3:
                sc.add_msg(g, MSG_VOTE, from_=2 + k % 4, term=3, index=off + 3, log_term=2)
            else:
                sc.add_msg(g, MSG_VOTE_RESP, from_=2 + k % 4, term=3, reject=rng.random() < 0.3)
        pos += length
    return sc


def long_scenario(length, lead_in=0):
    """`lead_in` single-record groups, then one single-node group with a run of
    `length` records: msgHup (WON), a higher-term msgVote (back to follower),
    over and over -- every win appends an entry of its own term that the next
    msgVote's isUpToDate reads back."""
    sc = Scenario()
    for k in range(lead_in):
        g = sc.add_group([1, 2], [(1, 1, 2), (2, 0, 2)], term=2)
        sc.add_msg(g, MSG_VOTE, from_=2, term=3, index=1, log_term=2)
    g = sc.add_group([1], [(1, 0, 1)], gid=1, term=1, room=length)
    term = 1
    for k in range(length):
        if k % 2 == 0:
            sc.add_hup(g)
            term += 1
        else:
            term += 1
            sc.add_msg(g, MSG_VOTE, from_=9, term=term, index=k, log_term=term - 1 - (k % 4 == 3))
    return sc


def wide_scenario(n):
    """n three-node groups with one record each (a third each of msgHup,
    msgVote and the winning msgVoteResp); cheap to build."""
    sc = Scenario(snaps=False)
    for g in range(n):
        kind = g % 3
        if kind == 2:
            sc.add_group([1, 2, 2], [(1, 2, 3), (2, 0, 3), (3, 0, 3)], term=3, committed=1, state=CANDIDATE, vote=1,
                         voted=1, granted=1)
            sc.add_msg(g, MSG_VOTE_RESP, from_=2, term=3)
        else:
            sc.add_group([1, 2, 2], [(1, 0, 3), (2, 0, 3), (3, 0, 3)], term=2, committed=1)
            if kind == 0:
                sc.add_hup(g)
            else:
                sc.add_msg(g, MSG_VOTE, from_=2, term=3, index=2, log_term=2)
    return sc
