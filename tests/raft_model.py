"""One layout-free model of the reference's raft: a plain transcription of
raft/raft.go (raft, progress, Step and the three step functions), raft/log.go
(raftLog) and the parts of raft/node.go the library restates (newReady and
node.run's accept of a Ready), on Python ints masked to 64 bits.

It is Go-shaped and knows nothing about the device records: prs is a dict,
ents a list of entries, msgs a list of message dicts.  An entry's Data is real
bytes where from_arrays is given the data buffer; the tests do not give it, so
there Data stays None and the entry carries its Data's place (data_off,
data_len, data_nil) as extra keys that no function of the model reads: Step
never looks into Data, and the tests compare Data by content themselves.
Go's panics are raised as Panic carrying a class name.  Every per-call
restatement (log_append_cases / lead_step_cases / lead_prop_cases /
vote_step_cases on one side, follow_cases / compact_cases on the other) is
compared with this one statement, so the two families are compared with each
other.  This module imports none of them.

Broadcast order: Go ranges over the prs map, whose order is unspecified.
This library's rule is ascending slot order of the peer list the node was
created with, or that a snapshot rebuilt; prs is an insertion-ordered dict,
so that is the order every broadcast here iterates in.

Left to the caller, as everywhere in include/ewal.h: removed[], msgDenied and
addNode / removeNode.  They are not modelled.

Only from_arrays / to_arrays (at the end) know the layout of the group
records."""
import copy

M64 = (1 << 64) - 1
NONE = 0
FOLLOWER, CANDIDATE, LEADER = 0, 1, 2
(MSG_HUP, MSG_BEAT, MSG_PROP, MSG_APP, MSG_APP_RESP, MSG_VOTE, MSG_VOTE_RESP, MSG_SNAP, MSG_DENIED) = range(9)
ENTRY_NORMAL, ENTRY_CONF_CHANGE = 0, 1
DEFAULT_COMPACT_THRESHOLD = 10000

# Panic classes
(BOUNDS, COMMITTED_CONFLICT, NIL_PROGRESS, NEED_SNAPSHOT, FIRST_ENTRY, LEADER_TO_CANDIDATE, FOLLOWER_TO_LEADER,
 NIL_ENTRY, DOUBLE_CONF, NO_LEADER, PROP_LENGTH, COMPACT_APPLIED, COMPACT_BOUNDS) = (
    "bounds", "committed_conflict", "nil_progress", "need_snapshot", "first_entry", "leader_to_candidate",
    "follower_to_leader", "nil_entry", "double_conf", "no_leader", "prop_length", "compact_applied", "compact_bounds")


class Panic(Exception):
    """A Go panic; name is its class."""

    def __init__(self, name):
        super().__init__(name)
        self.name = name


def Entry(Term=0, Index=0, Type=ENTRY_NORMAL, Data=None, **extra):
    return dict(Term=Term & M64, Index=Index & M64, Type=Type, Data=Data, **extra)


def Message(Type, To=0, From=0, Term=0, LogTerm=0, Index=0, Entries=None, Commit=0, Snapshot=None, Reject=False):
    return dict(Type=Type, To=To, From=From, Term=Term, LogTerm=LogTerm, Index=Index, Entries=Entries, Commit=Commit,
                Snapshot=Snapshot, Reject=Reject)


def Snapshot(Index=0, Term=0, Nodes=None, RemovedNodes=None, Data=None, **extra):
    return dict(Index=Index, Term=Term, Nodes=Nodes, RemovedNodes=RemovedNodes, Data=Data, **extra)


class RaftLog:   # log.go:13-34
    def __init__(self):
        self.ents = [Entry()]
        self.unstable = self.committed = self.applied = self.offset = 0
        self.snapshot = Snapshot()
        self.compactThreshold = DEFAULT_COMPACT_THRESHOLD

    def maybeAppend(self, index, logTerm, committed, ents):   # log.go:49-69
        lastnewi = (index + len(ents)) & M64
        if self.matchTerm(index, logTerm):
            frm = (index + 1) & M64
            ci = self.findConflict(frm, ents)
            if ci == 0:
                pass
            elif ci <= self.committed:
                raise Panic(COMMITTED_CONFLICT)
            else:
                k = (ci - frm) & M64
                if k > len(ents):
                    raise Panic(BOUNDS)
                self.append((ci - 1) & M64, ents[k:])
            tocommit = min(committed, lastnewi)
            if self.committed < tocommit:
                self.committed = tocommit
            return True
        return False

    def append(self, after, ents):   # log.go:71-75
        self.ents = self.slice(self.offset, (after + 1) & M64) + [dict(e) for e in ents]
        self.unstable = min(self.unstable, (after + 1) & M64)
        return self.lastIndex()

    def findConflict(self, frm, ents):   # log.go:77-84
        for i, ne in enumerate(ents):
            oe = self.at((frm + i) & M64)
            if oe is None or oe["Term"] != ne["Term"]:
                return (frm + i) & M64
        return 0

    def unstableEnts(self):   # log.go:86-94
        return [dict(e) for e in self.slice(self.unstable, (self.lastIndex() + 1) & M64)]

    def resetUnstable(self):   # log.go:96-98
        self.unstable = (self.lastIndex() + 1) & M64

    def nextEnts(self):   # log.go:102-107
        if self.committed > self.applied:
            return self.slice((self.applied + 1) & M64, (self.committed + 1) & M64)
        return []

    def resetNextEnts(self):   # log.go:109-113
        if self.committed > self.applied:
            self.applied = self.committed

    def lastIndex(self):   # log.go:115-117
        return (len(self.ents) - 1 + self.offset) & M64

    def term(self, i):   # log.go:119-124
        e = self.at(i)
        if e is not None:
            return e["Term"]
        return 0

    def entries(self, i):   # log.go:126-134
        if i == self.offset:
            raise Panic(FIRST_ENTRY)
        return self.slice(i, (self.lastIndex() + 1) & M64)

    def isUpToDate(self, i, term):   # log.go:136-139
        e = self.at(self.lastIndex())
        if e is None:
            raise Panic(NIL_ENTRY)
        return term > e["Term"] or (term == e["Term"] and i >= self.lastIndex())

    def matchTerm(self, i, term):   # log.go:141-146
        e = self.at(i)
        if e is not None:
            return e["Term"] == term
        return False

    def maybeCommit(self, maxIndex, term):   # log.go:148-154
        if maxIndex > self.committed and self.term(maxIndex) == term:
            self.committed = maxIndex
            return True
        return False

    def compact(self, i):   # log.go:161-169
        if self.isOutOfAppliedBounds(i):
            raise Panic(COMPACT_BOUNDS)
        self.ents = self.slice(i, (self.lastIndex() + 1) & M64)
        self.unstable = max((i + 1) & M64, self.unstable)
        self.offset = i
        return len(self.ents)

    def snap(self, d, index, term, nodes, removed):   # log.go:171-179
        self.snapshot = Snapshot(Index=index, Term=term, Nodes=nodes, RemovedNodes=removed, Data=d)

    def shouldCompact(self):   # log.go:181-183
        return ((self.applied - self.offset) & M64) > self.compactThreshold

    def restore(self, s):   # log.go:185-192
        self.ents = [Entry(Term=s["Term"])]
        self.unstable = (s["Index"] + 1) & M64
        self.committed = s["Index"]
        self.applied = s["Index"]
        self.offset = s["Index"]
        self.snapshot = s

    def at(self, i):   # log.go:194-199
        if self.isOutOfBounds(i):
            return None
        k = (i - self.offset) & M64
        if k >= len(self.ents):
            raise Panic(BOUNDS)   # Go indexes past ents
        return self.ents[k]

    def slice(self, lo, hi):   # log.go:202-210
        if lo >= hi:
            return []
        if self.isOutOfBounds(lo) or self.isOutOfBounds((hi - 1) & M64):
            return []
        a, b = (lo - self.offset) & M64, (hi - self.offset) & M64
        if a > b or b > len(self.ents):
            raise Panic(BOUNDS)
        return self.ents[a:b]

    def isOutOfBounds(self, i):   # log.go:212-217
        return i < self.offset or i > self.lastIndex()

    def isOutOfAppliedBounds(self, i):   # log.go:219-224
        return i < self.offset or i > self.applied


class Progress:   # raft.go:67-90
    def __init__(self, match=0, next=0):
        self.match, self.next = match, next

    def update(self, n):
        self.match = n
        self.next = (n + 1) & M64

    def maybeDecrTo(self, to):
        if self.match != 0 or (self.next - 1) & M64 != to:
            return False
        self.next = (self.next - 1) & M64
        if self.next < 1:
            self.next = 1
        return True


class Raft:
    """raft.  trace collects, per Step, the names of the branches taken; the
    tests read it to name a record's action, the model itself never does."""

    def __init__(self, id, peers):   # raft.go:135-154
        if id == NONE:
            raise Panic("none_id")
        self.id, self.Term, self.Vote, self.Commit = id, 0, NONE, 0
        self.lead = NONE
        self.raftLog = RaftLog()
        self.prs = {p: Progress() for p in peers}
        self.state, self.votes, self.msgs, self.pendingConf, self.elapsed = FOLLOWER, {}, [], False, 0
        self.trace = []
        self.becomeFollower(0, NONE)

    def hasLeader(self):   # raft.go:156
        return self.lead != NONE

    def softState(self):   # raft.go:160-162; ShouldStop is removed[]'s: the caller's
        return dict(Lead=self.lead, RaftState=self.state, Nodes=self.nodes())

    def hardState(self):
        return dict(Term=self.Term, Vote=self.Vote, Commit=self.Commit)

    def poll(self, id, v):   # raft.go:177-187
        if id not in self.votes:
            self.votes[id] = v
        return sum(1 for vv in self.votes.values() if vv)

    def send(self, m):   # raft.go:190-199
        m["From"] = self.id
        if m["Type"] != MSG_PROP:
            m["Term"] = self.Term
        self.msgs.append(m)

    def sendAppend(self, to):   # raft.go:202-217
        pr = self.prs.get(to)
        if pr is None:
            raise Panic(NIL_PROGRESS)
        m = Message(0, To=to, Index=(pr.next - 1) & M64)
        if self.needSnapshot(m["Index"]):
            m["Type"] = MSG_SNAP
            m["Snapshot"] = self.raftLog.snapshot
        else:
            m["Type"] = MSG_APP
            m["LogTerm"] = self.raftLog.term((pr.next - 1) & M64)
            m["Entries"] = [dict(e) for e in self.raftLog.entries(pr.next)]
            m["Commit"] = self.raftLog.committed
        self.send(m)

    def sendHeartbeat(self, to):   # raft.go:219-226
        self.send(Message(MSG_APP, To=to))

    def bcastAppend(self):   # raft.go:229-236
        for i in list(self.prs):
            if i == self.id:
                continue
            self.sendAppend(i)

    def bcastHeartbeat(self):   # raft.go:238-246
        for i in list(self.prs):
            if i == self.id:
                continue
            self.sendHeartbeat(i)

    def maybeCommit(self):   # raft.go:248-258
        mis = sorted((pr.match for pr in self.prs.values()), reverse=True)
        if self.q() - 1 >= len(mis):
            raise Panic(BOUNDS)
        return self.raftLog.maybeCommit(mis[self.q() - 1], self.Term)

    def reset(self, term):   # raft.go:260-273
        self.Term = term
        self.lead = NONE
        self.Vote = NONE
        self.elapsed = 0
        self.votes = {}
        for i in self.prs:
            self.prs[i] = Progress(next=(self.raftLog.lastIndex() + 1) & M64)
            if i == self.id:
                self.prs[i].match = self.raftLog.lastIndex()
        self.pendingConf = False

    def q(self):   # raft.go:275-277
        return len(self.prs) // 2 + 1

    def appendEntry(self, e):   # raft.go:279-285
        e = dict(e, Term=self.Term, Index=(self.raftLog.lastIndex() + 1) & M64)
        self.raftLog.append(self.raftLog.lastIndex(), [e])
        if self.id not in self.prs:
            raise Panic(NIL_PROGRESS)
        self.prs[self.id].update(self.raftLog.lastIndex())
        self.maybeCommit()

    def becomeFollower(self, term, lead):   # raft.go:309-315
        self.reset(term)
        self.lead = lead
        self.state = FOLLOWER

    def becomeCandidate(self):   # raft.go:317-327
        if self.state == LEADER:
            raise Panic(LEADER_TO_CANDIDATE)
        self.reset((self.Term + 1) & M64)
        self.Vote = self.id
        self.state = CANDIDATE

    def becomeLeader(self):   # raft.go:329-349
        if self.state == FOLLOWER:
            raise Panic(FOLLOWER_TO_LEADER)
        self.reset(self.Term)
        self.lead = self.id
        self.state = LEADER
        for e in self.raftLog.entries((self.raftLog.committed + 1) & M64):
            if e["Type"] != ENTRY_CONF_CHANGE:
                continue
            if self.pendingConf:
                raise Panic(DOUBLE_CONF)
            self.pendingConf = True
        self.appendEntry(Entry(Data=None))
        self.trace.append("became_leader")

    def readMessages(self):   # raft.go:351-356
        msgs = self.msgs
        self.msgs = []
        return msgs

    def campaign(self):   # raft.go:358-370
        self.becomeCandidate()
        if self.q() == self.poll(self.id, True):
            self.becomeLeader()
        for i in list(self.prs):
            if i == self.id:
                continue
            lasti = self.raftLog.lastIndex()
            self.send(Message(MSG_VOTE, To=i, Index=lasti, LogTerm=self.raftLog.term(lasti)))
        self.trace.append("campaigned")

    def Step(self, m):   # raft.go:372-408, without removed[] and msgDenied
        self.trace = []
        try:
            if m["Type"] == MSG_HUP:
                self.campaign()
            if m["Term"] == 0:
                pass
            elif m["Term"] > self.Term:
                lead = m["From"]
                if m["Type"] == MSG_VOTE:
                    lead = NONE
                self.becomeFollower(m["Term"], lead)
                self.trace.append("term_switch")
            elif m["Term"] < self.Term:
                self.trace.append("ignored")
                return
            (stepFollower, stepCandidate, stepLeader)[self.state](self, m)
        finally:
            self.Commit = self.raftLog.committed

    def handleAppendEntries(self, m):   # raft.go:410-416
        if self.raftLog.maybeAppend(m["Index"], m["LogTerm"], m["Commit"], m["Entries"] or []):
            self.send(Message(MSG_APP_RESP, To=m["From"], Index=self.raftLog.lastIndex()))
            self.trace.append("appended")
        else:
            self.send(Message(MSG_APP_RESP, To=m["From"], Index=m["Index"], Reject=True))
            self.trace.append("rejected")

    def handleSnapshot(self, m):   # raft.go:418-424
        if self.restore(m["Snapshot"]):
            self.send(Message(MSG_APP_RESP, To=m["From"], Index=self.raftLog.lastIndex()))
            self.trace.append("restored")
        else:
            self.send(Message(MSG_APP_RESP, To=m["From"], Index=self.raftLog.committed))
            self.trace.append("snap_stale")

    def compact(self, index, nodes, d, removed=()):   # raft.go:522-531; removed: r.removedNodes(), the caller's
        if index > self.raftLog.applied:
            raise Panic(COMPACT_APPLIED)
        self.raftLog.snap(d, index, self.raftLog.term(index), nodes, removed)
        self.raftLog.compact(index)

    def restore(self, s):   # raft.go:535-554
        if s["Index"] <= self.raftLog.committed:
            return False
        self.raftLog.restore(s)
        self.prs = {}
        for n in s["Nodes"]:
            last = self.raftLog.lastIndex()
            if n == self.id:
                self.setProgress(n, last, (last + 1) & M64)
            else:
                self.setProgress(n, 0, (last + 1) & M64)
        return True

    def needSnapshot(self, i):   # raft.go:556-564
        if i < self.raftLog.offset:
            if self.raftLog.snapshot["Term"] == 0:
                raise Panic(NEED_SNAPSHOT)
            return True
        return False

    def nodes(self):   # raft.go:566-572, in slot order
        return list(self.prs)

    def setProgress(self, id, match, next):   # raft.go:582-584
        self.prs[id] = Progress(match, next)

    def promotable(self):   # raft.go:592-595
        return self.id in self.prs


def stepLeader(r, m):   # raft.go:439-470
    t = m["Type"]
    if t == MSG_BEAT:
        r.bcastHeartbeat()
        r.trace.append("beat")
    elif t == MSG_PROP:
        if len(m["Entries"] or []) != 1:
            raise Panic(PROP_LENGTH)
        e = m["Entries"][0]
        if e["Type"] == ENTRY_CONF_CHANGE:
            if r.pendingConf:
                r.trace.append("dropped")
                return
            r.pendingConf = True
        r.appendEntry(e)
        r.bcastAppend()
        r.trace.append("proposed")
    elif t == MSG_APP_RESP:
        pr = r.prs.get(m["From"])
        if pr is None:
            raise Panic(NIL_PROGRESS)
        if m["Reject"]:
            if pr.maybeDecrTo(m["Index"]):
                r.sendAppend(m["From"])
                r.trace.append("probe")
            else:
                r.trace.append("stale")
        else:
            pr.update(m["Index"])
            if r.maybeCommit():
                r.bcastAppend()
                r.trace.append("committed")
            else:
                r.trace.append("updated")
    elif t == MSG_VOTE:
        r.send(Message(MSG_VOTE_RESP, To=m["From"], Reject=True))
        r.trace.append("vote_rejected")
    else:
        r.trace.append("no_case")


def stepCandidate(r, m):   # raft.go:472-494
    t = m["Type"]
    if t == MSG_PROP:
        raise Panic(NO_LEADER)
    elif t == MSG_APP:
        r.becomeFollower(r.Term, m["From"])
        r.trace.append("conceded")
        r.handleAppendEntries(m)
    elif t == MSG_SNAP:
        r.becomeFollower(m["Term"], m["From"])
        r.trace.append("conceded")
        r.handleSnapshot(m)
    elif t == MSG_VOTE:
        r.send(Message(MSG_VOTE_RESP, To=m["From"], Reject=True))
        r.trace.append("vote_rejected")
    elif t == MSG_VOTE_RESP:
        gr = r.poll(m["From"], not m["Reject"])
        if r.q() == gr:
            r.becomeLeader()
            r.bcastAppend()
            r.trace.append("won")
        elif r.q() == len(r.votes) - gr:
            r.becomeFollower(r.Term, NONE)
            r.trace.append("lost")
        else:
            r.trace.append("polled")
    else:
        r.trace.append("no_case")


def stepFollower(r, m):   # raft.go:496-520
    t = m["Type"]
    if t == MSG_PROP:
        if r.lead == NONE:
            raise Panic(NO_LEADER)
        m = dict(m, To=r.lead)
        r.send(m)
        r.trace.append("forwarded")
    elif t == MSG_APP:
        r.elapsed = 0
        r.lead = m["From"]
        r.handleAppendEntries(m)
    elif t == MSG_SNAP:
        r.elapsed = 0
        r.handleSnapshot(m)
    elif t == MSG_VOTE:
        if (r.Vote == NONE or r.Vote == m["From"]) and r.raftLog.isUpToDate(m["Index"], m["LogTerm"]):
            r.elapsed = 0
            r.Vote = m["From"]
            r.send(Message(MSG_VOTE_RESP, To=m["From"]))
            r.trace.append("vote_granted")
        else:
            r.send(Message(MSG_VOTE_RESP, To=m["From"], Reject=True))
            r.trace.append("vote_rejected")
    else:
        r.trace.append("no_case")


class Node:
    """node.run's state around one raft (node.go:190-260): the previous soft
    and hard state and snapshot index that newReady compares with."""

    def __init__(self, r):
        self.r = r
        self.prevSoftSt, self.prevHardSt, self.prevSnapi = r.softState(), r.hardState(), r.raftLog.snapshot["Index"]

    def newReady(self):   # node.go:332-348
        r = self.r
        rd = dict(SoftState=None, HardState=dict(Term=0, Vote=0, Commit=0), Entries=r.raftLog.unstableEnts(),
                  Snapshot=Snapshot(), CommittedEntries=[dict(e) for e in r.raftLog.nextEnts()], Messages=list(r.msgs))
        if r.softState() != self.prevSoftSt:
            rd["SoftState"] = r.softState()
        if r.hardState() != self.prevHardSt:
            rd["HardState"] = r.hardState()
        if self.prevSnapi != r.raftLog.snapshot["Index"]:
            rd["Snapshot"] = r.raftLog.snapshot
        return rd

    @staticmethod
    def containsUpdates(rd):   # node.go:83-86
        return (rd["SoftState"] is not None or rd["HardState"] != dict(Term=0, Vote=0, Commit=0) or
                rd["Snapshot"]["Index"] != 0 or len(rd["Entries"]) > 0 or len(rd["CommittedEntries"]) > 0 or
                len(rd["Messages"]) > 0)

    def accept(self, rd):   # node.go:239-255
        if rd["SoftState"] is not None:
            self.prevSoftSt = rd["SoftState"]
        if rd["HardState"] != dict(Term=0, Vote=0, Commit=0):
            self.prevHardSt = rd["HardState"]
        if rd["Snapshot"]["Index"] != 0:
            self.prevSnapi = rd["Snapshot"]["Index"]
        self.r.raftLog.resetNextEnts()
        self.r.raftLog.resetUnstable()
        self.r.msgs = []


def saved(r):
    """A deep copy of r, for the caller that wants a panicking Step undone
    (Go's process is gone; the library leaves the group as it was)."""
    return copy.deepcopy(r.__dict__)


def put_back(r, b):
    r.__dict__.clear()
    r.__dict__.update(b)


# ---- the adapters: the only code here that knows the group records ----------------------
#
# groups (32 words): id, Term, committed, offset, len(ents), the window's first
#   slot in ents, n_peers, 7 peer ids, 7 match, 7 next, 4 reserved
# pstate (4): window capacity, unstable, pendingConf, reserved
# vstate (8): state, Vote, lead, elapsed, voted mask, granted mask (over the peer slots), 2 reserved
# rstate (8): prevHardSt (Term, Vote, Commit), prevSoftSt (Lead, RaftState), prevSnapi, applied, soft_dirty
# snaps (8): Index, Term, data_off, data_len, nodes_off, n_nodes, removed_off, n_removed
# ents (5): Term, Index, data_off, data_len, Type | data_nil << 32

PEERS = 7
SNAP_FIELDS = ("Index", "Term", "data_off", "data_len", "nodes_off", "n_nodes", "removed_off", "n_removed")
SNAP_FIELDS_LOWER = tuple(k.lower() for k in SNAP_FIELDS)


def snapshot_of_row(row, u64=None, data=None):
    """A model Snapshot of an 8-word snapshot record; Nodes and Data are read
    where their arrays are given."""
    w = [int(x) for x in row]
    s = Snapshot(**dict(zip(SNAP_FIELDS, w)))
    if u64 is not None:
        s["Nodes"] = [int(x) for x in u64[w[4]:w[4] + w[5]]]
        s["RemovedNodes"] = [int(x) for x in u64[w[6]:w[6] + w[7]]]
    if data is not None:
        s["Data"] = bytes(data[w[2]:w[2] + w[3]])
    return s


def row_of_snapshot(s):
    return [s.get(k, 0) & M64 for k in SNAP_FIELDS]


def entry_of_row(row, data=None):
    w = [int(x) for x in row]
    nil = w[4] >> 32            # 0: Data is (data_off, data_len); 1: nil; 2: not in the data buffer
    d = None
    if data is not None and nil == 0:
        d = bytes(data[w[2]:w[2] + w[3]])
    return Entry(Term=w[0], Index=w[1], Type=w[4] & 0xFFFFFFFF, Data=d, data_off=w[2], data_len=w[3], data_nil=nil)


def row_of_entry(e):
    return [e["Term"], e["Index"], e.get("data_off", 0), e.get("data_len", 0),
            (e["Type"] & 0xFFFFFFFF) | (e.get("data_nil", 1) << 32)]


def from_arrays(arrays, g, data=None, u64=None):
    """The model node (a Node around its Raft) of group g's row of groups,
    pstate, vstate, rstate, snaps and its window of ents.  arrays: a dict of
    uint64 row arrays; rstate and snaps may be None.  More than PEERS peers,
    or a vote of a peer without a slot, cannot be stated in the records."""
    w = [int(x) for x in arrays["groups"][g]]
    s = [int(x) for x in arrays["pstate"][g]]
    v = [int(x) for x in arrays["vstate"][g]] if arrays.get("vstate") is not None else [0] * 8
    slots = min(w[6], PEERS)
    r = Raft.__new__(Raft)
    r.id, r.Term, r.Commit = w[0], w[1], w[2]
    r.state, r.Vote, r.lead, r.elapsed = v[0], v[1], v[2], v[3]
    r.prs = {w[7 + k]: Progress(w[14 + k], w[21 + k]) for k in range(slots)}
    r.votes = {w[7 + k]: bool(v[5] >> k & 1) for k in range(slots) if v[4] >> k & 1}
    r.msgs, r.trace, r.pendingConf = [], [], bool(s[2])
    lg = r.raftLog = RaftLog()
    lg.ents = [entry_of_row(e, data) for e in arrays["ents"][w[5]:w[5] + w[4]]]
    lg.offset, lg.committed, lg.unstable = w[3], w[2], s[1]
    if arrays.get("snaps") is not None:
        lg.snapshot = snapshot_of_row(arrays["snaps"][g], u64, data)
    n = Node.__new__(Node)
    n.r = r
    if arrays.get("rstate") is not None:
        rs = [int(x) for x in arrays["rstate"][g]]
        n.prevHardSt = dict(Term=rs[0], Vote=rs[1], Commit=rs[2])
        n.prevSoftSt = dict(Lead=rs[3], RaftState=rs[4], Nodes=None if rs[7] else r.nodes())
        n.prevSnapi, lg.applied = rs[5], rs[6]
    else:
        n.prevHardSt, n.prevSoftSt, n.prevSnapi = r.hardState(), r.softState(), lg.snapshot["Index"]
    n.n_peers = w[6]
    return n


def to_arrays(n, arrays, g):
    """Writes node n back into row g of the arrays (in place): the inverse of
    from_arrays.  The window keeps its first slot and capacity; slots past
    len(ents) keep what they held."""
    r, lg = n.r, n.r.raftLog
    gr = arrays["groups"]
    first, cap = int(gr[g, 5]), int(arrays["pstate"][g, 0])
    assert len(lg.ents) <= cap and len(r.prs) <= PEERS
    gr[g, 0:5] = [r.id, r.Term, lg.committed, lg.offset, len(lg.ents)]
    np_ = len(r.prs)
    if [int(x) for x in gr[g, 7:7 + np_]] != list(r.prs) or min(int(gr[g, 6]), PEERS) != np_:
        gr[g, 6] = np_            # prs was rebuilt (a snapshot's Nodes): every slot is rewritten
        gr[g, 7:28] = 0
    for k, (p, pr) in enumerate(r.prs.items()):
        gr[g, 7 + k], gr[g, 14 + k], gr[g, 21 + k] = p, pr.match, pr.next
    arrays["pstate"][g, 1:3] = [lg.unstable, int(r.pendingConf)]
    voted = granted = 0
    for k, p in enumerate(r.prs):
        if p in r.votes:
            voted |= 1 << k
            granted |= (1 << k) if r.votes[p] else 0
    assert all(p in r.prs for p in r.votes)
    if arrays.get("vstate") is not None:
        arrays["vstate"][g, 0:6] = [r.state, r.Vote, r.lead, r.elapsed, voted, granted]
    for k, e in enumerate(lg.ents):
        arrays["ents"][first + k] = row_of_entry(e)
    if arrays.get("snaps") is not None:
        arrays["snaps"][g] = row_of_snapshot(lg.snapshot)
    if arrays.get("rstate") is not None:
        soft_dirty = int(n.prevSoftSt["Nodes"] != r.nodes())
        arrays["rstate"][g] = [n.prevHardSt["Term"], n.prevHardSt["Vote"], n.prevHardSt["Commit"],
                               n.prevSoftSt["Lead"], n.prevSoftSt["RaftState"], n.prevSnapi, lg.applied, soft_dirty]
