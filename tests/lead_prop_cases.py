"""The checker of the batched leader msgProp / msgBeat step
(elead_local_batch_device): lead_step_cases.Raft extended with appendEntry
(raft/raft.go:279-285), stepLeader's msgProp and msgBeat cases (:441-455) and
bcastHeartbeat / sendHeartbeat (:219-226, :238-246), written from the Go text
on Python ints masked to 64 bits, pinned by the reference's own tables
(tests/golden/raft_prop_kats.json), and the scenario builders the host and GPU
tests share."""
import json
import os
import random

import numpy as np

from etcd_amd import raftlead as R
from etcd_amd import raftprop as P

import lead_step_cases as K
from lead_step_cases import (M64, OK, PANIC_BOUNDS, PANIC_FIRST_ENTRY, PANIC_NEED_SNAPSHOT,  # noqa: F401
                             PANIC_NIL_PROGRESS, UNSUPPORTED, CANARY, MSG_APP, MSG_SNAP, Panic)

NOT_STEPPED, BEAT, APPENDED, DROPPED, PANICKED = range(5)
MSG_BEAT, MSG_PROP = 1, 2
CONF_CHANGE = 1
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raft_prop_kats.json")


class Raft(K.Raft):
    """The leader with what a proposal touches: raftLog.unstable (on the log)
    and raft.pendingConf."""

    def __init__(self, id_, term, log, prs, snapshot=None, pending_conf=False):
        super().__init__(id_, term, log, prs, snapshot)
        self.pending_conf = bool(pending_conf)

    def send_heartbeat(self, to):   # raft.go:219-226
        self.send(dict(to=to, type=MSG_APP, index=0, log_term=0, commit=0, ents=None, snap=None))

    def bcast_heartbeat(self):   # raft.go:238-246
        for p, _ in self.prs:
            if p == self.id:
                continue
            self.send_heartbeat(p)

    def append_entry(self):   # raft.go:279-285; returns (e.Index, the entry's position in ents)
        index = (self.log.last_index() + 1) & M64
        self.log.append(self.log.last_index(), [self.term])
        pr = self.pr(self.id)
        if pr is None:
            raise Panic(PANIC_NIL_PROGRESS)
        pr.update(self.log.last_index())
        self.maybe_commit()
        return index, len(self.log.ents) - 1

    def step_msg_beat(self):   # raft.go:441-442
        self.bcast_heartbeat()
        return BEAT, 0, 0

    def step_msg_prop(self, etype):   # raft.go:443-455
        if etype == CONF_CHANGE:
            if self.pending_conf:
                return DROPPED, 0, 0
            self.pending_conf = True
        index, pos = self.append_entry()
        self.bcast_append()
        return APPENDED, index, pos


def step(r, kind, etype=0):
    """One local message on r (Step's term switch: Term == 0, a local
    message).  Returns (status, action, messages, index, pos); a panic leaves r
    as it was and sends nothing."""
    before = (list(r.log.ents), r.log.committed, r.log.unstable, r.pending_conf,
              [(pr.match, pr.next) for _, pr in r.prs])
    r.msgs = []
    try:
        action, index, pos = r.step_msg_beat() if kind == MSG_BEAT else r.step_msg_prop(etype)
    except Panic as p:
        r.log.ents, r.log.committed, r.log.unstable, r.pending_conf = before[:4]
        for (_, pr), (m, n) in zip(r.prs, before[4]):
            pr.match, pr.next = m, n
        r.msgs = []
        return p.status, PANICKED, [], 0, 0
    return OK, action, r.msgs, index, pos


def load_kats():
    with open(KATS) as f:
        return json.load(f)


class Scenario:
    """Leader groups with their logs, their state records and one call's
    local messages; packs the device arrays and computes, with the
    restatement, every array the call leaves."""

    def __init__(self, snaps=True, data_len_total=1 << 20):
        self.groups, self.logs, self.snaps, self.state, self.locals = [], [], [], [], []
        self.with_snaps = snaps
        self.data_len_total = data_len_total

    def add_group(self, terms, prs, gid=None, term=2, committed=0, log_offset=0, snap=None, n_peers=None, room=4,
                  unstable=None, pending_conf=0):
        g = len(self.groups)
        grp = dict(id=gid if gid is not None else prs[0][0], term=term, committed=committed, log_offset=log_offset,
                   prs=[tuple(p) for p in prs])
        if n_peers is not None:
            grp["n_peers"] = n_peers
        self.groups.append(grp)
        self.logs.append(list(terms))
        self.snaps.append(snap)
        self.state.append(dict(ents_cap=len(terms) + room, pending_conf=pending_conf,
                               unstable=(log_offset + len(terms)) & M64 if unstable is None else unstable))
        return g

    def add_beat(self, group):
        self.locals.append(dict(group=group, kind=MSG_BEAT))

    def add_prop(self, group, etype=0, data_off=0, data_len=0, data_nil=None):
        self.locals.append(dict(group=group, kind=MSG_PROP, etype=etype, data_off=data_off, data_len=data_len,
                                data_nil=data_len == 0 if data_nil is None else data_nil))

    def add_run(self, group, what):
        """what: a string of P (proposal), C (ConfChange proposal), B (beat)."""
        for k, c in enumerate(what):
            if c == "B":
                self.add_beat(group)
            else:
                self.add_prop(group, etype=CONF_CHANGE if c == "C" else 0, data_off=7 * k, data_len=3 + k)

    def pack(self):
        """(group rows (G, 32), state rows (G, 4), snap rows (G, 8) or None,
        entry rows with the canary in every free slot, local rows (n, 6))."""
        grows, erows = P.pack_logs(self.groups, self.logs, self.state)
        first = 0
        for log, st in zip(self.logs, self.state):
            erows[first + len(log):first + st["ents_cap"]] = np.uint64(CANARY)
            first += st["ents_cap"]
        srows = R.pack_snaps(self.snaps) if self.with_snaps else None
        return grows, P.pack_state(self.state), srows, erows, P.pack_locals(self.locals)

    def raft_of(self, g, grows, strows):
        w = [int(x) for x in grows[g]]
        log = K.LeaderLog(self.logs[g], w[3], w[2])
        log.unstable = int(strows[g, 1])
        return Raft(w[0], w[1], log, [(w[7 + k], w[14 + k], w[21 + k]) for k in range(min(w[6], R.MAX_PEERS))],
                    self.snaps[g] if self.with_snaps else None, pending_conf=int(strows[g, 2]))

    def expected(self):
        """(results (n, 6), groups (G, 32), state (G, 4), entries, messages
        (n_msgs, 18)) as uint64 arrays: the bytes a successful call leaves.
        Also sets outcomes, messages (dicts), emitted (per record: the entry
        and the messages as the host program reads them), n_msgs, n_appended."""
        grows, strows, _, erows, _ = self.pack()
        n = len(self.locals)
        res = np.zeros((n, P.RESULT_WORDS), dtype=np.uint64)
        rows, self.outcomes, self.messages, self.emitted, self.runs = [], [], [], [], []
        i = 0
        while i < n:
            g = self.locals[i]["group"]
            r = self.raft_of(g, grows, strows)
            unsupported = int(grows[g, 6]) > R.MAX_PEERS
            efirst = int(grows[g, 5])
            stopped = False
            self.runs.append((g, i))
            while i < n and self.locals[i]["group"] == g:
                m = self.locals[i]
                index = pos = 0
                if stopped:
                    status, action, msgs = OK, NOT_STEPPED, []
                elif unsupported:
                    status, action, msgs = UNSUPPORTED, PANICKED, []
                else:
                    status, action, msgs, index, pos = step(r, m["kind"], m.get("etype", 0))
                stopped = stopped or status != OK
                em = []
                if action == APPENDED:
                    erows[efirst + pos] = np.array(
                        [r.term, index, m["data_off"], m["data_len"],
                         (m["etype"] & 0xFFFFFFFF) | ((1 if m["data_nil"] else 0) << 32)], dtype=np.uint64)
                    em.append((0, pos, r.term, index))
                for x in msgs:
                    ents = x["ents"] or (0, 0)
                    em.append((1, x["type"], x["to"], x["index"], x["log_term"], x["commit"], ents[0], ents[1]))
                o = dict(status=status, action=action, msg_first=len(rows), n_msgs=len(msgs), index=index, pos=pos,
                         ent_pos=efirst + pos if action == APPENDED else 0, committed=r.log.committed)
                self.outcomes.append(o)
                self.emitted.append(em)
                res[i] = np.array([status | (action << 32), o["msg_first"], o["n_msgs"], index, o["ent_pos"],
                                   o["committed"]], dtype=np.uint64)
                rows += [K.msg_row(x, efirst) for x in msgs]
                self.messages += [dict(x) for x in msgs]
                i += 1
            if not unsupported:
                grows[g, 2] = np.uint64(r.log.committed)
                grows[g, 4] = np.uint64(len(r.log.ents))
                for k, (_, pr) in enumerate(r.prs):
                    grows[g, 14 + k], grows[g, 21 + k] = np.uint64(pr.match), np.uint64(pr.next)
                strows[g, 1], strows[g, 2] = np.uint64(r.log.unstable), np.uint64(int(r.pending_conf))
        self.n_msgs = len(rows)
        self.n_appended = sum(1 for o in self.outcomes if o["action"] == APPENDED)
        return res, grows, strows, erows, np.array(rows, dtype=np.uint64).reshape(len(rows), R.MSG_WORDS)

    def case_file(self, path):
        """The runs as the host program (tests/host/lead_prop_forms.cpp) reads them."""
        grows0, strows0, _, _, _ = self.pack()
        _, grows, strows, _, _ = self.expected()
        out = [str(len(self.runs))]
        for g, first in self.runs:
            w = [int(x) for x in grows0[g]]
            snap = self.snaps[g] if self.with_snaps else None
            out.append(" ".join(str(x) for x in w[0:5] + [w[6]] + w[7:28] + [int(strows0[g, 1]), int(strows0[g, 2]),
                                                                            int(bool(snap and snap.get("term", 0)))]))
            out.append(" ".join(str(t) for t in self.logs[g]))
            i = first
            recs = []
            while i < len(self.locals) and self.locals[i]["group"] == g:
                m, o = self.locals[i], self.outcomes[i]
                line = [m["kind"], m.get("etype", 0), o["status"], o["action"], o["n_msgs"], o["index"], o["pos"],
                        o["committed"], len(self.emitted[i])]
                for em in self.emitted[i]:
                    line += list(em)
                recs.append(" ".join(str(x) for x in line))
                i += 1
            out.append(str(len(recs)))
            out += recs
            e = [int(x) for x in grows[g]]
            out.append(" ".join(str(x) for x in [e[2], e[4], int(strows[g, 1]), int(strows[g, 2])] + e[14:28]))
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


def kat_scenario(idle=0):
    """The tables of raft_prop_kats.json, one group each, interleaved with
    `idle` groups that get no record.  Returns (scenario, [(name, group)])."""
    k = load_kats()
    sc = Scenario()
    rng = random.Random(5)
    named = []
    cases = k["cases"]
    for j, c in enumerate(cases):
        for _ in range(idle // len(cases) + (j < idle % len(cases))):
            sc.add_group([1, 1, rng.randrange(1, 9)], [(1, 2, 3), (2, 0, 3), (3, rng.randrange(3), 3)],
                         log_offset=rng.randrange(100), committed=1)
        g = sc.add_group(c["log_terms"], c["prs"], gid=c["id"], term=c["term"], committed=c["committed"],
                         log_offset=c["log_offset"], pending_conf=c["pending_conf"])
        sc.add_run(g, c["run"])
        named.append((c["name"], g))
    return sc, named


def check_kats(sc, named):
    """The tables' wanted values against the scenario's outcomes."""
    k = load_kats()
    _, grows, strows, _, _ = sc.expected()
    first = {g: i for g, i in sc.runs}
    for (name, g), c in zip(named, k["cases"]):
        assert name == c["name"]
        i, w = first[g], c["want"]
        outs = sc.outcomes[i:i + len(c["run"])]
        msgs = sc.messages[outs[0]["msg_first"]:outs[-1]["msg_first"] + outs[-1]["n_msgs"]]
        if "actions" in w:
            assert [o["action"] for o in outs] == w["actions"], name
        if "committed" in w:
            assert outs[-1]["committed"] == w["committed"], name
        if "n_msgs" in w:
            assert len(msgs) == w["n_msgs"], name
        if "index" in w:
            assert outs[-1]["index"] == w["index"], name
        if "nlog" in w:
            assert int(grows[g, 4]) == w["nlog"], name
        if "pending_conf" in w:
            assert int(strows[g, 2]) == w["pending_conf"], name
        if "msgs" in w:
            got = [dict(type=m["type"], to=m["to"], index=m["index"], log_term=m["log_term"], commit=m["commit"],
                        n_ents=(m["ents"] or (0, 0))[1], term=m["term"]) for m in msgs]
            assert got == w["msgs"], (name, got)


NEXTS = ("below", "at", "above")
RUNS = ("P", "B", "PP", "PCP", "CC", "BPB")


def lattice_scenario(seed=3):
    """peers {1, 3, 4, 7} x offset {0, 5} x RUNS x pending_conf {0, 1} x a
    peer's next {below, at, above the offset} (288 groups), then groups whose
    id is not among the peers and one with eight peers.  A 4-entry log whose
    last term is the leader's."""
    rng = random.Random(seed)
    sc = Scenario()
    for np_ in (1, 3, 4, 7):
        for off in (0, 5):
            for what in RUNS:
                for pend in (0, 1):
                    for where in NEXTS:
                        lead = rng.randrange(np_)
                        ids = [100 + 10 * k + rng.randrange(10) for k in range(np_)]
                        last = off + 3
                        odd = (lead + 1) % np_
                        prs = []
                        for k, p in enumerate(ids):
                            if k == lead:
                                prs.append((p, last, last + 1))
                            elif k == odd:
                                nxt = {"below": (off - 1) & M64, "at": off, "above": off + 1 + rng.randrange(4)}[where]
                                prs.append((p, rng.choice([0, last]), nxt))
                            else:
                                prs.append((p, rng.choice([0, off + 1, last]), off + 1 + rng.randrange(4)))
                        snap = dict(index=off, term=1, data_off=3, data_len=4, nodes_off=1, n_nodes=2, removed_off=5,
                                    n_removed=1) if off and rng.random() < 0.7 else None
                        g = sc.add_group([1, 1, 2, 3], prs, gid=ids[lead], term=3, committed=off + 1, log_offset=off,
                                         snap=snap, pending_conf=pend, unstable=off + rng.randrange(6))
                        sc.add_run(g, what)
    three = [(1, 3, 4), (2, 0, 3), (3, 3, 4)]
    for what in ("P", "BPB", "CB"):
        sc.add_run(sc.add_group([1, 1, 2, 3], three, gid=9, term=3, committed=1), what)
    g = sc.add_group([1, 1, 2, 3], three + [(4, 0, 1), (5, 0, 1), (6, 0, 1), (7, 0, 1)], gid=1, term=3, n_peers=8)
    sc.add_run(g, "BP")
    return sc


def boundary_scenario(n, seed=9):
    """n records in runs of 1-5, except that a run of 6 starts three records
    before the 64th, 256th and 1024th record: a run straddles each wave and
    workgroup seam.  Three peers."""
    rng = random.Random(seed)
    sc = Scenario()
    pos = 0
    while pos < n:
        to_seam = min([b - 3 - pos for b in (64, 256, 1024) if b - 3 >= pos] or [n])
        length = 6 if to_seam == 0 else min(rng.randrange(1, 6), to_seam)
        length = min(length, n - pos)
        off = rng.choice([0, 9])
        g = sc.add_group([1, 1, 2, 2], [(1, off + 3, off + 4), (2, rng.choice([0, off + 3]), off + 3), (3, 0, off + 4)],
                         term=2, committed=off + 1, log_offset=off, room=6, pending_conf=rng.randrange(2))
        sc.add_run(g, "".join(rng.choice("PPPCB") for _ in range(length)))
        pos += length
    return sc


def long_scenario(lengths, lead_in=0, seed=6):
    """`lead_in` single-record groups, then one group per length with a run of
    that many records (mostly proposals)."""
    rng = random.Random(seed)
    sc = Scenario()
    for _ in range(lead_in):
        sc.add_run(sc.add_group([1, 2], [(1, 1, 2), (2, 0, 2)], term=2, room=1), "P")
    for length in lengths:
        g = sc.add_group([1, 1, 2], [(1, 2, 3), (2, 2, 3), (3, 0, 1)], term=2, committed=1, room=length)
        sc.add_run(g, "".join(rng.choice("PPPPPPCB") for _ in range(length)))
    return sc


def wide_scenario(n, tail, seed=4):
    """n groups of three peers with one proposal each, then one run of `tail`
    records; cheap to build."""
    rng = random.Random(seed)
    sc = Scenario(snaps=False)
    for g in range(n):
        sc.add_group([1, 2, 2], [(1, 2, 3), (2, 0, 3), (3, 0, 2)], term=2, committed=rng.randrange(2), room=1)
        sc.add_prop(g, data_off=g, data_len=1)
    g = sc.add_group([1, 2, 2], [(1, 2, 3), (2, 2, 3), (3, 0, 2)], term=2, room=tail)
    sc.add_run(g, "P" * tail)
    return sc


def random_scenario(seed, G=1500, n=3000):
    """Random leaders (0-8 peers, logs of 0-12 entries, three kinds of offset)
    and about n records in runs of 1-8."""
    rng = random.Random(seed)
    sc = Scenario()
    for g in range(G):
        np_ = rng.choice([1, 2, 3, 3, 3, 4, 5, 5, 5, 6, 7])
        nlog = rng.randint(1, 12) if rng.random() < 0.97 else 0
        off = rng.choice([0, rng.randrange(1, 5000), (1 << 62) + rng.randrange(1 << 40)])
        t, terms = rng.randrange(1, 4), []
        for _ in range(nlog):
            t += rng.random() < 0.3
            terms.append(t)
        if rng.random() < 0.15:
            t += 1
        last = (off + nlog - 1) & M64
        lead = rng.randrange(np_)
        ids = rng.sample(range(1, 1 << 20), np_)
        prs = []
        for k, p in enumerate(ids):
            if k == lead:
                prs.append((p, last, (last + 1) & M64))
            elif rng.random() < 0.5:
                roll = rng.random()
                prs.append((p, 0, off if roll < 0.06 else (off - 1) & M64 if roll < 0.1 else
                            off + 1 + rng.randrange(nlog + 2)))
            else:
                m = off + rng.randrange(nlog + 1)
                prs.append((p, m, m + 1))
        snap = dict(index=off, term=1, data_off=rng.randrange(100), data_len=rng.randrange(100),
                    nodes_off=rng.randrange(9), n_nodes=np_, removed_off=rng.randrange(9),
                    n_removed=rng.randrange(3)) if off and rng.random() < 0.6 else None
        roll = rng.random()
        gid = 7 << 20 if roll < 0.02 else ids[lead]                    # an id that is not a key of prs
        n_peers = 8 if roll > 0.985 else 0 if roll > 0.98 else None
        if n_peers == 8:                                               # seven distinct ids: the record is valid
            prs += [((1 << 20) + k, 0, off + 1) for k in range(7 - np_)]
        sc.add_group(terms, prs, gid=gid, term=t, committed=off + rng.randrange(0, nlog + 1), log_offset=off,
                     snap=snap, n_peers=n_peers, room=8, pending_conf=int(rng.random() < 0.3),
                     unstable=(off + rng.randrange(nlog + 3)) & M64)
    order = list(range(G))
    rng.shuffle(order)
    for g in order:
        if len(sc.locals) >= n:
            break
        sc.add_run(g, "".join(rng.choice("PPPCCBB") for _ in range(rng.choice([1, 1, 2, 2, 3, 3, 4, 5, 6, 7, 8]))))
    return sc
