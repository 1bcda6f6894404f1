"""Cases and the Python restatement for the batched Ready
(eready_batch_device): newReady (raft/node.go:332-348), node.run's accept
branch (:239-255) and the record order of wal.Save (wal/wal.go:281-288) over
the records the call reads.  Holds the loader of the reference's own tables
(tests/golden/raft_ready_kats.json), an edge lattice and the seeded random
generator that tests/host/ready_forms.cpp restates draw for draw."""
import json
import os

import numpy as np

from vote_step_cases import SplitMix

M64 = (1 << 64) - 1
OK, PANIC_BOUNDS, UNSUPPORTED = 0, 33, 48
E_INVAL, E_NOMEM = -2, -3
SOFT, HARD, SNAP, UPDATES = 1, 2, 4, 8
SAVE_ENTRY, SAVE_STATE, SAVE_CUT = 2, 3, 4
GROUP_WORDS, STATE_WORDS, VSTATE_WORDS, RSTATE_WORDS, SNAP_WORDS, ENTRY_WORDS = 32, 4, 8, 8, 8, 5
RESULT_WORDS, SAVE_WORDS = 12, 7
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raft_ready_kats.json")
RSTATE_KEYS = ("hs_term", "hs_vote", "hs_commit", "lead", "state", "snapi", "applied", "soft_dirty")


# ---- the restatement -------------------------------------------------------------

def log_slice(off, nlog, lo, hi):
    """raftLog.slice(lo, hi) (raft/log.go:202-210) as (status, first position, count); count 0 is nil."""
    last = (nlog - 1 + off) & M64
    if lo >= hi:
        return OK, 0, 0
    if lo < off or lo > last or hi - 1 < off or hi - 1 > last:
        return OK, 0, 0
    lo_p, hi_p = lo - off, hi - off
    if lo_p > hi_p or hi_p > nlog:
        return PANIC_BOUNDS, 0, 0
    return OK, lo_p, hi_p - lo_p


def new_ready(g, log):
    """newReady + containsUpdates (without Messages) + what accepting leaves,
    for one group.  g: term, committed, log_offset, unstable, vote, lead,
    state, snap_index and the eight eready_state words; log: the entry rows
    (term, index, data_off, data_len, type | data_nil << 32)."""
    off, nlog = g["log_offset"], len(log)
    last = (nlog - 1 + off) & M64
    void = dict(status=OK, flags=0, term=0, vote=0, commit=0, ents_pos=0, n_ents=0, committed_pos=0, n_committed=0,
                n_save=0, lead=0, state=0, applied=g["applied"], unstable=g["unstable"])
    st, upos, un = log_slice(off, nlog, g["unstable"], (last + 1) & M64)
    cpos = cn = 0
    if st == OK and g["committed"] > g["applied"]:
        st, cpos, cn = log_slice(off, nlog, (g["applied"] + 1) & M64, (g["committed"] + 1) & M64)
    if st == OK and any((int(e[4]) >> 32) == 2 for e in log[upos:upos + un]):
        st = UNSUPPORTED                      # an unstable entry whose Data is not in d_data
    if st != OK:
        return dict(void, status=st)
    o = dict(void, ents_pos=upos, n_ents=un, committed_pos=cpos, n_committed=cn)
    if g["lead"] != g["plead"] or g["state"] != g["pstate"] or g["soft_dirty"]:
        o.update(flags=SOFT, lead=g["lead"], state=g["state"])
    if (g["term"], g["vote"], g["committed"]) != (g["hs_term"], g["hs_vote"], g["hs_commit"]):
        o.update(term=g["term"], vote=g["vote"], commit=g["committed"])
    if o["term"] or o["vote"] or o["commit"]:
        o["flags"] |= HARD
    if g["snap_index"] != g["snapi"] and g["snap_index"] != 0:
        o["flags"] |= SNAP
    if o["flags"] or un or cn:
        o["flags"] |= UPDATES
    o["n_save"] = un + (1 if o["flags"] & HARD else 0)
    if g["committed"] > g["applied"]:
        o["applied"] = g["committed"]
    o["unstable"] = (last + 1) & M64
    return o


def save_rows(o, log):
    """wal.Save(rd.HardState, rd.Entries) as ewal_save_rec word rows."""
    rows = []
    if o["flags"] & HARD:
        rows.append([SAVE_STATE, o["term"], o["vote"], o["commit"], 0, 0, 0])
    for e in log[o["ents_pos"]:o["ents_pos"] + o["n_ents"]]:
        w4 = int(e[4])
        rows.append([SAVE_ENTRY | ((w4 & 0xFFFFFFFF) << 32), int(e[0]), int(e[1]), 0, int(e[2]), int(e[3]), w4 >> 32])
    return rows


# ---- scenarios ---------------------------------------------------------------------

def entry(term=0, index=0, etype=0, data_off=0, data_len=0, data_nil=1):
    return [term, index, data_off, data_len, (etype & 0xFFFFFFFF) | (data_nil << 32)]


class Scenario:
    """G groups, each with its log window (room entries of slack behind it)."""

    def __init__(self):
        self.groups, self.logs, self.rooms, self.names = [], [], [], []
        self.with_snaps = True

    def add_group(self, log, room=0, name=None, **kw):
        g = dict(id=1, term=0, committed=0, log_offset=0, unstable=0, vote=0, lead=0, state=0, snap_index=0,
                 hs_term=0, hs_vote=0, hs_commit=0, plead=0, pstate=0, snapi=0, applied=0, soft_dirty=0)
        unknown = set(kw) - set(g)
        assert not unknown, unknown
        g.update(kw)
        self.groups.append(g)
        self.logs.append([list(e) for e in log])
        self.rooms.append(room)
        self.names.append(name)
        return len(self.groups) - 1

    def add_idle(self, k, nlog=2):
        """k groups with nothing to report: all stable, applied, HardState and SoftState as saved."""
        for _ in range(k):
            self.add_group([entry(1, i) for i in range(nlog)], term=1, committed=nlog - 1, unstable=nlog, vote=1,
                           lead=1, state=2, hs_term=1, hs_vote=1, hs_commit=nlog - 1, plead=1, pstate=2,
                           applied=nlog - 1)

    def pack(self):
        """(elead_group, elead_prop_state, evote_state, eready_state, elead_snap, ewal_entry) word rows."""
        G = len(self.groups)
        grows = np.zeros((G, GROUP_WORDS), dtype=np.uint64)
        srows = np.zeros((G, STATE_WORDS), dtype=np.uint64)
        vrows = np.zeros((G, VSTATE_WORDS), dtype=np.uint64)
        rrows = np.zeros((G, RSTATE_WORDS), dtype=np.uint64)
        nrows = np.zeros((G, SNAP_WORDS), dtype=np.uint64)
        ents, first = [], 0
        for k, (g, log, room) in enumerate(zip(self.groups, self.logs, self.rooms)):
            grows[k, :7] = [g["id"], g["term"], g["committed"], g["log_offset"], len(log), first, 1]
            grows[k, 7] = g["id"]
            srows[k, :2] = [len(log) + room, g["unstable"]]
            vrows[k, :3] = [g["state"], g["vote"], g["lead"]]
            rrows[k] = [g["hs_term"], g["hs_vote"], g["hs_commit"], g["plead"], g["pstate"], g["snapi"], g["applied"],
                        g["soft_dirty"]]
            nrows[k, :2] = [g["snap_index"], 1 if g["snap_index"] else 0]
            ents.extend(log)
            ents.extend([[0] * ENTRY_WORDS] * room)
            first += len(log) + room
        erows = np.array(ents, dtype=np.uint64).reshape(len(ents), ENTRY_WORDS)
        return grows, srows, vrows, rrows, (nrows if self.with_snaps else None), erows

    def expected(self, sel=None, emit=True):
        """What the call leaves: (eready_result rows, ewal_save_rec rows, the
        new elead_prop_state rows, the new eready_state rows, n_ready).  Also
        self.outcomes, the per-selection new_ready dicts."""
        grows, srows, vrows, rrows, _, _ = self.pack()
        sel = list(range(len(self.groups))) if sel is None else list(sel)
        res = np.zeros((len(sel), RESULT_WORDS), dtype=np.uint64)
        saves, self.outcomes, n_ready = [], [], 0
        for i, k in enumerate(sel):
            g, log = self.groups[k], self.logs[k]
            snaps_g = dict(g, snap_index=g["snap_index"] if self.with_snaps else 0)
            o = new_ready(snaps_g, log)
            self.outcomes.append(o)
            first = int(grows[k, 5])
            res[i] = [o["status"] | (o["flags"] << 32), o["term"], o["vote"], o["commit"],
                      first + o["ents_pos"] if o["n_ents"] else 0, o["n_ents"],
                      first + o["committed_pos"] if o["n_committed"] else 0, o["n_committed"], len(saves), o["n_save"],
                      o["lead"], o["state"]]
            rows = save_rows(o, log) if o["status"] == OK else []
            assert len(rows) == o["n_save"]
            saves.extend(rows)
            n_ready += 1 if o["flags"] & UPDATES else 0
            if emit and o["status"] == OK:
                if o["flags"] & SOFT:
                    rrows[k, 3], rrows[k, 4], rrows[k, 7] = g["lead"], g["state"], 0
                if o["flags"] & HARD:
                    rrows[k, :3] = [o["term"], o["vote"], o["commit"]]
                if o["flags"] & SNAP:
                    rrows[k, 5] = snaps_g["snap_index"]
                rrows[k, 6] = o["applied"]
                srows[k, 1] = o["unstable"]
        srec = np.array(saves, dtype=np.uint64).reshape(len(saves), SAVE_WORDS)
        return res, srec, srows, rrows, n_ready


# ---- the reference's own tables ----------------------------------------------------

def load_kats():
    with open(KATS) as f:
        return {k: v for k, v in json.load(f).items() if not k.startswith("_")}


def kat_scenario(idle=0):
    """One group per step of every table (`idle` idle groups before each), the
    entries' Data laid out one after another.  Returns (scenario, [(test name,
    step number, group, step)], the Data bytes)."""
    sc, named, data = Scenario(), [], bytearray()
    for name, table in load_kats().items():
        for j, step in enumerate(table["steps"]):
            sc.add_idle(idle)
            log = []
            for term, index, etype, hexdata in step["log"]:
                raw = bytes.fromhex(hexdata) if hexdata is not None else b""
                log.append(entry(term, index, etype, len(data) if raw else 0, len(raw), 1 if hexdata is None else 0))
                data += raw
            grp = dict(step["group"])
            prev = dict(step["prev"])
            for k in ("lead", "state"):
                if k in prev:
                    prev["p" + k] = prev.pop(k)
            g = sc.add_group(log, name="%s_%d" % (name, j), unstable=step["unstable"], **grp, **prev)
            named.append((name, j, g, step))
    return sc, named, bytes(data)


def check_kats(sc, named, outcomes=None):
    """Every step's Ready against the table's, and a chained step's `prev`
    against what accepting the step before leaves."""
    if outcomes is None:
        sc.expected()
        outcomes = {g: sc.outcomes[g] for _, _, g, _ in named}
    before = None
    for name, j, g, step in named:
        o, w, tag = outcomes[g], step["want"], (name, j)
        assert o["status"] == OK, tag
        assert bool(o["flags"] & SOFT) == (w["soft"] is not None), tag
        if w["soft"] is not None:
            assert [o["lead"], o["state"]] == w["soft"], tag
        assert [o["term"], o["vote"], o["commit"]] == w["hs"], tag
        assert bool(o["flags"] & HARD) == any(w["hs"]), tag
        assert ([o["ents_pos"], o["n_ents"]] if o["n_ents"] else None) == w["entries"], tag
        assert ([o["committed_pos"], o["n_committed"]] if o["n_committed"] else None) == w["committed"], tag
        assert bool(o["flags"] & SNAP) == (w["snap"] != 0), tag
        assert (bool(o["flags"] & UPDATES) or w["n_msgs"] > 0) == w["contains"], tag
        if "we" in step:                     # TestSoftStateEqual / TestIsHardStateEqual against the empty state
            assert (o["flags"] & (SOFT | HARD) == 0) == step["we"], tag
        if "after_unstable" in step:
            assert o["unstable"] == step["after_unstable"], tag
        if step.get("chained"):
            bo, bg = before
            acc = dict(hs_term=bg["hs_term"], hs_vote=bg["hs_vote"], hs_commit=bg["hs_commit"], plead=bg["plead"],
                       pstate=bg["pstate"], snapi=bg["snapi"], applied=bo["applied"], soft_dirty=bg["soft_dirty"])
            if bo["flags"] & SOFT:
                acc.update(plead=bg["lead"], pstate=bg["state"], soft_dirty=0)
            if bo["flags"] & HARD:
                acc.update(hs_term=bo["term"], hs_vote=bo["vote"], hs_commit=bo["commit"])
            if bo["flags"] & SNAP:
                acc["snapi"] = bg["snap_index"]
            assert {k: sc.groups[g][k] for k in acc} == acc, tag
            assert sc.groups[g]["unstable"] == bo["unstable"], tag
        before = (o, sc.groups[g])


# ---- the edge lattice --------------------------------------------------------------

def _log(n, off, **kw):
    return [entry(1 + k // 2, (off + k) & M64, data_off=8 * k, data_len=k % 3, data_nil=0 if k % 3 else k % 2, **kw)
            for k in range(n)]


def lattice_scenario():
    """unstable below / at / past log_offset and lastIndex x applied / committed
    on both sides of the window, on a 4-entry log at offsets 0, 5 and 2^64 - 2
    (a wrapped last index), an empty log at offset 0 and at offset 7; the
    all-zero HardState that differs from prev; a snapshot index of 0 against a
    non-zero snapi; data_nil == 2 inside and outside the unstable range."""
    sc = Scenario()
    for off, n in ((0, 4), (5, 4), (M64 - 1, 4), (0, 0), (7, 0), (M64, 1), (M64 - 3, 4)):
        last = (n - 1 + off) & M64
        marks = sorted({0, (off - 1) & M64, off, (off + 1) & M64, (last - 1) & M64, last, (last + 1) & M64,
                        (last + 2) & M64, M64})
        for unstable in marks:
            for applied, committed in ((off, off), (off, last), ((off - 1) & M64, last), (off, (last + 1) & M64),
                                       ((off + 1) & M64, (off + 2) & M64), (last, off), (M64, 0), (0, M64),
                                       ((last - 1) & M64, last)):
                sc.add_group(_log(n, off), term=2, vote=1, log_offset=off, unstable=unstable, applied=applied,
                             committed=committed, hs_term=2, hs_vote=1, hs_commit=committed if unstable & 1 else 0,
                             name="lat_%x_%d_%x" % (off, n, unstable))
    # a HardState that differs from prev but is the empty state: never reported, never accepted
    sc.add_group(_log(2, 0), unstable=2, hs_term=3, hs_vote=1, hs_commit=1, name="zero_hs")
    sc.add_group(_log(2, 0), unstable=2, name="zero_hs_equal")
    # the snapshot: index 0 against a non-zero snapi is no snapshot; equal is none; different is one
    for snap_index, snapi in ((0, 4), (4, 4), (4, 3), (4, 0), (M64, 0)):
        sc.add_group(_log(2, 4), log_offset=4, unstable=6, committed=4, applied=4, hs_commit=4, snap_index=snap_index,
                     snapi=snapi, name="snap_%x_%x" % (snap_index, snapi))
    # the SoftState: each word alone, the dirty bit alone
    for lead, state, plead, pstate, dirty in ((1, 0, 0, 0, 0), (0, 2, 0, 0, 0), (1, 2, 1, 2, 0), (1, 2, 1, 2, 1),
                                              (0, 0, 0, 1, 0), (3, 1, 2, 1, 1)):
        sc.add_group(_log(2, 0), unstable=2, lead=lead, state=state, plead=plead, pstate=pstate, soft_dirty=dirty,
                     name="soft")
    # data_nil == 2: unstable (unsupported), stable (fine), committed but stable (fine), at both ends of a long run
    for pos, unstable, n in ((3, 2, 5), (1, 2, 5), (4, 4, 5), (2, 3, 5), (0, 0, 3), (69, 1, 70), (5, 1, 70), (4, 1, 70),
                             (68, 1, 69), (299, 0, 300)):
        log = _log(n, 0)
        log[pos][4] = (log[pos][4] & 0xFFFFFFFF) | (2 << 32)
        sc.add_group(log, term=1, committed=n - 1, unstable=unstable, applied=0, name="outside_%d_%d" % (pos, unstable))
    return sc


# ---- the random generator (shared, draw for draw, with tests/host/ready_forms.cpp) ----

OFF_TABLE = (0, 0, 0, 5, 1000, 1000, M64 - 1, 7)


def random_group(seed, j):
    """(group dict for Scenario.add_group, log rows)."""
    r = SplitMix(seed, j)
    off = OFF_TABLE[r.rnd(8)]
    nlog = r.rnd(7)
    log, data_off = [], 0
    for k in range(nlog):
        etype = 1 if r.rnd(4) == 0 else 0
        data_len = r.rnd(100) if r.rnd(3) else 0
        data_nil = r.rnd(2) if data_len == 0 else 0
        if r.rnd(40) == 0:
            data_nil = 2
        log.append(entry(1 + r.rnd(3), (off + k) & M64, etype, data_off, data_len, data_nil))
        data_off += data_len
    end = (off + nlog) & M64
    rel = r.rnd(6)
    unstable = (end, end, (off + r.rnd(nlog + 1)) & M64, (off + r.rnd(nlog + 2)) & M64, 0, (off - 1) & M64)[rel]
    committed = (off + r.rnd(nlog + 2)) & M64
    rel = r.rnd(4)
    span = (committed - off) & M64
    applied = (committed, (off + r.rnd(span + 1)) & M64, (committed - 1) & M64, off)[rel]
    term = 1 + r.rnd(5)
    vote = r.rnd(3)
    lead, state = r.rnd(3), r.rnd(3)
    g = dict(term=term, committed=committed, log_offset=off, unstable=unstable, vote=vote, lead=lead, state=state,
             applied=applied)
    if r.rnd(3) == 0:
        g.update(hs_term=term, hs_vote=vote, hs_commit=committed)
    else:
        g.update(hs_term=(term - r.rnd(2)) & M64, hs_vote=vote, hs_commit=(committed - r.rnd(2)) & M64)
    g["plead"] = lead if r.rnd(2) else r.rnd(3)
    g["pstate"] = state if r.rnd(2) else r.rnd(3)
    g["soft_dirty"] = 1 if r.rnd(8) == 0 else 0
    g["snap_index"] = (off if off else 3) if r.rnd(3) == 0 else 0
    g["snapi"] = g["snap_index"] if r.rnd(2) else r.rnd(3)
    return g, log


def random_scenario(seed, groups=3000, first=0):
    sc = Scenario()
    for j in range(first, first + groups):
        g, log = random_group(seed, j)
        sc.add_group(log, **g)
    return sc


CLASSES = ("void", "soft", "hard", "snap", "updates", "ents", "ents_nil", "committed", "committed_nil")


def classes_of(o):
    """The class counters a group adds to (CLASSES order)."""
    if o["status"] != OK:
        return [1, 0, 0, 0, 0, 0, 0, 0, 0]
    f = o["flags"]
    return [0, 1 if f & SOFT else 0, 1 if f & HARD else 0, 1 if f & SNAP else 0, 1 if f & UPDATES else 0,
            1 if o["n_ents"] else 0, 0 if o["n_ents"] else 1, 1 if o["n_committed"] else 0,
            0 if o["n_committed"] else 1]


def _fnv(h, v):
    return ((h ^ (v & M64)) * 0x100000001B3) & M64


def digest(seed, groups):
    """The digest tests/host/ready_forms.cpp prints, from the restatement:
    (hash, class counts)."""
    h, counts = 0xCBF29CE484222325, [0] * len(CLASSES)
    for j in range(groups):
        g, log = random_group(seed, j)
        o = new_ready(g, log)
        counts = [a + b for a, b in zip(counts, classes_of(o))]
        for v in (o["status"], o["flags"], o["term"], o["vote"], o["commit"], o["ents_pos"], o["n_ents"],
                  o["committed_pos"], o["n_committed"], o["n_save"], o["lead"], o["state"], o["applied"], o["unstable"]):
            h = _fnv(h, v)
        for row in (save_rows(o, log) if o["status"] == OK else []):
            for v in row:
                h = _fnv(h, v)
    return h, counts


# ---- shapes of the GPU suite -------------------------------------------------------

def run_scenario(lengths, idle_between=0):
    """One group per unstable run length (a log of length + 2 entries whose
    last `length` are unstable, one newly committed), `idle_between` idle groups
    after each."""
    sc = Scenario()
    for k, n in enumerate(lengths):
        log = [entry(1 + (k + i) % 3, i, i % 2, 16 * i, (i * 7 + k) % 11, 0) for i in range(n + 2)]
        sc.add_group(log, term=3, vote=1 + k % 2, committed=1, applied=0, unstable=2, hs_term=3, hs_vote=1,
                     hs_commit=0 if k % 3 else 1, lead=1, state=2, plead=1, pstate=2, name="run_%d" % n)
        sc.add_idle(idle_between)
    return sc
