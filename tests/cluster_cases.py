"""The step calls stated over raft_model: for each batched call, what the call
adds to raft.Step -- runs of adjacent records per group, a panic that leaves
the group as it was and puts the rest of its run at NOT_STEPPED, the follower
call's deferral, and the limits of the records (include/ewal.h: more than seven
peers, a vote without a slot, a snapshot that does not fit) -- wrapped around
the one model.  Every function takes the arrays a call reads, decodes each
named group with raft_model.from_arrays, steps the model, encodes it with
raft_model.to_arrays and returns the arrays, result rows and emsg_out rows the
call must leave, so a restatement's expected() -- either family's -- or the
device's output is compared with it word for word.  The numbers in this part
are include/ewal.h's; it reads no *_cases.py.

Below it, the cluster driver: `clusters x nodes` groups in one set of arrays, a
lossy network and the host's part of Step (the router), over a pluggable
backend -- the model itself, the restatements' expected(), or the device."""
import numpy as np

import raft_model as M
from raft_model import M64, PEERS

MAX_NODES = 64
OK, UNSUPPORTED = 0, 48
STATUS = {M.BOUNDS: 33, M.COMMITTED_CONFLICT: 38, M.NIL_PROGRESS: 39, M.NEED_SNAPSHOT: 40, M.FIRST_ENTRY: 41,
          M.LEADER_TO_CANDIDATE: 42, M.NIL_ENTRY: 43, M.DOUBLE_CONF: 44, M.COMPACT_APPLIED: 45,
          M.COMPACT_BOUNDS: 46}   # EWAL_PANIC_*
MSG_WORDS = 18
ARRAYS = ("groups", "pstate", "vstate", "rstate", "snaps", "ents")
CANARY = 0xC0FFEE00DEADBEEF
# every counter a call returns beside its arrays; a backend returns those of its call, all of them
COUNTERS = ("n_msgs", "n_won", "n_committed", "n_appended", "n_restored", "n_save", "n_ready", "n_compacted",
            "n_moved")


class Unsupported(Exception):
    """A record the group records cannot state (EWAL_UNSUPPORTED_ENCODING)."""


def _step(r, m, limits=None):
    """Step(m) on r.  Returns the status; a panic or an unsupported record
    leaves r as it was, with nothing sent.  limits(r, before) may raise
    Unsupported after the step."""
    before = M.saved(r)
    r.msgs = []
    try:
        r.Step(m)
        if limits:
            limits(r, before)
    except M.Panic as p:
        M.put_back(r, before)
        r.msgs, r.trace = [], []
        return STATUS[p.name]
    except Unsupported:
        M.put_back(r, before)
        r.msgs, r.trace = [], []
        return UNSUPPORTED
    return OK


def msg_row(m, node, efirst):
    """The emsg_out words of a model message sent by node, whose window starts at efirst."""
    row = [0] * MSG_WORDS
    row[0:7] = [m["Type"], m["To"], m["From"], m["Term"], m["LogTerm"], m["Index"], m["Commit"]]
    if m["Entries"]:
        # the entries are a view of the sender's window
        row[7], row[8] = (efirst + m["Entries"][0]["Index"] - node.r.raftLog.offset) & M64, len(m["Entries"])
    if m["Snapshot"] is not None:
        row[9:17] = M.row_of_snapshot(m["Snapshot"])
    row[17] = int(m["Reject"])
    return row


def _copies(a, keys):
    return {k: (None if a.get(k) is None else a[k].copy()) for k in keys}


def _rows(rows, width):
    return np.array(rows, dtype=np.uint64).reshape(len(rows), width)


# ---- efollow_step_batch_device ---------------------------------------------------------------

F_NOT_STEPPED, F_IGNORED, F_NO_CASE, F_APPENDED, F_REJECTED, F_RESTORED, F_SNAP_STALE, F_DEFERRED, F_PANICKED = range(9)
F_ACTION = dict(ignored=F_IGNORED, no_case=F_NO_CASE, appended=F_APPENDED, rejected=F_REJECTED, restored=F_RESTORED,
                snap_stale=F_SNAP_STALE)


def follow_call(a):
    """a: the dict follow_cases.Scenario.pack() gives (groups, pstate, vstate,
    rstate, snaps, ents, src, in_snaps, u64, msgs).  Returns a dict with the
    arrays after the call, res_rows (n, 12), msg_rows (m, 18), and counters."""
    out = _copies(a, ("groups", "pstate", "vstate", "rstate", "snaps", "ents"))
    src = a["ents"] if a["src"] is None else a["src"]
    n = len(a["msgs"])
    res, rows = np.zeros((n, 12), dtype=np.uint64), []
    n_appended = n_restored = 0
    i = 0
    while i < n:
        g = int(a["msgs"][i][0])
        node = M.from_arrays(out, g, u64=a["u64"])
        r, efirst = node.r, int(out["groups"][g, 5])
        stopped = deferring = grown = False
        while i < n and int(a["msgs"][i][0]) == g:
            w = [int(x) for x in a["msgs"][i]]
            ents = [M.entry_of_row(e) for e in src[w[7]:w[7] + w[8]]]
            for e in ents:
                if e["data_nil"] == 0:
                    e["data_off"] = (e["data_off"] + w[9]) & M64
            m = M.Message(w[1], From=w[2], Term=w[3], Index=w[4], LogTerm=w[5], Commit=w[6], Entries=ents)
            if w[1] == M.MSG_SNAP:
                m["Snapshot"] = M.snapshot_of_row(a["in_snaps"][w[10]], a["u64"])
            status, action, flags, msgs, ins = OK, F_NOT_STEPPED, 0, [], (0, 0, 0, 0)
            if stopped:
                pass
            elif node.n_peers > PEERS:
                status, action = UNSUPPORTED, F_PANICKED
            elif deferring or (grown and (w[8] > 0 or w[1] == M.MSG_SNAP)):
                action, deferring = F_DEFERRED, True
            else:
                lg0 = r.raftLog
                offset0, nlog0 = lg0.offset, len(lg0.ents)
                ci = _conflict(lg0, w[4], w[5], ents) if w[1] == M.MSG_APP else 0

                def limits(r, before):
                    if "restored" not in r.trace:
                        return
                    votes = {} if ("term_switch" in r.trace or "conceded" in r.trace) else before["votes"]
                    nodes = m["Snapshot"]["Nodes"]
                    if len(nodes) > MAX_NODES or len(set(nodes)) > PEERS or votes:
                        raise Unsupported()
                status = _step(r, m, limits)
                if status != OK:
                    action = F_PANICKED
                else:
                    action = [F_ACTION[t] for t in r.trace if t in F_ACTION][-1]
                    flags = ("term_switch" in r.trace) | ("conceded" in r.trace) << 1
                    msgs = r.readMessages()
                    if action == F_APPENDED and ci:
                        k = (ci - w[4] - 1) & M64
                        ins = (ci, k, len(ents) - k, (ci - offset0) & M64)
                        assert ins[3] <= nlog0
            stopped = stopped or status != OK
            ci, app_k, n_app, dst_pos = ins
            if n_app:
                grown = True
                n_appended += n_app
            if action == F_RESTORED:
                grown = True
                n_restored += 1
            res[i] = [status | (action << 32), len(rows), len(msgs), ci, w[7] + app_k if n_app else 0, n_app,
                      efirst + dst_pos if n_app else 0, r.raftLog.lastIndex(), r.raftLog.committed, r.Term,
                      r.state | (flags << 32), 0]
            rows += [msg_row(x, node, efirst) for x in msgs]
            i += 1
        if node.n_peers <= PEERS:
            M.to_arrays(node, out, g)
    out.update(res_rows=res, msg_rows=_rows(rows, MSG_WORDS), n_msgs=len(rows), n_appended=n_appended,
               n_restored=n_restored)
    return out


def _conflict(lg, index, term, ents):
    """efollow_result.conflict: findConflict's value inside maybeAppend, 0 where it is not reached."""
    try:
        return lg.findConflict((index + 1) & M64, ents) if lg.matchTerm(index, term) else 0
    except M.Panic:
        return 0


# ---- evote_step_batch_device -----------------------------------------------------------------

(V_NOT_STEPPED, V_IGNORED, V_GRANTED, V_REJECTED, V_CAMPAIGNED, V_WON, V_LOST, V_POLLED, V_NO_CASE,
 V_PANICKED) = range(10)
V_ACTION = dict(ignored=V_IGNORED, vote_granted=V_GRANTED, vote_rejected=V_REJECTED, won=V_WON, lost=V_LOST,
                polled=V_POLLED, no_case=V_NO_CASE)


def vote_call(a):
    """a: groups, pstate, vstate, snaps (or None), ents and msgs, a list of
    dicts (group, kind, from_, term, index, log_term, reject).  Returns the
    arrays after the call, res_rows (n, 6) and msg_rows."""
    out = _copies(a, ("groups", "pstate", "vstate", "snaps", "ents"))
    n = len(a["msgs"])
    res, rows = np.zeros((n, 6), dtype=np.uint64), []
    i = 0
    while i < n:
        g = a["msgs"][i]["group"]
        node = M.from_arrays(out, g)
        r, efirst = node.r, int(out["groups"][g, 5])
        stopped = False
        while i < n and a["msgs"][i]["group"] == g:
            x = a["msgs"][i]
            # a msgHup is a local message (raft.go:296, node.go:281-284): the record's term is not read
            m = M.Message(x["kind"], From=x["from_"], Term=0 if x["kind"] == M.MSG_HUP else x["term"],
                          Index=x["index"], LogTerm=x["log_term"], Reject=bool(x["reject"]))
            status, action, flags, msgs = OK, V_NOT_STEPPED, 0, []
            if stopped:
                pass
            elif node.n_peers > PEERS:
                status, action = UNSUPPORTED, V_PANICKED
            elif x["kind"] == M.MSG_HUP and r.state != M.LEADER and r.id not in r.prs:
                status, action = UNSUPPORTED, V_PANICKED     # not promotable: its self vote has no slot
            elif (x["kind"] == M.MSG_VOTE_RESP and r.state == M.CANDIDATE and x["from_"] not in r.prs and
                  (x["term"] == 0 or x["term"] == r.Term)):
                status, action = UNSUPPORTED, V_PANICKED     # Go would count it; the mask cannot
            else:
                status = _step(r, m)
                if status != OK:
                    action = V_PANICKED
                elif x["kind"] == M.MSG_HUP:
                    action = V_WON if r.state == M.LEADER else V_CAMPAIGNED
                else:
                    action = [V_ACTION[t] for t in r.trace if t in V_ACTION][-1]
                    flags = int("term_switch" in r.trace)
                msgs = r.readMessages()
            stopped = stopped or status != OK
            res[i] = [status | (action << 32), len(rows), len(msgs), r.Term, r.Vote, r.state | (flags << 32)]
            rows += [msg_row(y, node, efirst) for y in msgs]
            i += 1
        if node.n_peers <= PEERS:
            M.to_arrays(node, out, g)
    n_won = sum(1 for r in res if int(r[0]) >> 32 == V_WON)
    out.update(res_rows=res, msg_rows=_rows(rows, MSG_WORDS), n_msgs=len(rows), n_won=n_won)
    return out


# ---- elead_step_batch_device -----------------------------------------------------------------

L_NOT_STEPPED, L_IGNORED, L_STEP_DOWN, L_STALE, L_PROBE, L_UPDATED, L_COMMITTED, L_PANICKED = range(8)
L_ACTION = dict(ignored=L_IGNORED, stale=L_STALE, probe=L_PROBE, updated=L_UPDATED, committed=L_COMMITTED)


def leader_view(a):
    """The leader-side calls read a group without its evote_state and with a
    window that holds exactly the log: every named group is a leader."""
    G = len(a["groups"])
    b = dict(a)
    if b.get("pstate") is None:
        b["pstate"] = np.zeros((G, 4), dtype=np.uint64)
        b["pstate"][:, 0] = a["groups"][:, 4]
    b["vstate"] = np.zeros((G, 8), dtype=np.uint64)
    b["vstate"][:, 0] = M.LEADER
    return b


def lead_step_call(a):
    """a: groups, snaps (or None), ents, and resps, a list of dicts (group,
    from_, term, index, reject).  A higher term is the caller's to step
    (ELEAD_STEP_DOWN: nothing changes, the rest of the run is not stepped)."""
    b = leader_view(a)
    out = _copies(b, ("groups", "pstate", "vstate", "snaps", "ents"))
    n = len(a["resps"])
    res, rows = np.zeros((n, 6), dtype=np.uint64), []
    i = 0
    while i < n:
        g = a["resps"][i]["group"]
        node = M.from_arrays(out, g)
        r, efirst = node.r, int(out["groups"][g, 5])
        stopped = False
        while i < n and a["resps"][i]["group"] == g:
            x = a["resps"][i]
            m = M.Message(M.MSG_APP_RESP, From=x["from_"], Term=x["term"], Index=x["index"], Reject=bool(x["reject"]))
            status, action, msgs = OK, L_NOT_STEPPED, []
            if stopped:
                pass
            elif node.n_peers > PEERS:
                status, action = UNSUPPORTED, L_PANICKED
            elif x["term"] > r.Term:
                action = L_STEP_DOWN
            else:
                status = _step(r, m)
                action = L_PANICKED if status != OK else [L_ACTION[t] for t in r.trace if t in L_ACTION][-1]
                msgs = r.readMessages()
            stopped = stopped or status != OK or action == L_STEP_DOWN
            pr = None if node.n_peers > PEERS else r.prs.get(x["from_"])
            res[i] = [status | (action << 32), len(rows), len(msgs), r.raftLog.committed, pr.match if pr else 0,
                      pr.next if pr else 0]
            rows += [msg_row(y, node, efirst) for y in msgs]
            i += 1
        if node.n_peers <= PEERS:
            M.to_arrays(node, out, g)
    return dict(groups=out["groups"], ents=out["ents"], res_rows=res, msg_rows=_rows(rows, MSG_WORDS),
                n_msgs=len(rows), n_committed=sum(1 for r in res if int(r[0]) >> 32 == L_COMMITTED))


# ---- elead_local_batch_device ----------------------------------------------------------------

P_NOT_STEPPED, P_BEAT, P_APPENDED, P_DROPPED, P_PANICKED = range(5)
P_ACTION = dict(beat=P_BEAT, proposed=P_APPENDED, dropped=P_DROPPED)


def lead_local_call(a):
    """a: groups, pstate, snaps (or None), ents, and locals, a list of dicts
    (group, kind, and for a msgProp etype, data_off, data_len, data_nil)."""
    b = leader_view(a)
    out = _copies(b, ("groups", "pstate", "vstate", "snaps", "ents"))
    n = len(a["locals"])
    res, rows, n_appended = np.zeros((n, 6), dtype=np.uint64), [], 0
    i = 0
    while i < n:
        g = a["locals"][i]["group"]
        node = M.from_arrays(out, g)
        r, efirst = node.r, int(out["groups"][g, 5])
        stopped = False
        while i < n and a["locals"][i]["group"] == g:
            x = a["locals"][i]
            m = M.Message(x["kind"], From=r.id)
            if x["kind"] == M.MSG_PROP:
                m["Entries"] = [M.Entry(Type=x.get("etype", 0), data_off=x["data_off"], data_len=x["data_len"],
                                        data_nil=int(bool(x["data_nil"])))]
            status, action, msgs, index, pos = OK, P_NOT_STEPPED, [], 0, 0
            if stopped:
                pass
            elif node.n_peers > PEERS:
                status, action = UNSUPPORTED, P_PANICKED
            else:
                status = _step(r, m)
                action = P_PANICKED if status != OK else [P_ACTION[t] for t in r.trace if t in P_ACTION][-1]
                msgs = r.readMessages()
                if action == P_APPENDED:
                    index, pos = r.raftLog.lastIndex(), efirst + len(r.raftLog.ents) - 1
                    n_appended += 1
            stopped = stopped or status != OK
            res[i] = [status | (action << 32), len(rows), len(msgs), index, pos, r.raftLog.committed]
            rows += [msg_row(y, node, efirst) for y in msgs]
            i += 1
        if node.n_peers <= PEERS:
            M.to_arrays(node, out, g)
    return dict(groups=out["groups"], pstate=out["pstate"], ents=out["ents"], res_rows=res,
                msg_rows=_rows(rows, MSG_WORDS), n_msgs=len(rows), n_appended=n_appended)


# ---- eready_batch_device ---------------------------------------------------------------------

R_SOFT, R_HARD, R_SNAP, R_UPDATES = 1, 2, 4, 8
SAVE_ENTRY, SAVE_STATE = 2, 3
NO_HARD = dict(Term=0, Vote=0, Commit=0)


def ready_call(a):
    """a: groups, pstate, vstate, rstate, snaps (or None), ents, and sel, the
    selected group numbers (None: every group in order).  newReady without its
    Messages, node.run's accept, and wal.Save's record order.  Returns pstate,
    rstate, res_rows (n, 12), save_rows (m, 7) and n_ready."""
    out = _copies(a, ARRAYS)
    sel = range(len(a["groups"])) if a.get("sel") is None else [int(g) for g in a["sel"]]
    res, saves, n_ready = np.zeros((len(sel), 12), dtype=np.uint64), [], 0
    for i, g in enumerate(sel):
        node = M.from_arrays(out, g)
        r, lg, efirst = node.r, node.r.raftLog, int(out["groups"][g, 5])
        try:
            rd = node.newReady()
        except M.Panic as p:
            res[i, 0], res[i, 8] = STATUS[p.name], len(saves)
            continue
        if any(e["data_nil"] == 2 for e in rd["Entries"]):      # an unstable entry whose Data is not in d_data
            res[i, 0], res[i, 8] = UNSUPPORTED, len(saves)
            continue
        un, cn = len(rd["Entries"]), len(rd["CommittedEntries"])
        hard = rd["HardState"] != NO_HARD
        flags = (R_SOFT if rd["SoftState"] is not None else 0) | (R_HARD if hard else 0) | \
            (R_SNAP if rd["Snapshot"]["Index"] != 0 else 0)
        if flags or un or cn:
            flags |= R_UPDATES
            n_ready += 1
        hs, soft = rd["HardState"], rd["SoftState"] or dict(Lead=0, RaftState=0)
        res[i] = [flags << 32, hs["Term"], hs["Vote"], hs["Commit"],
                  (efirst + lg.unstable - lg.offset) & M64 if un else 0, un,
                  (efirst + lg.applied + 1 - lg.offset) & M64 if cn else 0, cn, len(saves), un + hard,
                  soft["Lead"], soft["RaftState"]]
        if hard:
            saves.append([SAVE_STATE, hs["Term"], hs["Vote"], hs["Commit"], 0, 0, 0])
        for e in rd["Entries"]:
            saves.append([SAVE_ENTRY | (e["Type"] << 32), e["Term"], e["Index"], 0, e["data_off"], e["data_len"],
                          e["data_nil"]])
        node.accept(rd)
        M.to_arrays(node, out, g)
    return dict(pstate=out["pstate"], rstate=out["rstate"], res_rows=res, save_rows=_rows(saves, 7),
                n_save=len(saves), n_ready=n_ready)


# ---- ecompact_batch_device -------------------------------------------------------------------

K_NOT_STEPPED, K_NOT_DUE, K_COMPACTED, K_PANICKED = range(4)
AT_APPLIED = 1


def compact_call(a):
    """a: groups, pstate, rstate, snaps, ents, and reqs, the (n, 12) ecompact_req
    rows (group, flags, index, threshold, the snapshot's data, nodes and removed
    ranges).  node.Compact, or EtcdServer.snapshot's "at applied, when due".
    Returns groups, pstate, snaps, ents, res_rows (n, 8), n_compacted, n_moved."""
    b = dict(a, vstate=None)
    out = _copies(b, ARRAYS)
    n = len(a["reqs"])
    res, n_compacted, n_moved = np.zeros((n, 8), dtype=np.uint64), 0, 0
    for i in range(n):
        q = [int(x) for x in a["reqs"][i]]
        g = q[0]
        node = M.from_arrays(out, g)
        r, lg, efirst = node.r, node.r.raftLog, int(out["groups"][g, 5])
        index, off0 = q[2], lg.offset
        if q[1] & AT_APPLIED:
            lg.compactThreshold = q[3]
            if not lg.shouldCompact():
                res[i, 0] = K_NOT_DUE << 32
                continue
            index = lg.applied           # EtcdServer.snapshot compacts at the applied index
        before = M.saved(r)
        try:
            r.compact(index, (q[6], q[7]), (q[4], q[5]), (q[8], q[9]))
            if not lg.ents:
                raise Unsupported()      # Go is left with a zero-length log: reported, never guessed
        except (M.Panic, Unsupported) as p:
            M.put_back(r, before)
            res[i, 0] = (STATUS[p.name] if isinstance(p, M.Panic) else UNSUPPORTED) | (K_PANICKED << 32)
            continue
        # the three slices are ranges of the caller's arrays: the record keeps the ranges
        lg.snapshot.update(dict(zip(M.SNAP_FIELDS[2:], q[4:10])))
        shift = (lg.offset - off0) & M64
        res[i] = [K_COMPACTED << 32, lg.snapshot["Index"], lg.snapshot["Term"], len(lg.ents), shift, efirst + shift,
                  efirst, lg.unstable]
        n_compacted += 1
        n_moved += len(lg.ents) if shift else 0
        M.to_arrays(node, out, g)
    return dict(groups=out["groups"], pstate=out["pstate"], snaps=out["snaps"], ents=out["ents"], res_rows=res,
                n_compacted=n_compacted, n_moved=n_moved)


# ---- backends: one call on the cluster's arrays ----------------------------------------------------
#
# A backend's vote / follow / lead_step / local take the dict `a` the model's
# functions above take and return the same kind of dict.  Arrays a call cannot
# write may be missing from what a backend returns; its counters may not.


class ModelBackend:
    vote, follow, lead_step, local = staticmethod(vote_call), staticmethod(follow_call), \
        staticmethod(lead_step_call), staticmethod(lead_local_call)
    ready, compact = staticmethod(ready_call), staticmethod(compact_call)


def _named(records):
    return sorted({r["group"] for r in records})


def _written(before, packed, expected):
    """What a restatement wrote, put onto `before`: its scenario is rebuilt from
    the arrays without the words it does not read (Data positions, canaries), so
    only the words its expected() changes are its statement."""
    out = before.copy()
    mask = packed != expected
    out[mask] = expected[mask]
    return out


class RestatedBackend:
    """Each call is the expected() of its *_cases.py, the scenario rebuilt from
    the arrays: the named groups as they are, every other group a placeholder
    with the same window."""

    def _group_kw(self, a, g, terms_only):
        w = [int(x) for x in a["groups"][g]]
        s = [int(x) for x in a["pstate"][g]]
        ents = a["ents"][w[5]:w[5] + w[4]]
        log = [int(e[0]) for e in ents] if terms_only else \
            [dict(term=int(e[0]), type=int(e[4]) & 0xFFFFFFFF) for e in ents]
        sn = [int(x) for x in a["snaps"][g]]
        kw = dict(prs=[(w[7 + k], w[14 + k], w[21 + k]) for k in range(w[6])], gid=w[0], term=w[1], committed=w[2],
                  log_offset=w[3], snap=dict(zip(M.SNAP_FIELDS_LOWER, sn)) if any(sn) else None)
        return log, kw, w, s

    def follow(self, a):
        import follow_cases as FC
        assert FC.validate(a) == FC.OK
        return FC.expected(a)

    def vote(self, a):
        import vote_step_cases as VC
        sc, named = VC.Scenario(), set(_named(a["msgs"]))
        for g in range(len(a["groups"])):
            cap = len(a["ents"]) // len(a["groups"])
            if g not in named:
                sc.add_group([1], [(1, 0, 1)], room=cap - 1)
                continue
            log, kw, w, s = self._group_kw(a, g, False)
            v = [int(x) for x in a["vstate"][g]]
            sc.add_group(log, room=cap - w[4], unstable=s[1], pending_conf=s[2], state=v[0], vote=v[1], lead=v[2],
                         elapsed=v[3], voted=v[4], granted=v[5], **kw)
        sc.msgs = [dict(m) for m in a["msgs"]]
        p = sc.pack()
        res, grows, strows, vrows, erows, rows = sc.expected()
        return dict(res_rows=res, msg_rows=rows, groups=_written(a["groups"], p[0], grows),
                    pstate=_written(a["pstate"], p[1], strows), vstate=_written(a["vstate"], p[2], vrows),
                    ents=_written(a["ents"], p[4], erows), n_msgs=sc.n_msgs, n_won=sc.n_won)

    def lead_step(self, a):
        import lead_step_cases as LC
        sc, named = LC.Scenario(), set(_named(a["resps"]))
        for g in range(len(a["groups"])):
            if g not in named:
                sc.add_group([1], [(1, 0, 1)])
                continue
            log, kw, w, s = self._group_kw(a, g, True)
            sc.add_group(log, **kw)
        sc.resps = [dict(r) for r in a["resps"]]
        p = sc.pack()
        res, grows, rows = sc.expected()
        rows = rows.copy()
        for r, x in zip(res, a["resps"]):      # its windows are packed densely: the messages' views are moved to ours
            g = x["group"]
            for k in range(int(r[1]), int(r[1]) + int(r[2])):
                if int(rows[k, 8]):
                    rows[k, 7] = rows[k, 7] - p[0][g, 5] + a["groups"][g, 5]
        return dict(res_rows=res, msg_rows=rows, groups=_written(a["groups"], p[0], grows), n_msgs=sc.n_msgs,
                    n_committed=sc.n_committed)

    def local(self, a):
        import lead_prop_cases as PC
        sc, named = PC.Scenario(), set(_named(a["locals"]))
        for g in range(len(a["groups"])):
            cap = len(a["ents"]) // len(a["groups"])
            if g not in named:
                sc.add_group([1], [(1, 0, 1)], room=cap - 1)
                continue
            log, kw, w, s = self._group_kw(a, g, True)
            sc.add_group(log, room=cap - w[4], unstable=s[1], pending_conf=s[2], **kw)
        sc.locals = [dict(m) for m in a["locals"]]
        p = sc.pack()
        res, grows, strows, erows, rows = sc.expected()
        return dict(res_rows=res, msg_rows=rows, groups=_written(a["groups"], p[0], grows),
                    pstate=_written(a["pstate"], p[1], strows), ents=_written(a["ents"], p[3], erows),
                    n_msgs=sc.n_msgs, n_appended=sc.n_appended)

    def ready(self, a):
        import ready_cases as RC
        sc = RC.Scenario()
        cap = len(a["ents"]) // len(a["groups"])
        named = set(range(len(a["groups"])) if a.get("sel") is None else (int(g) for g in a["sel"]))
        for g in range(len(a["groups"])):
            if g not in named:
                sc.add_group([RC.entry()], room=cap - 1)
                continue
            w, s, v, rs = ([int(x) for x in a[k][g]] for k in ("groups", "pstate", "vstate", "rstate"))
            keys = ("hs_term", "hs_vote", "hs_commit", "plead", "pstate", "snapi", "applied", "soft_dirty")
            prev = dict(zip(keys, rs))
            log = [[int(x) for x in e] for e in a["ents"][w[5]:w[5] + w[4]]]
            sc.add_group(log, room=cap - w[4], id=w[0], term=w[1], committed=w[2], log_offset=w[3], unstable=s[1],
                         vote=v[1], lead=v[2], state=v[0], snap_index=int(a["snaps"][g, 0]), **prev)
        p = sc.pack()
        res, srec, srows, rrows, n_ready = sc.expected(None if a.get("sel") is None else [int(g) for g in a["sel"]])
        return dict(res_rows=res, save_rows=srec, pstate=_written(a["pstate"], p[1], srows),
                    rstate=_written(a["rstate"], p[3], rrows), n_save=len(srec), n_ready=n_ready)

    def compact(self, a):
        import compact_cases as CC
        b = dict(a, n_u64=len(a["u64"]))
        assert CC.validate(b) == CC.OK
        return CC.expected(b)


class DeviceBackend:
    """The real entry points on one ctx: every array is uploaded, the call is
    sized by its size query, then made, and every array is downloaded."""

    def __init__(self, ctx):
        self.ctx = ctx

    def _run(self, a, names, call, in_rows, res_bytes, counters, out_bytes=144, out_key="msg_rows"):
        """call(bufs by name, d_in, n, d_res, d_out, cap) -> the call's counters,
        the number of output records first; d_out None is the size query (or
        the peek), which must give the same counters and results as the call."""
        from etcd_amd.raftlead import _up
        ctx, n = self.ctx, len(in_rows)
        bufs = {k: _up(ctx, np.ascontiguousarray(a[k])) for k in names}
        extra = [_up(ctx, in_rows), ctx.alloc(n * res_bytes + 64)]
        try:
            before = {k: bufs[k].download(a[k].nbytes) for k in names}
            asked = tuple(call(bufs, extra[0], n, extra[1], None, 0))
            total = asked[0] if out_bytes else 0
            for k in names:                       # the size query modifies nothing
                assert bufs[k].download(a[k].nbytes) == before[k], k
            peeked = extra[1].download(n * res_bytes)
            extra.append(ctx.alloc((total + 1) * max(out_bytes, 8) + 64))
            counts = tuple(call(bufs, extra[0], n, extra[1], extra[2], total))
            assert counts == asked and len(counts) == len(counters), (counters, asked, counts)
            out = {k: np.frombuffer(bufs[k].download(a[k].nbytes), dtype=np.uint64).reshape(a[k].shape).copy()
                   for k in names}
            assert extra[1].download(n * res_bytes) == peeked      # ... and has filled the results already
            out["res_rows"] = np.frombuffer(peeked, dtype=np.uint64).reshape(n, -1).copy()
            if out_bytes:
                raw = extra[2].download(total * out_bytes) if total else b""
                out[out_key] = np.frombuffer(raw, dtype=np.uint64).reshape(-1, out_bytes // 8).copy()
            out.update(zip(counters, counts))
        finally:
            for b in list(bufs.values()) + extra:
                b.free()
        return out

    def vote(self, a):
        from etcd_amd import raftvote as V
        G, ne = len(a["groups"]), len(a["ents"])
        return self._run(a, ("groups", "pstate", "vstate", "snaps", "ents"),
                         lambda b, d_in, n, d_res, d_out, cap: V.vote_batch_device(
                             self.ctx, b["groups"], b["pstate"], b["vstate"], G, b["snaps"], b["ents"], ne, d_in, n,
                             d_res, d_out, cap), V.pack_msgs(a["msgs"]), 48, ("n_msgs", "n_won"))

    def lead_step(self, a):
        from etcd_amd import raftlead as R
        G, ne = len(a["groups"]), len(a["ents"])
        return self._run(a, ("groups", "snaps", "ents"),
                         lambda b, d_in, n, d_res, d_out, cap: R.lead_step_batch_device(
                             self.ctx, b["groups"], G, b["snaps"], b["ents"], ne, d_in, n, d_res, d_out, cap),
                         R.pack_resps(a["resps"]), 48, ("n_msgs", "n_committed"))

    def local(self, a):
        from etcd_amd import raftprop as P
        G, ne = len(a["groups"]), len(a["ents"])
        return self._run(a, ("groups", "pstate", "snaps", "ents"),
                         lambda b, d_in, n, d_res, d_out, cap: P.local_batch_device(
                             self.ctx, b["groups"], b["pstate"], G, b["snaps"], b["ents"], ne, a["data_len"], d_in, n,
                             d_res, d_out, cap), P.pack_locals(a["locals"]), 48, ("n_msgs", "n_appended"))

    def ready(self, a):
        from etcd_amd import raftready as RD
        G, ne = len(a["groups"]), len(a["ents"])
        sel = np.arange(G, dtype=np.uint64) if a.get("sel") is None else np.array(a["sel"], dtype=np.uint64)

        def call(b, d_in, n, d_res, d_out, cap):
            return RD.ready_batch_device(self.ctx, b["groups"], b["pstate"], b["vstate"], b["rstate"], G, b["snaps"],
                                         b["ents"], ne, None if a.get("sel") is None else d_in, n, d_res, d_out, cap)
        return self._run(a, ARRAYS, call, sel, 96, ("n_save", "n_ready"), 56, "save_rows")

    def compact(self, a):
        from etcd_amd import raftcompact as RC
        G, ne = len(a["groups"]), len(a["ents"])

        def call(b, d_in, n, d_res, d_out, cap):
            return RC.compact_batch_device(self.ctx, b["groups"], b["pstate"], b["rstate"], G, b["snaps"], b["ents"],
                                           ne, a["data_len"], len(a["u64"]), d_in, n, d_res,
                                           RC.PEEK if d_out is None else 0)
        return self._run(a, ("groups", "pstate", "rstate", "snaps", "ents"), call, np.ascontiguousarray(a["reqs"]), 64,
                         ("n_compacted", "n_moved"), 0)

    def follow(self, a):
        from etcd_amd import raftfollow as F
        from etcd_amd.raftlead import _up
        ctx = self.ctx
        G, ne = len(a["groups"]), len(a["ents"])
        side = [_up(ctx, np.ascontiguousarray(a[k])) for k in ("src", "in_snaps", "u64")]
        try:
            return self._run(a, ARRAYS,
                             lambda b, d_in, n, d_res, d_out, cap: F.follow_batch_device(
                                 ctx, b["groups"], b["pstate"], b["vstate"], b["rstate"], G, b["snaps"], b["ents"], ne,
                                 side[0], len(a["src"]), side[1], len(a["in_snaps"]), side[2], len(a["u64"]), d_in, n,
                                 d_res, d_out, cap), np.ascontiguousarray(a["msgs"]), 96,
                             ("n_msgs", "n_appended", "n_restored"))
        finally:
            for b in side:
                b.free()


# ---- the wire: a message leaves its sender as bytes ------------------------------------------------
#
# emsg_out.ents_first is a view of the sender's window; it goes stale when the
# sender compacts or truncates before delivery (include/ewal.h, the compaction's
# notes).  A network that delays messages carries bytes: Marshal right after the
# emitting call, Unmarshal at the receiver, the entries' Data appended to the
# cluster's data buffer.

def marshal_rows(rows, ents, data, u64):
    """raftpb.Message.Marshal of emsg_out rows whose entries are ents[ents_first, + n_ents), by the oracle."""
    from oracle import oracle as O
    out = []
    for row in rows:
        w = [int(x) for x in row]
        es = []
        for e in ents[w[7]:w[7] + w[8]]:
            e = [int(x) for x in e]
            d = None if e[4] >> 32 else bytes(data[e[2]:e[2] + e[3]])
            es.append(O.entry_marshal(e[4] & 0xFFFFFFFF, e[0], e[1], d))
        snap = O.snapshot_marshal(bytes(data[w[11]:w[11] + w[12]]), [int(x) for x in u64[w[13]:w[13] + w[14]]], w[9],
                                  w[10], [int(x) for x in u64[w[15]:w[15] + w[16]]])
        out.append(O.message_marshal(w[0], w[1], w[2], w[3], w[4], w[5], es, w[6], snap, bool(w[17] & 1)))
    return out


MSG_KEYS = ("status", "type", "to", "from_", "term", "log_term", "index", "commit", "reject")


def _plain(m):
    """What the router reads of a decoded message."""
    return (tuple(m[k] for k in MSG_KEYS), [(e["type"], e["term"], e["index"], e["data"]) for e in m["ents"]],
            (m["snap"]["index"], m["snap"]["term"], m["snap"]["data"] or b"", list(m["snap"]["nodes"]),
             list(m["snap"]["removed"])))


class HostWire:
    def encode(self, rows, ents, data, u64):
        return marshal_rows(rows, ents, data, u64)

    def decode(self, bodies):
        from oracle import oracle as O
        return [O.message_unmarshal(b) for b in bodies]


class DeviceWire:
    """emsg_encode_batch_device and emsg_decode_batch_device; every body and
    every decoded message is also compared with the oracle's."""

    def __init__(self, ctx):
        self.ctx = ctx

    def encode(self, rows, ents, data, u64):
        from etcd_amd import raftmsg as RM
        from etcd_amd.raftlead import _up
        ctx, n = self.ctx, len(rows)
        blob = np.frombuffer(bytes(data) + b"\0" * (8 - len(data) % 8), dtype=np.uint8)
        bufs = [_up(ctx, blob), _up(ctx, np.ascontiguousarray(rows)), _up(ctx, np.ascontiguousarray(ents)),
                _up(ctx, np.ascontiguousarray(u64))]
        try:
            args = (ctx, bufs[0], len(data), bufs[1], n, bufs[2], len(ents), bufs[3], len(u64))
            _, _, total = RM.encode_messages_device(*args, None, 0)
            bufs.append(ctx.alloc(total + 64))
            offs, lens, total = RM.encode_messages_device(*args, bufs[4], total)
            raw = bufs[4].download(total)
        finally:
            for b in bufs:
                b.free()
        got = [raw[o:o + k] for o, k in zip(offs, lens)]
        assert got == marshal_rows(rows, ents, data, u64)
        return got

    def decode(self, bodies):
        from etcd_amd import raftmsg as RM
        got = RM.decode_messages(self.ctx, bodies)
        want = HostWire().decode(bodies)
        assert [_plain(m) for m in got] == [_plain(m) for m in want]
        return got


# ---- the cluster -----------------------------------------------------------------------------

class SplitMix:
    """follow_cases.SplitMix, draw for draw."""

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


class Tally(dict):
    def add(self, key, k=1):
        self[key] = self.get(key, 0) + k


class Cluster:
    """`clusters` raft clusters of `nodes` nodes in one set of arrays: `idle`
    canary groups (garbage in every record; no record ever names them), then
    cluster c's node id at group idle + c * nodes + id - 1, then `idle` more.
    Every node starts as RestartNode leaves an empty one.  Each window is `cap`
    entries; the slots past nlog start as canaries.

    The router below is the host's part of Step ("What each entry point replaces"):
      msgHup, msgVote, msgVoteResp   -> the election call
      msgApp, msgSnap                -> the follower call
      msgAppResp                     -> the msgAppResp call where the receiving
                                        group is a leader; otherwise dropped (the
                                        model then has m.Term < r.Term: asserted)
      msgProp                        -> the local call at a leader; at a follower
                                        that knows a leader forwarded to lead; at
                                        a node without a leader refused (Go
                                        panics "no leader")
      msgBeat                        -> leaders only
    A group's records are adjacent, in arrival order.  Records a call leaves
    unstepped (*_NOT_STEPPED, EFOLLOW_DEFERRED) go back to the head of their
    group's queue for the next call of that kind.

    A message in flight is its Marshal bytes, made when the call that emitted
    it returns; the receiver's Unmarshal puts its entries into the call's source
    array and their Data at the end of the cluster's data buffer."""

    def __init__(self, nodes, clusters, backend, cap=64, idle=2, seed=1, wire=None):
        self.nodes, self.clusters, self.backend, self.cap, self.idle = nodes, clusters, backend, cap, idle
        self.wire = wire or HostWire()
        self.G = G = 2 * idle + nodes * clusters
        self.base = idle
        rng = SplitMix(seed, 1 << 40)
        a = dict(groups=np.zeros((G, 32), dtype=np.uint64), pstate=np.zeros((G, 4), dtype=np.uint64),
                 vstate=np.zeros((G, 8), dtype=np.uint64), rstate=np.zeros((G, 8), dtype=np.uint64),
                 snaps=np.zeros((G, 8), dtype=np.uint64), ents=np.full((G * cap, 5), CANARY, dtype=np.uint64))
        for g in range(G):
            if self.cluster_of(g) is None:
                for k in ARRAYS[:5]:
                    a[k][g] = [rng.next() for _ in range(a[k].shape[1])]
                continue
            id_ = (g - idle) % nodes + 1
            a["groups"][g, :7] = [id_, 0, 0, 0, 1, g * cap, nodes]
            a["groups"][g, 7:7 + nodes] = range(1, nodes + 1)
            a["groups"][g, 21:21 + nodes] = 1
            a["pstate"][g] = [cap, 1, 0, 0]
            a["ents"][g * cap] = [0, 0, 0, 0, 1 << 32]
        self.a = a
        self.data = bytearray()
        self.u64 = np.arange(1, nodes + 1, dtype=np.uint64)      # the Nodes of every snapshot
        self.touched = set()
        self.saves = {}                       # group -> its Ready stream's ewal_save_rec rows, in order
        self.ri = {}                          # group -> the index its WAL is read from (past its last restore)
        self.flight = []                      # messages in flight: dicts (to, row, ents)
        self.queue = {"vote": {}, "follow": {}, "lead_step": {}, "local": {}}    # per kind: group -> records put back
        self.tally = Tally()
        self.calls = []                       # (kind, n records)
        self.leaders = {}                     # (cluster, term) -> leader id, ever
        self.committed = {}                   # (cluster, index) -> (term, type, data), ever
        self.refused = 0
        self.longest = 1                      # the longest log any node ever held, measured after every call

    def cluster_of(self, g):
        k = g - self.base
        return k // self.nodes if 0 <= k < self.nodes * self.clusters else None

    def group(self, c, id_):
        return self.base + c * self.nodes + id_ - 1

    def state(self, g):
        return int(self.a["vstate"][g, 0])

    # -- one call: the backend against the model, every array bit for bit --

    def call(self, kind, **records):
        a = dict(self.a, data_len=len(self.data), **records)
        want = getattr(ModelBackend, kind)(a)
        if not isinstance(self.backend, ModelBackend):
            got = getattr(self.backend, kind)(a)
            for k in COUNTERS:
                if k in want or k in got:      # every counter of the call, from every backend
                    assert k in want and k in got and got[k] == want[k], (kind, k, got.get(k), want.get(k))
            for k in ("res_rows", "msg_rows", "save_rows") + ARRAYS:
                if k not in want and k not in self.a:
                    continue
                w = want.get(k, self.a.get(k))
                g = got.get(k)
                if g is None:
                    g = self.a[k]                  # the backend says the call does not write it
                if not np.array_equal(g, w):
                    at = tuple(int(x) for x in np.argwhere(np.asarray(g) != np.asarray(w))[0]) \
                        if np.shape(g) == np.shape(w) else ("shape", np.shape(g), np.shape(w))
                    raise AssertionError("%s call %d: %s differs at %r" % (kind, len(self.calls), k, at))
        for k in ARRAYS:
            if want.get(k) is not None:
                self.a[k] = want[k]
        for k in COUNTERS:
            if want.get(k):
                self.tally.add("counted_" + k, want[k])
        self.longest = max(self.longest, int(self.a["groups"][self.base:self.G - self.idle, 4].max()))
        return want["res_rows"], want.get("msg_rows", want.get("save_rows"))

    def emit(self, senders, res, rows):
        """The call's messages go into flight as bytes."""
        if not len(rows):
            return
        rows, ents, who = rows.copy(), [], []
        for g, r in zip(senders, res):
            for k in range(int(r[1]), int(r[1]) + int(r[2])):
                w = [int(x) for x in rows[k]]
                if w[8]:
                    assert self.a["groups"][g, 5] <= w[7] and w[7] + w[8] <= self.a["groups"][g, 5] + \
                        self.a["groups"][g, 4]
                    rows[k, 7] = len(ents)         # the encoder is given the messages' entries and no others
                    ents += [list(e) for e in self.a["ents"][w[7]:w[7] + w[8]]]
                who.append(g)
                self.tally.add("sent_type_%d" % w[0])
        bodies = self.wire.encode(rows, _rows(ents, 5), self.data, self.u64)
        for g, row, body in zip(who, rows, bodies):
            c = self.cluster_of(g)
            self.flight.append(dict(to=self.group(c, int(row[1])), frm=self.group(c, int(row[2])), body=body))

    def receive(self, flight):
        """Unmarshal of the delivered bodies: (kind of call, group, record) each."""
        out = []
        for f, m in zip(flight, self.wire.decode([f["body"] for f in flight])):
            assert m["status"] == OK and self.group(self.cluster_of(f["to"]), m["to"]) == f["to"]
            t = m["type"]
            if t in (M.MSG_VOTE, M.MSG_VOTE_RESP):
                out.append(("vote", f["to"], dict(m=dict(kind=t, from_=m["from_"], term=m["term"], index=m["index"],
                                                         log_term=m["log_term"], reject=m["reject"]))))
            elif t == M.MSG_APP_RESP:
                out.append(("lead_step", f["to"], dict(m=dict(from_=m["from_"], term=m["term"], index=m["index"],
                                                              reject=m["reject"]))))
            else:
                assert t in (M.MSG_APP, M.MSG_SNAP)
                ents = [(e["term"], e["index"], e["type"], e["data"]) for e in m["ents"]]
                row = [t, m["to"], m["from_"], m["term"], m["log_term"], m["index"], m["commit"], 0, len(ents)] + \
                    [0] * 8 + [int(m["reject"])]
                if t == M.MSG_SNAP:
                    sn = m["snap"]
                    assert not sn["data"] and not sn["removed"]
                    row[9:17] = [sn["index"], sn["term"], 0, 0, self.place(sn["nodes"]), len(sn["nodes"]), 0, 0]
                out.append(("follow", f["to"], dict(row=row, ents=ents)))
        return out

    def place(self, nodes):
        """Where a snapshot's Nodes stand in the cluster's u64 array (appended when they are new)."""
        n = len(nodes)
        for off in range(0, len(self.u64) - n + 1):
            if [int(x) for x in self.u64[off:off + n]] == list(nodes):
                return off
        self.u64 = np.concatenate([self.u64, np.array(nodes, dtype=np.uint64)])
        return len(self.u64) - n

    def _batch(self, kind, arrivals):
        """The records of one call: what was put back first, then the arrivals,
        each group's adjacent, in arrival order.  arrivals: (group, record)."""
        per = self.queue[kind]
        self.queue[kind] = {}
        for g, rec in arrivals:
            per.setdefault(g, []).append(rec)
        return [(g, rec) for g in sorted(per) for rec in per[g]]

    def _done(self, kind, batch, res, unstepped):
        self.calls.append((kind, len(batch)))
        self.touched |= {g for g, _ in batch}
        # runs across the 64- and the 256-record seams
        for i in range(1, len(batch)):
            if batch[i][0] == batch[i - 1][0]:
                if i % 64 == 0:
                    self.tally.add("run_across_64")
                if i % 256 == 0:
                    self.tally.add("run_across_256")
        for (g, rec), r in zip(batch, res):
            status, action = int(r[0]) & 0xFFFFFFFF, int(r[0]) >> 32
            self.tally.add("%s_action_%d" % (kind, action))
            self.tally.add("%s_records" % kind)
            if status != OK:
                self.tally.add("status_%d" % status)
            if action in unstepped:
                self.queue[kind].setdefault(g, []).append(rec)
                rec["put_back"] = rec.get("put_back", 0) + 1
            elif rec.get("put_back"):
                self.tally.add("%s_restepped" % kind)

    def vote(self, arrivals):
        batch = self._batch("vote", arrivals)
        if not batch:
            return
        msgs = [dict(rec["m"], group=g) for g, rec in batch]
        res, rows = self.call("vote", msgs=msgs)
        for (g, rec), r in zip(batch, res):
            if int(r[5]) >> 32 & 1:
                self.tally.add("vote_term_switch")
            if int(r[0]) == 42 | (V_PANICKED << 32):             # EWAL_PANIC_LEADER_TO_CANDIDATE: nothing changed
                assert rec.get("at_leader")
                self.tally.add("hup_at_leader")
                self.tally.add("status_42", -1)
        self._done("vote", batch, res, (V_NOT_STEPPED,))
        self.emit([g for g, _ in batch], res, rows)

    def follow(self, arrivals):
        batch = self._batch("follow", arrivals)
        if not batch:
            return
        # the call's Data goes into a blob of its own, appended to the cluster's data buffer: the source entries
        # hold positions in the blob, every message's data_delta is the blob's base (rec["ents"]: term, index, type,
        # Data; a record put back is laid out again for the call that steps it)
        src, in_snaps, msgs, blob = [], [], np.zeros((len(batch), 12), dtype=np.uint64), bytearray()
        base = len(self.data)
        for i, (g, rec) in enumerate(batch):
            w = rec["row"]
            msgs[i, :10] = [g, w[0], w[2], w[3], w[5], w[4], w[6], len(src) if w[8] else 0, w[8], base]
            if w[0] == M.MSG_SNAP:
                msgs[i, 9], msgs[i, 10] = 0, len(in_snaps)
                in_snaps.append(w[9:17])
            for term, index, type_, d in rec["ents"]:
                src.append([term, index, len(blob) if d is not None else 0, len(d or b""),
                            type_ | ((1 if d is None else 0) << 32)])
                blob += d or b""
                if d and base:
                    self.tally.add("follow_data_delta")
            if w[8]:
                src.append([CANARY] * 5)
        self.data += blob
        nlog0 = self.a["groups"][:, 4].copy()
        res, rows = self.call("follow", msgs=msgs, src=_rows(src, 5), in_snaps=_rows(in_snaps, 8),
                              u64=self.u64)
        seen = set()
        for (g, rec), r in zip(batch, res):
            flags = int(r[10]) >> 32
            if flags & 1:
                self.tally.add("follow_term_switch")
            if flags & 2:
                self.tally.add("follow_conceded")
            if int(r[5]) and g not in seen and int(r[6]) < g * self.cap + int(nlog0[g]):
                self.tally.add("follow_truncated")       # conflict <= lastIndex: entries the node held are cut
            if int(r[5]):
                seen.add(g)
            if int(r[0]) >> 32 == F_RESTORED:
                # the log starts over at the snapshot: so does what ReadAll can be asked for
                self.saves[g], self.ri[g] = [], int(r[7]) + 1
        self._done("follow", batch, res, (F_NOT_STEPPED, F_DEFERRED))
        self.emit([g for g, _ in batch], res, rows)

    def lead_step(self, arrivals):
        keep = []
        for g, rec in arrivals:
            if self.state(g) == M.LEADER:
                keep.append((g, rec))
            else:
                # not a leader any more: Step would read m.Term < r.Term and ignore it
                assert 0 < rec["m"]["term"] < int(self.a["groups"][g, 1])
                self.tally.add("app_resp_dropped")
        for g in list(self.queue["lead_step"]):
            assert self.state(g) == M.LEADER
        batch = self._batch("lead_step", keep)
        if not batch:
            return
        res, rows = self.call("lead_step", resps=[dict(rec["m"], group=g) for g, rec in batch])
        self._done("lead_step", batch, res, (L_NOT_STEPPED,))
        assert not self.tally.get("lead_step_action_%d" % L_STEP_DOWN)
        self.emit([g for g, _ in batch], res, rows)

    def local(self, arrivals):
        batch = self._batch("local", [(g, rec) for g, rec in arrivals if self.state(g) == M.LEADER])
        if not batch:
            return
        res, rows = self.call("local", locals=[dict(rec["m"], group=g) for g, rec in batch])
        self._done("local", batch, res, (P_NOT_STEPPED,))
        self.emit([g for g, _ in batch], res, rows)

    def ready(self, sel):
        """Ready over sel (group numbers, any order; None: every group in order, the
        call's d_sel == NULL, for a cluster without idle groups): newReady, the
        accept, the WAL's records."""
        if sel is None:
            assert self.idle == 0
            res, saves = self.call("ready", sel=None)
            sel = list(range(self.G))
            self.tally.add("ready_without_sel")
        elif not len(sel):
            return
        else:
            res, saves = self.call("ready", sel=np.array(sel, dtype=np.uint64))
        self.calls.append(("ready", len(sel)))
        for g, r in zip(sel, res):
            assert int(r[0]) & 0xFFFFFFFF == OK
            if int(r[0]) >> 32 & R_SNAP:
                self.tally.add("ready_snap")
            if int(r[9]):
                self.saves.setdefault(g, []).append(saves[int(r[8]):int(r[8]) + int(r[9])].copy())
            self.tally.add("ready_saved", int(r[9]))

    def compact(self, groups, threshold):
        """EtcdServer.snapshot's compaction at the applied index, where applied - offset > threshold."""
        reqs = _rows([[g, AT_APPLIED, 0, threshold, 0, 0, 0, self.nodes, 0, 0, 0, 0] for g in groups], 12)
        res, _ = self.call("compact", reqs=reqs, u64=self.u64)
        self.calls.append(("compact", len(groups)))
        for r in res:
            status, action = int(r[0]) & 0xFFFFFFFF, int(r[0]) >> 32
            assert status == OK
            self.tally.add("compact_action_%d" % action)
            if action == K_COMPACTED and int(r[4]) and int(r[3]):
                self.tally.add("compact_move_overlap" if int(r[4]) < int(r[3]) else "compact_move_disjoint")

    # -- the host's side of a proposal --

    def propose(self, g, data, etype=0):
        """(group that takes it, record) or None where the router refuses it."""
        hops = 0
        while self.state(g) != M.LEADER:
            lead = int(self.a["vstate"][g, 2])
            if lead == M.NONE or hops == 2:
                self.refused += 1              # Go: panic("no leader"); it never reaches a call
                return None
            g, hops = self.group(self.cluster_of(g), lead), hops + 1
            self.tally.add("proposal_forwarded")
        off = len(self.data)
        self.data += data or b""
        return g, dict(m=dict(kind=M.MSG_PROP, etype=etype, data_off=off if data else 0, data_len=len(data or b""),
                              data_nil=data is None))

    # -- safety, on the decoded arrays --

    def check_safety(self):
        a = self.a
        for c in range(self.clusters):
            logs = []
            for id_ in range(1, self.nodes + 1):
                g = self.group(c, id_)
                n = M.from_arrays(a, g)
                r, lg = n.r, n.r.raftLog
                assert lg.committed <= lg.lastIndex() and lg.applied <= lg.committed, (c, id_)
                assert [e["Index"] for e in lg.ents[1:]] == list(range(lg.offset + 1, lg.offset + len(lg.ents)))
                if r.state == M.LEADER:
                    assert self.leaders.setdefault((c, r.Term), r.id) == r.id, "two leaders in term %d" % r.Term
                # Marshal writes a nil Data and an empty one alike: the receiver's is empty
                what = {lg.offset + k: (e["Term"], e["Type"], b"" if e["data_nil"] else
                                        bytes(self.data[e["data_off"]:e["data_off"] + e["data_len"]]))
                        for k, e in enumerate(lg.ents) if k}
                what[lg.offset] = (lg.ents[0]["Term"],)           # the entry under the offset is known by its term
                logs.append(what)
                for i in range(lg.offset + 1, lg.committed + 1):
                    assert self.committed.setdefault((c, i), what[i]) == what[i], "committed entry %d changed" % i
            for x in range(len(logs)):           # log matching: equal (index, term) implies equal prefixes
                for y in range(x):
                    both = sorted(set(logs[x]) & set(logs[y]), reverse=True)
                    agree = False
                    for i in both:
                        if agree:
                            assert logs[x][i][0] == logs[y][i][0], "log matching broken at %d" % i
                        if logs[x][i][0] == logs[y][i][0]:
                            assert len(logs[x][i]) == 1 or len(logs[y][i]) == 1 or logs[x][i] == logs[y][i]
                            agree = True

    def check_idle(self, first):
        """No call ever names an idle group or a free window slot it does not fill: they stay as they began."""
        for g in range(self.G):
            if self.cluster_of(g) is None:
                for k in ARRAYS[:5]:
                    assert np.array_equal(self.a[k][g], first[k][g]), (k, g)
                assert np.all(self.a["ents"][g * self.cap:(g + 1) * self.cap] == np.uint64(CANARY))
        self.tally.add("free_slots_never_written", int(np.sum(self.a["ents"][:, 0] == np.uint64(CANARY))))


# ---- the lossy network ----------------------------------------------------------------------------

def play_lossy(nodes, clusters, backend, ticks, seed, cap, threshold=3, wire=None):
    """The fuzz: per tick and cluster, drawn from SplitMix(seed, cluster): election
    timeouts at non-leaders (often where the node knows no leader, seldom where
    it does, rarely at a leader), proposals at leaders and by
    proxy, beats, delivery of a subset of the messages in flight with drop,
    duplicate and delay, partitions that appear and heal.  Ticks t % 8 in (0, 1,
    2) are calm (nothing is lost or delayed outside a partition, every leader
    beats: a beat, its msgApp and their answers each fill a call), t % 8 == 5
    stormy (almost everything waits).  Two thundering ticks (1 and 2 * ticks // 3): every
    partition heals and every non-leader's timeout fires at once.  One call of
    each kind per tick, in the order election, follower, msgAppResp, local; then
    Ready and the compaction "at applied, when due" (applied - offset >
    threshold), which sooner or later leaves a slow follower behind the leader's
    offset: msgSnap and restore.  Returns the cluster."""
    cl = Cluster(nodes, clusters, backend, cap=cap, seed=seed, wire=wire)
    first = {k: v.copy() for k, v in cl.a.items()}
    rngs = [SplitMix(seed, c) for c in range(clusters)]
    cut = [set() for _ in range(clusters)]
    thunder = (1, 2 * ticks // 3)
    for t in range(ticks):
        calm, storm = t % 8 in (0, 1, 2), t % 8 == 5
        arrivals = {"vote": [], "follow": [], "lead_step": [], "local": []}
        delivered = []
        flight, cl.flight = cl.flight, []
        per = [[] for _ in range(clusters)]
        for m in flight:
            per[cl.cluster_of(m["to"])].append(m)
        for c in range(clusters):
            r = rngs[c]
            if t in thunder:
                cut[c].clear()
            elif cut[c]:
                if r.rnd(4) == 0:
                    cut[c].clear()
            elif r.rnd(10) == 0:
                cut[c].add(cl.group(c, 1 + r.rnd(nodes)))
            for id_ in range(1, nodes + 1):
                g = cl.group(c, id_)
                leader = cl.state(g) == M.LEADER
                hup = dict(m=dict(kind=M.MSG_HUP, from_=id_, term=0, index=0, log_term=0, reject=False))
                if not leader and (t in thunder or r.rnd((40 if int(cl.a["vstate"][g, 2]) else 2) * nodes) == 0):
                    arrivals["vote"].append((g, hup))
                elif leader and r.rnd(40) == 0:
                    arrivals["vote"].append((g, dict(hup, at_leader=True)))
                if leader and (calm or r.rnd(3) == 0):
                    arrivals["local"].append((g, dict(m=dict(kind=M.MSG_BEAT))))
                if r.rnd(2 if leader else 10) == 0:
                    n = r.rnd(41)
                    data = None if n == 0 and r.rnd(2) else bytes(r.rnd(256) for _ in range(n))
                    etype = 1 if r.rnd(50) == 0 else 0
                    # a host that proposes a ConfChange may well repeat it: the second one is the pendingConf drop
                    for _ in range(1 + (etype and r.rnd(2))):
                        p = cl.propose(g, data, etype)
                        if p:
                            arrivals["local"].append(p)
            for m in per[c]:
                if (r.rnd(16) != 0) if storm else (not calm and r.rnd(6) == 0):
                    cl.flight.append(m)                  # delayed: later messages overtake it
                    cl.tally.add("delayed")
                    continue
                if m["to"] in cut[c] or m["frm"] in cut[c] or (not calm and r.rnd(16) == 0):
                    cl.tally.add("dropped")
                    continue
                if not calm and r.rnd(16) == 0:
                    cl.flight.append(dict(m))
                    cl.tally.add("duplicated")
                delivered.append(m)
        for kind, g, rec in cl.receive(delivered):
            arrivals[kind].append((g, rec))
        cl.vote(arrivals["vote"])
        cl.follow(arrivals["follow"])
        cl.lead_step(arrivals["lead_step"])
        cl.local(arrivals["local"])
        real = list(range(cl.base, cl.G - cl.idle))
        # Ready: every group on even ticks, the groups this tick touched, last first, on odd ones
        cl.ready(real if t % 2 == 0 else sorted(cl.touched, reverse=True))
        cl.touched = set()
        cl.compact(real, threshold)
        cl.check_safety()
    cl.check_idle(first)
    return cl


# ---- the reference's network tests ------------------------------------------------------------------

def play_network(sc, backend, copies=1, wire=None, idle=2):
    """One scenario of tests/golden/raft_network_kats.json on `copies` identical
    clusters: raft_test.go's network -- send delivers one message at a time in
    the order of its queue and appends what the stepped node sends, filtered by
    cut / isolate / ignore as they stand then -- so every call holds one record
    per copy.  At the end one Ready over every group: by d_sel, or with idle=0
    (no canary groups) by d_sel == NULL.  Returns the cluster."""
    peers = sc["peers"]
    nodes = len(peers)
    cl = Cluster(nodes, copies, backend, cap=16, idle=idle, seed=5, wire=wire)
    first = {k: v.copy() for k, v in cl.a.items()}
    nop = {i + 1 for i, p in enumerate(peers) if p == "nop"}
    dropm, ignorem = set(), set()

    def per_copy(id_, rec):
        return [(cl.group(c, id_), dict(rec)) for c in range(copies)]

    def sent():
        """What the last call's nodes sent, as one message per copy; every copy sent the same."""
        flight, cl.flight = cl.flight, []
        by = [[m for m in flight if cl.cluster_of(m["frm"]) == c] for c in range(copies)]
        for c in range(1, copies):
            assert [m["body"] for m in by[c]] == [m["body"] for m in by[0]]
        out = []
        for k, m in enumerate(by[0]):
            kind, _, rec = cl.receive([m])[0]
            w = rec["row"] if kind == "follow" else None
            type_ = w[0] if w else rec["m"].get("kind", M.MSG_APP_RESP)
            frm, to = (m["frm"] - cl.base) % nodes + 1, (m["to"] - cl.base) % nodes + 1
            if type_ in ignorem or (frm, to) in dropm:
                continue
            out.append(dict(to=to, copies=[b[k] for b in by]))
        return out

    def deliver(m):
        to = m["to"]
        if to in nop:
            return []
        if "copies" in m:
            recs = cl.receive(m["copies"])
            getattr(cl, recs[0][0])([(g, rec) for _, g, rec in recs])
        elif m["type"] == "hup":
            cl.vote(per_copy(to, dict(m=dict(kind=M.MSG_HUP, from_=to, term=0, index=0, log_term=0, reject=False))))
        elif m["type"] == "prop":
            took = [cl.propose(cl.group(c, to), m["data"].encode()) for c in range(copies)]
            cl.local([p for p in took if p])
        else:
            row = [M.MSG_APP, to, m["from"], m["term"], 0, 0, 0, 0, len(m["ents"])] + [0] * 9
            cl.follow(per_copy(to, dict(row=row, ents=[(e["term"], 0, 0, None) for e in m["ents"]])))
        return sent()

    for op in sc["ops"]:
        if op[0] == "cut":
            dropm |= {(op[1], op[2]), (op[2], op[1])}
        elif op[0] == "isolate":
            dropm |= {(op[1], i) for i in range(1, nodes + 1)} | {(i, op[1]) for i in range(1, nodes + 1)}
        elif op[0] == "ignore":
            ignorem.add(op[1])
        elif op[0] == "recover":
            dropm, ignorem = set(), set()
        elif op[0] == "check":
            check_network(cl, {str(op[1]["node"]): {k: v for k, v in op[1].items() if k != "node"}}, copies)
        else:
            msgs = [op[1]]
            while msgs:
                msgs += deliver(msgs.pop(0))
            cl.check_safety()
    assert not any(cl.queue[k] for k in cl.queue)
    stepped = [g for g in range(cl.base, cl.G - cl.idle) if (g - cl.base) % nodes + 1 not in nop]
    cl.ready(stepped if idle else None)
    for g in stepped:                        # every node's Ready saved its whole log and applied what is committed
        n = M.from_arrays(cl.a, g)
        assert n.r.raftLog.unstable == n.r.raftLog.lastIndex() + 1 and n.r.raftLog.applied == n.r.raftLog.committed
        assert n.prevHardSt == n.r.hardState()
    cl.check_safety()
    cl.check_idle(first)
    check_network(cl, sc["want"], copies)
    assert cl.refused == sc.get("refused", 0) * copies
    return cl


def check_network(cl, want, copies):
    """The values the reference's test asserts, in every copy."""
    for c in range(copies):
        for id_, w in want.items():
            n = M.from_arrays(cl.a, cl.group(c, int(id_)))
            r, lg = n.r, n.r.raftLog

            def data(e):
                return None if e["data_nil"] else bytes(cl.data[e["data_off"]:e["data_off"] + e["data_len"]]).decode()
            if "committed" in w:
                assert lg.committed == w["committed"], (c, id_, lg.committed)
            if "state" in w:
                assert r.state == w["state"], (c, id_, r.state)
            if "term" in w:
                assert r.Term == w["term"], (c, id_, r.Term)
            if "log" in w:
                # a follower's nil Data came over the wire as an empty one
                assert [[e["Term"], e["Index"], data(e) or None] for e in lg.ents] == w["log"], (c, id_)
            if "committed_data" in w:
                got = [data(e) for e in lg.slice(lg.offset + 1, lg.committed + 1) if not e["data_nil"]]
                assert got == w["committed_data"], (c, id_, got)


# ---- the WAL of a group: its Ready stream saved and read back ------------------------------------------

def wal_sample(cl):
    """Five groups: the first, the last, the two that were a leader at some point
    nearest the middle, and one that restored from a snapshot."""
    real = list(range(cl.base, cl.G - cl.idle))
    mid = (real[0] + real[-1]) // 2
    led = sorted({cl.group(c, id_) for (c, _), id_ in cl.leaders.items()} - {real[0], real[-1]},
                 key=lambda g: (abs(g - mid), g))
    sample = [real[0]] + sorted(led[:2]) + [real[-1]]
    # and the group that restored from a snapshot and saved the most since: it is read from its restore point
    since = {g: sum(len(part) for part in cl.saves.get(g, [])) for g in cl.ri if g not in sample}
    return sample + sorted(since, key=lambda g: (-since[g], g))[:1]


def check_wal(cl, g, ctx=None):
    """Every Ready's records of group g since its last restore, after one Cut:
    the oracle's encoder writes them, the oracle's ReadAll reads them back, and
    what it returns is the last saved HardState and the stable part of the
    model's log.  With a ctx, ewal_save_device writes the same bytes in one
    chained call and ewal_readall_device reads the same answer."""
    from oracle import oracle as O
    rows = [r for part in cl.saves.get(g, []) for r in part]
    ri = cl.ri.get(g, 1)
    enc = O.WalEncoder(0)
    enc.save_crc(0)
    enc.encode(1, None)
    state, saved = None, {}
    for r in rows:
        w = [int(x) for x in r]
        if w[0] & 0xFFFFFFFF == SAVE_STATE:
            enc.save_state(w[1], w[2], w[3])
            state = dict(term=w[1], vote=w[2], commit=w[3])
        else:
            assert w[0] & 0xFFFFFFFF == SAVE_ENTRY
            d = None if w[6] else bytes(cl.data[w[4]:w[4] + w[5]])
            enc.save_entry(w[0] >> 32, w[1], w[2], d)
            for i in [i for i in saved if i >= w[2]]:
                del saved[i]                     # an entry saved again cuts what followed it (wal.go ReadAll)
            saved[w[2]] = (w[0] >> 32, w[1], d or b"")
    raw = enc.getvalue()
    if not saved:
        ri = 0            # nothing was saved from ri on: ReadAll would answer ErrIndexNotFound (wal.go, enti < ri)
    back = O.readall(raw, ri)
    assert back["status"] == O.OK, (g, back["status"])
    got = {e["index"]: (e["type"], e["term"], e["data"] or b"") for e in back["ents"]}
    assert got == saved and sorted(got) == list(range(ri, ri + len(got))), g
    n = M.from_arrays(cl.a, g)
    lg = n.r.raftLog
    if state is not None:
        assert {k: back["state"][k] for k in state} == state
        # the last HardState saved is the one node.run remembers, restored or not
        assert state == dict(term=n.prevHardSt["Term"], vote=n.prevHardSt["Vote"], commit=n.prevHardSt["Commit"])
    if got:
        assert max(got) == lg.unstable - 1, (g, max(got), lg.unstable)
    stable = [e for k, e in enumerate(lg.ents) if k and e["Index"] < lg.unstable and e["Index"] >= ri]
    assert stable or not got or max(got) <= lg.offset
    for e in stable:
        d = b"" if e["data_nil"] else bytes(cl.data[e["data_off"]:e["data_off"] + e["data_len"]])
        assert got[e["Index"]] == (e["Type"], e["Term"], d), (g, e["Index"])
    if ctx is None:
        return len(rows), len(got), ri
    import ctypes
    from etcd_amd import _lib as L
    from etcd_amd import wal as W
    from etcd_amd.raftlead import _up
    recs = np.concatenate([_rows([[4, 0, 0, 0, 0, 0, 1]], 7), _rows([list(r) for r in rows], 7)])     # SAVE_CUT, nil
    cap = 128 * len(recs) + sum(int(r[5]) for r in rows) + 4096
    bufs = [_up(ctx, np.frombuffer(bytes(cl.data) + b"\0" * (8 - len(cl.data) % 8), dtype=np.uint8)), _up(ctx, recs),
            ctx.alloc(cap)]
    try:
        out_len, crc = ctypes.c_uint64(), ctypes.c_uint32()
        L.check(L.lib.ewal_save_device(ctx.handle, bufs[0].ptr, len(cl.data), bufs[1].ptr, len(recs), 0, bufs[2].ptr,
                                       cap, ctypes.byref(out_len), ctypes.byref(crc), None))
        dev = bufs[2].download(out_len.value)
        assert dev == raw and crc.value == enc.crc, g
        rd = W.readall_device(bufs[2], out_len.value, ri, host_view=memoryview(dev), with_ents=True)
    finally:
        for b in bufs:
            b.free()
    assert rd.status == L.OK and rd.last_crc == crc.value
    assert {e.Index: (e.Type, e.Term, bytes(e.Data or b"")) for e in rd.ents} == got
    assert (rd.state.Term, rd.state.Vote, rd.state.Commit) == \
        tuple(back["state"][k] for k in ("term", "vote", "commit"))
    return len(rows), len(got), ri
