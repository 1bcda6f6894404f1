"""Cases and the restatement for the three membership calls (include/ewal.h:
econf_batch_device, econf_scan_committed_device, econf_gate_batch_device).

The restatement is raft_model, imported unchanged, plus what it leaves to the
caller: ConfRaft adds r.removed, addNode / removeNode (raft/raft.go:426-435),
the head of Step (:376-387), the removed half of restore (:549-552) and
node.run's ApplyConfChange switch (raft/node.go:228-236); conf_change_unmarshal
is ConfChange.Unmarshal (raft/raftpb/raft.pb.go:705-813) to pb_model's
standard, field by field in the generated code's order.  Only the adapters
know the records' layout.  tests/host/conf_forms.cpp draws draw_request() and draw_bytes()
draw for draw."""
import json
import os

import numpy as np

import pb_model as P
import raft_model as R
from vote_step_cases import SplitMix

M64 = (1 << 64) - 1
OK, ERR_EOF, ERR_WRONG_TYPE, ERR_ENTRY_TYPE, PANIC_BOUNDS, NONTERMINATING, PANIC_CONF_TYPE, UNSUPPORTED = \
    0, 2, 7, 8, 33, 37, 47, 48
E_INVAL, E_NOMEM = -2, -3
ADD, REMOVE, DENIED, RELOAD = 1, 2, 3, 4
NOT_STEPPED, ADDED, REMOVED, DENIED_BACK, STOPPED, RELOADED, PANICKED = range(7)
ACTION_NAMES = ("not_stepped", "added", "removed", "denied_back", "stopped", "reloaded", "panicked")
G_PASS, G_DENIED, G_DROPPED = 1, 2, 3
FROM_SELF = 0xFFFFFFFF
PEERS, MAX_REMOVED, SKIP_DEPTH = 7, 14, 16
INT_MAX = (1 << 31) - 1
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raft_conf_kats.json")


def load_kats():
    return json.load(open(KATS))


class Unsupported(Exception):
    """A request the records cannot state (EWAL_UNSUPPORTED_ENCODING)."""


# ---- the model ------------------------------------------------------------------------------

class ConfRaft(R.Raft):
    """raft_model.Raft with r.removed (an insertion-ordered dict, as prs is)."""

    def __init__(self, id, peers):
        super().__init__(id, peers)
        self.removed = {}

    def shouldStop(self):   # raft.go:158
        return bool(self.removed.get(self.id))

    def softState(self):   # raft.go:160-162
        return dict(super().softState(), ShouldStop=self.shouldStop())

    def addNode(self, id):   # raft.go:426-429
        self.setProgress(id, 0, (self.raftLog.lastIndex() + 1) & M64)
        self.pendingConf = False

    def removeNode(self, id):   # raft.go:431-435
        self.prs.pop(id, None)
        self.pendingConf = False
        self.removed[id] = True

    def Step(self, m):   # raft.go:376-387, then the rest
        try:
            if self.removed.get(m["From"]):
                if m["From"] != self.id:
                    self.send(R.Message(R.MSG_DENIED, To=m["From"]))
                return "denied_back"
            if m["Type"] == R.MSG_DENIED:
                self.removed[self.id] = True
                return "stopped"
        finally:
            self.Commit = self.raftLog.committed
        return super().Step(m)

    def restoreRemoved(self, s):   # raft.go:549-552
        self.removed = {}
        for n in s["RemovedNodes"] or []:
            self.removed[n] = True

    def applyConfChange(self, type_, node):   # node.go:228-236
        if type_ == 0:
            self.addNode(node)
        elif type_ == 1:
            self.removeNode(node)
        else:
            raise R.Panic("conf_type")


def conf_change_marshal(id=0, type_=0, node=0, context=b""):   # raft.pb.go:1108-1130
    def varint(v):
        out = bytearray()
        while v >= 0x80:
            out.append((v & 0x7F) | 0x80)
            v >>= 7
        out.append(v)
        return bytes(out)
    return (b"\x08" + varint(id & M64) + b"\x10" + varint(type_ & M64) + b"\x18" + varint(node & M64) + b"\x22" +
            varint(len(context)) + bytes(context))


def _conf_change(data, m, run):
    l = len(data)
    index = 0
    while index < l:
        wire, index = P._wire(data, index, l)
        if wire is None:
            return P.ERR_UNEXPECTED_EOF
        field_num = P.i32(wire >> 3)
        wire_type = wire & 0x7
        if field_num in (1, 2, 3):
            if wire_type != 0:
                return P.ERR_WRONG_TYPE
            key = ("id", "type", "node")[field_num - 1]
            shift = 0
            while True:
                if index >= l:
                    return P.ERR_UNEXPECTED_EOF
                b = P.at(data, index)
                index += 1
                if field_num == 2:
                    m[key] = P.i32(m[key] | P.shl32(b & 0x7F, shift))
                else:
                    m[key] |= P.shl64(b & 0x7F, shift)
                if b < 0x80:
                    break
                shift += 7
        elif field_num == 4:
            if wire_type != 2:
                return P.ERR_WRONG_TYPE
            byte_len = 0
            shift = 0
            while True:
                if index >= l:
                    return P.ERR_UNEXPECTED_EOF
                b = P.at(data, index)
                index += 1
                byte_len = P.i64(byte_len | P.shl64(b & 0x7F, shift))
                if b < 0x80:
                    break
                shift += 7
            post_index = P.i64(index + byte_len)
            if post_index > l:
                return P.ERR_UNEXPECTED_EOF
            m["context"] = (m["context"] or b"") + P.cut(data, index, post_index)
            index = post_index
        else:
            index, err, seg = P._unknown(data, index, wire, l, run)
            if err is not None:
                return err
            m["unrec"] = (m["unrec"] or b"") + seg
    return None


def conf_change_unmarshal(data):
    """ConfChange.Unmarshal: (status, the struct as Go leaves it, the Run).  A
    run Go completes whose unknown groups nest deeper than the device walker's
    stack is UNSUPPORTED, as emsg_decode_batch_device words it."""
    m = dict(id=0, type=0, node=0, context=None, unrec=None)
    run = P.Run()
    try:
        err = _conf_change(bytes(data or b""), m, run)
        st = OK if err is None else err
    except P.GoPanic:
        st = PANIC_BOUNDS
    except P.NeverReturns:
        st = NONTERMINATING
    if st == OK and run.pushes > SKIP_DEPTH:
        st = UNSUPPORTED
    return st, m, run


def kind_of(type_):
    return (type_ & 0xFFFFFFFF) + 1


# ---- econf_batch_device: the adapters ----------------------------------------------------------
#
# arrays: groups (G, 32), pstate (G, 4), vstate (G, 8), rstate (G, 8), cstate (G, 16) uint64 rows, snaps (G, 8) or
# None, u64 (a flat array).  reqs: (n, 4) rows {group, kind, node, pad}.

def group(id=1, term=1, peers=(1, 2, 3), n_peers=None, off=0, nlog=1, pending=0, state=R.FOLLOWER, voted=0, granted=0,
          dirty=0, removed=(), match=None, next_=None):
    return dict(id=id, term=term, peers=tuple(peers), n_peers=len(peers) if n_peers is None else n_peers, off=off,
                nlog=nlog, pending=pending, state=state, voted=voted, granted=granted, dirty=dirty,
                removed=tuple(removed), match=match, next=next_)


def arrays_of(groups, snaps=None, u64=()):
    G = len(groups)
    a = dict(groups=np.zeros((G, 32), np.uint64), pstate=np.zeros((G, 4), np.uint64),
             vstate=np.zeros((G, 8), np.uint64), rstate=np.zeros((G, 8), np.uint64),
             cstate=np.zeros((G, 16), np.uint64), snaps=None, u64=np.array(list(u64), dtype=np.uint64))
    for g, d in enumerate(groups):
        a["groups"][g, 0:7] = [d["id"], d["term"], 0, d["off"], d["nlog"], 0, d["n_peers"]]
        for k, p in enumerate(d["peers"][:PEERS]):
            a["groups"][g, 7 + k] = p
            a["groups"][g, 14 + k] = d["match"][k] if d["match"] else 10 + k
            a["groups"][g, 21 + k] = d["next"][k] if d["next"] else 11 + k
        a["pstate"][g] = [8, 0, d["pending"], 0]
        a["vstate"][g, 0:6] = [d["state"], 0, 0, 0, d["voted"], d["granted"]]
        a["rstate"][g, 7] = d["dirty"]
        a["cstate"][g, 0] = len(d["removed"])
        for k, v in enumerate(d["removed"]):
            a["cstate"][g, 1 + k] = v
    if snaps is not None:
        a["snaps"] = np.zeros((G, 8), np.uint64)
        for g, s in enumerate(snaps):
            if s:
                a["snaps"][g, 6:8] = s          # (removed_off, n_removed)
    return a


def reqs_of(reqs):
    rows = np.zeros((len(reqs), 4), np.uint64)
    for k, r in enumerate(reqs):
        rows[k, :len(r)] = np.array([x & M64 for x in r], dtype=np.uint64)
    return rows


def copy_arrays(a):
    return {k: (None if v is None else v.copy()) for k, v in a.items()}


def _model_of(a, g):
    w = [int(x) for x in a["groups"][g]]
    v = [int(x) for x in a["vstate"][g]]
    c = [int(x) for x in a["cstate"][g]]
    r = ConfRaft.__new__(ConfRaft)
    r.id, r.Term, r.Commit, r.Vote, r.lead, r.elapsed = w[0], w[1], w[2], v[1], v[2], v[3]
    r.state, r.msgs, r.trace = v[0], [], []
    r.pendingConf = bool(int(a["pstate"][g, 2]))
    slots = min(w[6], PEERS)
    r.prs = {w[7 + k]: R.Progress(w[14 + k], w[21 + k]) for k in range(slots)}
    r.votes = {w[7 + k]: bool(v[5] >> k & 1) for k in range(slots) if v[4] >> k & 1}
    r.raftLog = R.RaftLog()
    r.raftLog.ents = [R.Entry() for _ in range(w[4])]
    r.raftLog.offset = w[3]
    r.removed = {x: True for x in c[1:1 + c[0]]}
    return r


def _write_back(a, g, r, high):
    """Row g from the model: the slots [len(prs), high) were freed by a remove and are zero."""
    gr = a["groups"]
    gr[g, 6] = len(r.prs)
    for k, (p, pr) in enumerate(r.prs.items()):
        gr[g, 7 + k], gr[g, 14 + k], gr[g, 21 + k] = p, pr.match, pr.next
    for k in range(len(r.prs), high):
        gr[g, 7 + k] = gr[g, 14 + k] = gr[g, 21 + k] = 0
    a["pstate"][g, 2] = int(r.pendingConf)
    voted = granted = 0
    for k, p in enumerate(r.prs):
        if p in r.votes:
            voted |= 1 << k
            granted |= (1 << k) if r.votes[p] else 0
    a["vstate"][g, 4:6] = [voted, granted]
    a["cstate"][g, 0] = len(r.removed)
    for k, x in enumerate(r.removed):
        a["cstate"][g, 1 + k] = x


def step_request(r, n_peers, kind, node, snap_removed=None):
    """One request on the model r (n_peers: the record's word, which may
    exceed what it holds).  Returns (action, messages); raises Unsupported or
    raft_model.Panic with r untouched."""
    if n_peers > PEERS:
        raise Unsupported("n_peers")
    if kind == ADD:
        if node not in r.prs and len(r.prs) == PEERS:
            raise Unsupported("an eighth peer")
        r.applyConfChange(0, node)
        return ADDED, []
    if kind == REMOVE:
        if node in r.prs and r.state == R.CANDIDATE and node in r.votes:
            raise Unsupported("r.votes keeps the key")
        if node not in r.removed and len(r.removed) == MAX_REMOVED:
            raise Unsupported("a 15th removed id")
        r.applyConfChange(1, node)
        r.votes.pop(node, None)            # never read before the next reset
        return REMOVED, []
    if kind == DENIED:
        if not r.removed.get(node) and r.id not in r.removed and len(r.removed) == MAX_REMOVED:
            raise Unsupported("a 15th removed id")
        r.msgs = []
        what = r.Step(R.Message(R.MSG_DENIED, From=node))
        return (DENIED_BACK if what == "denied_back" else STOPPED), r.msgs
    if kind == RELOAD:
        if len(dict.fromkeys(snap_removed)) > MAX_REMOVED:
            raise Unsupported("more than 14 removed ids")
        r.restoreRemoved(dict(RemovedNodes=list(snap_removed)))
        return RELOADED, []
    r.applyConfChange(kind - 1, node)      # panics
    raise AssertionError("unreachable")


def runs_of(reqs):
    """[(first, end)] of the maximal runs of equal group words."""
    out, i, n = [], 0, len(reqs)
    while i < n:
        j = i
        while j + 1 < n and reqs[j + 1, 0] == reqs[i, 0]:
            j += 1
        out.append((i, j + 1))
        i = j + 1
    return out


def _group_ok(a, g):
    w = [int(x) for x in a["groups"][g]]
    v = [int(x) for x in a["vstate"][g]]
    c = [int(x) for x in a["cstate"][g]]
    s = [int(x) for x in a["pstate"][g]]
    rs = [int(x) for x in a["rstate"][g]]
    if any(w[28:32]) or s[3] or v[6] or v[7] or c[15]:
        return False
    if c[0] > MAX_REMOVED or s[2] > 1 or rs[7] > 1 or v[0] > 2:
        return False
    slots = min(w[6], PEERS)
    mask = (1 << slots) - 1
    if (v[4] | v[5]) & ~mask or v[5] & ~v[4]:
        return False
    return len(set(w[7:7 + slots])) == slots


def validate_batch(a, reqs, msgs_cap=None, G=None, n=None):
    """The call's status class: OK, E_INVAL or E_NOMEM (msgs_cap None: the size query)."""
    G = len(a["groups"]) if G is None else G
    n = len(reqs) if n is None else n
    if n >= INT_MAX or G >= INT_MAX:
        return E_INVAL
    if n == 0:
        return OK
    n_u64 = len(a["u64"])
    seen = set()
    for i, j in runs_of(reqs):
        g = int(reqs[i, 0])
        if g >= G or g in seen:
            return E_INVAL
        seen.add(g)
        for k in range(i, j):
            if int(reqs[k, 3]) != 0:
                return E_INVAL
            if int(reqs[k, 1]) == RELOAD:
                if a["snaps"] is None:
                    return E_INVAL
                off, cnt = int(a["snaps"][g, 6]), int(a["snaps"][g, 7])
                if off > n_u64 or cnt > n_u64 - off:
                    return E_INVAL
        if not _group_ok(a, g):
            return E_INVAL
    if msgs_cap is not None and expected_batch(a, reqs)["n_msgs"] > msgs_cap:
        return E_NOMEM
    return OK


def expected_batch(a, reqs, emit=True):
    """What a valid call leaves: res_rows (n, 6), msg_rows (n_msgs, 18), the
    five arrays afterwards (the inputs' copies when not emit), n_msgs,
    n_changed, outcomes [(status, action)]."""
    out = copy_arrays(a)
    n = len(reqs)
    res = np.zeros((n, 6), np.uint64)
    msgs, outcomes, n_changed = [], [], 0
    for i, j in runs_of(reqs):
        g = int(reqs[i, 0])
        r = _model_of(out, g)
        n_peers = int(out["groups"][g, 6])
        high = len(r.prs)
        dirty = int(out["rstate"][g, 7])
        stopped = False
        for k in range(i, j):
            kind, node = int(reqs[k, 1]), int(reqs[k, 2])
            status, action, sent = OK, NOT_STEPPED, []
            if not stopped:
                before = (r.nodes(), r.shouldStop())
                snap_removed = None
                if kind == RELOAD:
                    off, cnt = int(a["snaps"][g, 6]), int(a["snaps"][g, 7])
                    snap_removed = [int(x) for x in a["u64"][off:off + cnt]]
                try:
                    action, sent = step_request(r, n_peers, kind, node, snap_removed)
                    n_peers = len(r.prs)
                    high = max(high, len(r.prs))
                    if (r.nodes(), r.shouldStop()) != before:
                        dirty = 1
                    if action != DENIED_BACK:
                        n_changed += 1
                    if kind == RELOAD:
                        out["cstate"][g, 1:15] = 0
                except Unsupported:
                    status, action, stopped = UNSUPPORTED, PANICKED, True
                except R.Panic as e:
                    assert e.name == "conf_type"
                    status, action, stopped = PANIC_CONF_TYPE, PANICKED, True
            res[k] = [status | (action << 32), len(msgs), len(sent), n_peers, len(r.removed), 0]
            outcomes.append((status, action))
            for m in sent:
                assert (m["Type"], m["From"], m["Term"]) == (R.MSG_DENIED, r.id, r.Term)
                msgs.append([R.MSG_DENIED, m["To"], m["From"], m["Term"]] + [0] * 14)
        if int(a["groups"][g, 6]) <= PEERS:
            _write_back(out, g, r, high)
        out["rstate"][g, 7] = dirty
    x = dict(res_rows=res, msg_rows=np.array(msgs, dtype=np.uint64).reshape(-1, 18), n_msgs=len(msgs),
             n_changed=n_changed, outcomes=outcomes)
    x["arrays"] = out if emit else copy_arrays(a)
    return x


# ---- econf_scan_committed_device ------------------------------------------------------------------

def entry_row(term, index, type_, data_off=0, data_len=0, data_nil=0):
    return [term, index, data_off, data_len, (type_ & 0xFFFFFFFF) | (data_nil << 32)]


def scan_case(per_sel, G=None, sel=None):
    """A scan call of per-selection entry lists: an entry is (type, data bytes or
    None for nil) or (type, data, data_nil).  Returns dict(ready (n, 12), ents,
    data, sel, G, n).  Selection i's committed range follows selection i - 1's,
    after one entry of padding that no range names."""
    ready = np.zeros((len(per_sel), 12), np.uint64)
    ents, data = [], bytearray()
    for i, lst in enumerate(per_sel):
        ents.append(entry_row(9, 9, 1, 0, 0, 1))
        ready[i, 6:8] = [len(ents) if lst else 0, len(lst)]
        for k, e in enumerate(lst):
            type_, d = e[0], e[1]
            nil = e[2] if len(e) > 2 else (1 if d is None else 0)
            d = d or b""
            ents.append(entry_row(2 + i % 3, 100 * i + k + 1, type_, len(data) if d else 0, len(d), nil))
            data += d
    n = len(per_sel)
    return dict(ready=ready, ents=np.array(ents, dtype=np.uint64).reshape(-1, 5), data=bytes(data), sel=sel,
                G=n if G is None else G, n=n)


def validate_scan(c, reqs_cap=None):
    n, G = c["n"], c["G"]
    if n >= INT_MAX or G >= INT_MAX or len(c["ents"]) >= INT_MAX or (c["sel"] is None and n != G):
        return E_INVAL
    for i in range(n):
        g = int(c["sel"][i]) if c["sel"] is not None else i
        first, cnt = int(c["ready"][i, 6]), int(c["ready"][i, 7])
        if g >= G or (cnt and (first > len(c["ents"]) or cnt > len(c["ents"]) - first)):
            return E_INVAL
    for i in range(n):
        first, cnt = int(c["ready"][i, 6]), int(c["ready"][i, 7])
        for e in c["ents"][first:first + cnt]:
            w = [int(x) for x in e]
            type_, nil = P.i32(w[4]), P.i32(w[4] >> 32)
            if type_ == 1 and (nil < 0 or nil > 2 or
                               (nil != 2 and (w[2] > len(c["data"]) or w[3] > len(c["data"]) - w[2]))):
                return E_INVAL
    if reqs_cap is not None and expected_scan(c)["n_reqs"] > reqs_cap:
        return E_NOMEM
    return OK


def expected_scan(c):
    """scan_rows (n, 6), req_rows, applied_rows, n_reqs, n_entries, statuses."""
    n = c["n"]
    scan = np.zeros((n, 6), np.uint64)
    reqs, applied, n_entries = [], [], 0
    for i in range(n):
        g = int(c["sel"][i]) if c["sel"] is not None else i
        first, cnt = int(c["ready"][i, 6]), int(c["ready"][i, 7])
        n_entries += cnt
        status = detail = bad_pos = 0
        scanned, req_first = cnt, len(reqs)
        for k in range(cnt):
            w = [int(x) for x in c["ents"][first + k]]
            type_, nil = P.i32(w[4]), w[4] >> 32
            st = OK
            if type_ == 1:
                if nil == 2:
                    st = UNSUPPORTED
                else:
                    st, m, _ = conf_change_unmarshal(b"" if nil else c["data"][w[2]:w[2] + w[3]])
                if st == OK:
                    reqs.append([g, kind_of(m["type"]), m["node"], 0])
                    applied.append([m["id"], w[1], w[0], first + k])
            elif type_ != 0:
                st, detail = ERR_ENTRY_TYPE, type_ & 0xFFFFFFFF
            if st != OK:
                status, bad_pos, scanned = st, first + k, k
                break
        scan[i] = [status | (detail << 32), req_first, len(reqs) - req_first, bad_pos, scanned, 0]
    return dict(scan_rows=scan, req_rows=np.array(reqs, dtype=np.uint64).reshape(-1, 4),
                applied_rows=np.array(applied, dtype=np.uint64).reshape(-1, 4), n_reqs=len(reqs), n_entries=n_entries,
                statuses=[int(x) & 0xFFFFFFFF for x in scan[:, 0]])


def nested_groups(tags, field=9):
    """An unknown group field whose start-group tags nest `tags` deep."""
    return bytes([field << 3 | 3]) * tags + bytes([field << 3 | 4]) * tags


def scan_edge_bodies():
    """(name, Data) of the decode edges the issue lists; every one is an EntryConfChange's Data."""
    base = conf_change_marshal(300, 1, 128, b"ab")
    out = [("empty", b""), ("nil", None), ("plain", base),
           ("ten_byte_varint", b"\x08" + b"\xff" * 9 + b"\x01\x18\x05"),
           ("eleven_byte_varint", b"\x18" + b"\x80" * 10 + b"\x01"),
           ("repeated_field", b"\x18\x01\x18\x06\x10\x01\x10\x00\x08\x10\x08\x01"),
           ("type_past_32_bits", b"\x10\x80\x80\x80\x80\x10\x18\x02"),
           ("type_minus_one", b"\x10" + b"\xff" * 9 + b"\x01\x18\x02"),
           ("unknown_varint", b"\x28\x07" + base), ("unknown_fixed64", b"\x29" + bytes(8) + base),
           ("unknown_bytes", b"\x2a\x02zz" + base), ("unknown_fixed32_cut", b"\x2d\x00\x00"),
           ("wire_type_6", b"\x2e\x00"), ("end_group_alone", b"\x2c\x08\x01"),
           ("group_depth_16", nested_groups(SKIP_DEPTH + 1) + base),
           ("group_depth_17", nested_groups(SKIP_DEPTH + 2) + base),
           ("group_unterminated", b"\x4b\x08\x01"),
           ("context_past_end", b"\x22\x05ab"), ("context_negative", b"\x22" + b"\xff" * 9 + b"\x01")]
    for f in (1, 2, 3):
        out.append(("wrong_wire_f%d" % f, bytes([f << 3 | 2, 0])))
    out.append(("wrong_wire_f4", b"\x20\x00"))
    out += [("cut_%d" % k, base[:k]) for k in range(len(base))]
    return out


# ---- econf_gate_batch_device --------------------------------------------------------------------

def expected_gate(grows, crows, recs, from_word):
    """res_rows (n, 4), pass_rows, msg_rows, n_pass, n_msgs, actions."""
    n = len(recs)
    res = np.zeros((n, 4), np.uint64)
    passed, msgs, actions = [], [], []
    for i in range(n):
        g = int(recs[i, 0])
        r = ConfRaft.__new__(ConfRaft)
        r.id, r.Term, r.msgs = int(grows[g, 0]), int(grows[g, 1]), []
        r.raftLog = R.RaftLog()
        c = [int(x) for x in crows[g]]
        r.removed = {x: True for x in c[1:1 + c[0]]}
        frm = r.id if from_word == FROM_SELF else int(recs[i, from_word])
        if r.removed.get(frm):               # Step's first lines, raft.go:376-382
            assert r.Step(R.Message(R.MSG_VOTE, From=frm)) == "denied_back"
            action = G_DENIED if r.msgs else G_DROPPED
        else:
            action = G_PASS
        res[i] = [action << 32, len(passed) if action == G_PASS else 0, len(msgs) if action == G_DENIED else 0, 0]
        if action == G_PASS:
            passed.append(recs[i].copy())
        for m in r.msgs:
            msgs.append([R.MSG_DENIED, m["To"], r.id, r.Term] + [0] * 14)
        actions.append(action)
    return dict(res_rows=res, pass_rows=np.array(passed, dtype=np.uint64).reshape(-1, recs.shape[1]),
                msg_rows=np.array(msgs, dtype=np.uint64).reshape(-1, 18), n_pass=len(passed), n_msgs=len(msgs),
                actions=actions)


def validate_gate(grows, crows, recs, rec_bytes, from_word, pass_cap=None, msgs_cap=None):
    n, G = len(recs), len(grows)
    if rec_bytes not in (48, 64, 96) or (from_word != FROM_SELF and not 1 <= from_word < rec_bytes // 8):
        return E_INVAL
    if (pass_cap is None) != (msgs_cap is None):
        return E_INVAL
    for i in range(n):
        g = int(recs[i, 0])
        if g >= G or int(crows[g, 0]) > MAX_REMOVED or int(crows[g, 15]) != 0:
            return E_INVAL
    x = expected_gate(grows, crows, recs, from_word)
    if pass_cap is not None and (x["n_pass"] > pass_cap or x["n_msgs"] > msgs_cap):
        return E_NOMEM
    return OK


# ---- generators ----------------------------------------------------------------------------------

NP_TABLE = (0, 1, 2, 3, 3, 3, 3, 4, 5, 5, 6, 6, 7, 7, 3, 8)
KIND_TABLE = (1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 0)
NREM_TABLE = (0, 0, 0, 0, 1, 1, 2, 2, 3, 5, 5, 8, 12, 13, 13, 14)
STATE_TABLE = (0, 0, 0, 1, 2, 2, 0, 2)
LEN_TABLE = (0, 1, 3, 14, 15, 20)


def draw_request(r):
    """One random group and request from the SplitMix r, as conf_forms.cpp draws
    it: (group dict, kind, node, the snapshot's RemovedNodes)."""
    np_ = NP_TABLE[r.rnd(16)]
    pid = [10 + 3 * k for k in range(PEERS)]
    idmode, ik = r.rnd(4), r.rnd(7)
    id_ = 999 if idmode == 0 else pid[ik]
    term, off, nlog = r.rnd(5), r.rnd(3), r.rnd(4)
    pending, state = r.rnd(2), STATE_TABLE[r.rnd(8)]
    slots = min(np_, PEERS)
    mask = (1 << slots) - 1
    voted = r.next() & mask
    voted &= r.next()
    granted = voted & r.next()
    dirty = r.rnd(2)
    nrem = NREM_TABLE[r.rnd(16)]
    rem = [100 + k for k in range(nrem)]
    remmode = r.rnd(4)
    if nrem and remmode == 0:
        rem[0] = pid[2]
    if nrem and remmode == 1:
        rem[0] = id_
    kind = KIND_TABLE[r.rnd(16)]
    nodemode, a, b = r.rnd(5), r.rnd(7), r.rnd(14)
    node = (500 + a % 3, pid[0], pid[a], id_, 100 + b)[nodemode]
    ln, m = LEN_TABLE[r.rnd(6)], r.rnd(16) + 1
    snap = [100 + (k % m) for k in range(ln)]
    g = group(id=id_, term=term, peers=pid[:slots], n_peers=np_, off=off, nlog=nlog, pending=pending, state=state,
              voted=voted, granted=granted, dirty=dirty, removed=rem, match=list(range(PEERS)),
              next_=[k + 1 for k in range(PEERS)])
    return g, kind, node, snap


def draw_bytes(r):
    """A random ConfChange body, as conf_forms.cpp draws it (no groups: the
    host program's Skip has none)."""
    out = bytearray()
    for _ in range(r.rnd(6)):
        what = r.rnd(10)
        v = r.next() >> r.rnd(64)
        if what < 3:
            out.append((what + 1) << 3)
            while v >= 0x80:
                out.append((v & 0x7F) | 0x80)
                v >>= 7
            out.append(v)
        elif what == 3:
            ln = v % 4
            out += bytes([0x22, ln]) + bytes([0x61] * ln)
        elif what == 4:
            out += bytes([((v % 4) + 1) << 3 | (5 if v % 4 < 3 else 0), 0, 0, 0, 0])
        elif what == 5:
            out += bytes([0x28, v & 0x7F])
        elif what == 6:
            out += bytes([0x29]) + bytes([v & 0xFF] * 8)
        elif what == 7:
            out += bytes([0x2A, 2, 1, 2])
        elif what == 8:
            out += bytes([0x2D, 1, 2, 3, 4])
        else:
            out += bytes([0x2E if v & 1 else 0x2C])
    if r.rnd(4) == 0 and out:
        del out[r.rnd(len(out) + 1):]
    return bytes(out)


def fold(h, v):
    return ((h ^ (v & M64)) * 0x100000001B3) & M64


def digest(seed, runs):
    """(digest, the request actions' counts, the decode statuses' counts {status: n},
    the gate actions' counts) over draw cases 0 .. runs - 1, as conf_forms prints them."""
    h, acts, sts, gates = 0xCBF29CE484222325, [0] * 7, {}, [0] * 4
    for run in range(runs):
        r = SplitMix(seed, run)
        mode = r.rnd(3)
        if mode == 0:
            g, kind, node, snap = draw_request(r)
            a = arrays_of([g], snaps=[(0, len(snap))], u64=snap)
            x = expected_batch(a, reqs_of([(0, kind, node)]))
            status, action = x["outcomes"][0]
            acts[action] += 1
            h = fold(fold(fold(h, status), action), x["n_msgs"])
            o = x["arrays"]
            for v in [o["groups"][0, 6]] + list(o["groups"][0, 7:28]) + [o["pstate"][0, 2]] + \
                    list(o["vstate"][0, 4:6]) + [o["rstate"][0, 7]] + list(o["cstate"][0, 0:15]):
                h = fold(h, int(v))
        elif mode == 1:
            st, m, _ = conf_change_unmarshal(draw_bytes(r))
            sts[st] = sts.get(st, 0) + 1
            for v in (st, m["id"], m["type"] & 0xFFFFFFFF, m["node"]):
                h = fold(h, v)
        else:
            g, _, node, _ = draw_request(r)
            a = arrays_of([g])
            recs = np.array([[0, node, 0, 0, 0, 0]], dtype=np.uint64)
            action = expected_gate(a["groups"], a["cstate"], recs, 1)["actions"][0]
            gates[action] += 1
            h = fold(h, action)
    return h, acts, sts, gates


def random_batch(seed, G, n_runs):
    """A random econf_batch_device call over G groups: n_runs runs of 1 .. 4
    requests (a few longer), each naming another group.  Returns (arrays, reqs)."""
    groups, snaps, u64 = [], [], []
    picks = []
    for g in range(G):
        r = SplitMix(seed, g)
        d, kind, node, snap = draw_request(r)
        groups.append(d)
        snaps.append((len(u64), len(snap)))
        u64 += snap
        picks.append(r)
    order = list(range(G))
    rr = SplitMix(seed, 1 << 40)
    for k in range(G - 1, 0, -1):
        j = rr.rnd(k + 1)
        order[k], order[j] = order[j], order[k]
    reqs = []
    for g in order[:n_runs]:
        r = picks[g]
        ln = (1, 1, 1, 2, 2, 3, 4, 9)[r.rnd(8)]
        for _ in range(ln):
            _, kind, node, _ = draw_request(r)
            # a run's later requests rarely panic: most of a run is stepped
            if kind == 0 and r.rnd(4):
                kind = 1
            reqs.append((g, kind, node))
    return arrays_of(groups, snaps=snaps, u64=u64), reqs_of(reqs)


def random_scan(seed, n):
    """A random scan call of n selections with 0 .. 5 entries each (a few with 70)."""
    r = SplitMix(seed, 2 << 40)
    per = []
    for i in range(n):
        cnt = (0, 1, 1, 2, 3, 3, 5, 70)[r.rnd(8)] if r.rnd(16) else 70
        lst = []
        for _ in range(cnt):
            t = r.rnd(16)
            if t < 7:
                lst.append((0, b"x" * r.rnd(4)))
            elif t == 15 and r.rnd(4) == 0:
                lst.append((2 + r.rnd(3), b""))
            elif t < 14:
                lst.append((1, conf_change_marshal(r.next() >> r.rnd(64), r.rnd(2), r.rnd(9), b"c" * r.rnd(3))))
            else:
                lst.append((1, draw_bytes(r)))
        per.append(lst)
    return scan_case(per)


def random_gate(seed, G, n, words, from_word):
    """A random gate call: G groups as draw_request makes them, n records of
    `words` words whose From is drawn from the group's removed ids, its own id
    and strangers."""
    groups = [draw_request(SplitMix(seed, g))[0] for g in range(G)]
    a = arrays_of(groups)
    r = SplitMix(seed, 3 << 40)
    recs = np.zeros((n, words), np.uint64)
    for i in range(n):
        g = r.rnd(G)
        d = groups[g]
        pool = list(d["removed"]) + [d["id"], 999, 10]
        recs[i, 0] = g
        for w in range(1, words):
            recs[i, w] = r.next() >> 8
        if from_word != FROM_SELF:
            recs[i, from_word] = pool[r.rnd(len(pool))]
    return a, recs
