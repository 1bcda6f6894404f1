"""Cases and the Python restatement for the batched StartNode / RestartNode
(enode_batch_device): raft.StartNode and raft.RestartNode (raft/node.go:125-161)
on raft_model's Raft / Node / to_arrays, with loadState / loadEnts
(raft/raft.go:597-606) and conf_cases' r.removed added.  Holds both
constructors, validate(), expected(), the call builder, the boundary lattice,
the seeded generators (random_call for the device, draw_case / digest for
tests/host/node_forms.cpp, restated draw for draw) and the loader of the
reference's tables (tests/golden/raft_node_kats.json)."""
import json
import os

import numpy as np

import conf_cases as K
import raft_model as M
from vote_step_cases import SplitMix

M64 = (1 << 64) - 1
OK, UNSUPPORTED, PANIC_NONE_ID = 0, 48, 49
E_INVAL, E_NOMEM = -2, -3
KIND_NONE, KIND_RESTART, KIND_START = 0, 1, 2
NONE, RESTARTED, RESTARTED_SNAP, STARTED, PANICKED = range(5)
ACTION_NAMES = ("none", "restarted", "restarted_snap", "started", "panicked")
NO_SNAP = M64
PEERS, MAX_REMOVED, MAX_NODES = 7, 14, 64
INT_MAX = (1 << 31) - 1
GROUP_WORDS, STATE_WORDS, VSTATE_WORDS, RSTATE_WORDS, CSTATE_WORDS, SNAP_WORDS, ENTRY_WORDS = 32, 4, 8, 8, 16, 8, 5
REQ_WORDS, PEER_WORDS, RESULT_WORDS = 16, 4, 6
RECORDS = (("groups", GROUP_WORDS), ("pstate", STATE_WORDS), ("vstate", VSTATE_WORDS), ("rstate", RSTATE_WORDS),
           ("cstate", CSTATE_WORDS), ("snaps", SNAP_WORDS))
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raft_node_kats.json")


def load_kats():
    return json.load(open(KATS))


# ---- the model ------------------------------------------------------------------------------

class NodeRaft(K.ConfRaft):
    """conf_cases' raft with the whole of raft.restore, loadState and loadEnts."""

    def restore(self, s):   # raft.go:535-554
        if not super().restore(s):
            return False
        self.restoreRemoved(s)
        return True

    def loadEnts(self, ents):   # raft.go:597-599, log.go:40-43
        self.raftLog.ents = ents
        self.raftLog.unstable = (self.raftLog.offset + len(ents)) & M64

    def loadState(self, st):   # raft.go:601-606
        self.raftLog.committed = st["Commit"]
        self.Term, self.Vote, self.Commit = st["Term"], st["Vote"], st["Commit"]


def _check_supported(s):
    """What the records cannot state of a restore that runs."""
    nodes, removed = s["Nodes"] or [], s["RemovedNodes"] or []
    if len(nodes) > MAX_NODES or len(dict.fromkeys(nodes)) > PEERS or len(dict.fromkeys(removed)) > MAX_REMOVED:
        raise K.Unsupported()


def RestartNode(id, snapshot, st, ents):   # node.go:151-161; returns node.run's state around the raft
    r = NodeRaft(id, [])
    restored = False
    if snapshot is not None:
        if snapshot["Index"] > r.raftLog.committed:
            _check_supported(snapshot)
        restored = r.restore(snapshot)
    r.loadState(st)
    r.loadEnts(ents)
    n = M.Node(r)
    n.restored = restored
    return n


def StartNode(id, peers):   # node.go:128-146; peers: (id, context) pairs
    r = NodeRaft(id, [])
    ents = []
    for i, (pid, context) in enumerate(peers):
        data = K.conf_change_marshal(0, 0, pid, context or b"")
        ents.append(M.Entry(Type=M.ENTRY_CONF_CHANGE, Term=1, Index=i + 1, Data=data, data_len=len(data), data_nil=0))
    r.raftLog.append(0, ents)
    r.raftLog.committed = len(ents)
    n = M.Node(r)
    # Go's r.Commit is copied at the first Step only; the records' HardState is {term, vote, committed}, so the
    # previous one is seeded with the log's committed: the first Ready carries no HardState either way
    n.prevHardSt = dict(Term=0, Vote=0, Commit=len(ents))
    return n


# ---- the call ---------------------------------------------------------------------------------

def entry_row(term, index, type_=0, data_off=0, data_len=0, data_nil=0):
    return [term & M64, index & M64, data_off, data_len, (type_ & 0xFFFFFFFF) | (data_nil << 32)]


def snapshot(index=0, term=0, nodes=(), removed=(), data_off=0, data_len=0):
    return dict(index=index & M64, term=term & M64, nodes=list(nodes), removed=list(removed), data_off=data_off,
                data_len=data_len)


def restart(id=1, ents=(), st=(0, 0, 0), snap=None, cap=None, delta=0, group=None):
    """A kind-1 request: ents entry rows, st (term, vote, commit), snap a snapshot() or None."""
    return dict(kind=KIND_RESTART, id=id, ents=[list(e) for e in ents], st=tuple(st), snap=snap, cap=cap, delta=delta,
                group=group)


def start(id=1, peers=((1, b""),), cap=None, group=None):
    """A kind-2 request: peers (id, context) pairs."""
    return dict(kind=KIND_START, id=id, peers=[(p, bytes(c or b"")) for p, c in peers], cap=cap, group=group)


def none(group=None):
    return dict(kind=KIND_NONE, group=group)


def _canary(seed, shape):
    r = SplitMix(seed, shape[0])
    return np.array([[r.next() for _ in range(shape[1])] for _ in range(shape[0])], dtype=np.uint64).reshape(shape)


def call_of(specs, G=None, groups=None, slack=2, seed=1, data_base=0, data_cap=None, data_fill=0):
    """A call over the request specs (restart(), start(), none()): every array
    laid out, the record rows, the windows and d_data full of canary words
    (invalid ones included), each window `cap` slots (default: what the node
    needs plus `slack` canary slots).  groups: the group of each request
    (default 0 .. n-1, or a spec's own)."""
    n = len(specs)
    G = max(n, 1) if G is None else G
    order = list(range(n)) if groups is None else list(groups)
    reqs = np.zeros((n, REQ_WORDS), np.uint64)
    src, in_snaps, u64, peers, ctx = [], [], [7, 7], [], bytearray(b"\xee")
    at = 3                                           # the windows start past a few canary slots
    need = 0
    for k, s in enumerate(specs):
        g = s["group"] if s.get("group") is not None else order[k]
        reqs[k, 0], reqs[k, 1], reqs[k, 11] = g, s["kind"], NO_SNAP
        if s["kind"] == KIND_NONE:
            continue
        nlog = len(s["ents"]) if s["kind"] == KIND_RESTART else 1 + len(s["peers"])
        cap = nlog + slack if s["cap"] is None else s["cap"]
        reqs[k, 2], reqs[k, 3], reqs[k, 4] = s["id"], at, cap
        at += cap + 1
        if s["kind"] == KIND_RESTART:
            src.append(entry_row(99, 99, 0, 1, 1, 0))    # a gap between the shards' ranges
            reqs[k, 5], reqs[k, 6], reqs[k, 7] = len(src), len(s["ents"]), s["delta"]
            src += s["ents"]
            reqs[k, 8:11] = np.array(s["st"], dtype=np.uint64)
            if s["snap"] is not None:
                sn = s["snap"]
                reqs[k, 11] = len(in_snaps)
                in_snaps.append([sn["index"], sn["term"], sn["data_off"], sn["data_len"], len(u64), len(sn["nodes"]),
                                 len(u64) + len(sn["nodes"]), len(sn["removed"])])
                u64 += sn["nodes"] + sn["removed"] + [5]
        else:
            reqs[k, 5], reqs[k, 6] = len(peers), len(s["peers"])
            for pid, c in s["peers"]:
                peers.append([pid, len(ctx), len(c), 0])
                ctx += c + b"\xee"
                need += len(K.conf_change_marshal(0, 0, pid, c))
    c = dict(G=G, n=n, reqs=reqs, n_ents_total=at + 2,
             src=np.array(src, dtype=np.uint64).reshape(-1, ENTRY_WORDS),
             in_snaps=np.array(in_snaps, dtype=np.uint64).reshape(-1, SNAP_WORDS),
             u64=np.array(u64, dtype=np.uint64), peers=np.array(peers, dtype=np.uint64).reshape(-1, PEER_WORDS),
             ctx=bytes(ctx), data_base=data_base, data_cap=need + data_fill if data_cap is None else data_cap)
    for j, (name, words) in enumerate(RECORDS):
        c[name] = _canary(seed * 16 + j, (G, words))
    c["ents"] = _canary(seed * 16 + 9, (at + 2, ENTRY_WORDS))
    r = SplitMix(seed, 77)
    c["data"] = bytes(r.next() & 0xFF for _ in range(c["data_cap"]))
    return c


def copy_call(c):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def _req(c, i):
    w = [int(x) for x in c["reqs"][i]]
    return dict(group=w[0], kind=w[1], id=w[2], ents_first=w[3], ents_cap=w[4], src_first=w[5], n_src=w[6],
                data_delta=w[7], st=dict(Term=w[8], Vote=w[9], Commit=w[10]), snap=w[11], pad=w[12:16])


def _inside(first, count, total):
    return count <= total and first <= total - count


def validate(c, G=None, n=None):
    """The status the call returns: OK, E_INVAL or E_NOMEM, INVAL winning.
    data_cap None: the size query."""
    G = c["G"] if G is None else G
    n = c["n"] if n is None else n
    if n >= INT_MAX or G >= INT_MAX:
        return E_INVAL
    inval = nomem = False
    named, nbytes = set(), 0
    for i in range(n):
        q = _req(c, i)
        if q["group"] >= G or q["kind"] > KIND_START or any(q["pad"]):
            inval = True
            continue
        if q["group"] in named:
            inval = True
        named.add(q["group"])
        if q["kind"] == KIND_NONE:
            continue
        if not _inside(q["ents_first"], q["ents_cap"], c["n_ents_total"]):
            inval = True
            continue
        if q["kind"] == KIND_RESTART:
            if not _inside(q["src_first"], q["n_src"], len(c["src"])):
                inval = True
                continue
            if q["snap"] != NO_SNAP:
                if q["snap"] >= len(c["in_snaps"]):
                    inval = True
                    continue
                s = [int(x) for x in c["in_snaps"][q["snap"]]]
                if not _inside(s[4], s[5], len(c["u64"])) or not _inside(s[6], s[7], len(c["u64"])):
                    inval = True
                    continue
            nomem |= q["n_src"] > q["ents_cap"]
        else:
            if not _inside(q["src_first"], q["n_src"], len(c["peers"])):
                inval = True
                continue
            bad = False
            for p in c["peers"][q["src_first"]:q["src_first"] + q["n_src"]]:
                p = [int(x) for x in p]
                if p[3] != 0 or not _inside(p[1], p[2], len(c["ctx"])):
                    bad = True
                    break
                if q["id"] != 0:
                    nbytes += len(K.conf_change_marshal(0, 0, p[0], b"")) + p[2]
            if bad:
                inval = True
                continue
            nomem |= 1 + q["n_src"] > q["ents_cap"]
    if not inval and not nomem and c["data_cap"] is not None and nbytes > c["data_cap"]:
        nomem = True
    return E_INVAL if inval else E_NOMEM if nomem else OK


def build(c, q):
    """The node of request q (a _req dict) of call c: (status, action, the model
    Node or None, the peers' marshalled bytes)."""
    try:
        if q["kind"] == KIND_START:
            peers = []
            for p in c["peers"][q["src_first"]:q["src_first"] + q["n_src"]]:
                p = [int(x) for x in p]
                peers.append((p[0], c["ctx"][p[1]:p[1] + p[2]]))
            n = StartNode(q["id"], peers)
            return OK, STARTED, n, [e["Data"] for e in n.r.raftLog.ents[1:]]
        snap = None
        if q["snap"] != NO_SNAP:
            snap = M.snapshot_of_row(c["in_snaps"][q["snap"]], c["u64"])
        ents = []
        for row in c["src"][q["src_first"]:q["src_first"] + q["n_src"]]:
            row = [int(x) for x in row]
            if row[4] >> 32 == 0:
                row[2] = (row[2] + q["data_delta"]) & M64
            ents.append(M.entry_of_row(row))
        n = RestartNode(q["id"], snap, q["st"], ents)
        return OK, RESTARTED_SNAP if n.restored else RESTARTED, n, []
    except M.Panic as p:
        assert p.name == "none_id"
        return PANIC_NONE_ID, PANICKED, None, []
    except K.Unsupported:
        return UNSUPPORTED, PANICKED, None, []


def write_rows(a, g, n, first, cap):
    """Every word of group g's records, its snapshot row and its window's first
    len(ents) slots from the model node n: to_arrays on zeroed rows."""
    for name, _ in RECORDS:
        a[name][g] = 0
    a["groups"][g, 5], a["pstate"][g, 0] = first, cap
    M.to_arrays(n, a, g)
    removed = list(n.r.removed)
    a["cstate"][g, 0] = len(removed)
    a["cstate"][g, 1:1 + len(removed)] = np.array(removed, dtype=np.uint64)


def expected(c, emit=True):
    """What a valid call leaves: the arrays, d_data, the result rows and the
    counters.  emit False: the size query."""
    a = {k: c[k].copy() for k in ("groups", "pstate", "vstate", "rstate", "cstate", "snaps", "ents")}
    data = bytearray(c["data"])
    res = np.zeros((c["n"], RESULT_WORDS), np.uint64)
    outcomes, pos, n_copied, n_built = [], 0, 0, 0
    for i in range(c["n"]):
        q = _req(c, i)
        if q["kind"] == KIND_NONE:
            outcomes.append((OK, NONE))
            continue
        status, action, n, bodies = build(c, q)
        outcomes.append((status, action))
        res[i, 0] = status | (action << 32)
        if status != OK:
            continue
        n_built += 1
        lg = n.r.raftLog
        res[i, 1:5] = np.array([len(lg.ents), lg.committed, lg.offset, len(n.r.prs)], dtype=np.uint64)
        if q["kind"] == KIND_START:
            res[i, 5] = pos
            for e, body in zip(lg.ents[1:], bodies):
                e["data_off"] = (c["data_base"] + pos) & M64
                if emit:
                    data[pos:pos + len(body)] = body
                pos += len(body)
        else:
            n_copied += q["n_src"]
        if emit:
            write_rows(a, q["group"], n, q["ents_first"], q["ents_cap"])
    return dict(arrays=a, data=bytes(data), res_rows=res, outcomes=outcomes, n_data=pos, n_copied=n_copied,
                n_built=n_built)


def mix_of(outcomes):
    acts = [0] * 5
    for _, action in outcomes:
        acts[action] += 1
    return acts


# ---- the boundary lattice ---------------------------------------------------------------

IDS = (1, 127, 128, (1 << 14) - 1, 1 << 56, (1 << 63) - 1, 1 << 63, M64)   # varints of 1, 1, 2, 2, 9, 9, 10, 10 bytes
E3 = (entry_row(0, 0, 0, 0, 0, 1), entry_row(1, 1, 0, 0, 0, 1), entry_row(1, 2, 0, 40, 3, 0))


def lattice_specs():
    """The requests of the lattice, each with a name."""
    out = [("none", none()), ("restart_none_id", restart(id=0, ents=E3)), ("start_none_id", start(id=0)),
           ("restart_plain", restart(id=1, ents=E3, st=(1, 0, 1))),
           ("restart_split_entry", restart(id=2, ents=[entry_row(3, 9, 1, 5, 6, 2), entry_row(3, 10, 0, 7, 0, 0)],
                                           st=(3, 2, 10), delta=1000)),
           ("restart_nil_snapshot_zero_state", restart(id=3, ents=E3[:1]))]
    for n_src in (0, 1):
        out.append(("restart_n_src_%d" % n_src, restart(id=4, ents=E3[:n_src], st=(2, 4, 0), delta=1 << 40)))
    for index in (0, 1, M64):
        for commit in sorted({(index - 1) & M64, index, (index + 1) & M64, 0}):
            sn = snapshot(index, 5, nodes=(1, 2, 3), removed=(8, 9), data_off=3, data_len=4)
            out.append(("snap_index_%x_commit_%x" % (index, commit),
                        restart(id=2, ents=E3[:2], st=(5, 1, commit), snap=sn)))
    out.append(("snap_no_entries", restart(id=1, ents=(), st=(7, 0, 100), snap=snapshot(100, 7, nodes=(1, 2)))))
    out.append(("own_id_absent", restart(id=9, ents=E3, st=(1, 0, 50), snap=snapshot(50, 1, nodes=(1, 2, 3)))))
    out.append(("duplicate_nodes", restart(id=2, ents=E3, st=(1, 0, 50),
                                           snap=snapshot(50, 1, nodes=(3, 2, 3, 2, 2, 1), removed=(4, 4, 5, 4)))))
    out.append(("no_nodes", restart(id=2, ents=E3, st=(1, 0, 50), snap=snapshot(50, 1))))
    for k in (7, 8):
        out.append(("distinct_nodes_%d" % k, restart(id=3, ents=E3, st=(1, 0, 6),
                                                     snap=snapshot(6, 1, nodes=[1 + j % k for j in range(2 * k)]))))
    out.append(("nodes_64", restart(id=5, ents=E3, st=(1, 0, 6), snap=snapshot(6, 1, nodes=[1 + j % 7 for j in range(64)]))))
    out.append(("nodes_65", restart(id=5, ents=E3, st=(1, 0, 6), snap=snapshot(6, 1, nodes=[1 + j % 7 for j in range(65)]))))
    out.append(("nodes_65_index_0", restart(id=5, ents=E3, st=(1, 0, 6), snap=snapshot(0, 1, nodes=[1] * 65))))
    for k in (14, 15):
        out.append(("removed_%d" % k, restart(id=3, ents=E3, st=(1, 0, 6),
                                              snap=snapshot(6, 1, nodes=(1, 2, 3), removed=[20 + j % k for j in range(k + 3)]))))
    out.append(("removed_self", restart(id=3, ents=E3, st=(1, 0, 6), snap=snapshot(6, 1, nodes=(1, 2), removed=(3,)))))
    for id_ in IDS:
        out.append(("start_id_%x" % id_, start(id=id_, peers=[(id_, b"")])))
    for clen in (0, 1, 127, 128):
        out.append(("start_ctx_%d" % clen, start(id=1, peers=[(1, bytes(range(clen))), (2, b""), (3, b"x" * clen)])))
    out.append(("start_no_peers", start(id=1, peers=())))
    out.append(("start_9_peers", start(id=2, peers=[(j + 1, b"c%d" % j) for j in range(9)])))
    return out


def lattice_calls():
    """(name, call) pairs: every lattice request alone, then all of them in one
    call scattered over more groups than requests."""
    specs = lattice_specs()
    calls = [(name, call_of([s], G=3, groups=[k % 3], seed=k + 1, data_base=k * 1000, data_fill=k % 3))
             for k, (name, s) in enumerate(specs)]
    n = len(specs)
    G = n + n // 2 + 3
    calls.append(("all", call_of([s for _, s in specs], G=G, groups=permuted(n, G, 7), seed=99, data_base=1 << 33,
                                 data_fill=5)))
    return calls


def permuted(n, G, seed):
    """n distinct group numbers of G, in a seeded order that is not sorted."""
    r = SplitMix(seed, n)
    idx = list(range(G))
    for k in range(G - 1, 0, -1):
        j = r.rnd(k + 1)
        idx[k], idx[j] = idx[j], idx[k]
    return idx[:n]


def inval_calls():
    """(name, call) for every class the device rejects."""
    def base():
        sn = snapshot(5, 2, nodes=(1, 2, 3), removed=(4,))
        return call_of([restart(id=1, ents=E3, st=(2, 0, 5), snap=sn), start(id=2, peers=[(1, b"ab"), (2, b"")]),
                          none(), restart(id=3, ents=E3[:1])], G=6, groups=[4, 0, 2, 5])

    def edit(name, f):
        c = base()
        f(c)
        return name, c

    def word(key, row, col, val):
        def f(c):
            c[key][row, col] = np.uint64(val & M64)
        return f
    ne = base()["n_ents_total"]
    out = [edit("group_past_G", word("reqs", 1, 0, 6)), edit("group_twice", word("reqs", 3, 0, 4)),
           edit("group_twice_kind_0", word("reqs", 2, 0, 0)), edit("kind_3", word("reqs", 2, 1, 3)),
           edit("window_past_end", word("reqs", 0, 3, ne - 2)), edit("window_wraps", word("reqs", 1, 3, M64 - 1)),
           edit("window_cap_huge", word("reqs", 3, 4, M64)), edit("src_past_end", word("reqs", 0, 5, 8)),
           edit("src_wraps", word("reqs", 3, 5, M64)), edit("peers_past_end", word("reqs", 1, 6, 3)),
           edit("peers_wrap", word("reqs", 1, 5, M64)), edit("snap_past_end", word("reqs", 0, 11, 1)),
           edit("nodes_past_end", word("in_snaps", 0, 5, 99)), edit("nodes_wrap", word("in_snaps", 0, 4, M64)),
           edit("removed_past_end", word("in_snaps", 0, 6, 99)), edit("removed_wrap", word("in_snaps", 0, 7, M64)),
           edit("context_past_end", word("peers", 0, 2, 99)), edit("context_wraps", word("peers", 1, 1, M64)),
           edit("peer_pad", word("peers", 1, 3, 1))]
    out += [edit("pad_%d" % k, word("reqs", k % 4, 12 + k, 1)) for k in range(4)]
    return out


# ---- the seeded generators -------------------------------------------------------------

KIND_TABLE = (1, 1, 1, 1, 2, 2, 2, 0)
ID_TABLE = (0, 1, 2, 3, 127, 128, 1 << 56, 1 << 63)
NSRC_TABLE = (0, 1, 2, 3, 5, 9)
INDEX_TABLE = (0, 1, 5, 100, M64, 1 << 40)
NN_TABLE = (0, 1, 3, 3, 7, 12, 64, 65)
POOL_TABLE = (3, 7, 8, 20)
NR_TABLE = (0, 1, 3, 14, 15, 20)
RPOOL_TABLE = (3, 14, 15, 30)
CLEN_TABLE = (0, 1, 127, 128)


def draw_case(seed, run):
    """One random request, drawn exactly as tests/host/node_forms.cpp draws it:
    a dict with kind, id, n_src, st, has_snap, the snapshot and the peers
    (id, ctx_len)."""
    r = SplitMix(seed, run)
    kind = KIND_TABLE[r.rnd(8)]
    id_ = ID_TABLE[r.rnd(8)]
    n_src = NSRC_TABLE[r.rnd(6)]
    term, vote, cmode = r.rnd(5), r.rnd(4), r.rnd(4)
    has_snap = r.rnd(3) != 0
    index = INDEX_TABLE[r.rnd(6)]
    sterm = r.rnd(7)
    commit = (0, index - 1, index + 1, r.rnd(200))[cmode] & M64
    nn, pool = NN_TABLE[r.rnd(8)], POOL_TABLE[r.rnd(4)]
    nodes = [1 + r.rnd(pool) for _ in range(nn)]
    nr, rpool = NR_TABLE[r.rnd(6)], RPOOL_TABLE[r.rnd(4)]
    removed = [1 + r.rnd(rpool) for _ in range(nr)]
    peers = [(ID_TABLE[r.rnd(8)], CLEN_TABLE[r.rnd(4)]) for _ in range(n_src)]
    return dict(kind=kind, id=id_, n_src=n_src, st=(term, vote, commit), has_snap=has_snap,
                snap=snapshot(index, sterm, nodes, removed), peers=peers)


def spec_of(d):
    """The request spec of a drawn case; the entries and Contexts are made up from its numbers."""
    if d["kind"] == KIND_NONE:
        return none()
    if d["kind"] == KIND_START:
        return start(id=d["id"], peers=[(p, bytes([(p + j) & 0xFF for j in range(n)])) for p, n in d["peers"]])
    ents = [entry_row(1 + j // 3, j, j % 2, 10 * j, j, (0, 0, 1, 2)[j % 4]) for j in range(d["n_src"])]
    return restart(id=d["id"], ents=ents, st=d["st"], snap=d["snap"] if d["has_snap"] else None, delta=d["id"] & 0xFFFF)


def fold(h, v):
    return ((h ^ (v & M64)) * 0x100000001B3) & M64


def digest(seed, runs):
    """(digest, the actions' counts) over draw_case(seed, 0 .. runs - 1), as
    node_forms prints them: status, action and, of a built node, the 68 words
    of its five records (ents_first = the run, ents_cap = n_src + 1), whether
    the snapshot was taken, and every peer's marshalled size and head bytes."""
    h, acts = 0xCBF29CE484222325, [0] * 5
    for run in range(runs):
        d = draw_case(seed, run)
        c = call_of([spec_of(d)], G=1)
        q = _req(c, 0)
        if d["kind"] == KIND_NONE:
            status, action, n = OK, NONE, None
        else:
            status, action, n, _ = build(c, q)
        acts[action] += 1
        h = fold(fold(h, status), action)
        if n is None:
            continue
        a = {name: np.zeros((1, words), np.uint64) for name, words in RECORDS}
        a["ents"] = np.zeros((c["n_ents_total"], ENTRY_WORDS), np.uint64)
        write_rows(a, 0, n, 0, d["n_src"] + 1)
        a["groups"][0, 5] = run
        for name in ("groups", "pstate", "vstate", "rstate", "cstate"):
            for v in a[name][0]:
                h = fold(h, int(v))
        h = fold(h, int(action == RESTARTED_SNAP))
        if d["kind"] == KIND_START:
            for pid, clen in d["peers"]:
                body = K.conf_change_marshal(0, 0, pid, b"x" * clen)
                head = body[:len(body) - clen]
                h = fold(h, len(body))
                for b in head:
                    h = fold(h, b)
    return h, acts


def random_call(seed, n, G, counts=(0, 1, 2, 63, 64, 65)):
    """n random requests scattered over G groups: draw_case's requests with the
    kind-1 entry counts redrawn from `counts`, so the copy pass crosses a wave
    and a 256-thread workgroup."""
    specs = []
    for i in range(n):
        d = draw_case(seed, i)
        r = SplitMix(seed ^ 0x5EED, i)
        if d["kind"] == KIND_RESTART:
            d["n_src"] = counts[r.rnd(len(counts))]
        if r.rnd(3) and d["id"] == 0:
            d["id"] = 1 + r.rnd(3)
        specs.append(spec_of(d))
    return call_of(specs, G=G, groups=permuted(n, G, seed), seed=seed, data_base=seed << 20, data_fill=seed % 4)


# ---- the device --------------------------------------------------------------------------

ARRAY_KEYS = ("groups", "pstate", "vstate", "rstate", "cstate", "snaps", "ents")


def run_device(ctx, c, size_query=False):
    """The call c through etcd_amd.raftnode.node_batch: its output dict (a failing call raises EwalError)."""
    from etcd_amd import raftnode as RN
    return RN.node_batch(ctx, c["groups"], c["pstate"], c["vstate"], c["rstate"], c["cstate"], c["snaps"], c["ents"],
                         c["reqs"], src=c["src"], in_snaps=c["in_snaps"], u64=c["u64"], peers=c["peers"],
                         ctx_bytes=c["ctx"], data=c["data"], data_base=c["data_base"], data_cap=c["data_cap"],
                         size_query=size_query)


def assert_parity(c, got, want, emit=True):
    """Bit-exact: the five records, the snapshot rows, every window slot, d_data,
    the result rows and the counters."""
    for k in ("n_data", "n_copied", "n_built"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert np.array_equal(got["res_rows"], want["res_rows"]), \
        ("res_rows", np.argwhere(got["res_rows"] != want["res_rows"])[:4].tolist())
    for k in ARRAY_KEYS:
        w = want["arrays"][k] if emit else c[k]
        if not np.array_equal(got[k], w):
            at = np.argwhere(got[k] != w)[:4].tolist()
            raise AssertionError("%s differs at %r: got %r, want %r" % (k, at, [int(got[k][tuple(p)]) for p in at],
                                                                        [int(w[tuple(p)]) for p in at]))
    assert got["data"] == (want["data"] if emit else c["data"]), "d_data"


def check_call(ctx, c):
    """The size query, which must modify nothing, then the call; both against the restatement."""
    assert validate(c) == OK
    want = expected(c)
    assert_parity(c, run_device(ctx, c, size_query=True), want, emit=False)
    got = run_device(ctx, c)
    assert_parity(c, got, want)
    return got, want
