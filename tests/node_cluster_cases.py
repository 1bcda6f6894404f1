"""StartNode and RestartNode end to end: 3 nodes x 22 clusters (66 groups, more
than one wave).

1. Every group is started by enode_batch_device's kind 2; the result must
   equal, word for word, what conf_cluster_cases' ConfCluster.__init__ writes by
   hand (records, windows, ConfChange bytes; canary groups and slots untouched).
2. The groups play Ready -> scan -> apply, a timed election, two proposals and
   their commit with the existing calls (ConfCluster's interval).
3. Each node's Ready records become its own WAL (the oracle's encoder; on the
   device ewal_save_device, which must write the same bytes).
4. "Crash": all 66 WALs are replayed (the oracle's ReadAll; on the device
   ewal_readall_batch_device over the concatenated WALs).
5. The requests come from enode_reqs_from_batch and the restart is kind 1 from
   ewal_batch_entries_device's array: no entry is copied to the host for the
   call.  data_delta = the shard's place, so the WAL buffer itself is d_data
   from here on.
6. Every rebuilt record equals the model's RestartNode(id, 10, 1, nil, st,
   ents); one Ready reports exactly the committed entries 1..commit with no
   HardState and nothing to save; scan -> apply gives every node its three peers
   back; ticks elect a leader per cluster at a term above the pre-crash one.

`host` is RestatedHost (the CPU run: node_cases' restatement and the oracle) or
test_gpu_node_cluster.py's DeviceHost, which makes the real calls and compares
them with the restatement bit for bit."""
import numpy as np

import cluster_cases as C
import conf_cluster_cases as CC
import node_cases as N
import raft_model as M

NODES, CLUSTERS = 3, 22
ARRAYS5 = ("groups", "pstate", "vstate", "rstate", "snaps", "ents")


class NodeCluster(CC.ConfCluster):
    """ConfCluster at 22 clusters that keeps every Ready's save records per group."""

    def __init__(self, checks, backend, wire=None):
        CC.CLUSTERS, keep = CLUSTERS, CC.CLUSTERS
        try:
            super().__init__(checks, backend, wire)
        finally:
            CC.CLUSTERS = keep

    def ready_scan_apply(self):
        res, saves = self.call("ready", sel=np.array(self.real, dtype=np.uint64))
        self.calls.append(("ready", len(self.real)))
        for g, r in zip(self.real, res):
            assert int(r[0]) & 0xFFFFFFFF == C.OK
            if int(r[9]):
                self.saves.setdefault(g, []).append(saves[int(r[8]):int(r[8]) + int(r[9])].copy())
        c = dict(ready=res, ents=self.a["ents"], data=bytes(self.data), sel=self.real, G=self.G, n=len(self.real))
        x = self.checks.check_scan(c)
        assert not any(x["statuses"])
        self.apply(x["req_rows"])
        return res, x

    def leading_now(self):
        return [[i for i in range(1, NODES + 1) if self.state(self.group(c, i)) == M.LEADER] for c in range(CLUSTERS)]


def start_call(cl):
    """The kind-2 call that starts every real group of the cluster cl, on canary-filled copies of its arrays."""
    G, n = cl.G, len(cl.real)
    reqs = np.zeros((n, N.REQ_WORDS), np.uint64)
    for k, g in enumerate(cl.real):
        reqs[k, :7] = [g, N.KIND_START, cl.node_of(g), g * cl.cap, cl.cap, 0, NODES]
        reqs[k, 11] = N.NO_SNAP
    c = dict(G=G, n=n, reqs=reqs, n_ents_total=G * cl.cap, src=np.zeros((0, 5), np.uint64),
             in_snaps=np.zeros((0, 8), np.uint64), u64=np.zeros(0, np.uint64),
             peers=np.array([[k + 1, 0, 0, 0] for k in range(NODES)], dtype=np.uint64), ctx=b"", data_base=0,
             data_cap=len(cl.data), data=bytes(len(cl.data)))
    for j, (name, words) in enumerate(N.RECORDS):
        c[name] = N._canary(40 + j, (G, words))
    c["ents"] = np.full((G * cl.cap, 5), C.CANARY, dtype=np.uint64)
    return c


def check_start(cl, host):
    c = start_call(cl)
    assert N.validate(c) == N.OK
    got = host.node_call(c)
    real = np.array(cl.real)
    hand = {k: cl.a[k] for k in ("groups", "pstate", "vstate", "rstate", "snaps")}
    hand["vstate"] = hand["vstate"].copy()
    hand["vstate"][real, 3] = 0                      # ConfCluster winds node 1's clock forward by hand
    hand["cstate"] = cl.cstate
    for k, w in hand.items():
        assert np.array_equal(got[k][real], w[real]), k
    idle = np.array([g for g in range(cl.G) if g not in set(cl.real)])
    for k, _ in N.RECORDS:
        assert np.array_equal(got[k][idle], c[k][idle]), k
    for g in cl.real:
        first = g * cl.cap
        assert np.array_equal(got["ents"][first:first + 1 + NODES], cl.a["ents"][first:first + 1 + NODES]), g
        assert (got["ents"][first + 1 + NODES:first + cl.cap] == C.CANARY).all()
    assert got["data"] == bytes(cl.data) and got["n_data"] == len(cl.data) and got["n_built"] == len(cl.real)


def save_rows_of(cl, g):
    return [r for part in cl.saves.get(g, []) for r in part]


def wal_of(cl, g):
    """Group g's WAL as the oracle's encoder writes it: the head (crc 0, nil metadata), then every Ready's records."""
    from oracle import oracle as O
    enc = O.WalEncoder(0)
    enc.save_crc(0)
    enc.encode(1, None)
    for r in save_rows_of(cl, g):
        w = [int(x) for x in r]
        if w[0] & 0xFFFFFFFF == C.SAVE_STATE:
            enc.save_state(w[1], w[2], w[3])
        else:
            assert w[0] & 0xFFFFFFFF == C.SAVE_ENTRY
            enc.save_entry(w[0] >> 32, w[1], w[2], None if w[6] else bytes(cl.data[w[4]:w[4] + w[5]]))
    return enc.getvalue()


def replayed(raw):
    """The oracle's ReadAll of one WAL from index 0: (st, the entries as
    ewal_entry rows with Data's place in the WAL, the entries themselves).  Data
    is the last field of an Entry and the Entry the last field of its record, so
    an entry's bytes are their last occurrence before the next frame."""
    from oracle import oracle as O
    back = O.readall(raw, 0)
    assert back["status"] == O.OK
    rows, end = [], len(raw)
    for e in reversed(back["ents"]):
        d = e["data"]
        if d:
            at = raw.rfind(d, 0, end)
            assert at > 0
            rows.append(N.entry_row(e["term"], e["index"], e["type"], at, len(d), 0))
            end = at
        else:
            rows.append(N.entry_row(e["term"], e["index"], e["type"], 0, 0, 1))
    st = back["state"]
    return (st["term"], st["vote"], st["commit"]), rows[::-1], back["ents"]


def restart_call(cl, wals, src_first=None, src=None):
    """The kind-1 call that restarts every real group from its replayed WAL, on
    copies of the cluster's arrays as the crash left them.  src_first / src: the
    ranges and the entry rows a device replay produced (default: the oracle's,
    laid end to end)."""
    G, n = cl.G, len(cl.real)
    reqs = np.zeros((n, N.REQ_WORDS), np.uint64)
    rows, off, back = [], 0, []
    for s, g in enumerate(cl.real):
        st, ents, plain = replayed(wals[s])
        first = len(rows) if src_first is None else src_first[s]
        reqs[s, :12] = np.array([g, N.KIND_RESTART, cl.node_of(g), g * cl.cap, cl.cap, first, len(ents), off,
                                 st[0], st[1], st[2], N.NO_SNAP], dtype=np.uint64)
        rows += ents
        back.append((st, ents, plain))
        off += len(wals[s])
    c = dict(G=G, n=n, reqs=reqs, n_ents_total=G * cl.cap,
             src=np.array(rows, dtype=np.uint64).reshape(-1, 5) if src is None else src,
             in_snaps=np.zeros((0, 8), np.uint64), u64=np.zeros(0, np.uint64), peers=np.zeros((0, 4), np.uint64),
             ctx=b"", data_base=0, data_cap=0, data=b"", cstate=cl.cstate.copy())
    for k in ARRAYS5:
        c[k] = cl.a[k].copy()
    return c, back


class RestatedHost:
    """The CPU run: node_cases' restatement for the call, the oracle for the WALs."""

    def node_call(self, c):
        x = N.expected(c)
        return dict(x["arrays"], data=x["data"], n_data=x["n_data"], n_built=x["n_built"], n_copied=x["n_copied"])

    def wals(self, cl):
        return [wal_of(cl, g) for g in cl.real]

    def restart(self, cl, wals):
        c, back = restart_call(cl, wals)
        assert N.validate(c) == N.OK
        return self.node_call(c), back


def play(cl, host):
    """The scenario on the cluster cl; every step is asserted."""
    real = cl.real
    check_start(cl, host)
    # Ready -> scan -> apply, the election, two proposals and their commit
    res, x = cl.ready_scan_apply()
    assert x["n_reqs"] == NODES * len(real)
    for _ in range(10):
        cl.interval()
        if all(ld == [1] for ld in cl.leading_now()):
            break
    assert all(ld == [1] for ld in cl.leading_now())
    for _ in range(3):
        cl.interval()
    for body in (b"foo", b"barbaz"):
        cl.interval([cl.propose(cl.group(c, 1), body + b"%d" % c) for c in range(CLUSTERS)])
    last = NODES + 3                                 # three ConfChanges, the leader's empty entry, two proposals
    for _ in range(10):
        cl.interval()
        if all(int(cl.a["groups"][g, 2]) == last and int(cl.a["rstate"][g, 2]) == last for g in real):
            break
    assert all(int(cl.a["groups"][g, 2]) == last and int(cl.a["rstate"][g, 2]) == last for g in real)
    term_before = {g: int(cl.a["groups"][g, 1]) for g in real}
    # the WALs, the crash, the replay, the restart
    wals = host.wals(cl)
    blob = b"".join(wals)
    got, back = host.restart(cl, wals)
    offs = np.cumsum([0] + [len(w) for w in wals[:-1]]).tolist()
    zero = {name: np.zeros((1, words), np.uint64) for name, words in N.RECORDS}
    for s, g in enumerate(real):
        st, _, plain = back[s]
        assert st == (term_before[g], int(cl.a["vstate"][g, 1]), last) and len(plain) == 1 + last
        assert [e["index"] for e in plain] == list(range(1 + last))
        # the model's RestartNode(id, 10, 1, nil, st, ents), on the entries as the oracle read them
        ents = [M.Entry(Term=e["term"], Index=e["index"], Type=e["type"], Data=e["data"] or None) for e in plain]
        n = N.RestartNode(cl.node_of(g), None, dict(Term=st[0], Vote=st[1], Commit=st[2]), ents)
        a = {k: v.copy() for k, v in zero.items()}
        a["ents"] = np.zeros((cl.cap, 5), np.uint64)
        N.write_rows(a, 0, n, 0, cl.cap)
        a["groups"][0, 5] = g * cl.cap
        for k, _ in N.RECORDS:
            assert np.array_equal(got[k][g], a[k][0]), (k, g)
        first = g * cl.cap
        for k, e in enumerate(plain):
            w = [int(v) for v in got["ents"][first + k]]
            assert w[:2] == [e["term"], e["index"]] and w[4] & 0xFFFFFFFF == e["type"]
            d = b"" if w[4] >> 32 else blob[w[2]:w[2] + w[3]]          # Data's place means the WAL buffer itself
            assert d == (e["data"] or b""), (g, k)
            assert w[4] >> 32 or offs[s] <= w[2] < offs[s] + len(wals[s])
    assert got["n_built"] == len(real) and got["n_copied"] == len(real) * (1 + last) and got["n_data"] == 0
    for k in ARRAYS5:
        cl.a[k] = got[k]
    cl.cstate = got["cstate"]
    cl.data = bytearray(blob)
    cl.flight = []
    cl.queue = {k: {} for k in cl.queue}
    # one Ready: the committed entries 1 .. commit, no HardState, nothing to save (TestNodeRestart's shape)
    res, x = cl.ready_scan_apply()
    for g, r in zip(real, res):
        w = [int(v) for v in r]
        assert w[0] >> 32 == C.R_UPDATES and w[1:4] == [0, 0, 0] and w[4:6] == [0, 0] and w[9] == 0
        assert w[6:8] == [g * cl.cap + 1, last]
    assert x["n_reqs"] == NODES * len(real)
    assert all([int(v) for v in cl.a["groups"][g, 6:10]] == [3, 1, 2, 3] for g in real)
    res, _ = cl.ready_scan_apply()
    assert all(int(r[7]) == 0 and int(r[9]) == 0 for r in res)
    # time alone elects a leader per cluster, at a term above the pre-crash one
    for _ in range(80):
        cl.interval()
        if all(len(ld) == 1 for ld in cl.leading_now()):
            break
    for c, ld in enumerate(cl.leading_now()):
        assert len(ld) == 1, (c, ld)
        g = cl.group(c, ld[0])
        assert int(cl.a["groups"][g, 1]) > term_before[g]
    return cl
