"""Membership end to end: 3 nodes x 64 groups that start as StartNode leaves
them (raft/node.go:128-146: no peers, three committed ConfChangeAddNode
entries) and reach their first election, a removal and the removed node's
denial with no per-group host work.  Only existing calls plus the three
membership calls are used; every existing call is compared with raft_model by
cluster_cases' Cluster, every membership call goes through the `checks` the
cluster is given: conf_cases' restatement alone (RestatedChecks, the CPU run),
or the device compared with it bit for bit (test_gpu_conf_cluster.py).

Even clusters cut node 3 off when its removal is proposed: it never learns of
it, campaigns, and its msgVote is denied at the gate of nodes 1 and 2; the
msgDenied, as kind 3 at node 3, is ECONF_STOPPED with soft_dirty.  In odd
clusters node 3 applies its own removal from its log and its tick turns
ETICK_NOT_PROMOTABLE."""
import numpy as np

from etcd_amd import raftlead as RL
from etcd_amd import raftvote as RV

import cluster_cases as C
import conf_cases as K
import raft_model as M
import tick_cases as TK
import tick_cluster_cases as T

NODES, CLUSTERS, SEED = 3, 64, 5
R_SOFT = 1


class RestatedChecks:
    """The three membership calls by the restatement alone."""

    @staticmethod
    def check_batch(a, reqs):
        assert K.validate_batch(a, reqs) == K.OK
        return K.expected_batch(a, reqs)

    @staticmethod
    def check_scan(c):
        assert K.validate_scan(c) == K.OK
        return K.expected_scan(c)

    @staticmethod
    def check_gate(a, recs, from_word):
        assert K.validate_gate(a["groups"], a["cstate"], recs, recs.shape[1] * 8, from_word) == K.OK
        return K.expected_gate(a["groups"], a["cstate"], recs, from_word)

NODES, CLUSTERS, SEED = 3, 64, 5
R_SOFT = 1


class ConfCluster(T.Cluster):
    def __init__(self, checks, backend, wire=None):
        super().__init__(NODES, CLUSTERS, backend, cap=32, seed=SEED, wire=wire)
        self.checks = checks
        self.real = list(range(self.base, self.G - self.idle))
        self.cstate = np.zeros((self.G, 16), np.uint64)
        a = self.a
        for g in self.real:
            id_ = self.node_of(g)
            first = g * self.cap
            a["groups"][g, :7] = [id_, 0, NODES, 0, 1 + NODES, first, 0]       # committed = len(ents), no peers
            a["groups"][g, 7:28] = 0
            a["pstate"][g] = [self.cap, 0, 0, 0]                               # raftLog.append(0, ents): unstable 0
            for k in range(NODES):
                body = K.conf_change_marshal(0, 0, k + 1)
                a["ents"][first + 1 + k] = [1, k + 1, len(self.data), len(body), 1]
                self.data += body
            # Go's first Ready has no HardState: r.Commit is copied at the first Step.  The caller seeds hs_commit.
            a["rstate"][g] = [0, 0, NODES, 0, 0, 0, 0, 0]
            a["vstate"][g, 3] = 18 if id_ == 1 else 0                          # node 1's clock runs out first

    def node_of(self, g):
        return (g - self.base) % self.nodes + 1

    def apply(self, reqs):
        """econf_batch_device against the restatement; the arrays move on."""
        reqs = reqs if isinstance(reqs, np.ndarray) else K.reqs_of(list(reqs))
        if not len(reqs):
            return None
        arrays = dict(groups=self.a["groups"], pstate=self.a["pstate"], vstate=self.a["vstate"],
                      rstate=self.a["rstate"], cstate=self.cstate, snaps=None, u64=np.zeros(0, np.uint64))
        x = self.checks.check_batch(arrays, reqs)
        for k in ("groups", "pstate", "vstate", "rstate"):
            self.a[k] = x["arrays"][k]
        self.cstate = x["arrays"]["cstate"]
        for _, action in x["outcomes"]:
            self.tally.add("conf_action_%d" % action)
        return x

    def ready_scan_apply(self):
        """Ready over every node, the scan of its committed entries, their requests applied."""
        res, _ = self.call("ready", sel=np.array(self.real, dtype=np.uint64))
        self.calls.append(("ready", len(self.real)))
        c = dict(ready=res, ents=self.a["ents"], data=bytes(self.data), sel=self.real, G=self.G, n=len(self.real))
        x = self.checks.check_scan(c)
        assert not any(x["statuses"])
        self.tally.add("scanned", x["n_entries"])
        self.apply(x["req_rows"])
        return res, x

    def gate(self, arrivals, pack=RV.pack_msgs, from_word=2):
        """removed[m.From] in front of a step call (the election call's evote_msg, or the msgAppResp call's
        elead_resp with from_word 1): (the arrivals that pass, kind-3 requests for the msgDenied's receivers)."""
        if not arrivals:
            return [], []
        recs = pack([dict(rec["m"], group=g) for g, rec in arrivals])
        x = self.checks.check_gate(dict(groups=self.a["groups"], cstate=self.cstate), recs, from_word)
        passed = [ar for ar, act in zip(arrivals, x["actions"]) if act == K.G_PASS]
        denied = []
        for (g, _), act, r in zip(arrivals, x["actions"], x["res_rows"]):
            if act == K.G_DENIED:
                m = [int(v) for v in x["msg_rows"][int(r[2])]]
                assert m[0] == M.MSG_DENIED and m[2] == self.node_of(g) and m[3] == int(self.a["groups"][g, 1])
                denied.append((self.group(self.cluster_of(g), m[1]), K.DENIED, m[2]))
        self.tally.add("gate_denied", len(denied))
        self.tally.add("gate_passed", len(passed))
        return passed, sorted(denied)

    def interval(self, proposals=(), cut=False):
        """One interval: tick, delivery (even clusters' node 3 unreachable when cut), the gate, one call of each
        kind, Ready -> scan -> apply.  Returns (Ready's rows, the kind-3 requests the gate's msgDenied make)."""
        arrivals = {"vote": [], "follow": [], "lead_step": [], "local": []}
        arrivals["vote"], arrivals["local"] = self.tick(self.real, SEED)
        flight, self.flight = self.flight, []
        if cut:
            flight = [f for f in flight if not (self.node_of(f["to"]) == 3 and self.cluster_of(f["to"]) % 2 == 0)]
        for kind, g, rec in self.receive(flight):
            arrivals[kind].append((g, rec))
        arrivals["local"] += list(proposals)
        votes, denied = self.gate(arrivals["vote"])
        resps, late = self.gate(arrivals["lead_step"], RL.pack_resps, 1)
        self.apply(late)                                 # an answer of the removed node: its msgDenied changes nothing
        self.vote(votes)
        self.follow(arrivals["follow"])
        self.lead_step(resps)
        self.local(arrivals["local"])
        res, _ = self.ready_scan_apply()
        return res, denied

    def leading(self):
        return [[i for i in range(1, NODES + 1) if self.state(self.group(c, i)) == M.LEADER] for c in range(CLUSTERS)]

    def removed(self, g):
        return [int(v) for v in self.cstate[g, 1:1 + int(self.cstate[g, 0])]]


def play(cl):
    """The scenario on the cluster cl; every step is asserted."""
    t = cl.tally
    # Ready -> scan -> apply: three peers everywhere, in the log's order
    res, x = cl.ready_scan_apply()
    assert x["n_reqs"] == 3 * len(cl.real) and all(int(r[7]) == 3 for r in res)
    assert all([int(v) for v in cl.a["groups"][g, 6:10]] == [3, 1, 2, 3] for g in cl.real)
    assert all(int(cl.a["groups"][g, 21 + k]) == 4 for g in cl.real for k in range(3))
    assert t["conf_action_%d" % K.ADDED] == 3 * len(cl.real)
    # tick until the msgHup, and the election: node 1 leads every cluster
    for _ in range(8):
        cl.interval()
        if all(ld == [1] for ld in cl.leading()):
            break
    assert all(ld == [1] for ld in cl.leading())
    assert t["counted_n_hups"] >= CLUSTERS and t["vote_action_%d" % C.V_WON] == CLUSTERS
    for _ in range(3):                                   # the leader's empty entry commits everywhere
        cl.interval()
    # ConfChangeRemoveNode(3) twice: pending_conf, the second is dropped
    body = K.conf_change_marshal(77, 1, 3)
    props = []
    for c in range(CLUSTERS):
        props += [cl.propose(cl.group(c, 1), body, etype=1), cl.propose(cl.group(c, 1), body, etype=1)]
    cl.interval(props, cut=True)
    assert t["local_action_%d" % C.P_APPENDED] == CLUSTERS and t["local_action_%d" % C.P_DROPPED] == CLUSTERS
    assert all(int(cl.a["pstate"][cl.group(c, 1), 2]) == 1 for c in range(CLUSTERS))
    # replicate, commit, Ready, scan, apply
    for _ in range(8):
        cl.interval(cut=True)
        if all(int(cl.a["groups"][cl.group(c, i), 6]) == 2 for c in range(CLUSTERS) for i in (1, 2)):
            break
    for c in range(CLUSTERS):
        for i in (1, 2):
            g = cl.group(c, i)
            assert [int(v) for v in cl.a["groups"][g, 6:10]] == [2, 1, 2, 0] and cl.removed(g) == [3]
        assert int(cl.a["pstate"][cl.group(c, 1), 2]) == 0
        g3 = cl.group(c, 3)
        if c % 2 == 0:                                   # cut off: it has not heard
            assert int(cl.a["groups"][g3, 6]) == 3 and cl.removed(g3) == []
    # a later membership proposal is accepted
    body9 = K.conf_change_marshal(78, 1, 9)
    cl.interval([cl.propose(cl.group(c, 1), body9, etype=1) for c in range(CLUSTERS)], cut=True)
    assert t["local_action_%d" % C.P_APPENDED] == 2 * CLUSTERS and t["local_action_%d" % C.P_DROPPED] == CLUSTERS
    # odd clusters: node 3 has applied its own removal and is not promotable
    for _ in range(3):
        cl.interval(cut=True)
    for c in range(1, CLUSTERS, 2):
        g3 = cl.group(c, 3)
        assert [int(v) for v in cl.a["groups"][g3, 6:10]] == [2, 1, 2, 0] and cl.removed(g3) == [3]
    assert t["tick_action_%d" % TK.NOT_PROMOTABLE] >= CLUSTERS // 2
    # even clusters: node 3 campaigns, its msgVote is denied at nodes 1 and 2, and the msgDenied stops it
    stopped, soft_due = set(), set()
    for _ in range(30):
        res, denied = cl.interval(cut=True)
        for g in soft_due:                               # the Ready after the msgDenied reports the SoftState
            assert int(res[cl.real.index(g), 0]) >> 32 & R_SOFT
        soft_due = set()
        if denied:
            assert all(cl.node_of(g) == 3 and cl.cluster_of(g) % 2 == 0 and node in (1, 2) for g, _, node in denied)
            fresh = {g for g, _, _ in denied} - stopped
            x = cl.apply(denied)
            assert all(o == (K.OK, K.STOPPED) for o in x["outcomes"])
            for g in fresh:
                assert cl.removed(g) == [3] and int(cl.a["rstate"][g, 7]) == 1
            stopped |= fresh
            soft_due = fresh
        if len(stopped) == CLUSTERS // 2 and not soft_due:
            break
    assert len(stopped) == CLUSTERS // 2 and t["gate_denied"] >= CLUSTERS and t["gate_passed"] > 0
    # a hand-made msgVote of the removed node at every live node: one msgDenied each; kind 3 at a node that has
    # already removed itself changes nothing
    arrivals = [(cl.group(c, i), dict(m=dict(kind=M.MSG_VOTE, from_=3, term=99, index=0, log_term=0, reject=False)))
                for c in range(CLUSTERS) for i in (1, 2)]
    passed, denied = cl.gate(arrivals)
    assert not passed and len(denied) == 2 * CLUSTERS
    x = cl.apply([d for d in denied if cl.cluster_of(d[0]) % 2 == 1])
    assert all(o == (K.OK, K.STOPPED) for o in x["outcomes"])
    assert all(int(cl.a["rstate"][cl.group(c, 3), 7]) == 0 for c in range(1, CLUSTERS, 2))
    # the removal handed to a cut-off node 3 that campaigns: r.votes keeps its own key, which the masks cannot
    x = cl.apply([(cl.group(c, 3), K.REMOVE, 3) for c in range(0, CLUSTERS, 2)])
    assert all(o == (K.UNSUPPORTED, K.PANICKED) for o in x["outcomes"])
    for k in ("status_33", "status_39", "status_40", "status_41", "status_44", "status_48"):
        assert not t.get(k), (k, t.get(k))
