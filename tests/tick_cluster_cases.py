"""Clusters driven by time alone: cluster_cases.py's Cluster and backends with
one more call, the batched Tick (etick_batch_device), stated over raft_model.
The only stimulus is one tick per interval over every node, plus a few
proposals: every msgHup and every msgBeat a step call gets is a row of the
tick's own output, with d_draws NULL and a committed seed, so the elections
start when the randomised timeouts say, as in the reference
(etcdserver/server.go:255), not when a test-side dice roll does."""
import numpy as np

import cluster_cases as C
import raft_model as M
import tick_cases as K

ELECTION, HEARTBEAT = 10, 1              # the server's (tests/golden/raft_tick_kats.json)
TICK_COUNTERS = ("n_hups", "n_beats")


def tick_call(a):
    """a: the cluster's arrays with sel (group numbers), election, heartbeat and
    seed.  r.tick() on the model node of every selected group, the draw
    etick_draw(seed, id, Term, elapsed).  Returns vstate after the call,
    res_rows (n, 4), hup_rows (n_hups, 8), beat_rows (n_beats, 6) and the
    counters."""
    vstate = a["vstate"].copy()
    sel = [int(g) for g in a["sel"]]
    res, hups, beats = np.zeros((len(sel), K.RESULT_WORDS), dtype=np.uint64), [], []
    for i, g in enumerate(sel):
        node = M.from_arrays(a, g)
        assert node.n_peers <= M.PEERS
        r = node.r
        action, msg, drawn = K.tick_model(r, a["election"], a["heartbeat"],
                                          lambda r, e: K.draw(a["seed"], r.id, r.Term, e))
        pos = 0
        if msg == "hup":
            pos = len(hups)
            hups.append([g, M.MSG_HUP, r.id, 0, 0, 0, 0, 0])          # pb.Message{From: r.id, Type: msgHup}
        elif msg == "beat":
            pos = len(beats)
            beats.append([g, M.MSG_BEAT, 0, 0, 0, 0])
        res[i] = [C.OK | (action << 32), r.elapsed, pos, drawn]
        vstate[g, 3] = r.elapsed
    return dict(vstate=vstate, res_rows=res, hup_rows=C._rows(hups, K.HUP_WORDS), beat_rows=C._rows(beats, K.BEAT_WORDS),
                n_hups=len(hups), n_beats=len(beats))


def _tick_args(a):
    return dict(groups=a["groups"], vstate=a["vstate"], G=len(a["groups"]), n=len(a["sel"]),
                sel=[int(g) for g in a["sel"]], draws=None, seed=a["seed"], election=a["election"],
                heartbeat=a["heartbeat"])


class ModelBackend(C.ModelBackend):
    tick = staticmethod(tick_call)


class RestatedBackend(C.RestatedBackend):
    def tick(self, a):
        b = _tick_args(a)
        assert K.validate(b) == K.OK
        x = K.expected(b)
        return dict(vstate=x["vstate"], res_rows=x["res_rows"], hup_rows=x["hups"], beat_rows=x["beats"],
                    n_hups=x["n_hups"], n_beats=x["n_beats"])


class DeviceBackend(C.DeviceBackend):
    def tick(self, a):
        """The real entry point: the peek first, which must modify nothing and
        give the call's results and counters; both outputs sized exactly."""
        from etcd_amd import rafttick as RT
        from etcd_amd.raftlead import _up
        ctx, G, n = self.ctx, len(a["groups"]), len(a["sel"])
        names = ("groups", "vstate")
        bufs = {k: _up(ctx, np.ascontiguousarray(a[k])) for k in names}
        extra = [_up(ctx, np.array(a["sel"], dtype=np.uint64)), ctx.alloc(n * 32 + 64)]
        try:
            args = (ctx, bufs["groups"], bufs["vstate"], G, extra[0], n, a["election"], a["heartbeat"], None, a["seed"],
                    extra[1])
            asked = RT.tick_batch_device(*args)
            for k in names:
                assert bufs[k].download(a[k].nbytes) == a[k].tobytes(), k
            peeked = extra[1].download(n * 32)
            nh, nb = asked
            extra += [ctx.alloc((nh + 1) * 64 + 64), ctx.alloc((nb + 1) * 48 + 64)]
            extra[2].upload(np.full((nh + 1) * 8, C.CANARY, dtype=np.uint64).tobytes())
            extra[3].upload(np.full((nb + 1) * 6, C.CANARY, dtype=np.uint64).tobytes())
            assert RT.tick_batch_device(*args, extra[2], nh, extra[3], nb) == asked
            assert extra[1].download(n * 32) == peeked
            out = {k: np.frombuffer(bufs[k].download(a[k].nbytes), dtype=np.uint64).reshape(a[k].shape).copy()
                   for k in names}
            hups = np.frombuffer(extra[2].download((nh + 1) * 64), dtype=np.uint64).reshape(nh + 1, 8)
            beats = np.frombuffer(extra[3].download((nb + 1) * 48), dtype=np.uint64).reshape(nb + 1, 6)
            assert (hups[nh] == np.uint64(C.CANARY)).all() and (beats[nb] == np.uint64(C.CANARY)).all()
            out.update(res_rows=np.frombuffer(peeked, dtype=np.uint64).reshape(n, 4).copy(), hup_rows=hups[:nh].copy(),
                       beat_rows=beats[:nb].copy(), n_hups=nh, n_beats=nb)
        finally:
            for b in list(bufs.values()) + extra:
                b.free()
        return out


class Cluster(C.Cluster):
    """cluster_cases.Cluster with the tick in front of the router: its msgHup
    rows are the election call's records, its msgBeat rows the local call's."""

    def call(self, kind, **records):
        if kind != "tick":
            return super().call(kind, **records)
        a = dict(self.a, **records)
        want = tick_call(a)
        if not isinstance(self.backend, ModelBackend):
            got = self.backend.tick(a)
            for k in TICK_COUNTERS:
                assert got[k] == want[k], (kind, k, got[k], want[k])
            for k in ("res_rows", "hup_rows", "beat_rows") + C.ARRAYS:
                w = want.get(k, self.a.get(k))
                g = got.get(k)
                if g is None:
                    g = self.a[k]                  # the backend says the call does not write it
                if not np.array_equal(g, w):
                    at = tuple(int(x) for x in np.argwhere(np.asarray(g) != np.asarray(w))[0]) \
                        if np.shape(g) == np.shape(w) else ("shape", np.shape(g), np.shape(w))
                    raise AssertionError("tick call %d: %s differs at %r" % (len(self.calls), k, at))
        self.a["vstate"] = want["vstate"]
        for k in TICK_COUNTERS:
            self.tally.add("counted_" + k, want[k])
        return want["res_rows"], want["hup_rows"], want["beat_rows"]

    def tick(self, sel, seed):
        """One interval's node.Tick() at every group of sel.  Returns the
        arrivals it makes: (the election call's, the local call's)."""
        res, hups, beats = self.call("tick", sel=np.array(sel, dtype=np.uint64), election=ELECTION, heartbeat=HEARTBEAT,
                                     seed=seed)
        self.calls.append(("tick", len(sel)))
        for r in res:
            assert int(r[0]) & 0xFFFFFFFF == C.OK
            self.tally.add("tick_action_%d" % (int(r[0]) >> 32))
        votes = [(int(h[0]), dict(m=dict(kind=int(h[1]), from_=int(h[2]), term=int(h[3]), index=int(h[4]),
                                        log_term=int(h[5]), reject=bool(int(h[6]) & 0xFFFFFFFF)))) for h in hups]
        locals_ = [(int(b[0]), dict(m=dict(kind=int(b[1])))) for b in beats]
        assert all(rec["m"]["kind"] == M.MSG_HUP for _, rec in votes) and all(rec["m"]["kind"] == M.MSG_BEAT
                                                                              for _, rec in locals_)
        return votes, locals_


def is_heartbeat(row):
    """sendHeartbeat's empty msgApp (raft.go:219-226): no index, term, commit or entries."""
    return row[0] == M.MSG_APP and not (row[4] or row[5] or row[6] or row[8])


def play_timed(nodes, clusters, backend, intervals, seed, cap=32, wire=None, propose_every=7):
    """`intervals` ticks of a reliable network with one interval of latency: per
    interval the tick over every node (in ascending order on even intervals, in
    descending order on odd ones), the delivery of everything in flight, every
    propose_every-th interval one proposal per cluster (at a rotating node: the
    router forwards it to the leader the node knows, or refuses it), one call of
    each kind in the order election, follower, msgAppResp, local, then Ready
    over every node, then the safety check.  The nodes' clocks do not start
    together: cluster c's node id begins at elapsed (5 c + 3 id) % election --
    the draw is a function of (seed, id, term, elapsed), so clusters that began
    alike would stay alike.  Returns the cluster; cl.elected has the interval
    in which each cluster first had a leader, cl.needed the number of intervals
    after which timed_conditions first held (None: never)."""
    cl = Cluster(nodes, clusters, backend, cap=cap, seed=seed, wire=wire)
    for c in range(clusters):
        for id_ in range(1, nodes + 1):
            cl.a["vstate"][cl.group(c, id_), 3] = (5 * c + 3 * id_) % ELECTION
    first = {k: v.copy() for k, v in cl.a.items()}
    real = list(range(cl.base, cl.G - cl.idle))
    cl.elected, cl.needed = {}, None
    for t in range(intervals):
        arrivals = {"vote": [], "follow": [], "lead_step": [], "local": []}
        arrivals["vote"], arrivals["local"] = cl.tick(real if t % 2 == 0 else real[::-1], seed)
        cl.tally.add("hups_from_tick", len(arrivals["vote"]))
        cl.tally.add("beats_from_tick", len(arrivals["local"]))
        flight, cl.flight = cl.flight, []
        for kind, g, rec in cl.receive(flight):
            arrivals[kind].append((g, rec))
        if t % propose_every == propose_every - 1:
            for c in range(clusters):
                p = cl.propose(cl.group(c, 1 + (t + c) % nodes), bytes([t % 256, c % 256]))
                if p:
                    arrivals["local"].append(p)
                    cl.tally.add("proposed")
        cl.vote(arrivals["vote"])
        # a follower whose clock a heartbeat of this interval must stop
        waiting = [g for g, rec in arrivals["follow"] if is_heartbeat(rec["row"]) and cl.state(g) == M.FOLLOWER and
                   int(cl.a["vstate"][g, 3]) > 0 and int(cl.a["groups"][g, 1]) == rec["row"][3]]
        cl.follow(arrivals["follow"])
        cl.tally.add("heartbeat_reset_elapsed", sum(1 for g in waiting if int(cl.a["vstate"][g, 3]) == 0))
        cl.lead_step(arrivals["lead_step"])
        cl.local(arrivals["local"])
        cl.ready(real)
        cl.touched = set()
        cl.check_safety()
        for c in range(clusters):
            if c not in cl.elected and any(cl.state(cl.group(c, i)) == M.LEADER for i in range(1, nodes + 1)):
                cl.elected[c] = t
        if cl.needed is None:
            try:
                timed_conditions(cl)
                cl.needed = t + 1
            except AssertionError:
                pass
    cl.check_idle(first)
    return cl


def timed_conditions(cl):
    """The coverage a run must reach, from the tallies alone."""
    t = cl.tally
    assert len(cl.elected) == cl.clusters, sorted(set(range(cl.clusters)) - set(cl.elected))
    # every election message chain began at a tick: the election call never got a msgHup from anywhere else
    assert t.get("hups_from_tick") and t.get("counted_n_hups") == t["hups_from_tick"]
    assert t.get("beats_from_tick") and t.get("counted_n_beats") == t["beats_from_tick"]
    assert t.get("vote_action_%d" % C.V_WON, 0) >= cl.clusters
    assert 0 < t.get("local_action_%d" % C.P_BEAT, 0) <= t["beats_from_tick"]
    assert t.get("heartbeat_reset_elapsed") and t.get("tick_action_%d" % K.HELD)
    for k in (K.IDLE, K.HUP, K.BEAT):
        assert t.get("tick_action_%d" % k), k
    assert not t.get("tick_action_%d" % K.PANICKED) and not t.get("tick_action_%d" % K.NOT_PROMOTABLE)
    for k in ("status_33", "status_38", "status_39", "status_40", "status_41", "status_42", "status_43", "status_44",
              "status_48"):
        assert not t.get(k), (k, t.get(k))
    assert t.get("proposed") and t.get("counted_n_committed") and t.get("ready_saved")
