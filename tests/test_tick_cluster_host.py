"""Clusters driven by time alone, on the CPU: tick_cluster_cases.play_timed with
every call -- the tick included -- made by the restatements' expected() and
compared, after every call, bit for bit with raft_model's.  The only stimulus
is one tick per interval over all nodes, plus a few proposals; every msgHup and
msgBeat is a row of the tick's output.  The device test plays the same runs."""
import pytest

import tick_cases as K
import tick_cluster_cases as T

# (nodes, clusters, seed, intervals): the interval count is the one after which the model first meets
# timed_conditions on that seed -- every cluster has elected a leader from a tick's msgHup (with split votes and a
# lost election on the way), a tick's msgBeat round has reset a follower's elapsed, a tick has held (ETICK_HELD) and a
# proposal has committed
TIMED = [(3, 1, 21, 14), (3, 65, 21, 14)]


def test_model_ticks():
    """tickElection / tickHeartbeat over raft_model.Raft equal the restatement's tick() on the lattice's groups."""
    import raft_model as M
    for election, heartbeat in K.lattice_pairs():
        for g in K.lattice_groups(election, heartbeat):
            if g["n_peers"] > K.PEERS:
                continue
            r = M.Raft.__new__(M.Raft)
            r.id, r.Term, r.state, r.elapsed = g["id"], g["term"], g["state"], g["elapsed"]
            r.prs = {p: M.Progress() for p in g["peers"][:g["n_peers"]]}
            action, msg, drawn = K.tick_model(r, election, heartbeat, lambda r, e: g["draw"])
            want = K.tick(g["state"], g["elapsed"], g["id"], g["term"], g["n_peers"], g["peers"], election, heartbeat,
                          g["draw"])
            assert (K.OK, action, r.elapsed, drawn) == want, g
            assert msg == {K.HUP: "hup", K.BEAT: "beat"}.get(action)


@pytest.mark.parametrize("nodes,clusters,seed,intervals", TIMED)
def test_timed_clusters_restated(nodes, clusters, seed, intervals):
    cl = T.play_timed(nodes, clusters, T.RestatedBackend(), intervals, seed)
    print(sorted(cl.tally.items()), cl.elected, cl.refused, cl.longest)
    T.timed_conditions(cl)
    assert cl.needed == intervals, cl.needed          # no interval more than the conditions need
    assert [n for k, n in cl.calls if k == "tick"] == [nodes * clusters] * intervals
