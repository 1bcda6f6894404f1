"""raft_model against the reference's tables and against both restatement
families: the one model steps the random scenarios of every step call and must
leave, word for word, what each call's own restatement leaves."""
import numpy as np
import pytest

import cluster_cases as C
import follow_cases as FC
import lead_prop_cases as PC
import lead_step_cases as LC
import raft_model as M
import vote_step_cases as VC


def same(name, got, want):
    got, want = np.asarray(got, dtype=np.uint64), np.asarray(want, dtype=np.uint64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d words differ, first at %s: model %d, restatement %d" % (
        name, len(bad), tuple(bad[0]), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


# ---- the follower family -------------------------------------------------------------------------

def check_follow(a):
    assert FC.validate(a) == FC.OK
    want, got = FC.expected(a), C.follow_call(a)
    for k in ("res_rows", "msg_rows", "groups", "pstate", "vstate", "rstate", "snaps", "ents"):
        same("follow " + k, got[k], want[k])
    assert (got["n_msgs"], got["n_appended"], got["n_restored"]) == \
        (want["n_msgs"], want["n_appended"], want["n_restored"])
    return want


@pytest.mark.parametrize("seed,same_array,delta", [(1, False, 0), (2, True, 0), (3, False, 1000)])
def test_model_steps_the_follower_call(seed, same_array, delta):
    sc = FC.random_scenario(seed, 1500, same_array=same_array, idle_every=7, data_delta=delta)
    want = check_follow(sc.pack())
    acts = {o["action"] for o in want["outcomes"]}
    assert acts == set(range(9))          # every action, DEFERRED and PANICKED included
    assert {o["status"] for o in want["outcomes"]} == set(FC.STATUSES)
    assert len(want["outcomes"]) > 3000


def test_model_gives_the_follower_tables():
    for idle in (0, 2):
        sc, named = FC.kat_scenario(idle)
        a = sc.pack()
        got = C.follow_call(a)
        # check_kats reads the tables' wanted values out of whatever stands in for expected(): the model's arrays
        outs = []
        for i, row in enumerate(got["res_rows"]):
            w = [int(x) for x in row]
            outs.append(dict(status=w[0] & 0xFFFFFFFF, action=w[0] >> 32, last_index=w[7], committed=w[8], term=w[9],
                             state=w[10] & 0xFFFFFFFF, group=int(a["msgs"][i][0])))
        msgs = []
        for i, row in enumerate(got["res_rows"]):
            for mrow in got["msg_rows"][int(row[1]):int(row[1]) + int(row[2])]:
                msgs.append(dict(type=int(mrow[0]), reject=bool(mrow[17]), group=int(a["msgs"][i][0])))
        FC.check_kats(sc, named, a, dict(got, outcomes=outs, messages=msgs))


# ---- the tables' wanted values read from the model's rows ----------------------------------------------

class ModelView:
    """What a leader-family check_kats reads of a scenario -- expected(),
    outcomes, messages, runs, msgs -- filled from the model's output alone, so
    the reference's recorded values are compared with the model, not with the
    restatement.  records: the scenario's input dicts; extra(w): the
    call-specific result words as outcome keys."""

    def __init__(self, sc, records, got, arrays, extra):
        self.msgs, self._arrays = records, arrays
        self.outcomes, self.messages, self.runs = [], [], []
        for i, (x, row) in enumerate(zip(records, got["res_rows"])):
            w = [int(v) for v in row]
            if i == 0 or records[i - 1]["group"] != x["group"]:
                self.runs.append((x["group"], i))
            self.outcomes.append(dict(status=w[0] & 0xFFFFFFFF, action=w[0] >> 32, msg_first=w[1], n_msgs=w[2],
                                      **extra(w)))
            for m in got["msg_rows"][w[1]:w[1] + w[2]]:
                m = [int(v) for v in m]
                efirst = int(got["groups"][x["group"], 5])
                self.messages.append(dict(group=x["group"], type=m[0], to=m[1], from_=m[2], term=m[3], log_term=m[4],
                                          index=m[5], commit=m[6], ents=(m[7] - efirst, m[8]) if m[8] else None,
                                          reject=bool(m[17])))

    def expected(self):
        return self._arrays


# ---- the leader family: election ---------------------------------------------------------------------

def vote_arrays(sc):
    grows, strows, vrows, srows, erows, _ = sc.pack()
    return dict(groups=grows, pstate=strows, vstate=vrows, snaps=srows, ents=erows, msgs=sc.msgs)


def check_vote(sc):
    res, grows, strows, vrows, erows, rows = sc.expected()
    got = C.vote_call(vote_arrays(sc))
    for k, w in (("res_rows", res), ("msg_rows", rows), ("groups", grows), ("pstate", strows), ("vstate", vrows),
                 ("ents", erows)):
        same("vote " + k, got[k], w)


@pytest.mark.parametrize("seed", [1, 7])
def test_model_steps_the_election_call(seed):
    sc = VC.random_scenario(seed, runs=1200)
    check_vote(sc)
    assert {o["action"] for o in sc.outcomes} == set(range(10))
    assert {o["status"] for o in sc.outcomes} == set(VC.STATUSES)
    assert len(sc.outcomes) > 3000


def test_model_steps_the_election_lattice_and_tables():
    check_vote(VC.lattice_scenario())
    sc, named = VC.kat_scenario(idle=1)
    check_vote(sc)
    VC.check_kats(sc, named)
    got = C.vote_call(vote_arrays(sc))               # ... and the tables against the model's own rows
    view = ModelView(sc, sc.msgs, got, (None, got["groups"], got["pstate"], got["vstate"], None, None),
                     lambda w: dict(term=w[3], vote=w[4], state=w[5] & 0xFFFFFFFF, flags=w[5] >> 32))
    VC.check_kats(view, named)


def test_model_plays_leader_election():
    """TestLeaderElection through the model alone, over the restated router."""
    rows = VC.load_kats()["TestLeaderElection"]["rows"]

    def call(sc):
        got = C.vote_call(vote_arrays(sc))
        msgs = []
        for i, row in enumerate(got["res_rows"]):
            for m in got["msg_rows"][int(row[1]):int(row[1]) + int(row[2])]:
                w = [int(x) for x in m]
                msgs.append(dict(group=sc.msgs[i]["group"], type=w[0], to=w[1], from_=w[2], term=w[3], log_term=w[4],
                                 index=w[5], reject=bool(w[17])))
        return (got["groups"], got["pstate"], got["vstate"], got["ents"]), msgs

    heads, _, _, _ = VC.play_election(rows, call=call)
    assert heads == [(c["wstate"], c["wterm"]) for c in rows]


# ---- the leader family: msgAppResp ---------------------------------------------------------------------

def check_lead_step(sc):
    grows, srows, erows, _ = sc.pack()
    res, wgroups, rows = sc.expected()
    got = C.lead_step_call(dict(groups=grows, snaps=srows, ents=erows, resps=sc.resps))
    for k, w in (("res_rows", res), ("msg_rows", rows), ("groups", wgroups), ("ents", erows)):
        same("lead_step " + k, got[k], w)


def test_model_steps_the_leader_response_call():
    sc = LC.random_scenario(5, G=1500, n=3000)
    check_lead_step(sc)
    assert {o["action"] for o in sc.outcomes} == set(range(8))
    check_lead_step(LC.lattice_scenario())
    check_lead_step(LC.kat_scenario(idle=5))
    sc, kats = LC.kat_scenario(), LC.kat_cases()     # the 18 tables against the model's own rows: one response each
    grows, srows, erows, _ = sc.pack()
    got = C.lead_step_call(dict(groups=grows, snaps=srows, ents=erows, resps=sc.resps))
    view = ModelView(sc, sc.resps, got, None, lambda w: dict(committed=w[3], match=w[4], next=w[5]))
    assert len(kats) == len(view.outcomes) == 18
    for (name, _, _, want), o in zip(kats, view.outcomes):
        LC.check_kat(name, want, o, view.messages[o["msg_first"]:o["msg_first"] + o["n_msgs"]])


# ---- the leader family: msgProp / msgBeat --------------------------------------------------------------

def check_lead_local(sc):
    grows, strows, srows, erows, _ = sc.pack()
    res, wgroups, wstate, wents, rows = sc.expected()
    got = C.lead_local_call(dict(groups=grows, pstate=strows, snaps=srows, ents=erows, locals=sc.locals))
    for k, w in (("res_rows", res), ("msg_rows", rows), ("groups", wgroups), ("pstate", wstate), ("ents", wents)):
        same("lead_local " + k, got[k], w)


def test_model_steps_the_leader_local_call():
    sc = PC.random_scenario(3)
    check_lead_local(sc)
    assert {o["action"] for o in sc.outcomes} == set(range(5))
    sc, named = PC.kat_scenario(idle=4)
    check_lead_local(sc)
    PC.check_kats(sc, named)
    grows, strows, srows, erows, _ = sc.pack()       # ... and the tables against the model's own rows
    got = C.lead_local_call(dict(groups=grows, pstate=strows, snaps=srows, ents=erows, locals=sc.locals))
    view = ModelView(sc, sc.locals, got, (None, got["groups"], got["pstate"], None, None),
                     lambda w: dict(index=w[3], committed=w[5]))
    PC.check_kats(view, named)


# ---- the cluster: the lossy network on the restated backend ------------------------------------------------

# (nodes, clusters, seed, ticks, window); the device test plays the same runs.  The window is 2 * the run's longest
# log + 2: the follower call wants room for every entry of a message, whether or not it overlaps the log
# (EWAL_E_NOMEM where nlog + n_ents > ents_cap), and a message carries at most a whole log
LOSSY = [(3, 129, 11, 30, 28), (5, 65, 12, 30, 28), (7, 43, 13, 30, 38)]       # longest logs: 13, 13, 18


def lossy_conditions(cl):
    """The coverage a run must reach, from the tallies alone."""
    t = cl.tally
    for k in ("status_33", "status_38", "status_39", "status_40", "status_41", "status_43", "status_44", "status_48",
              "status_42"):
        assert not t.get(k), (k, t.get(k))             # no panic but the deliberate msgHup at a leader
    assert t.get("hup_at_leader")
    stepped = sum(t.get(k + "_records", 0) for k in ("vote", "follow", "lead_step", "local"))
    noops = (t.get("vote_action_%d" % C.V_IGNORED, 0) + t.get("vote_action_%d" % C.V_NOT_STEPPED, 0) +
             t.get("vote_action_%d" % C.V_NO_CASE, 0) + t.get("follow_action_%d" % C.F_IGNORED, 0) +
             t.get("follow_action_%d" % C.F_NOT_STEPPED, 0) + t.get("follow_action_%d" % C.F_DEFERRED, 0) +
             t.get("follow_action_%d" % C.F_NO_CASE, 0) + t.get("lead_step_action_%d" % C.L_IGNORED, 0) +
             t.get("lead_step_action_%d" % C.L_NOT_STEPPED, 0) + t.get("local_action_%d" % C.P_NOT_STEPPED, 0))
    assert 2 * noops <= stepped, (noops, stepped)
    for k in ("vote_action_%d" % C.V_WON, "vote_action_%d" % C.V_LOST, "vote_action_%d" % C.V_REJECTED,
              "vote_term_switch", "follow_term_switch", "follow_conceded", "lead_step_action_%d" % C.L_PROBE,
              "lead_step_action_%d" % C.L_STALE, "lead_step_action_%d" % C.L_COMMITTED,
              "follow_action_%d" % C.F_REJECTED, "follow_action_%d" % C.F_DEFERRED, "follow_restepped",
              "follow_truncated", "local_action_%d" % C.P_DROPPED, "app_resp_dropped", "proposal_forwarded",
              "run_across_64", "run_across_256", "duplicated", "delayed", "dropped", "sent_type_7",
              "follow_action_%d" % C.F_RESTORED, "follow_action_%d" % C.F_SNAP_STALE,
              "compact_action_%d" % C.K_COMPACTED, "compact_action_%d" % C.K_NOT_DUE, "compact_move_disjoint",
              "compact_move_overlap", "ready_snap", "ready_saved", "free_slots_never_written", "follow_data_delta",
              "counted_n_msgs", "counted_n_won", "counted_n_committed", "counted_n_appended", "counted_n_restored",
              "counted_n_save", "counted_n_ready", "counted_n_compacted", "counted_n_moved"):
        assert t.get(k), k
    for kind in ("vote", "follow", "lead_step"):
        sizes = [n for k, n in cl.calls if k == kind]
        assert max(sizes) > 256 and min(sizes) < 64, (kind, min(sizes), max(sizes))


def check_wal_sample(cl, ctx=None):
    """The four groups and the restored one; the restored one is read from its restore point and has entries there."""
    sample = C.wal_sample(cl)
    assert len(set(sample)) == 5 and sample[4] in cl.ri and not any(g in cl.ri for g in sample[1:3])
    read = [C.check_wal(cl, g, ctx) for g in sample]
    assert read[4][1] > 0 and read[4][2] == cl.ri[sample[4]] > 1, read
    assert any(n for _, n, _ in read[:4])
    return read


@pytest.mark.parametrize("nodes,clusters,seed,ticks,cap", LOSSY)
def test_lossy_network_restated(nodes, clusters, seed, ticks, cap):
    cl = C.play_lossy(nodes, clusters, C.RestatedBackend(), ticks, seed, cap)
    print(sorted(cl.tally.items()), cl.refused, cl.longest)
    lossy_conditions(cl)
    assert cl.longest * 2 + 2 == cap, cl.longest       # the committed window is the run's own
    print(check_wal_sample(cl))


# ---- the reference's network tests on the restated backend ----------------------------------------------------

def network_scenarios():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raft_network_kats.json")) as f:
        return json.load(f)["scenarios"]


@pytest.mark.parametrize("sc", network_scenarios(), ids=lambda sc: sc["name"])
def test_network_scenario_restated(sc):
    cl = C.play_network(sc, C.RestatedBackend(), copies=1, idle=0)    # no idle groups: Ready with d_sel == NULL
    assert cl.tally.get("ready_without_sel") == 1
    cl = C.play_network(sc, C.RestatedBackend(), copies=65)
    if sc["name"].startswith("TestProposal_") and sc.get("refused"):
        assert not cl.tally.get("local_records")         # the refused proposal never reached a call


# ---- Ready and compaction: the follower family's second file, and ready_cases ------------------------------

def ready_arrays(sc, sel=None):
    grows, srows, vrows, rrows, nrows, erows = sc.pack()
    return dict(groups=grows, pstate=srows, vstate=vrows, rstate=rrows, snaps=nrows, ents=erows, sel=sel)


def check_ready(sc, sel=None):
    res, srec, srows, rrows, n_ready = sc.expected(sel)
    got = C.ready_call(ready_arrays(sc, sel))
    for k, w in (("res_rows", res), ("save_rows", srec), ("pstate", srows), ("rstate", rrows)):
        same("ready " + k, got[k], w)
    assert got["n_ready"] == n_ready
    return got


def test_model_gives_the_ready_call():
    import ready_cases as RC
    sc = RC.random_scenario(4, groups=3000)
    check_ready(sc)
    assert {o["status"] for o in sc.outcomes} == {RC.OK, RC.PANIC_BOUNDS, RC.UNSUPPORTED}
    check_ready(sc, sel=list(range(2999, -1, -3)))
    check_ready(RC.lattice_scenario())
    sc, named, _ = RC.kat_scenario(idle=1)
    got = check_ready(sc)
    first = sc.pack()[0][:, 5]
    outcomes = {}
    for _, _, g, _ in named:                     # the tables' wanted values out of the model's rows
        w = [int(x) for x in got["res_rows"][g]]
        outcomes[g] = dict(status=w[0] & 0xFFFFFFFF, flags=w[0] >> 32, term=w[1], vote=w[2], commit=w[3],
                           ents_pos=w[4] - int(first[g]) if w[5] else 0, n_ents=w[5],
                           committed_pos=w[6] - int(first[g]) if w[7] else 0, n_committed=w[7], lead=w[10], state=w[11],
                           applied=int(got["rstate"][g, 6]), unstable=int(got["pstate"][g, 1]))
    RC.check_kats(sc, named, outcomes)


def check_compact(a):
    import compact_cases as CC
    assert CC.validate(a) == CC.OK
    want, got = CC.expected(a), C.compact_call(a)
    for k in ("res_rows", "groups", "pstate", "snaps", "ents"):
        same("compact " + k, got[k], want[k])
    assert (got["n_compacted"], got["n_moved"]) == (want["n_compacted"], want["n_moved"])
    return want


def test_model_gives_the_compaction_call():
    import compact_cases as CC
    want = check_compact(CC.random_scenario(6, 3000, 2500, idle_every=9))
    acts, stats, cls = CC.mix_of(want["outcomes"])
    assert all(acts[1:]) and all(stats) and all(cls)
    a, rounds = CC.compaction_play()              # TestCompaction, round after round on the model's own arrays
    for rnd in rounds:
        a = CC.after(a, a, [CC.req(g, index) for g, index, _ in rnd])
        got = C.compact_call(a)
        check_compact(a)
        for (g, index, wleft), r in zip(rnd, got["res_rows"]):
            if wleft < 0:
                assert int(r[0]) >> 32 == C.K_PANICKED and int(r[0]) & 0xFFFFFFFF in (45, 46)
            else:
                assert (int(r[0]), int(r[3]), int(got["groups"][g, 4])) == (C.K_COMPACTED << 32, wleft, wleft)
        a = CC.after(a, got, [])
    check_compact(CC.side_effects_call()[0])
    check_compact(CC.compact_table_call()[0])


# ---- the terms-only append: raft_append_kats.json through the model's raftLog alone ------------------------

def model_log(terms, offset, committed, unstable):
    lg = M.RaftLog()
    lg.ents = [M.Entry(Term=t, Index=offset + k) for k, t in enumerate(terms)]
    lg.offset, lg.committed, lg.unstable = offset, committed, unstable
    return lg


def test_model_gives_the_append_tables_and_the_first_restatement():
    import log_append_cases as AC
    kats = AC.kat_messages()
    assert len(kats) == 15
    for name, base, rterm, m, want in kats:
        lg = model_log(base["ents"], base["offset"], base["committed"], base["unstable"])
        ents = [M.Entry(Term=t, Index=m["index"] + 1 + k) for k, t in enumerate(m["ents"])]
        ok = lg.maybeAppend(m["index"], m["log_term"], m["commit"], ents)
        assert lg.lastIndex() == want["w_index"], name
        if "w_commit" in want:
            assert lg.committed == want["w_commit"] and (not ok) == want["w_reject"], name
        if "w_terms" in want:
            assert [e["Term"] for e in lg.ents[1:]] == want["w_terms"] and lg.unstable == want["w_unstable"], name
    # log_append_cases.RaftLog is the root of the leader family: the same random messages on both
    rng = C.SplitMix(21, 0)
    for _ in range(4000):
        off = (0, 0, 7, M.M64 - 3)[rng.rnd(4)]
        terms = sorted(1 + rng.rnd(4) for _ in range(rng.rnd(7)))
        committed, unstable = (off + rng.rnd(len(terms) + 1)) & M.M64, (off + rng.rnd(len(terms) + 2)) & M.M64
        index = (off + rng.rnd(len(terms) + 2) - (rng.rnd(8) == 0)) & M.M64
        pos = (index - off) & M.M64
        log_term = terms[pos] if pos < len(terms) and rng.rnd(4) else rng.rnd(5)
        new = sorted(1 + rng.rnd(5) for _ in range(rng.rnd(5)))
        commit = (off + rng.rnd(len(terms) + 4)) & M.M64
        a, b = AC.RaftLog(terms, off, committed, unstable), model_log(terms, off, committed, unstable)
        try:
            got = ("ok", a.maybe_append(index, log_term, commit, new))
        except AC.Panic as p:
            got = ("panic", p.status)
        try:
            want = ("ok", b.maybeAppend(index, log_term, commit,
                                        [M.Entry(Term=t, Index=index + 1 + k) for k, t in enumerate(new)]))
        except M.Panic as p:
            want = ("panic", C.STATUS[p.name])
        assert got == want
        if got[0] == "ok":
            assert (a.ents, a.committed, a.unstable) == ([e["Term"] for e in b.ents], b.committed, b.unstable)
