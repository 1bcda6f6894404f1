"""CPU tests of the batched election step: the ABI, the restatement in
vote_step_cases.py against the reference's own tables and its edges, the
generators' class mixes, and the host program (tests/host/vote_step_forms.cpp)
that runs the kernels' own step (etcd_amd/csrc/vote_step.h) over 100 000 random
runs, plain and under ASan + UBSan, and prints a digest the restatement must
reproduce.  The GPU parity suite is test_gpu_vote_step.py."""
import collections
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from etcd_amd import _lib as L
from etcd_amd import raftvote as V

import vote_step_cases as K

M64 = K.M64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
THREE = [(1, 0, 3), (2, 0, 3), (3, 0, 3)]
RUNS = 100000


def test_abi_sizes_and_symbols():
    assert C.sizeof(L.VoteState) == L.lib.evote_state_size() == 64
    assert C.sizeof(L.VoteMsg) == L.lib.evote_msg_size() == 64
    assert C.sizeof(L.VoteResult) == L.lib.evote_result_size() == 48
    for name in ("evote_step_batch_device", "evote_state_size", "evote_msg_size", "evote_result_size"):
        assert name in L.header_symbols() and hasattr(L.lib, name), name
    assert (V.VSTATE_WORDS, V.MSG_IN_WORDS, V.RESULT_WORDS) == (8, 8, 6)
    assert (L.VOTE_NOT_STEPPED, L.VOTE_IGNORED, L.VOTE_GRANTED, L.VOTE_REJECTED, L.VOTE_CAMPAIGNED, L.VOTE_WON,
            L.VOTE_LOST, L.VOTE_POLLED, L.VOTE_NO_CASE, L.VOTE_PANICKED) == \
        (K.NOT_STEPPED, K.IGNORED, K.GRANTED, K.REJECTED, K.CAMPAIGNED, K.WON, K.LOST, K.POLLED, K.NO_CASE,
         K.PANICKED) == tuple(range(10))
    assert (L.VOTE_MSG_HUP, L.VOTE_MSG_VOTE, L.VOTE_MSG_VOTE_RESP) == (K.MSG_HUP, K.MSG_VOTE, K.MSG_VOTE_RESP) == (0, 5, 6)
    assert (L.PANIC_LEADER_TO_CANDIDATE, L.PANIC_NIL_ENTRY, L.PANIC_DOUBLE_CONF) == (42, 43, 44)
    assert len(V.ACTIONS) == 10 and all(L.status_string(s).startswith("panic") for s in (42, 43, 44))
    import etcd_amd
    assert etcd_amd.vote_batch is V.vote_batch and etcd_amd.vote_batch_device is V.vote_batch_device


def test_null_ctx_is_inval():
    nm, nw = C.c_uint64(7), C.c_uint64(7)
    assert L.lib.evote_step_batch_device(None, None, None, None, 0, None, None, 0, None, 0, None, None, 0,
                                         C.byref(nm), C.byref(nw)) == L.E_INVAL
    assert (nm.value, nw.value) == (0, 0)


def test_packers():
    rows = V.pack_msgs([dict(group=3, kind="hup", from_=1), dict(group=4, kind="vote", from_=2, term=5, index=6,
                                                                 log_term=7),
                        dict(group=M64, kind=6, from_=9, term=1, reject=True)])
    m = L.VoteMsg.from_buffer_copy(rows[1].tobytes())
    assert (m.group, m.kind, m.from_, m.term, m.index, m.log_term, m.reject, m.pad, m.pad2) == (4, 5, 2, 5, 6, 7, 0, 0, 0)
    m = L.VoteMsg.from_buffer_copy(rows[2].tobytes())
    assert (m.group, m.kind, m.from_, m.reject) == (M64, 6, 9, 1) and int(rows[0, 1]) == 0
    vs = V.pack_vstate([dict(state="candidate", vote=3, lead=4, elapsed=5, voted=6, granted=2), dict()])
    s = L.VoteState.from_buffer_copy(vs[0].tobytes())
    assert (s.state, s.vote, s.lead, s.elapsed, s.voted, s.granted, s.reserved[0], s.reserved[1]) == \
        (1, 3, 4, 5, 6, 2, 0, 0)
    assert V.unpack_vstate(vs)[0] == dict(state=1, vote=3, lead=4, elapsed=5, voted=6, granted=2)
    raw = np.array([5 << 32 | 44, 1, 2, 3, 4, 1 << 32 | 2], dtype=np.uint64).tobytes()
    r = L.VoteResult.from_buffer_copy(raw)
    assert (r.status, r.action, r.msg_first, r.n_msgs, r.term, r.vote, r.state, r.flags) == (44, 5, 1, 2, 3, 4, 2, 1)
    assert V.results_from(raw, 1)[0] == dict(status=44, action=5, msg_first=1, n_msgs=2, term=3, vote=4, state=2, flags=1)


def test_restatement_passes_the_reference_tables():
    sc, named = K.kat_scenario()
    names = collections.Counter(n.rsplit("_", 1)[0] if n[-1].isdigit() else n for n, _, _ in named)
    assert names == dict(TestRecvMsgVote=20, TestAllServerStepdown=3, TestStateTransition=4, TestSingleNodeCandidate=1,
                         TestRecoverPendingConfig=3)
    K.check_kats(sc, named)
    rows = K.load_kats()["TestLeaderElection"]["rows"]
    assert len(rows) == 7
    got = K.play_election(rows)[0]
    assert got == [(row["wstate"], row["wterm"]) for row in rows], got


def _one(log, prs, msgs, **kw):
    sc = K.Scenario()
    g = sc.add_group(log, prs, **kw)
    for m in msgs:
        sc.add_msg(g, **m)
    res, grows, strows, vrows, erows, rows = sc.expected()
    return sc, grows, strows, vrows, erows


def _acts(sc):
    return [(o["status"], o["action"]) for o in sc.outcomes]


def _vote(from_, term=0, index=0, log_term=0):
    return dict(kind=K.MSG_VOTE, from_=from_, term=term, index=index, log_term=log_term)


def _resp(from_, term=0, reject=False):
    return dict(kind=K.MSG_VOTE_RESP, from_=from_, term=term, reject=reject)


HUP = dict(kind=K.MSG_HUP)


def test_restatement_edges():
    # the short circuit: with Vote set to another node isUpToDate is not evaluated, an empty log cannot panic
    sc, *_ = _one([], THREE, [_vote(2, term=1)], gid=1, term=1, log_offset=5, vote=3)
    assert _acts(sc) == [(0, K.REJECTED)]
    sc, grows, strows, vrows, erows = _one([], THREE, [_vote(2, term=1), _vote(2, term=1)], gid=1, term=1, log_offset=5)
    assert _acts(sc) == [(K.PANIC_NIL_ENTRY, K.PANICKED), (0, K.NOT_STEPPED)] and sc.n_msgs == 0
    pk = sc.pack()
    assert all(np.array_equal(a, b) for a, b in zip((grows, strows, vrows, erows), (pk[0], pk[1], pk[2], pk[4])))
    # ... a higher term clears Vote first: the panic then undoes the becomeFollower too
    sc, grows, _, vrows, _ = _one([], THREE, [_vote(2, term=9)], gid=1, term=1, log_offset=5, vote=3, state=K.LEADER)
    assert _acts(sc) == [(K.PANIC_NIL_ENTRY, K.PANICKED)]
    assert (sc.outcomes[0]["term"], sc.outcomes[0]["vote"], sc.outcomes[0]["state"], sc.outcomes[0]["flags"]) == \
        (1, 3, K.LEADER, 0)
    # an empty log at offset 0: lastIndex() is 2^64 - 1, inside [offset, lastIndex()], and at() indexes past ents
    sc, *_ = _one([], THREE, [_vote(2, term=1)], gid=1, term=1)
    assert _acts(sc) == [(K.PANIC_BOUNDS, K.PANICKED)]
    # a wrapped lastIndex: three entries at offset 2^64 - 2 give lastIndex() == 0 < offset
    sc, *_ = _one([1, 1, 1], THREE, [_vote(2, term=1)], gid=1, term=1, log_offset=M64 - 1)
    assert _acts(sc) == [(K.PANIC_NIL_ENTRY, K.PANICKED)]
    # ... msgHup there: every next becomes 1, the msgVote carries index 0 and log_term 0
    sc, grows, *_ = _one([1, 1, 1], THREE, [HUP], gid=1, term=1, log_offset=M64 - 1)
    assert _acts(sc) == [(0, K.CAMPAIGNED)] and [int(x) for x in grows[0, 21:24]] == [1, 1, 1]
    assert [(m["index"], m["log_term"], m["term"]) for m in sc.messages] == [(0, 0, 2)] * 2
    # q == gr is tested before q == len(votes) - gr: n_peers 1 and 2
    sc, _, _, vrows, _ = _one([0], [(1, 0, 1)], [_resp(1, reject=True), _resp(1)], gid=1, term=1, state=K.CANDIDATE)
    assert _acts(sc) == [(0, K.LOST), (0, K.NO_CASE)]                       # 1 == 1 - 0
    sc, *_ = _one([0], [(1, 0, 1), (2, 0, 1)], [_resp(2, reject=True)], gid=1, term=1, state=K.CANDIDATE, voted=1,
                  granted=1)
    assert _acts(sc) == [(0, K.POLLED)]                                     # q 2: gr 1, rejected 1
    sc, *_ = _one([0], [(1, 0, 1), (2, 0, 1)], [_resp(2, reject=True), _resp(1)], gid=1, term=1, state=K.CANDIDATE)
    assert _acts(sc) == [(0, K.POLLED), (0, K.POLLED)]
    sc, *_ = _one([0], [(1, 0, 1), (2, 0, 1)], [_resp(2), _resp(1)], gid=1, term=1, state=K.CANDIDATE)
    assert _acts(sc) == [(0, K.POLLED), (0, K.WON)]
    sc, *_ = _one([0], [(1, 0, 1), (2, 0, 1)], [_resp(2, reject=True), _resp(1, reject=True)], gid=1, term=1,
                  state=K.CANDIDATE)
    assert _acts(sc) == [(0, K.POLLED), (0, K.LOST)]
    # a duplicate answer from the same peer does not count, whatever it says
    sc, _, _, vrows, _ = _one([0], THREE, [HUP, _resp(2, term=2, reject=True), _resp(2, term=2), _resp(3, term=2)],
                              gid=1, term=1)
    assert _acts(sc) == [(0, K.CAMPAIGNED), (0, K.POLLED), (0, K.POLLED), (0, K.WON)]
    assert sc.outcomes[-1]["n_msgs"] == 2 and [m["type"] for m in sc.messages] == [5, 5, 3, 3]
    # a higher-term msgVoteResp: becomeFollower(m.Term, m.From) -- lead = from (Go's quirk), then no case
    sc, grows, _, vrows, _ = _one([0], THREE, [_resp(3, term=7)], gid=1, term=1, state=K.CANDIDATE, voted=1, granted=1)
    assert _acts(sc) == [(0, K.NO_CASE)] and sc.outcomes[0]["flags"] == 1
    assert [int(x) for x in vrows[0, :6]] == [K.FOLLOWER, 0, 3, 0, 0, 0] and int(grows[0, 1]) == 7
    # ... and a higher-term msgVote: lead = None; the vote is granted afterwards (Vote was cleared)
    sc, _, _, vrows, _ = _one([0, 1], THREE, [_vote(2, term=7, index=1, log_term=1)], gid=1, term=1, state=K.LEADER,
                              vote=3, lead=1)
    assert _acts(sc) == [(0, K.GRANTED)] and [int(x) for x in vrows[0, :3]] == [K.FOLLOWER, 2, 0]
    assert sc.messages[0]["term"] == 7 and not sc.messages[0]["reject"]
    # msgHup after a win in the same run: leader -> candidate panics, the win stays
    sc, grows, _, vrows, erows = _one([0], [(1, 0, 1)], [HUP, HUP, HUP], gid=1, term=0)
    assert _acts(sc) == [(0, K.WON), (K.PANIC_LEADER_TO_CANDIDATE, K.PANICKED), (0, K.NOT_STEPPED)]
    assert (int(grows[0, 1]), int(grows[0, 2]), int(grows[0, 4]), int(vrows[0, 0])) == (1, 1, 2, K.LEADER)
    assert [int(x) for x in erows[1]] == [1, 1, 0, 0, 1 << 32]
    # a second win in one run: the first win's entry keeps ITS term for the next msgVote and the next campaign
    sc, grows, _, _, erows = _one([0], [(1, 0, 1)], [HUP, _vote(9, term=5, index=1, log_term=0),
                                                      _vote(9, term=6, index=0, log_term=1), HUP], gid=1, term=0,
                                  room=4)
    assert _acts(sc) == [(0, K.WON), (0, K.REJECTED), (0, K.REJECTED), (0, K.WON)]
    assert [[int(x) for x in e[:2]] for e in erows[1:3]] == [[1, 1], [7, 2]] and int(grows[0, 2]) == 2
    # id not among the peers: msgHup is unsupported (not promotable); a candidate that wins anyway has no prs[id]
    sc, *_ = _one([0], THREE, [HUP], gid=9, term=1)
    assert _acts(sc) == [(K.UNSUPPORTED, K.PANICKED)]
    sc, grows, strows, vrows, erows = _one([0], THREE, [_resp(2), _resp(3)], gid=9, term=1, state=K.CANDIDATE)
    assert _acts(sc) == [(0, K.POLLED), (K.PANIC_NIL_PROGRESS, K.PANICKED)]
    assert [int(x) for x in vrows[0, 4:6]] == [2, 2] and np.array_equal(grows, sc.pack()[0])
    # an answer from a node that is no peer: the mask cannot count it
    sc, *_ = _one([0], THREE, [_resp(8)], gid=1, term=1, state=K.CANDIDATE)
    assert _acts(sc) == [(K.UNSUPPORTED, K.PANICKED)]
    # becomeLeader's scan: committed + 1 == offset; one and two uncommitted ConfChange entries
    sc, *_ = _one([1, 1], THREE, [_resp(2)], gid=1, term=1, state=K.CANDIDATE, voted=1, granted=1, log_offset=5,
                  committed=4)
    assert _acts(sc) == [(K.PANIC_FIRST_ENTRY, K.PANICKED)]
    cc = dict(term=1, type=1)
    sc, _, strows, _, _ = _one([0, cc, 1], THREE, [_resp(2)], gid=1, term=1, state=K.CANDIDATE, voted=1, granted=1)
    assert _acts(sc) == [(0, K.WON)] and int(strows[0, 2]) == 1
    sc, _, strows, _, _ = _one([0, cc, 1], THREE, [_resp(2)], gid=1, term=1, state=K.CANDIDATE, voted=1, granted=1,
                               committed=1)
    assert _acts(sc) == [(0, K.WON)] and int(strows[0, 2]) == 0              # the ConfChange is committed: not scanned
    sc, grows, strows, vrows, erows = _one([0, cc, cc], THREE, [_resp(2)], gid=1, term=1, state=K.CANDIDATE, voted=1,
                                           granted=1, pending_conf=1)
    assert _acts(sc) == [(K.PANIC_DOUBLE_CONF, K.PANICKED)] and int(strows[0, 2]) == 1
    # the winner's broadcast panics in its second message (no snapshot for peer 3 after a wrapped reset): all as before
    sc, grows, strows, vrows, erows = _one([1, 1, 1], THREE, [_resp(2, term=1)], gid=1, term=1, state=K.CANDIDATE,
                                           voted=1, granted=1, log_offset=M64 - 1)
    assert _acts(sc) == [(K.PANIC_NEED_SNAPSHOT, K.PANICKED)] and sc.n_msgs == 0
    pk = sc.pack()
    assert all(np.array_equal(a, b) for a, b in zip((grows, strows, vrows, erows), (pk[0], pk[1], pk[2], pk[4])))
    # n_peers 8: unsupported on the first record
    sc, *_ = _one([0], THREE + [(4, 0, 1), (5, 0, 1), (6, 0, 1), (7, 0, 1)], [_vote(2), HUP], gid=1, term=1, n_peers=8)
    assert _acts(sc) == [(K.UNSUPPORTED, K.PANICKED), (0, K.NOT_STEPPED)]
    # a lower term is ignored; term 0 is local and is stepped at any Term
    sc, *_ = _one([0], THREE, [_vote(2, term=3), _vote(2, term=0), _resp(2, term=3)], gid=1, term=4, state=K.LEADER)
    assert _acts(sc) == [(0, K.IGNORED), (0, K.REJECTED), (0, K.IGNORED)]


def test_generators_reach_every_class():
    sc = K.lattice_scenario()
    sc.expected()
    assert len(sc.groups) == len(sc.msgs) == 9 * 3 * (3 + 36 + 12)
    acts = collections.Counter(o["action"] for o in sc.outcomes)
    assert all(acts[a] for a in range(1, 10)), acts
    for n in (1, 63, 64, 65, 255, 256, 257, 1025):
        b = K.boundary_scenario(n)
        assert len(b.msgs) == n
        b.expected()
        heads = [i for _, i in b.runs]
        for seam in (64, 256, 1024):
            if n > seam + 3:
                assert seam - 3 in heads and not any(seam - 3 < h <= seam + 2 for h in heads)
    sc = K.long_scenario(300)
    sc.expected()
    acts = collections.Counter(o["action"] for o in sc.outcomes)
    assert acts[K.WON] == 150 and acts[K.GRANTED] >= 50 and acts[K.REJECTED] >= 50, acts
    # every action and every status the call can give a record, at least 20 times per seed
    for seed in (1, 2):
        sc = K.random_scenario(seed)
        sc.expected()
        acts = collections.Counter(o["action"] for o in sc.outcomes)
        stats = collections.Counter(o["status"] for o in sc.outcomes)
        assert all(acts[a] >= 20 for a in range(10)), acts
        assert set(stats) == set(K.STATUSES) and all(stats[s] >= 20 for s in K.STATUSES), stats
        assert sum(m["type"] == K.MSG_SNAP for m in sc.messages) >= 20


@pytest.fixture(scope="module")
def restated_digest():
    return K.digest(7, RUNS)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1"] + SAN], ids=["plain", "asan_ubsan"])
def test_vote_step_forms(tmp_path, flags, restated_digest):
    exe = str(tmp_path / "vote_step_forms")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "etcd_amd", "csrc"), "-o",
                    exe, os.path.join(ROOT, "tests", "host", "vote_step_forms.cpp")], check=True)
    out = subprocess.run([exe, "7", str(RUNS)], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "ok", out.stdout + out.stderr
    assert re.match(r"runs %d records \d+$" % RUNS, lines[0])
    classes = [int(v) for _, v in re.findall(r"(\w+)=(\d+)", lines[1])]
    want, counts = restated_digest
    assert classes == counts and all(c >= 1000 for c in classes), (classes, counts)
    assert lines[2] == "digest %d" % want
