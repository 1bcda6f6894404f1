"""CPU tests of the batched follower step: the ABI, the restatement in
follow_cases.py against the reference's own tables and its edges, the
generator's class mix, and the host program (tests/host/follow_forms.cpp) that
runs the kernels' own step (etcd_amd/csrc/follow_step.h) over 100 000 random
runs, plain and under ASan + UBSan, and prints a digest the restatement must
reproduce.  The GPU parity suite is test_gpu_follow.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from etcd_amd import _lib as L
from etcd_amd import raftfollow as F

import follow_cases as K

M64 = K.M64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
THREE = [(1, 0, 1), (2, 0, 1), (3, 0, 1)]
RUNS = 100000


def test_abi_sizes_and_symbols():
    assert C.sizeof(L.FollowMsg) == L.lib.efollow_msg_size() == 96
    assert C.sizeof(L.FollowResult) == L.lib.efollow_result_size() == 96
    for name in ("efollow_step_batch_device", "efollow_msg_size", "efollow_result_size"):
        assert name in L.header_symbols() and hasattr(L.lib, name), name
    assert (F.MSG_IN_WORDS, F.RESULT_WORDS) == (K.IW, K.OW) == (12, 12)
    assert (L.FOLLOW_NOT_STEPPED, L.FOLLOW_IGNORED, L.FOLLOW_NO_CASE, L.FOLLOW_APPENDED, L.FOLLOW_REJECTED,
            L.FOLLOW_RESTORED, L.FOLLOW_SNAP_STALE, L.FOLLOW_DEFERRED, L.FOLLOW_PANICKED) == \
        (K.NOT_STEPPED, K.IGNORED, K.NO_CASE, K.APPENDED, K.REJECTED, K.RESTORED, K.SNAP_STALE, K.DEFERRED,
         K.PANICKED) == tuple(range(9))
    assert (L.FOLLOW_MSG_APP, L.FOLLOW_MSG_SNAP) == (K.MSG_APP, K.MSG_SNAP) == (3, 7)
    assert (L.PANIC_BOUNDS, L.PANIC_COMMITTED_CONFLICT, L.UNSUPPORTED_ENCODING) == K.STATUSES[1:]
    assert len(F.ACTIONS) == 9
    import etcd_amd
    assert etcd_amd.follow_batch is F.follow_batch and etcd_amd.follow_batch_device is F.follow_batch_device


def test_null_ctx_is_inval():
    nm, na, nr = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    assert L.lib.efollow_step_batch_device(None, None, None, None, None, 0, None, None, 0, None, 0, None, 0, None, 0,
                                           None, 0, None, None, 0, C.byref(nm), C.byref(na), C.byref(nr)) == L.E_INVAL
    assert (nm.value, na.value, nr.value) == (0, 0, 0)


def test_packers():
    rows = F.pack_msgs([dict(group=3, kind="app", from_=1, term=2, index=4, log_term=5, commit=6, ents_first=7, n_ents=8,
                             data_delta=M64), dict(group=M64, kind="snap", from_=9, snap=11)])
    m = L.FollowMsg.from_buffer_copy(rows[0].tobytes())
    assert (m.group, m.kind, m.from_, m.term, m.index, m.log_term, m.commit, m.ents_first, m.n_ents, m.data_delta,
            m.snap, m.pad) == (3, 3, 1, 2, 4, 5, 6, 7, 8, M64, 0, 0)
    m = L.FollowMsg.from_buffer_copy(rows[1].tobytes())
    assert (m.group, m.kind, m.from_, m.snap) == (M64, 7, 9, 11)
    raw = np.array([8 << 32 | 38, 1, 2, 3, 4, 5, 6, 7, 8, 9, 3 << 32 | 1, 0], dtype=np.uint64).tobytes()
    r = L.FollowResult.from_buffer_copy(raw)
    assert (r.status, r.action, r.msg_first, r.n_msgs, r.conflict, r.app_first, r.n_app, r.dst_first, r.last_index,
            r.committed, r.term, r.state, r.flags) == (38, 8, 1, 2, 3, 4, 5, 6, 7, 8, 9, 1, 3)
    assert F.results_from(raw, 1)[0] == dict(status=38, action=8, msg_first=1, n_msgs=2, conflict=3, app_first=4,
                                             n_app=5, dst_first=6, last_index=7, committed=8, term=9, state=1, flags=3)
    # leader-side emsg_out rows -> efollow_msg rows: msgApp, a msgVote that is dropped, msgSnap; ordered by group
    out = np.zeros((3, 18), dtype=np.uint64)
    out[0, :9] = [3, 2, 1, 5, 4, 9, 8, 100, 2]
    out[1, :4] = [5, 3, 1, 5]
    out[2, :4] = [7, 3, 1, 5]
    out[2, 9:17] = [20, 4, 0, 0, 6, 3, 9, 0]
    rows, snaps, order = F.msgs_from_out(out, [1, 0, 0], data_delta=16, snap_base=2)
    assert order == [2, 0] and [int(x) for x in snaps[0]] == [20, 4, 0, 0, 6, 3, 9, 0]
    assert [int(x) for x in rows[0]] == [0, 7, 1, 5, 0, 0, 0, 0, 0, 0, 2, 0]
    assert [int(x) for x in rows[1]] == [1, 3, 1, 5, 9, 4, 8, 100, 2, 16, 0, 0]


def test_restatement_passes_the_reference_tables():
    sc, named = K.kat_scenario()
    names = [n.rsplit("_", 1)[0] if n[-1].isdigit() else n for n, _, _ in named]
    assert names.count("TestHandleMsgApp") == 11 and names.count("TestAllServerStepdown") == 3
    assert {"TestStepIgnoreOldTermMsg", "TestRestore", "TestRestore_second", "TestRestoreFromSnapMsg",
            "TestCandidateConcede", "TestLogRestore"} <= set(names)
    K.check_kats(sc, named)


def _one(log, prs, add, **kw):
    """One group, the messages add(sc, g) gives it; returns (outcomes, expected dict, packed arrays)."""
    sc = K.Scenario()
    g = sc.add_group(log, prs, **kw)
    add(sc, g)
    a = sc.pack()
    assert K.validate(a) == K.OK
    x = K.expected(a)
    return x["outcomes"], x, a


def _acts(outs):
    return [(o["status"], o["action"]) for o in outs]


def test_slow_node_restore_play():
    """TestSlowNodeRestore on the restatement: node 3 is isolated while the
    leader appends and compacts (forged here on the host: a leader log cut at
    its applied index with the snapshot compact() would have taken), then gets
    the msgSnap the leader's sendAppend produces, then the next msgApp."""
    t = K.load_kats()["TestSlowNodeRestore"]
    last = t["n_props"] + 1                        # the election's entry, then n_props proposals
    snap_index, term = last, 1                     # compact at applied == committed == lastIndex
    sc = K.Scenario()
    g = sc.add_group([0], [(p, 0, 1) for p in t["peers"]], gid=t["slow"], term=1, room=4)
    sc.add_snap(g, from_=t["leader"], term=term, index=snap_index, snap_term=term, nodes=t["peers"])
    a = sc.pack()
    x = K.expected(a)
    assert _acts(x["outcomes"]) == [(0, K.RESTORED)]
    assert [int(v) for v in x["snaps"][g]] == [int(v) for v in a["in_snaps"][0]]       # follower.snap == lead.snap
    assert x["messages"][0]["index"] == snap_index and not x["messages"][0]["reject"]
    # "trigger a commit": the leader's next msgApp carries entry last + 1 and, once acknowledged, its commit
    b = dict(a, groups=x["groups"], pstate=x["pstate"], vstate=x["vstate"], rstate=x["rstate"], snaps=x["snaps"],
             ents=x["ents"], src=np.array([K.entry(term, last + 1)], dtype=np.uint64),
             msgs=np.array([[g, 3, t["leader"], term, last, term, last, 0, 1, 0, 0, 0],
                            [g, 3, t["leader"], term, last + 1, term, last + 1, 0, 0, 0, 0, 0]], dtype=np.uint64))
    y = K.expected(b)
    assert _acts(y["outcomes"]) == [(0, K.APPENDED), (0, K.APPENDED)]
    assert int(y["groups"][g][2]) == last + 1 == y["outcomes"][-1]["last_index"]  # follower.committed == lead.committed


def test_restatement_edges():
    app = lambda **kw: (lambda sc, g: sc.add_app(g, **kw))   # noqa: E731
    # a follower's msgSnap does not set lead (Go's quirk); its msgApp does
    outs, x, _ = _one([0], THREE, lambda sc, g: sc.add_snap(g, from_=2, term=1, index=5, snap_term=1, nodes=[1, 2, 3]),
                      gid=1, term=1, lead=0, elapsed=4)
    assert _acts(outs) == [(0, K.RESTORED)] and [int(v) for v in x["vstate"][0][:4]] == [0, 0, 0, 0]
    outs, x, _ = _one([0], THREE, app(from_=2, term=1), gid=1, term=1, lead=0, elapsed=4)
    assert _acts(outs) == [(0, K.APPENDED)] and [int(v) for v in x["vstate"][0][:4]] == [0, 0, 2, 0]
    # a candidate concedes to a msgApp at its own Term; to a local msgSnap at Term 0 (Go's quirk)
    outs, x, _ = _one([0], THREE, app(from_=2, term=3), gid=1, term=3, state=1, vote=1, voted=1, granted=1)
    assert _acts(outs) == [(0, K.APPENDED)] and outs[0]["flags"] == 2 and outs[0]["term"] == 3
    assert [int(v) for v in x["vstate"][0][:6]] == [0, 0, 2, 0, 0, 0]
    outs, x, _ = _one([0], THREE, lambda sc, g: sc.add_snap(g, from_=2, term=0, index=5, snap_term=1, nodes=[1, 2, 3]),
                      gid=1, term=3, state=1, vote=1, voted=1, granted=1)
    assert _acts(outs) == [(0, K.RESTORED)] and outs[0]["flags"] == 2 and outs[0]["term"] == 0
    assert x["messages"][0]["term"] == 0 and int(x["groups"][0][1]) == 0
    # a higher term switches first (flags 1), then the follower's case; a leader at an equal term has no case
    outs, x, _ = _one([0], THREE, app(from_=3, term=9), gid=1, term=3, state=2, lead=1)
    assert _acts(outs) == [(0, K.APPENDED)] and outs[0]["flags"] == 1 and int(x["vstate"][0][2]) == 3
    outs, x, a = _one([0], THREE, lambda sc, g: (sc.add_app(g, from_=3, term=3), sc.add_app(g, from_=3, term=0),
                                                  sc.add_app(g, from_=3, term=2)), gid=1, term=3, state=2, lead=1)
    assert _acts(outs) == [(0, K.NO_CASE), (0, K.NO_CASE), (0, K.IGNORED)] and x["n_msgs"] == 0
    assert all(np.array_equal(x[k], a[k]) for k in ("groups", "pstate", "vstate", "rstate", "snaps", "ents"))
    # index + n_ents wraps: lastnewi is small, the commit is clamped to it
    outs, x, _ = _one([1, 1], THREE, app(from_=2, term=1, index=M64, log_term=1, commit=M64, ents=[1, 1]), gid=1,
                      term=1, log_offset=M64 - 1, committed=M64 - 1, room=4)
    assert _acts(outs) == [(0, K.APPENDED)] and (outs[0]["conflict"], outs[0]["n_app"]) == (0, 0)
    assert outs[0]["committed"] == M64 - 1                  # min(commit, 1) does not raise it
    # nlog - 1 + log_offset wraps: every index is out of bounds, the response rejects
    outs, x, _ = _one([1, 1, 1], THREE, app(from_=2, term=1, index=M64, log_term=1), gid=1, term=1, log_offset=M64 - 1)
    assert _acts(outs) == [(0, K.REJECTED)] and outs[0]["last_index"] == 0 and x["messages"][0]["index"] == M64
    # an empty log at offset 0: lastIndex() is 2^64 - 1, at() indexes past ents
    outs, x, a = _one([], THREE, lambda sc, g: (sc.add_app(g, from_=2, term=5), sc.add_app(g, from_=2, term=5)), gid=1,
                      term=1)
    assert _acts(outs) == [(K.PANIC_BOUNDS, K.PANICKED), (0, K.NOT_STEPPED)]
    assert (outs[0]["term"], outs[0]["flags"]) == (1, 0)    # the term switch is undone too
    assert all(np.array_equal(x[k], a[k]) for k in ("groups", "pstate", "vstate", "rstate", "snaps", "ents"))
    # a conflict at or below committed
    outs, *_ = _one([0, 1, 1], THREE, app(from_=2, term=2, index=0, log_term=0, ents=[2]), gid=1, term=2, committed=1)
    assert _acts(outs) == [(K.PANIC_COMMITTED_CONFLICT, K.PANICKED)]
    # a conflict truncates: entries past the appended suffix are gone, unstable drops to ci
    outs, x, _ = _one([0, 1, 1, 1], THREE, app(from_=2, term=2, index=1, log_term=1, ents=[2], commit=9), gid=1, term=2)
    assert _acts(outs) == [(0, K.APPENDED)] and (outs[0]["conflict"], outs[0]["n_app"], outs[0]["dst_first"]) == (2, 1, 2)
    assert (int(x["groups"][0][4]), int(x["pstate"][0][1]), outs[0]["committed"]) == (3, 2, 2)
    # restore: duplicate Nodes collapse in first-occurrence order; id absent from Nodes gets no match
    snap = lambda nodes, **kw: (lambda sc, g: sc.add_snap(g, from_=2, term=1, index=7, snap_term=4, nodes=nodes, **kw))  # noqa: E731
    outs, x, _ = _one([0, 1], THREE, snap([3, 3, 1, 3, 9, 1]), gid=1, term=1)
    gw = [int(v) for v in x["groups"][0]]
    assert _acts(outs) == [(0, K.RESTORED)] and gw[6] == 3 and gw[7:14] == [3, 1, 9, 0, 0, 0, 0]
    assert gw[14:21] == [0, 7, 0, 0, 0, 0, 0] and gw[21:28] == [8, 8, 8, 0, 0, 0, 0] and gw[2:5] == [7, 7, 1]
    assert [int(v) for v in x["rstate"][0][6:8]] == [7, 1] and [int(v) for v in x["ents"][0]] == [4, 0, 0, 0, 1 << 32]
    outs, x, _ = _one([0, 1], THREE, snap([2, 3]), gid=1, term=1)
    assert [int(v) for v in x["groups"][0][14:16]] == [0, 0] and int(x["rstate"][0][7]) == 1
    outs, x, _ = _one([0, 1], THREE, snap([1, 2, 3, 1]), gid=1, term=1, pending_conf=1)
    assert int(x["rstate"][0][7]) == 0 and int(x["pstate"][0][2]) == 1    # the same peers: not dirty; pendingConf stays
    # ... unsupported: 65 nodes, 8 distinct ids, votes outstanding; n_peers 8 on the first record
    for nodes in ([1] * 65, list(range(1, 9))):
        outs, *_ = _one([0, 1], THREE, snap(nodes), gid=1, term=1)
        assert _acts(outs) == [(K.UNSUPPORTED, K.PANICKED)]
    assert _acts(_one([0, 1], THREE, snap([1] * 64 + []), gid=1, term=1)[0]) == [(0, K.RESTORED)]
    outs, *_ = _one([0, 1], THREE, snap([1, 2]), gid=1, term=1, voted=1)
    assert _acts(outs) == [(K.UNSUPPORTED, K.PANICKED)]
    outs, *_ = _one([0], THREE + [(k, 0, 1) for k in range(4, 8)], lambda sc, g: (sc.add_app(g), sc.add_app(g)), gid=1,
                    n_peers=8)
    assert _acts(outs) == [(K.UNSUPPORTED, K.PANICKED), (0, K.NOT_STEPPED)]
    # a stale snapshot answers with committed
    outs, x, _ = _one([0, 1, 1], THREE, lambda sc, g: sc.add_snap(g, from_=2, term=1, index=2, snap_term=1, nodes=[1]),
                      gid=1, term=1, committed=2)
    assert _acts(outs) == [(0, K.SNAP_STALE)] and x["messages"][0]["index"] == 2
    # the run rule: after an append, heartbeats are stepped on the grown log; entries and snapshots wait
    def run(sc, g):
        sc.add_app(g, from_=2, term=1, index=0, log_term=0, ents=[1, 1])
        sc.add_app(g, from_=2, term=1, index=2, log_term=1, commit=2)       # commit-only: sees the two new entries
        sc.add_app(g, from_=2, term=1, index=2, log_term=1, ents=[1])
        sc.add_app(g, from_=2, term=1, index=2, log_term=1, commit=2)       # the rest of the run waits too
    outs, x, _ = _one([0], THREE, run, gid=1, term=1, room=4)
    assert _acts(outs) == [(0, K.APPENDED), (0, K.APPENDED), (0, K.DEFERRED), (0, K.DEFERRED)]
    assert outs[1]["committed"] == 2 and x["n_msgs"] == 2 and x["n_appended"] == 2
    # ... an append that appends nothing does not start the waiting
    def run2(sc, g):
        sc.add_app(g, from_=2, term=1, index=0, log_term=0, ents=[1])
        sc.add_app(g, from_=2, term=1, index=1, log_term=1, ents=[1])
        sc.add_snap(g, from_=2, term=1, index=9, snap_term=1, nodes=[1])
    outs, *_ = _one([0, 1], THREE, run2, gid=1, term=1, room=4)
    assert _acts(outs) == [(0, K.APPENDED), (0, K.APPENDED), (0, K.DEFERRED)] and outs[0]["n_app"] == 0
    # a rebased data_off wraps; nil Data and Data outside d_data (data_nil 1, 2) keep their words
    ents = [K.entry(1, 1, 100, 4, 0, 0), K.entry(1, 2, 100, 4, 0, 1), K.entry(1, 3, 100, 4, 1, 2)]
    outs, x, _ = _one([0], THREE, app(from_=2, term=1, ents=ents, data_delta=M64 - 49), gid=1, term=1, room=4)
    assert [[int(v) for v in e] for e in x["ents"][1:4]] == [[1, 1, 50, 4, 0], ents[1], ents[2]]


def test_validate_classes():
    def pack(edit):
        sc = K.Scenario()
        g = sc.add_group([0, 1], THREE, gid=1, term=1, room=1)
        h = sc.add_group([0], THREE, gid=1, term=1, room=1)
        sc.add_app(g, from_=2, term=1, index=1, log_term=1, ents=[1])
        sc.add_snap(h, from_=2, term=1, index=3, snap_term=1, nodes=[1, 2])
        a = sc.pack()
        edit(a)
        return a

    def word(name, i, j, v):
        def f(a):
            a[name][i, j] = np.uint64(v)
        return f

    assert K.validate(pack(lambda a: None)) == K.OK
    inval = [word("msgs", 0, 0, 2), word("msgs", 0, 1, 4), word("msgs", 0, 11, 1), word("msgs", 0, 7, 2),
             word("msgs", 0, 8, M64), word("msgs", 1, 10, 1), word("in_snaps", 0, 5, 3), word("in_snaps", 0, 4, M64),
             word("groups", 0, 28, 1), word("groups", 0, 8, 1), word("pstate", 0, 3, 1), word("pstate", 0, 2, 2),
             word("pstate", 1, 0, 99), word("vstate", 0, 0, 3), word("vstate", 0, 4, 8), word("vstate", 0, 5, 1),
             word("vstate", 1, 7, 1), word("groups", 0, 4, 4),
             lambda a: a.update(rstate=None), lambda a: a.update(snaps=None),
             lambda a: a.update(msgs=np.concatenate([a["msgs"], a["msgs"][:1]]))]
    for k, edit in enumerate(inval):
        assert K.validate(pack(edit)) == K.E_INVAL, k
    # one entry too many for the window (the source array holds it: a canary follows every message's entries)
    assert K.validate(pack(word("msgs", 0, 8, 2))) == K.E_NOMEM

    def no_room(a):
        a["groups"][1, 4] = np.uint64(0)
        a["pstate"][1, 0] = np.uint64(0)
    assert K.validate(pack(no_room)) == K.E_NOMEM
    assert K.validate(pack(lambda a: (no_room(a), word("msgs", 0, 11, 1)(a)))) == K.E_INVAL   # INVAL wins


@pytest.fixture(scope="module")
def restated_digest():
    return K.digest(7, RUNS)


def test_generator_reaches_every_class(restated_digest):
    """The condition on the generator, from the restatement alone: a digest over
    all-IGNORED input would prove nothing."""
    _, acts, stats, records = restated_digest
    assert records > 2 * RUNS and sum(acts) == sum(stats) == records
    assert all(a >= records * 0.005 for a in acts), acts
    assert all(s >= records * 0.005 for s in stats), stats
    assert max(acts) <= records * 0.6, acts


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1"] + SAN], ids=["plain", "asan_ubsan"])
def test_follow_forms(tmp_path, flags, restated_digest):
    exe = str(tmp_path / "follow_forms")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "etcd_amd", "csrc"), "-o",
                    exe, os.path.join(ROOT, "tests", "host", "follow_forms.cpp")], check=True)
    out = subprocess.run([exe, "7", str(RUNS)], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "ok", out.stdout + out.stderr
    want, acts, stats, records = restated_digest
    assert lines[0] == "runs %d records %d" % (RUNS, records)
    assert [int(v) for _, v in re.findall(r"(\w+)=(\d+)", lines[1])] == acts
    assert [int(v) for _, v in re.findall(r"(\w+)=(\d+)", lines[2])] == stats
    assert lines[3] == "digest %d" % want
