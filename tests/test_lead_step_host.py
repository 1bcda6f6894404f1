"""The host side of the batched leader msgAppResp step (no GPU): the ABI's
struct sizes and symbols, the three new panic classes, the restatement of
stepLeader's msgAppResp case against the reference's own tables and at its
edges, the packers' round trips, the random generator's class mix, and the
argument check that needs no device."""
import collections
import ctypes as C

import numpy as np

from etcd_amd import _lib as L
from etcd_amd import raftlead as R

import lead_step_cases as K

M64 = K.M64


def test_abi_sizes_and_symbols():
    assert C.sizeof(L.LeadGroup) == L.lib.elead_group_size() == 256
    assert C.sizeof(L.LeadSnap) == L.lib.elead_snap_size() == 64
    assert C.sizeof(L.LeadResp) == L.lib.elead_resp_size() == 48
    assert C.sizeof(L.LeadResult) == L.lib.elead_result_size() == 48
    for name in ("elead_step_batch_device", "elead_group_size", "elead_snap_size", "elead_resp_size",
                 "elead_result_size"):
        assert name in L.header_symbols() and hasattr(L.lib, name), name
    assert (R.GROUP_WORDS, R.SNAP_WORDS, R.RESP_WORDS, R.RESULT_WORDS, R.MSG_WORDS) == \
        (32, 8, 6, 6, L.lib.emsg_out_size() // 8)
    assert (L.LEAD_NOT_STEPPED, L.LEAD_COMMITTED, L.LEAD_PANICKED) == (K.NOT_STEPPED, K.COMMITTED, K.PANICKED) == \
        (0, 6, 7)
    assert len(R.ACTIONS) == 8 and R.ACTIONS[K.PROBE] == "probe"


def test_new_status_strings():
    assert (L.PANIC_NIL_PROGRESS, L.PANIC_NEED_SNAPSHOT, L.PANIC_FIRST_ENTRY) == \
        (K.PANIC_NIL_PROGRESS, K.PANIC_NEED_SNAPSHOT, K.PANIC_FIRST_ENTRY) == (39, 40, 41)
    strs = [L.status_string(s) for s in (37, 38, 39, 40, 41, 48)]
    assert all(strs) and len(set(strs)) == 6
    assert "snapshot" in strs[3] and "first entry" in strs[4]
    try:
        L.check(40)
    except L.GoPanic as e:
        assert e.status == 40
    else:
        raise AssertionError("check(40) did not raise GoPanic")


def _run(g, m):
    sc = K.Scenario()
    sc.add_resp(sc.add_group(**g), **m)
    sc.expected()
    return sc.outcomes[0], sc.messages, sc


def test_restatement_passes_the_reference_tables():
    kats = K.kat_cases()
    assert [name for name, *_ in kats] == ["leader_app_resp"] * 3 + ["commit"] * 14 + ["provide_snap"]
    for name, g, m, want in kats:
        o, msgs, _ = _run(g, m)
        K.check_kat(name, want, o, msgs)
    # TestLeaderAppResp in full: stale, probe, accept + broadcast
    acts = [_run(g, m)[0]["action"] for name, g, m, _ in kats if name == "leader_app_resp"]
    assert acts == [K.STALE, K.PROBE, K.COMMITTED]
    o, msgs, _ = _run(*kats[2][1:3])
    assert [(x["to"], x["type"], x["index"], x["log_term"], x["commit"], x["ents"]) for x in msgs] == \
        [(2, 3, 2, 1, 2, (3, 1)), (3, 3, 2, 1, 2, (3, 1))] and (o["match"], o["next"]) == (2, 3)
    o, msgs, _ = _run(*kats[1][1:3])
    assert (msgs[0]["log_term"], msgs[0]["ents"], msgs[0]["from_"], msgs[0]["term"]) == (0, (2, 2), 1, 1)
    # TestProvideSnap: the snapshot travels, nothing else does
    o, msgs, sc = _run(*kats[17][1:3])
    assert o["action"] == K.PROBE and (o["match"], o["next"]) == (0, 10000)
    row = K.msg_row(msgs[0], 0)
    assert row[:9] == [7, 2, 1, 1, 0, 9999, 0, 0, 0] and row[9:17] == [10001, 10001, 0, 0, 0, 2, 0, 0]


def _grp(terms=(0, 1, 1), prs=((1, 2, 3), (2, 0, 3), (3, 0, 3)), **kw):
    return dict(dict(terms=list(terms), prs=[list(p) for p in prs], gid=1, term=1, committed=0, log_offset=0), **kw)


def test_restatement_edges():
    # update(2^64 - 1): next wraps to 0; the commit's broadcast then asks for entries(0) at offset 0
    o, msgs, sc = _run(_grp(), dict(from_=2, index=M64))
    assert (o["status"], o["action"], o["n_msgs"], msgs) == (K.PANIC_FIRST_ENTRY, K.PANICKED, 0, [])
    assert (o["match"], o["next"], o["committed"]) == (0, 3, 0)
    assert np.array_equal(sc.expected()[1], sc.pack()[0])            # the record is as it was
    pr = K.Progress(0, 0)
    pr.update(M64)
    assert (pr.match, pr.next) == (M64, 0)
    # ... while with one peer more the quorum index is old and nothing is sent: the update stands
    o, msgs, _ = _run(_grp(prs=((1, 2, 3), (2, 0, 3), (3, 0, 3), (4, 0, 3))), dict(from_=2, index=M64))
    assert (o["status"], o["action"], o["match"], o["next"]) == (K.OK, K.UPDATED, M64, 0)
    # maybeDecrTo's floor: next 1 -> 0 -> 1
    pr = K.Progress(0, 1)
    assert pr.maybe_decr_to(0) and pr.next == 1
    o, msgs, _ = _run(_grp(prs=((1, 2, 3), (2, 0, 1))), dict(from_=2, index=0, reject=True))
    assert (o["action"], o["next"]) == (K.PROBE, 1) and (msgs[0]["index"], msgs[0]["ents"]) == (0, (1, 2))
    # next 0: next - 1 wraps, the decrement does too and is not below 1
    pr = K.Progress(0, 0)
    assert pr.maybe_decr_to(M64) and pr.next == M64
    # an unknown from, on both branches
    for rej in (False, True):
        o, msgs, _ = _run(_grp(), dict(from_=9, index=2, reject=rej))
        assert (o["status"], o["action"], o["match"], o["next"], msgs) == (K.PANIC_NIL_PROGRESS, K.PANICKED, 0, 0, [])
    # needSnapshot with snapshot term 0, and with none
    low = _grp(terms=(3, 3), prs=((1, 11, 12), (2, 0, 10)), log_offset=10, committed=10)
    for snap in (None, dict(index=10, term=0)):
        o, msgs, _ = _run(dict(low, snap=snap), dict(from_=2, index=9, reject=True))
        assert (o["status"], o["action"], o["next"], msgs) == (K.PANIC_NEED_SNAPSHOT, K.PANICKED, 10, [])
    o, msgs, _ = _run(dict(low, snap=dict(index=10, term=3)), dict(from_=2, index=9, reject=True))
    assert (o["status"], o["action"], o["next"], msgs[0]["type"]) == (K.OK, K.PROBE, 9, 7)
    # a response from the leader's own id: its progress is updated like any other, the broadcast skips it
    o, msgs, _ = _run(_grp(prs=((1, 0, 1), (2, 2, 3), (3, 0, 3))), dict(from_=1, index=2))
    assert (o["action"], o["committed"], [m["to"] for m in msgs]) == (K.COMMITTED, 2, [2, 3])
    # even and odd quorum: 2 of 3, 3 of 4
    o, _, _ = _run(_grp(), dict(from_=2, index=2))
    assert (o["action"], o["committed"]) == (K.COMMITTED, 2)
    four = ((1, 2, 3), (2, 0, 3), (3, 0, 3), (4, 0, 3))
    o, _, _ = _run(_grp(prs=four), dict(from_=2, index=2))
    assert (o["action"], o["committed"]) == (K.UPDATED, 0)
    o, _, _ = _run(_grp(prs=((1, 2, 3), (2, 0, 3), (3, 2, 3), (4, 0, 3))), dict(from_=2, index=2))
    assert (o["action"], o["committed"]) == (K.COMMITTED, 2)
    # commit blocked by an old-term entry (TestCommit rows 2 and 6)
    for row in (1, 5):
        name, g, m, want = K.kat_cases()[3 + row]
        o, msgs, _ = _run(g, m)
        assert want["w"] == 0 and (o["action"], o["committed"], msgs) == (K.UPDATED, 0, [])
    # the term switch
    o, _, _ = _run(_grp(term=3), dict(from_=2, index=2, term=2))
    assert o["action"] == K.IGNORED
    sc = K.Scenario()
    g = sc.add_group(**_grp(term=3, terms=(0, 2, 3)))   # the quorum index 1 has an older term
    for t in (0, 4, 3):
        sc.add_resp(g, 2, 1, term=t)
    sc.expected()
    assert [o["action"] for o in sc.outcomes] == [K.UPDATED, K.STEP_DOWN, K.NOT_STEPPED]
    assert [(o["match"], o["next"]) for o in sc.outcomes] == [(1, 2)] * 3
    # an empty log at offset 0: lastIndex wraps, Go indexes past ents
    o, _, _ = _run(_grp(terms=()), dict(from_=2, index=2))
    assert (o["status"], o["action"]) == (K.PANIC_BOUNDS, K.PANICKED)
    # more than seven peers: reported, never guessed
    o, _, _ = _run(_grp(n_peers=8), dict(from_=2, index=2))
    assert (o["status"], o["action"], o["match"], o["next"]) == (K.UNSUPPORTED, K.PANICKED, 0, 0)


def test_packer_round_trips():
    groups = [dict(id=7, term=3, committed=4, log_offset=2, prs=[(7, 9, 10), (8, 0, 5), (M64, 1 << 63, 6)]),
              dict(id=1, term=1, prs=[])]
    rows, ents = R.pack_groups(groups, [[1, 2, 3], [5]])
    assert rows.shape == (2, 32) and rows.dtype == np.uint64 and rows.nbytes == 2 * L.lib.elead_group_size()
    g = L.LeadGroup.from_buffer_copy(rows[0].tobytes())
    assert (g.id, g.term, g.committed, g.log_offset, g.nlog, g.ents_first, g.n_peers) == (7, 3, 4, 2, 3, 0, 3)
    assert list(g.peer_id)[:3] == [7, 8, M64] and list(g.match)[:3] == [9, 0, 1 << 63] and list(g.next)[:3] == [10, 5, 6]
    assert list(g.reserved) == [0] * 4 and list(g.peer_id)[3:] == [0] * 4
    g = L.LeadGroup.from_buffer_copy(rows[1].tobytes())
    assert (g.nlog, g.ents_first, g.n_peers) == (1, 3, 0)
    back = R.unpack_groups(rows)
    assert back[0]["prs"] == groups[0]["prs"] and back[0]["log_offset"] == 2 and back[1]["prs"] == []
    e = L.EntryDesc.from_buffer_copy(ents[2].tobytes())
    assert (e.term, e.index, e.data_len, e.type, e.data_nil) == (3, 4, 0, 0, 1)
    s = L.LeadSnap.from_buffer_copy(R.pack_snaps([None, dict(index=5, term=6, n_nodes=2, removed_off=3)])[1].tobytes())
    assert (s.index, s.term, s.data_off, s.n_nodes, s.removed_off, s.n_removed) == (5, 6, 0, 2, 3, 0)
    r = L.LeadResp.from_buffer_copy(R.pack_resps([dict(group=1, from_=8, term=3, index=M64, reject=True)])[0].tobytes())
    assert (r.group, r.from_, r.term, r.index, r.reject, r.pad, r.pad2) == (1, 8, 3, M64, 1, 0, 0)
    res = L.LeadResult(status=40, action=7, msg_first=3, n_msgs=0, committed=9, match=1, next=2)
    assert R.results_from(bytes(res), 1) == [dict(status=40, action=7, msg_first=3, n_msgs=0, committed=9, match=1,
                                                  next=2)]
    m = L.OutMsg(type=7, to=2, from_=1, term=4, index=9, snap_index=10, snap_term=3, snap_n_nodes=2, reject=0)
    d = R.messages_from(bytes(m), 1)[0]
    assert (d["type"], d["to"], d["from_"], d["term"], d["index"], d["n_ents"], d["reject"]) == (7, 2, 1, 4, 9, 0, False)
    assert d["snap"] == dict(index=10, term=3, data_off=0, data_len=0, nodes_off=0, n_nodes=2, removed_off=0,
                             n_removed=0)


def test_lattice_and_boundary_builders():
    sc = K.lattice_scenario()
    assert len(sc.groups) == 7 * 9 * 5 * 3
    sc.expected()
    runs = collections.Counter(collections.Counter(r["group"] for r in sc.resps).values())
    assert set(runs) == set(range(1, 9))
    acts = collections.Counter(o["action"] for o in sc.outcomes)
    assert all(acts[a] >= 30 for a in range(8)), acts
    stats = collections.Counter(o["status"] for o in sc.outcomes)
    assert stats[K.PANIC_NIL_PROGRESS] and stats[K.PANIC_NEED_SNAPSHOT] and stats[K.PANIC_FIRST_ENTRY], stats
    assert sum(1 for m in sc.messages if m["type"] == K.MSG_SNAP) >= 30
    for n in (64, 257, 1025):
        sc = K.boundary_scenario(n)
        assert len(sc.resps) == n
        for b in (64, 256, 1024):
            if b + 3 <= n:
                assert len({r["group"] for r in sc.resps[b - 3:b + 3]}) == 1
                assert sc.resps[b - 4]["group"] != sc.resps[b - 3]["group"] != sc.resps[b + 3 if b + 3 < n else 0]["group"]


def test_random_generator_class_mix():
    for seed in (1, 2):
        sc = K.random_scenario(seed)
        sc.expected()
        n = len(sc.resps)
        assert 6000 <= n < 6008 and len(sc.groups) == 4096
        acts = collections.Counter(o["action"] for o in sc.outcomes)
        for a in (K.IGNORED, K.STALE, K.PROBE, K.UPDATED, K.COMMITTED):
            assert acts[a] >= 0.05 * n, (seed, acts)
        assert acts[K.STEP_DOWN] and acts[K.NOT_STEPPED]
        assert any(m["type"] == K.MSG_SNAP for m in sc.messages)
        assert any(o["status"] != K.OK for o in sc.outcomes)
        runs = collections.Counter(collections.Counter(r["group"] for r in sc.resps).values())
        assert all(runs[k] for k in range(1, 7)), runs
        order = [r["group"] for r in sc.resps]
        heads = [g for i, g in enumerate(order) if i == 0 or order[i - 1] != g]
        assert len(heads) == len(set(heads)) and heads != sorted(heads)   # adjacent runs, in no particular order


def test_null_ctx_is_inval():
    nm, nc = C.c_uint64(7), C.c_uint64(7)
    assert L.lib.elead_step_batch_device(None, None, 0, None, None, 0, None, 0, None, None, 0, C.byref(nm),
                                         C.byref(nc)) == L.E_INVAL
    assert (nm.value, nc.value) == (0, 0)
