"""The host side of the batched follower append (no GPU): the ABI's struct
sizes and symbols, the new panic class, the restatement of
raftLog.maybeAppend against the reference's own tables, the packer's round
trip, the random generator's class mix, and the argument check that needs no
device."""
import collections
import ctypes as C

import numpy as np

from etcd_amd import _lib as L
from etcd_amd import raftlog as R

import log_append_cases as K


def test_abi_sizes_and_symbols():
    assert C.sizeof(L.LogGroup) == L.lib.elog_group_size() == 64
    assert C.sizeof(L.LogApp) == L.lib.elog_app_size() == 64
    assert C.sizeof(L.LogAppResult) == L.lib.elog_app_result_size() == 48
    for name in ("elog_append_batch_device", "elog_group_size", "elog_app_size", "elog_app_result_size"):
        assert name in L.header_symbols() and hasattr(L.lib, name), name
    assert 0 < R.LANE_MAX == L.lib.elog_lane_max_entries()
    assert (R.GROUP_WORDS, R.APP_WORDS, R.RESULT_WORDS, R.RESP_WORDS) == (8, 8, 6, L.lib.emsg_out_size() // 8)


def test_committed_conflict_status():
    assert L.PANIC_COMMITTED_CONFLICT == K.PANIC_COMMITTED_CONFLICT == 38 and L.PANIC_BOUNDS == K.PANIC_BOUNDS
    s38, s37 = L.status_string(38), L.status_string(37)
    assert s38 and s38 != s37 and "committed" in s38


def test_restatement_passes_the_reference_tables():
    kats = K.kat_messages()
    assert [name for name, *_ in kats] == ["handle_msg_app"] * 11 + ["append"] * 4
    for _, base, rterm, m, want in kats:
        log = K.RaftLog(**base)
        res, resp = K.handle_append_entries(log, 1, rterm, 9, m["index"], m["log_term"], m["commit"], m["ents"])
        assert res["status"] == K.OK and (resp["type"], resp["to"], resp["from_"], resp["term"]) == (4, 9, 1, rterm)
        K.check_kat(want, log, res, resp)


def test_restatement_edges():
    # from wraps to 0 on a log that ends at 2^64 - 1: ci == 0 is "no conflict"
    log = K.RaftLog([3, 3], offset=K.M64 - 1, committed=K.M64 - 1, unstable=0)
    res, resp = K.handle_append_entries(log, 1, 3, 2, K.M64, 3, K.M64, [9, 9])
    assert (res["accepted"], res["conflict"], res["n_app"], log.ents) == (1, 0, 0, [3, 3])
    assert res["committed"] == K.M64 - 1 and resp["index"] == K.M64   # min(commit, lastnewi = 1) < committed
    # a heartbeat index = log_term = 0 on a compacted log: the reference rejects
    log = K.RaftLog([4, 4], offset=10)
    res, resp = K.handle_append_entries(log, 1, 4, 2, 0, 0, 11, [])
    assert res["accepted"] == 0 and resp["reject"] and resp["index"] == 0
    # an empty ents slice at offset 0: lastIndex wraps, Go indexes past ents
    res, resp = K.handle_append_entries(K.RaftLog([]), 1, 4, 2, 0, 0, 0, [])
    assert res["status"] == K.PANIC_BOUNDS and resp is None and res["last_index"] == K.M64
    # a conflict at or below committed
    log = K.RaftLog([1, 1, 1, 1], committed=2, unstable=4)
    res, resp = K.handle_append_entries(log, 1, 4, 2, 1, 1, 0, [2])
    assert res["status"] == K.PANIC_COMMITTED_CONFLICT and resp is None and log.ents == [1, 1, 1, 1]
    assert (res["last_index"], res["committed"], res["conflict"], res["n_app"]) == (3, 2, 0, 0)


def test_packer_round_trip():
    logs = [[1, 1, 2], [], [5], list(range(1, 30))]
    ids, term, comm, unst, off = [7, 8, 9, K.M64], [2, 3, 4, 5], [1, 0, 1 << 63, 20], [3, 0, 4, 29], [0, 5, 1 << 63, 100]
    rows, terms = R.pack_groups(ids, term, comm, unst, off, logs, capacity=1.5, room=2, fill=K.CANARY)
    assert rows.shape == (4, 8) and rows.dtype == np.uint64 and rows.nbytes == 4 * L.lib.elog_group_size()
    caps = [int(r[7]) for r in rows]
    assert caps == [5, 2, 3, 44] and len(terms) == sum(caps)
    assert [int(r[6]) for r in rows] == [0, 5, 7, 10]
    back = R.unpack_groups(rows, terms)
    assert [g["terms"] for g in back] == logs
    assert [(g["id"], g["term"], g["committed"], g["unstable"], g["log_offset"]) for g in back] == \
        list(zip(ids, term, comm, unst, off))
    owned = sum(len(t) for t in logs)
    assert int((terms == np.uint64(K.CANARY)).sum()) == len(terms) - owned
    first = L.LogGroup.from_buffer_copy(rows[3].tobytes())
    assert (first.id, first.log_offset, first.nlog, first.terms_off, first.terms_cap) == (K.M64, 100, 29, 10, 44)
    arows, erows = R.pack_apps([dict(group=3, from_=1, index=128, log_term=29, commit=5, ents=[30, 31]),
                                dict(group=0, from_=2, index=2, log_term=2, ents_at=(0, 2))])
    a = L.LogApp.from_buffer_copy(arows[0].tobytes())
    assert (a.group, a.from_, a.index, a.log_term, a.commit, a.ents_first, a.n_ents) == (3, 1, 128, 29, 5, 0, 2)
    assert [int(x) for x in arows[1]][5:7] == [0, 2]
    e = L.EntryDesc.from_buffer_copy(erows[1].tobytes())
    assert (e.term, e.index, e.data_len, e.type, e.data_nil) == (31, 130, 0, 0, 1)


def test_lattice_brackets_the_threshold():
    ls = K.lattice_lengths(R.LANE_MAX)
    assert ls[0] < R.LANE_MAX < ls[-1] and {R.LANE_MAX, R.LANE_MAX + 1} <= set(ls) and set(K.LENGTHS) <= set(ls)


def test_random_generator_class_mix():
    for seed in (1, 2):
        sc = K.random_scenario(seed)
        sc.expected()
        assert len(sc.apps) == 3000 and len(sc.groups) == 4096
        mix = collections.Counter(K.classify(o) for o in sc.outcomes)
        accept = sum(o["accepted"] for o in sc.outcomes)
        for cls in ("reject", "noop", "extension", "conflict"):
            assert mix[cls] >= 0.05 * 3000, (seed, mix)
        assert accept >= 0.05 * 3000 and mix["panic"] > 0
        assert sum(1 for a in sc.apps if len(a["ents"]) > R.LANE_MAX) >= 30


def test_null_ctx_is_inval():
    acc, app = C.c_uint64(7), C.c_uint64(7)
    assert L.lib.elog_append_batch_device(None, None, 0, None, 0, None, 0, None, 0, None, None, C.byref(acc),
                                          C.byref(app)) == L.E_INVAL
    assert (acc.value, app.value) == (0, 0)
