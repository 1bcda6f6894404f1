"""CPU tests of the batched log compaction: the ABI, the restatement in
compact_cases.py against the reference's own tables and its edges, the
generator's mix, and the host program (tests/host/compact_forms.cpp) that runs
the kernels' own decision (etcd_amd/csrc/compact_step.h) and a model of the
three-class move over 100 000 random requests, plain and under ASan + UBSan,
and prints a digest the restatement must reproduce.  The GPU parity suite is
test_gpu_compact.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from etcd_amd import _lib as L
from etcd_amd import raftcompact as RC

import compact_cases as K
import follow_cases as FK

M64 = FK.M64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
RUNS = 100000


def test_abi_sizes_and_symbols():
    assert C.sizeof(L.CompactReq) == L.lib.ecompact_req_size() == 96
    assert C.sizeof(L.CompactResult) == L.lib.ecompact_result_size() == 64
    for name in ("ecompact_batch_device", "ecompact_req_size", "ecompact_result_size"):
        assert name in L.header_symbols() and hasattr(L.lib, name), name
    assert (RC.REQ_WORDS, RC.RESULT_WORDS) == (K.QW, K.OW) == (12, 8)
    assert (L.COMPACT_NOT_STEPPED, L.COMPACT_NOT_DUE, L.COMPACT_COMPACTED, L.COMPACT_PANICKED) == \
        (K.NOT_STEPPED, K.NOT_DUE, K.COMPACTED, K.PANICKED) == tuple(range(4))
    assert (L.COMPACT_AT_APPLIED, L.COMPACT_PEEK, RC.AT_APPLIED, RC.PEEK) == (K.AT_APPLIED, 1, 1, 1)
    assert (L.PANIC_BOUNDS, L.PANIC_COMPACT_APPLIED, L.PANIC_COMPACT_BOUNDS, L.UNSUPPORTED_ENCODING) == \
        K.STATUSES[1:] == (33, 45, 46, 48)
    s45, s46 = L.status_string(45), L.status_string(46)
    assert s45.startswith("panic") and "applied" in s45 and s46.startswith("panic") and "bounds" in s46
    for st in (45, 46):
        with pytest.raises(L.GoPanic):
            L.check(st)
    hdr = open(L.HEADER).read()
    assert "EWAL_PANIC_COMPACT_APPLIED = 45" in hdr and "EWAL_PANIC_COMPACT_BOUNDS = 46" in hdr
    assert len(RC.ACTIONS) == 4
    import etcd_amd
    assert etcd_amd.compact_batch is RC.compact_batch and etcd_amd.compact_batch_device is RC.compact_batch_device


def test_null_ctx_is_inval():
    nc, nm = C.c_uint64(7), C.c_uint64(7)
    assert L.lib.ecompact_batch_device(None, None, None, None, 0, None, None, 0, 0, 0, None, 0, None, 0, C.byref(nc),
                                       C.byref(nm)) == L.E_INVAL
    assert (nc.value, nm.value) == (0, 0)


def test_packers():
    rows = RC.pack_reqs([dict(group=3, index=9, threshold=5, data_off=1, data_len=2, nodes_off=3, n_nodes=4,
                              removed_off=5, n_removed=6), dict(group=M64, at_applied=True, threshold=M64)])
    q = L.CompactReq.from_buffer_copy(rows[0].tobytes())
    assert (q.group, q.flags, q.index, q.threshold, q.data_off, q.data_len, q.nodes_off, q.n_nodes, q.removed_off,
            q.n_removed, q.pad[0], q.pad[1]) == (3, 0, 9, 5, 1, 2, 3, 4, 5, 6, 0, 0)
    q = L.CompactReq.from_buffer_copy(rows[1].tobytes())
    assert (q.group, q.flags, q.index, q.threshold) == (M64, 1, 0, M64)
    assert [int(v) for v in rows[0]] == K.req(3, 9, threshold=5, data=(1, 2), nodes=(3, 4), removed=(5, 6))
    raw = np.array([3 << 32 | 46, 1, 2, 3, 4, 5, 6, 7], dtype=np.uint64).tobytes()
    r = L.CompactResult.from_buffer_copy(raw)
    assert (r.status, r.action, r.index, r.term, r.n_left, r.shift, r.src_first, r.dst_first, r.unstable) == \
        (46, 3, 1, 2, 3, 4, 5, 6, 7)
    assert RC.results_from(raw, 1)[0] == dict(status=46, action=3, index=1, term=2, n_left=3, shift=4, src_first=5,
                                              dst_first=6, unstable=7)
    snaps = np.array([[0] * 8, [100, 1, 16, 9, 2, 3, 5, 1]], dtype=np.uint64)
    recs = RC.snap_save_recs(snaps, [1])
    r = recs[0]
    assert (r.index, r.term, r.data_off, r.data_len, r.nodes_off, r.n_nodes, r.removed_off, r.n_removed, r.unrec_off,
            r.unrec_len) == (100, 1, 16, 9, 2, 3, 5, 1, 0, 0)
    assert len(RC.snap_save_recs(snaps)) == 2


def test_restatement_passes_the_reference_tables():
    assert K.check_tables()
    k = K.load_kats()
    # TestNodeCompact and TestProvideSnap, as far as the compaction goes: a leader's log [dummy, nop, "foo"], all
    # applied, compacted at 2 under the table's snapshot; then log_offset == snapshot.Index with a non-zero Term is
    # exactly the state in which sendAppend to a peer at next == offset ships a msgSnap (raft/raft.go:202-217, 556-564)
    w = k["TestNodeCompact"]["snapshot"]
    sc = FK.Scenario()
    sc.add_group([0, 1, 1], [(1, 2, 3)], committed=2, applied=2, state=FK.LEADER)
    data = w["data"].encode()
    a = K.call_of(sc, [K.req(0, w["index"], data=(0, len(data)), nodes=(0, len(w["nodes"])),
                             removed=(1, len(w["removed"])))], len(data), 1)
    x = K.expected(a)
    assert [int(v) for v in x["snaps"][0]] == [w["index"], w["term"], 0, len(data), 0, 1, 1, 0]
    assert int(x["groups"][0][3]) == k["TestNodeCompact"]["woffset"] and int(x["groups"][0][4]) == 1
    assert np.array_equal(x["rstate"], a["rstate"])          # snapi is Ready's to move
    s = k["TestProvideSnap"]["snapshot"]
    sc = FK.Scenario()
    sc.add_group([s["term"]] * 3, [(1, s["index"] + 2, s["index"] + 3), (2, 0, s["index"])], term=s["term"],
                 log_offset=s["index"] - 1, committed=s["index"] + 1, applied=s["index"] + 1, state=FK.LEADER)
    x = K.expected(K.call_of(sc, [K.req(0, s["index"], nodes=(0, 2))], 0, 2))
    assert [int(v) for v in x["snaps"][0][:2]] == [s["index"], s["term"]] and int(x["groups"][0][3]) == s["index"]


def _one(log, q, **grp):
    sc = FK.Scenario()
    sc.add_group(log, [(1, 0, 1)], **grp)
    a = K.call_of(sc, [q], 100, 10)
    assert K.validate(a) == K.OK
    x = K.expected(a)
    return a, x, x["outcomes"][0]


def test_restatement_edges():
    # shift 0: nothing moves, the snapshot is replaced
    a, x, o = _one([3, 3, 4], K.req(0, 10, data=(1, 2)), log_offset=10, committed=12, applied=12)
    assert (o["action"], o["shift"], o["n_left"], o["cls"], o["term"]) == (K.COMPACTED, 0, 3, K.MOVE_NONE, 3)
    assert np.array_equal(x["ents"], a["ents"]) and [int(v) for v in x["snaps"][0][:4]] == [10, 3, 1, 2]
    assert x["n_moved"] == 0 and x["n_compacted"] == 1
    # index == applied == lastIndex: one entry is left, at the window's base
    a, x, o = _one([3, 3, 4], K.req(0, 12), log_offset=10, committed=12, applied=12)
    assert (o["action"], o["shift"], o["n_left"], o["cls"], o["term"]) == (K.COMPACTED, 2, 1, K.MOVE_DISJOINT, 4)
    assert [int(v) for v in x["ents"][0]] == [int(v) for v in a["ents"][2]] and x["n_moved"] == 1
    assert [int(v) for v in x["groups"][0][3:5]] == [12, 1]
    # index = offset - 1: out of bounds; applied + 1: exceeds applied; both leave everything as it was
    for index, status in ((9, K.PANIC_COMPACT_BOUNDS), (13, K.PANIC_COMPACT_APPLIED)):
        a, x, o = _one([3, 3, 4], K.req(0, index), log_offset=10, committed=12, applied=12)
        assert (o["status"], o["action"]) == (status, K.PANICKED) and not x["res_rows"][0][1:].any()
        assert all(np.array_equal(x[k], a[k]) for k in ("groups", "pstate", "snaps", "ents"))
    # applied > lastIndex: Go's slice is nil and the log would be left empty -- reported, never guessed
    a, x, o = _one([3, 3, 4], K.req(0, 13), log_offset=10, committed=12, applied=14)
    assert (o["status"], o["action"]) == (K.UNSUPPORTED, K.PANICKED)
    assert all(np.array_equal(x[k], a[k]) for k in ("groups", "pstate", "snaps", "ents"))
    # an empty log at offset 0: raftLog.term indexes past ents
    a, x, o = _one([], K.req(0, 0), log_offset=0, applied=0)
    assert (o["status"], o["action"]) == (K.PANIC_BOUNDS, K.PANICKED)
    # shouldCompact: (applied - offset) > threshold, strictly
    a, x, o = _one([1] * 8, K.req(0, at_applied=True, threshold=5), log_offset=10, committed=15, applied=15)
    assert (o["status"], o["action"]) == (K.OK, K.NOT_DUE) and not x["res_rows"][0][1:].any()
    assert all(np.array_equal(x[k], a[k]) for k in ("groups", "pstate", "snaps", "ents"))
    a, x, o = _one([1] * 8, K.req(0, at_applied=True, threshold=5), log_offset=10, committed=16, applied=16)
    assert (o["action"], o["index"], o["shift"], o["n_left"], o["cls"]) == (K.COMPACTED, 16, 6, 2, K.MOVE_DISJOINT)
    # a wrapped applied - offset is a huge number: due, then the compact index is below the offset
    a, x, o = _one([1] * 3, K.req(0, at_applied=True, threshold=1 << 40), log_offset=10, committed=9, applied=9)
    assert (o["status"], o["action"]) == (K.PANIC_COMPACT_BOUNDS, K.PANICKED)
    # unstable = max(index + 1, unstable)
    a, x, o = _one([1] * 8, K.req(0, 13), log_offset=10, committed=15, applied=15, unstable=12)
    assert o["unstable"] == 14 and int(x["pstate"][0][1]) == 14 and o["cls"] == K.MOVE_OVERLAP
    a, x, o = _one([1] * 8, K.req(0, 13), log_offset=10, committed=15, applied=15, unstable=17)
    assert o["unstable"] == 17 and np.array_equal(x["pstate"], a["pstate"])
    # index + 1 wraps to 0: the maximum is the old unstable
    a, x, o = _one([1], K.req(0, M64), log_offset=M64, committed=M64, applied=M64, unstable=5)
    assert (o["status"], o["action"]) == (K.UNSUPPORTED, K.PANICKED)      # lastIndex + 1 wraps: slice is nil


def test_validate_classes():
    def call(edit=None, reqs=None):
        sc = FK.Scenario()
        for _ in range(3):
            sc.add_group([1, 1, 1], [(1, 0, 1), (2, 0, 1)], committed=2, applied=2)
        a = K.call_of(sc, reqs or [K.req(0, 1, data=(10, 90), nodes=(2, 8), removed=(10, 0)), K.req(2, 2)], 100, 10)
        if edit:
            edit(a)
        return K.validate(a)

    def word(name, row, col, val):
        def f(a):
            a[name][row, col] = np.uint64(val & M64)
        return f
    assert call() == K.OK
    assert call(word("reqs", 0, 0, 3)) == K.E_INVAL            # group >= G
    assert call(word("reqs", 1, 0, 0)) == K.E_INVAL            # a group named twice
    assert call(word("reqs", 0, 1, 2)) == K.E_INVAL            # a flags bit other than bit 0
    assert call(word("reqs", 0, 10, 1)) == K.E_INVAL and call(word("reqs", 0, 11, 1)) == K.E_INVAL   # pad
    assert call(word("reqs", 0, 1, 1)) == K.E_INVAL            # AT_APPLIED with index != 0
    assert call(word("reqs", 0, 5, 91)) == K.E_INVAL           # Data outside
    assert call(word("reqs", 0, 4, M64)) == K.E_INVAL          # ... wrapping
    assert call(word("reqs", 0, 7, 9)) == K.E_INVAL and call(word("reqs", 0, 8, 11)) == K.E_INVAL
    assert call(word("reqs", 0, 6, M64 - 3)) == K.E_INVAL
    assert call(word("groups", 0, 28, 1)) == K.E_INVAL and call(word("pstate", 2, 3, 1)) == K.E_INVAL
    assert call(word("pstate", 2, 2, 2)) == K.E_INVAL          # pending_conf > 1
    assert call(word("groups", 2, 4, 99)) == K.E_INVAL         # nlog > ents_cap
    assert call(word("groups", 2, 5, M64)) == K.E_INVAL        # the window wraps
    assert call(word("groups", 0, 8, 1)) == K.E_INVAL          # two equal peer ids
    assert call(word("groups", 1, 28, 1)) == K.OK              # a group no request names is not looked at


@pytest.fixture(scope="module")
def restated_digest():
    return K.digest(7, RUNS)


def test_generator_mix(restated_digest):
    """The condition on the generator, from the restatement alone: every action
    the call reports and every status in at least 2 % of the requests, each move
    class in at least 10 % of the compacted ones."""
    _, acts, stats, cls = restated_digest
    assert acts[K.NOT_STEPPED] == 0 and sum(acts) == sum(stats) == RUNS and sum(cls) == acts[K.COMPACTED]
    assert all(a >= RUNS * 0.02 for a in acts[1:]), acts
    assert all(s >= RUNS * 0.02 for s in stats), stats
    assert all(c >= acts[K.COMPACTED] * 0.10 for c in cls), cls
    a = K.random_scenario(11, 5000, 4000, idle_every=9)
    assert K.validate(a) == K.OK
    acts, stats, cls = K.mix_of(K.expected(a)["outcomes"])
    assert all(v >= 4000 * 0.02 for v in acts[1:] + stats), (acts, stats)
    assert all(c >= acts[K.COMPACTED] * 0.10 for c in cls), cls


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1"] + SAN], ids=["plain", "asan_ubsan"])
def test_compact_forms(tmp_path, flags, restated_digest):
    exe = str(tmp_path / "compact_forms")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "etcd_amd", "csrc"), "-o",
                    exe, os.path.join(ROOT, "tests", "host", "compact_forms.cpp")], check=True)
    out = subprocess.run([exe, "7", str(RUNS)], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "ok", out.stdout + out.stderr
    want, acts, stats, cls = restated_digest
    assert lines[0] == "runs %d" % RUNS
    assert [int(v) for _, v in re.findall(r"(\w+)=(\d+)", lines[1])] == acts
    assert [int(v) for _, v in re.findall(r"(\w+)=(\d+)", lines[2])] == stats
    assert [int(v) for _, v in re.findall(r"(\w+)=(\d+)", lines[3])] == cls
    assert lines[4] == "digest %d" % want
