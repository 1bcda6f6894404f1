"""CPU tests of the batched StartNode / RestartNode: the ABI, the restatement in
node_cases.py against the reference's tables (TestNodeRestart, TestNode,
TestRestore) and its edges, every validate class, the lattice's reach, and the
host program (tests/host/node_forms.cpp) that runs the kernels' own decisions
(etcd_amd/csrc/node_start.h) over 100 000 random requests, plain and under
ASan + UBSan, and prints a digest the restatement must reproduce.  The GPU
parity suite is test_gpu_node.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from etcd_amd import _lib as L
from etcd_amd import raftnode as RN

import conf_cases as K
import node_cases as N
import raft_model as M

M64 = N.M64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
RUNS = 100000
NO_HARD = dict(Term=0, Vote=0, Commit=0)


def test_abi_sizes_and_symbols():
    assert C.sizeof(L.NodeReq) == L.lib.enode_req_size() == 128
    assert C.sizeof(L.NodePeer) == L.lib.enode_peer_size() == 32
    assert C.sizeof(L.NodeResult) == L.lib.enode_result_size() == 48
    for name in ("enode_batch_device", "enode_reqs_from_batch", "ewal_batch_entries_device", "enode_req_size",
                 "enode_peer_size", "enode_result_size"):
        assert name in L.header_symbols() and hasattr(L.lib, name), name
    assert (RN.REQ_WORDS, RN.PEER_WORDS, RN.RESULT_WORDS) == (N.REQ_WORDS, N.PEER_WORDS, N.RESULT_WORDS) == (16, 4, 6)
    assert (L.NODE_NONE, L.NODE_RESTARTED, L.NODE_RESTARTED_SNAP, L.NODE_STARTED, L.NODE_PANICKED) == \
        (N.NONE, N.RESTARTED, N.RESTARTED_SNAP, N.STARTED, N.PANICKED) == \
        (RN.NONE, RN.RESTARTED, RN.RESTARTED_SNAP, RN.STARTED, RN.PANICKED) == tuple(range(5))
    assert RN.ACTIONS == N.ACTION_NAMES and RN.NO_SNAP == N.NO_SNAP == L.NODE_NO_SNAP == M64
    hdr = open(L.HEADER).read()
    for k, name in enumerate(("NONE", "RESTARTED", "RESTARTED_SNAP", "STARTED", "PANICKED")):
        assert "ENODE_%s = %d" % (name, k) in hdr
    assert "EWAL_PANIC_NONE_ID = 49," in hdr and L.PANIC_NONE_ID == N.PANIC_NONE_ID == 49
    assert L.status_string(49) == "panic: cannot use none id"
    with pytest.raises(L.GoPanic):
        L.check(49)
    import etcd_amd
    assert etcd_amd.node_batch is RN.node_batch and etcd_amd.node_batch_device is RN.node_batch_device
    assert etcd_amd.reqs_from_batch is RN.reqs_from_batch and etcd_amd.entries_device is RN.entries_device
    raw = np.array([(N.STARTED << 32) | 48, 4, 3, 9, 2, 77], dtype=np.uint64).tobytes()
    r = L.NodeResult.from_buffer_copy(raw)
    assert (r.status, r.action, r.nlog, r.committed, r.log_offset, r.n_peers, r.data_first) == (48, N.STARTED, 4, 3, 9, 2, 77)
    assert RN.results_from(raw, 1)[0] == dict(status=48, action=N.STARTED, nlog=4, committed=3, log_offset=9, n_peers=2,
                                              data_first=77)
    rows = RN.pack_reqs([dict(group=3, kind=1, id=9, ents_first=4, ents_cap=5, src_first=6, n_src=7, data_delta=8,
                              hs_term=1, hs_vote=2, hs_commit=3)])
    q = L.NodeReq.from_buffer_copy(rows.tobytes())
    assert (q.group, q.kind, q.id, q.ents_first, q.ents_cap, q.src_first, q.n_src, q.data_delta, q.hs_term, q.hs_vote,
            q.hs_commit, q.snap, list(q.pad)) == (3, 1, 9, 4, 5, 6, 7, 8, 1, 2, 3, M64, [0] * 4)
    prow, ctx_bytes = RN.pack_peers([(1, b"ab"), (2, None), (3, b"c")])
    assert prow.tolist() == [[1, 0, 2, 0], [2, 2, 0, 0], [3, 2, 1, 0]] and ctx_bytes == b"abc"


def test_null_ctx_is_inval():
    counters = [C.c_uint64(7) for _ in range(3)]
    args = [None] * 7 + [0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, 0, None, 1, None]
    assert L.lib.enode_batch_device(None, *args[1:], *[C.byref(x) for x in counters]) == L.E_INVAL
    assert [x.value for x in counters] == [0, 0, 0]
    p, n = C.c_void_p(), C.c_uint64(0)
    assert L.lib.ewal_batch_entries_device(None, C.byref(p), C.byref(n)) == L.E_INVAL
    assert L.lib.enode_reqs_from_batch(None, None, 0, None, None) == L.E_INVAL


def _entries(kat, data):
    """Model entries of a table's entries; data: {name: bytes} for the named bodies."""
    out = []
    for e in kat:
        d = e["data"]
        d = None if d is None else data.get(d, d.encode())
        out.append(M.Entry(Term=e["term"], Index=e["index"], Type=e["type"], Data=d))
    return out


def _strip(ents):
    return [dict(Term=e["Term"], Index=e["Index"], Type=e["Type"], Data=e["Data"]) for e in ents]


def test_restatement_passes_node_restart():
    t = N.load_kats()["TestNodeRestart"]
    st = dict(Term=t["st"]["term"], Vote=t["st"]["vote"], Commit=t["st"]["commit"])
    n = N.RestartNode(t["id"], None, st, _entries(t["entries"], {}))
    rd = n.newReady()
    w = t["want"]
    assert rd["SoftState"] is None and rd["HardState"] == NO_HARD == dict(Term=w["hard"]["term"], Vote=w["hard"]["vote"],
                                                                           Commit=w["hard"]["commit"])
    assert rd["Entries"] == [] == w["entries"] and rd["Snapshot"]["Index"] == 0
    assert _strip(rd["CommittedEntries"]) == _strip(_entries(w["committed"], {}))
    n.accept(rd)
    assert not M.Node.containsUpdates(n.newReady())


def test_restatement_passes_node():
    """TestNode: StartNode(1, [{ID: 1}]), ApplyConfChange, Campaign, Propose -- the
    existing restatements of apply, campaign and propose on the built node."""
    t = N.load_kats()["TestNode"]
    cc = bytes.fromhex(t["ccdata_hex"])
    assert K.conf_change_marshal(0, 0, 1, b"") == cc
    n = N.StartNode(t["id"], [(p["id"], p["context"]) for p in t["peers"]])
    r = n.r
    assert [e["Data"] for e in r.raftLog.ents[1:]] == [cc] and r.raftLog.committed == 1 and r.raftLog.unstable == 0
    r.applyConfChange(0, 1)                           # n.ApplyConfChange(cc)
    r.Step(M.Message(M.MSG_HUP))                      # n.Campaign
    data = {"ccdata": cc}
    for k, w in enumerate(t["wants"]):
        if k == 1:
            r.Step(M.Message(M.MSG_PROP, From=t["id"], Entries=[M.Entry(Data=t["propose"].encode())]))
        # Go's prevHardSt starts at r.HardState = {0, 0, 0}: undo the seeding for the comparison with Go's own Ready
        if k == 0:
            n.prevHardSt = dict(NO_HARD)
        rd = n.newReady()
        if w["soft"] is None:
            assert rd["SoftState"] is None
        else:
            s = rd["SoftState"]
            assert (s["Lead"], s["RaftState"], s["Nodes"]) == (w["soft"]["lead"], w["soft"]["state"], w["soft"]["nodes"])
        assert rd["HardState"] == dict(Term=w["hard"]["term"], Vote=w["hard"]["vote"], Commit=w["hard"]["commit"])
        assert _strip(rd["Entries"]) == _strip(_entries(w["entries"], data))
        assert _strip(rd["CommittedEntries"]) == _strip(_entries(w["committed"], data))
        n.accept(rd)
    assert not M.Node.containsUpdates(n.newReady())


def test_restatement_passes_restore():
    t = N.load_kats()["TestRestore"]
    s = t["snapshot"]
    snap = M.Snapshot(Index=s["index"], Term=s["term"], Nodes=s["nodes"], RemovedNodes=s["removed"])
    n = N.RestartNode(t["id"], snap, dict(NO_HARD, Commit=s["index"]), [M.Entry(Term=s["term"])])
    r = n.r
    assert n.restored and r.raftLog.lastIndex() == t["last_index"] and r.raftLog.term(s["index"]) == t["last_term"]
    assert {str(k): [p.match, p.next] for k, p in r.prs.items()} == t["prs"]
    assert sorted(r.removed) == t["removed"] and r.raftLog.snapshot is snap
    assert r.restore(snap) is t["second_restore"]


def _one(spec, **kw):
    c = N.call_of([spec], G=1, **kw)
    assert N.validate(c) == N.OK
    x = N.expected(c)
    return c, x, {k: [int(v) for v in x["arrays"][k][0]] for k, _ in N.RECORDS}


def test_restatement_edges():
    # a fresh node: the dummy entry's place is taken by the loaded entries, all else zero
    c, x, a = _one(N.restart(id=7, ents=N.E3[:1]))
    first, cap = int(c["reqs"][0, 3]), int(c["reqs"][0, 4])
    assert a["groups"] == [7, 0, 0, 0, 1, first, 0] + [0] * 25 and a["pstate"] == [cap, 1, 0, 0]
    assert a["vstate"] == [0] * 8 and a["rstate"] == [0] * 8 and a["cstate"] == [0] * 16 and a["snaps"] == [0] * 8
    # loadState has no clamp; a zero HardState after a restore sets committed back to 0
    c, x, a = _one(N.restart(id=1, ents=N.E3, st=(0, 0, 0), snap=N.snapshot(9, 2, nodes=(1,))))
    assert a["groups"][:5] == [1, 0, 0, 9, 3] and a["pstate"][1] == 12 and a["rstate"] == [0, 0, 0, 0, 0, 9, 9, 0]
    assert a["groups"][6:8] == [1, 1] and (a["groups"][14], a["groups"][21]) == (9, 10)
    c, x, a = _one(N.restart(id=1, ents=N.E3, st=(3, 2, M64), snap=N.snapshot(9, 2, nodes=(2,))))
    assert a["groups"][:5] == [1, 3, M64, 9, 3] and a["vstate"][1] == 2 and a["rstate"][:3] == [3, 2, M64]
    assert (a["groups"][7], a["groups"][14], a["groups"][21]) == (2, 0, 10)
    # snapshot index 0: restore returns false, nothing of it is taken
    c, x, a = _one(N.restart(id=1, ents=N.E3, st=(1, 0, 1), snap=N.snapshot(0, 9, nodes=(1, 2), removed=(3,))))
    assert x["outcomes"] == [(N.OK, N.RESTARTED)] and a["groups"][6] == 0 and a["cstate"] == [0] * 16 and a["snaps"] == [0] * 8
    # index 2^64 - 1: unstable wraps
    c, x, a = _one(N.restart(id=1, ents=N.E3[:2], st=(1, 0, 1), snap=N.snapshot(M64, 9, nodes=(1,))))
    assert a["groups"][3] == M64 and a["pstate"][1] == 1 and (a["groups"][14], a["groups"][21]) == (M64, 0)
    # n_src 0: nlog 0, lastIndex wraps
    c, x, a = _one(N.restart(id=1, ents=()))
    assert a["groups"][4] == 0 and a["pstate"][1] == 0 and int(x["res_rows"][0, 1]) == 0
    # entries: rebased where data_nil == 0 only
    c, x, a = _one(N.restart(id=1, ents=[N.entry_row(1, 1, 0, 5, 6, 0), N.entry_row(1, 2, 0, 5, 6, 2),
                                         N.entry_row(1, 3, 0, 0, 0, 1)], delta=100))
    first = int(c["reqs"][0, 3])
    assert [int(v) for v in x["arrays"]["ents"][first:first + 3, 2]] == [105, 5, 0]
    # StartNode: the seeding, the bytes, the positions
    c, x, a = _one(N.start(id=3, peers=[(1, b""), (300, b"xy")]), data_base=1000, data_fill=2)
    first = int(c["reqs"][0, 3])
    b1, b2 = K.conf_change_marshal(0, 0, 1, b""), K.conf_change_marshal(0, 0, 300, b"xy")
    assert b1 == bytes([8, 0, 0x10, 0, 0x18, 1, 0x22, 0]) and b2 == bytes([8, 0, 0x10, 0, 0x18, 0xAC, 2, 0x22, 2]) + b"xy"
    assert a["groups"][:7] == [3, 0, 2, 0, 3, first, 0] and a["pstate"][1:3] == [0, 0] and a["rstate"] == [0, 0, 2, 0, 0, 0, 0, 0]
    assert x["arrays"]["ents"][first:first + 3].tolist() == [[0, 0, 0, 0, 1 << 32], [1, 1, 1000, len(b1), 1],
                                                             [1, 2, 1000 + len(b1), len(b2), 1]]
    assert x["data"][:len(b1 + b2)] == b1 + b2 and x["data"][len(b1 + b2):] == c["data"][len(b1 + b2):]
    assert x["n_data"] == len(b1 + b2) and [int(v) for v in x["res_rows"][0]] == [N.STARTED << 32, 3, 2, 0, 0, 0]
    # a panicking request leaves everything as it was
    for spec in (N.restart(id=0, ents=N.E3), N.start(id=0), N.restart(id=1, snap=N.snapshot(1, 1, nodes=range(8)))):
        c = N.call_of([spec], G=1)
        x = N.expected(c)
        assert x["outcomes"][0][1] == N.PANICKED and [int(v) for v in x["res_rows"][0, 1:]] == [0] * 5
        assert all(np.array_equal(x["arrays"][k], c[k]) for k in N.ARRAY_KEYS) and x["data"] == c["data"]
    # the size query modifies nothing but gives the same results
    c = N.call_of([s for _, s in N.lattice_specs()])
    x, y = N.expected(c), N.expected(c, emit=False)
    assert np.array_equal(x["res_rows"], y["res_rows"]) and (x["n_data"], x["n_copied"], x["n_built"]) == \
        (y["n_data"], y["n_copied"], y["n_built"])
    assert all(np.array_equal(y["arrays"][k], c[k]) for k in N.ARRAY_KEYS) and y["data"] == c["data"]


def test_validate_classes():
    names = [name for name, _ in N.inval_calls()]
    assert len(names) == len(set(names)) == 23
    for name, c in N.inval_calls():
        assert N.validate(c) == N.E_INVAL, name
    ok = N.call_of([N.restart(id=1, ents=N.E3, cap=3), N.start(id=1, peers=[(1, b""), (2, b"")], cap=3)])
    assert N.validate(ok) == N.OK
    assert N.validate(N.call_of([N.restart(id=1, ents=N.E3, cap=2)])) == N.E_NOMEM
    assert N.validate(N.call_of([N.start(id=1, peers=[(1, b""), (2, b"")], cap=2)])) == N.E_NOMEM
    c = N.call_of([N.start(id=1, peers=[(1, b"abc")])])
    need = c["data_cap"]
    assert N.validate(c) == N.OK and N.validate(dict(c, data_cap=need - 1)) == N.E_NOMEM
    assert N.validate(dict(c, data_cap=None)) == N.OK                         # the size query
    assert N.validate(N.call_of([N.start(id=0, peers=[(1, b"abc")])], data_cap=0)) == N.OK   # a panicking request has no bytes
    assert N.validate(N.call_of([N.restart(id=1, ents=N.E3, cap=2), N.start(id=2, group=0)], G=2)) == N.E_INVAL   # INVAL wins
    assert N.validate(ok, G=N.INT_MAX) == N.E_INVAL and N.validate(ok, n=N.INT_MAX) == N.E_INVAL
    # a snapshot's ranges are checked whatever its index is; a kind-0 request's other words are not looked at
    c = N.call_of([N.restart(id=1, ents=N.E3, snap=N.snapshot(0, 1, nodes=(1,)))])
    c["in_snaps"][0, 5] = 99
    assert N.validate(c) == N.E_INVAL
    c = N.call_of([N.none()])
    c["reqs"][0, 2:12] = M64
    assert N.validate(c) == N.OK and N.expected(c)["outcomes"] == [(N.OK, N.NONE)]


def test_lattice_reaches_every_edge():
    specs = dict(N.lattice_specs())
    assert len(specs) == len(N.lattice_specs())
    acts = [0] * 5
    for name, c in N.lattice_calls():
        assert N.validate(c) == N.OK, name
        x = N.expected(c)
        for k, v in enumerate(N.mix_of(x["outcomes"])):
            acts[k] += v
    assert all(acts), acts
    out = {name: N.expected(c)["outcomes"][0] for name, c in N.lattice_calls()[:-1]}
    assert out["distinct_nodes_7"] == (N.OK, N.RESTARTED_SNAP) and out["distinct_nodes_8"] == (N.UNSUPPORTED, N.PANICKED)
    assert out["nodes_64"] == (N.OK, N.RESTARTED_SNAP) and out["nodes_65"] == (N.UNSUPPORTED, N.PANICKED)
    assert out["nodes_65_index_0"] == (N.OK, N.RESTARTED)
    assert out["removed_14"] == (N.OK, N.RESTARTED_SNAP) and out["removed_15"] == (N.UNSUPPORTED, N.PANICKED)
    assert [len(K.conf_change_marshal(0, 0, i, b"")) - 7 for i in N.IDS] == [1, 1, 2, 2, 9, 9, 10, 10]


@pytest.fixture(scope="module")
def restated_digest():
    return N.digest(7, RUNS)


def test_generator_mix(restated_digest):
    """Every action in at least 5 % of the requests, from the restatement alone."""
    _, acts = restated_digest
    assert sum(acts) == RUNS and all(v >= RUNS * 0.05 for v in acts), acts
    for n in (65, 257):
        c = N.random_call(n, n, 300)
        assert N.validate(c) == N.OK and all(N.mix_of(N.expected(c)["outcomes"]))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1"] + SAN], ids=["plain", "asan_ubsan"])
def test_node_forms(tmp_path, flags, restated_digest):
    exe = str(tmp_path / "node_forms")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "etcd_amd", "csrc"), "-o",
                    exe, os.path.join(ROOT, "tests", "host", "node_forms.cpp")], check=True)
    out = subprocess.run([exe, "7", str(RUNS)], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "ok", out.stdout + out.stderr
    want, acts = restated_digest
    assert lines[0] == "runs %d" % RUNS
    assert [int(v) for _, v in re.findall(r"(\w+)=(\d+)", lines[1])] == acts
    assert lines[2] == "digest %d" % want
