"""CPU tests of the three membership calls: the ABI, the enum values in the
header and status 47's string, the restatement in conf_cases.py against the
reference's own tables (tests/golden/raft_conf_kats.json), every validate
class, the generators' mix, and the host program (tests/host/conf_forms.cpp)
that runs the kernels' own decisions (etcd_amd/csrc/conf_step.h) over 100 000
random requests, ConfChange bodies and gate records, plain and under ASan +
UBSan, and prints a digest the restatement must reproduce.  The GPU parity
suites are test_gpu_conf.py and test_gpu_conf_cluster.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from etcd_amd import _lib as L
from etcd_amd import raftconf as RC

import conf_cases as K
import raft_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
RUNS = 100000


def test_abi_sizes_symbols_and_enums():
    sizes = (("econf_state", L.ConfState, 128), ("econf_req", L.ConfReq, 32), ("econf_result", L.ConfResult, 48),
             ("econf_applied", L.ConfApplied, 32), ("econf_scan_result", L.ConfScanResult, 48),
             ("econf_gate_result", L.ConfGateResult, 32))
    for name, cls, want in sizes:
        assert C.sizeof(cls) == getattr(L.lib, name + "_size")() == want, name
    for name in ("econf_batch_device", "econf_scan_committed_device", "econf_gate_batch_device"):
        assert name in L.header_symbols() and hasattr(L.lib, name), name
    assert (RC.CSTATE_WORDS, RC.REQ_WORDS, RC.RESULT_WORDS, RC.APPLIED_WORDS, RC.SCAN_WORDS, RC.GATE_WORDS) == \
        (16, 4, 6, 4, 6, 4)
    hdr = open(L.HEADER).read()
    for k, name in enumerate(("NOT_STEPPED", "ADDED", "REMOVED", "DENIED_BACK", "STOPPED", "RELOADED", "PANICKED")):
        assert "ECONF_%s = %d" % (name, k) in hdr
        assert getattr(L, "CONF_" + name) == getattr(RC, name) == k
    assert (K.NOT_STEPPED, K.ADDED, K.REMOVED, K.DENIED_BACK, K.STOPPED, K.RELOADED, K.PANICKED) == tuple(range(7))
    assert "ECONF_G_PASS = 1, ECONF_G_DENIED = 2, ECONF_G_DROPPED = 3" in hdr
    assert (L.CONF_G_PASS, L.CONF_G_DENIED, L.CONF_G_DROPPED) == (K.G_PASS, K.G_DENIED, K.G_DROPPED) == (1, 2, 3)
    assert "#define ECONF_FROM_SELF 0xffffffffu" in hdr and L.CONF_FROM_SELF == K.FROM_SELF == RC.FROM_SELF
    assert (L.CONF_ADD, L.CONF_REMOVE, L.CONF_DENIED, L.CONF_RELOAD) == (K.ADD, K.REMOVE, K.DENIED, K.RELOAD)
    assert RC.ACTIONS == K.ACTION_NAMES
    assert "EWAL_PANIC_CONF_TYPE = 47," in hdr and L.PANIC_CONF_TYPE == K.PANIC_CONF_TYPE == 47
    assert L.status_string(47) == "panic: unexpected conf type"
    with pytest.raises(L.GoPanic):
        L.check(47)
    import etcd_amd
    for name in ("conf_batch", "conf_batch_device", "scan_committed", "scan_committed_device", "gate_batch",
                 "gate_batch_device", "pack_cstate", "unpack_cstate", "removed_u64"):
        assert getattr(etcd_amd, name) is getattr(RC, name) and name in etcd_amd.__all__
    raw = np.array([(K.REMOVED << 32) | 48, 7, 1, 3, 9, 0], dtype=np.uint64).tobytes()
    r = L.ConfResult.from_buffer_copy(raw)
    assert (r.status, r.action, r.msg_first, r.n_msgs, r.n_peers, r.n_removed) == (48, K.REMOVED, 7, 1, 3, 9)
    assert RC.results_from(raw, 1)[0] == dict(status=48, action=K.REMOVED, msg_first=7, n_msgs=1, n_peers=3,
                                              n_removed=9)


def test_pack_helpers():
    rows = RC.pack_cstate([[], [5, 9], list(range(1, 15))])
    assert rows.shape == (3, 16) and [int(x) for x in rows[:, 0]] == [0, 2, 14] and int(rows[2, 15]) == 0
    assert RC.unpack_cstate(rows) == [[], [5, 9], list(range(1, 15))]
    with pytest.raises(ValueError):
        RC.pack_cstate([list(range(15))])
    vals, ranges = RC.removed_u64(rows)
    assert ranges == [(0, 0), (0, 2), (2, 14)] and [int(x) for x in vals] == [5, 9] + list(range(1, 15))
    assert np.array_equal(RC.pack_reqs([(3, 2, 7), dict(group=1, kind=1, node=4)]),
                          np.array([[3, 2, 7, 0], [1, 1, 4, 0]], dtype=np.uint64))


def test_null_ctx_is_inval():
    a, b = C.c_uint64(7), C.c_uint64(7)
    assert L.lib.econf_batch_device(None, None, None, None, None, None, 0, None, None, 0, None, 0, None, None, 0,
                                    C.byref(a), C.byref(b)) == L.E_INVAL
    assert (a.value, b.value) == (0, 0)
    a, b = C.c_uint64(7), C.c_uint64(7)
    assert L.lib.econf_scan_committed_device(None, None, None, 0, 0, None, 0, None, 0, None, None, None, 0, C.byref(a),
                                             C.byref(b)) == L.E_INVAL
    assert (a.value, b.value) == (0, 0)
    a, b = C.c_uint64(7), C.c_uint64(7)
    assert L.lib.econf_gate_batch_device(None, None, None, 0, None, 0, 64, 2, None, None, 0, None, 0, C.byref(a),
                                         C.byref(b)) == L.E_INVAL
    assert (a.value, b.value) == (0, 0)


# ---- the restatement against the reference's tables ---------------------------------------------

def test_kat_add_and_remove_node():
    kat = K.load_kats()
    t = kat["TestAddNode"]
    r = K.ConfRaft(t["id"], t["peers"])
    r.pendingConf = t["pending_conf"]
    r.addNode(t["add"])
    assert r.pendingConf is t["want"]["pending_conf"] and sorted(r.nodes()) == t["want"]["nodes_sorted"]
    t = kat["TestRemoveNode"]
    r = K.ConfRaft(t["id"], t["peers"])
    r.pendingConf = t["pending_conf"]
    r.removeNode(t["remove"])
    assert r.pendingConf is t["want"]["pending_conf"] and r.nodes() == t["want"]["nodes"]
    assert r.removed == {k: True for k in t["want"]["removed"]}
    # ... and through the records
    a = K.arrays_of([K.group(id=1, peers=(1,), pending=1)])
    x = K.expected_batch(a, K.reqs_of([(0, K.ADD, 2)]))
    assert x["outcomes"] == [(K.OK, K.ADDED)] and [int(v) for v in x["arrays"]["groups"][0, 6:9]] == [2, 1, 2]
    assert int(x["arrays"]["pstate"][0, 2]) == 0 and int(x["arrays"]["rstate"][0, 7]) == 1
    a = K.arrays_of([K.group(id=1, peers=(1, 2), pending=1)])
    x = K.expected_batch(a, K.reqs_of([(0, K.REMOVE, 2)]))
    assert x["outcomes"] == [(K.OK, K.REMOVED)] and [int(v) for v in x["arrays"]["groups"][0, 6:9]] == [1, 1, 0]
    assert RC.unpack_cstate(x["arrays"]["cstate"]) == [[2]] and int(x["arrays"]["pstate"][0, 2]) == 0


def test_kat_msg_denied():
    kat = K.load_kats()
    t = kat["TestRecvMsgDenied"]
    assert t["msg"]["type"] == R.MSG_DENIED
    r = K.ConfRaft(t["id"], t["peers"])
    called = []
    r_step = R.stepFollower
    try:
        R.stepFollower = lambda rr, m: called.append(m)
        assert r.Step(R.Message(R.MSG_DENIED, From=t["msg"]["from"])) == "stopped"
    finally:
        R.stepFollower = r_step
    assert bool(called) is t["want"]["step_called"] and r.removed == {k: True for k in t["want"]["removed"]}
    assert r.shouldStop() and r.softState()["ShouldStop"] is True
    t = kat["TestRecvMsgFromRemovedNode"]
    assert (t["msg_type"], t["wmsg_type"]) == (R.MSG_VOTE, R.MSG_DENIED)
    for x in t["tests"]:
        r = K.ConfRaft(t["id"], t["peers"])
        r.removeNode(x["from"])
        assert r.Step(R.Message(R.MSG_VOTE, From=x["from"])) == "denied_back"
        assert len(r.msgs) == x["wmsgNum"] and all(m["Type"] == R.MSG_DENIED for m in r.msgs)
        # ... as kind 3 and through the gate
        a = K.arrays_of([K.group(id=t["id"], peers=t["peers"])])
        y = K.expected_batch(a, K.reqs_of([(0, K.REMOVE, x["from"]), (0, K.DENIED, x["from"])]))
        assert y["outcomes"][1] == (K.OK, K.DENIED_BACK) and y["n_msgs"] == x["wmsgNum"]
        recs = np.array([[0, R.MSG_VOTE, x["from"], 0, 0, 0, 0, 0]], dtype=np.uint64)
        z = K.expected_gate(y["arrays"]["groups"], y["arrays"]["cstate"], recs, 2)
        assert z["n_msgs"] == x["wmsgNum"] and z["n_pass"] == 0
        assert z["actions"] == [K.G_DENIED if x["wmsgNum"] else K.G_DROPPED]


def test_kat_promotable_and_pending_conf():
    kat = K.load_kats()
    t = kat["TestPromotable"]
    for x in t["tests"]:
        r = K.ConfRaft(t["id"], [])
        for p in x["peers"]:
            r.addNode(p)
        assert r.promotable() is x["wp"]
    t = kat["TestStepConfig"]
    r = K.ConfRaft(t["id"], t["peers"])
    r.becomeCandidate()
    r.becomeLeader()
    index = r.raftLog.lastIndex()
    r.Step(R.Message(R.MSG_PROP, From=1, To=1, Entries=[R.Entry(Type=R.ENTRY_CONF_CHANGE)]))
    assert r.raftLog.lastIndex() == index + t["want"]["last_index_delta"] and r.pendingConf is True
    t = kat["TestStepIgnoreConfig"]
    index = r.raftLog.lastIndex()
    r.Step(R.Message(R.MSG_PROP, From=1, To=1, Entries=[R.Entry(Type=R.ENTRY_CONF_CHANGE)]))
    assert r.raftLog.lastIndex() == index + t["want"]["second_last_index_delta"] and r.pendingConf is True
    # what the device could not do before: the applied ConfChange clears the flag and the next one is taken
    r.addNode(3)
    assert r.pendingConf is False
    r.Step(R.Message(R.MSG_PROP, From=1, To=1, Entries=[R.Entry(Type=R.ENTRY_CONF_CHANGE)]))
    assert r.raftLog.lastIndex() == index + 1
    t = kat["TestRecoverPendingConfig"]
    for x in t["tests"]:
        r = K.ConfRaft(t["id"], t["peers"])
        r.appendEntry(R.Entry(Type=x["ent_type"]))
        r.becomeCandidate()
        r.becomeLeader()
        assert r.pendingConf is x["wpending"]


def test_kat_conf_change_bytes():
    for x in K.load_kats()["ConfChangeMarshal"]["tests"]:
        ctx = bytes.fromhex(x["context"])
        want = bytes.fromhex(x["hex"])
        assert K.conf_change_marshal(x["id"], x["type"], x["node"], ctx) == want
        assert RC.conf_change_marshal(x["id"], x["type"], x["node"], ctx) == want
        st, m, _ = K.conf_change_unmarshal(want)
        assert (st, m["id"], m["type"], m["node"], m["context"] or b"") == (K.OK, x["id"], x["type"], x["node"], ctx)
    st, m, _ = K.conf_change_unmarshal(b"")
    assert (st, m["id"], m["type"], m["node"], K.kind_of(m["type"])) == (K.OK, 0, 0, 0, K.ADD)


def test_decode_edges():
    got = {name: K.conf_change_unmarshal(body) for name, body in K.scan_edge_bodies()}
    st = {k: v[0] for k, v in got.items()}
    assert st["empty"] == st["nil"] == st["plain"] == K.OK
    assert st["ten_byte_varint"] == K.OK and got["ten_byte_varint"][1]["id"] == K.M64
    assert st["eleven_byte_varint"] == K.OK and got["eleven_byte_varint"][1]["node"] == 0
    m = got["repeated_field"][1]
    assert (m["id"], m["type"], m["node"]) == (0x11, 1, 7)
    assert got["type_past_32_bits"][1]["type"] == 0 and K.kind_of(got["type_minus_one"][1]["type"]) == 1 << 32
    assert all(st["wrong_wire_f%d" % f] == K.ERR_WRONG_TYPE for f in (1, 2, 3, 4))
    assert st["wire_type_6"] == K.ERR_WRONG_TYPE and st["unknown_fixed32_cut"] == K.ERR_EOF
    assert st["unknown_varint"] == st["unknown_fixed64"] == st["unknown_bytes"] == st["end_group_alone"] == K.OK
    assert st["group_depth_16"] == K.OK and got["group_depth_16"][2].pushes == K.SKIP_DEPTH
    assert st["group_depth_17"] == K.UNSUPPORTED and st["group_unterminated"] == K.ERR_EOF
    assert st["context_past_end"] == K.ERR_EOF and st["context_negative"] == K.PANIC_BOUNDS
    cuts = [st["cut_%d" % k] for k in range(12)]
    assert cuts[0] == K.OK and set(cuts[1:]) == {K.OK, K.ERR_EOF} and cuts.count(K.ERR_EOF) >= 6


# ---- the validate classes -------------------------------------------------------------------------

def _word(name, row, col, val):
    def f(a):
        a[name][row, col] = np.uint64(val & K.M64)
    return f


def test_validate_batch_classes():
    def call(edit=None, reqs=((0, K.ADD, 9), (0, K.REMOVE, 2), (2, K.DENIED, 5), (2, K.RELOAD, 0))):
        a = K.arrays_of([K.group(id=1), K.group(id=2), K.group(id=3, removed=(5,))], snaps=[None, None, (1, 2)],
                        u64=(7, 8, 9))
        if edit:
            edit(a)
        return a, K.reqs_of(reqs)
    assert K.validate_batch(*call()) == K.OK
    assert K.validate_batch(*call(reqs=((3, K.ADD, 1),))) == K.E_INVAL                    # group >= G
    assert K.validate_batch(*call(reqs=((0, 1, 1), (1, 1, 1), (0, 1, 2)))) == K.E_INVAL   # a run not adjacent
    assert K.validate_batch(*call(reqs=((0, 1, 1, 1),))) == K.E_INVAL                     # pad
    for col in (28, 31):
        assert K.validate_batch(*call(_word("groups", 0, col, 1))) == K.E_INVAL           # reserved words
    assert K.validate_batch(*call(_word("pstate", 0, 3, 1))) == K.E_INVAL
    assert K.validate_batch(*call(_word("vstate", 2, 7, 1))) == K.E_INVAL
    assert K.validate_batch(*call(_word("cstate", 2, 15, 1))) == K.E_INVAL
    assert K.validate_batch(*call(_word("cstate", 0, 0, 15))) == K.E_INVAL                # n_removed > 14
    assert K.validate_batch(*call(_word("cstate", 0, 0, 14))) == K.OK
    assert K.validate_batch(*call(_word("groups", 0, 8, 1))) == K.E_INVAL                 # duplicate peer_id
    assert K.validate_batch(*call(_word("groups", 0, 10, 1))) == K.OK                     # ... past n_peers
    assert K.validate_batch(*call(_word("pstate", 2, 2, 2))) == K.E_INVAL                 # pending_conf > 1
    assert K.validate_batch(*call(_word("rstate", 0, 7, 2))) == K.E_INVAL                 # soft_dirty > 1
    assert K.validate_batch(*call(_word("vstate", 0, 0, 3))) == K.E_INVAL                 # state > 2
    assert K.validate_batch(*call(_word("vstate", 0, 4, 8))) == K.E_INVAL                 # a vote past n_peers
    assert K.validate_batch(*call(_word("vstate", 0, 5, 1))) == K.E_INVAL                 # granted outside voted
    assert K.validate_batch(*call(_word("snaps", 2, 7, 3))) == K.E_INVAL                  # the range past n_u64
    assert K.validate_batch(*call(_word("snaps", 2, 6, K.M64))) == K.E_INVAL              # ... wrapping
    assert K.validate_batch(*call(_word("pstate", 1, 3, 1))) == K.OK                      # a group no request names
    a, reqs = call()
    a["snaps"] = None
    assert K.validate_batch(a, reqs) == K.E_INVAL                                         # kind 4 without d_snaps
    a, reqs = call()
    assert K.expected_batch(a, reqs)["n_msgs"] == 1
    assert K.validate_batch(a, reqs, 1) == K.OK and K.validate_batch(a, reqs, 0) == K.E_NOMEM
    assert K.validate_batch(*call(_word("pstate", 2, 2, 2)), 0) == K.E_INVAL              # INVAL wins
    assert K.validate_batch(a, reqs, n=K.INT_MAX) == K.E_INVAL and K.validate_batch(a, reqs, G=K.INT_MAX) == K.E_INVAL


def test_validate_scan_and_gate_classes():
    c = K.scan_case([[(1, b"\x18\x02")], [], [(0, b"zz"), (1, None)]])
    assert K.validate_scan(c) == K.OK and K.expected_scan(c)["n_reqs"] == 2
    assert K.validate_scan(c, 2) == K.OK and K.validate_scan(c, 1) == K.E_NOMEM
    assert K.validate_scan(dict(c, sel=[0, 3, 1])) == K.E_INVAL                           # a selected group >= G
    assert K.validate_scan(dict(c, G=5)) == K.E_INVAL                                     # d_sel NULL with n != G
    assert K.validate_scan(dict(c, G=5, sel=[4, 0, 2])) == K.OK
    for col, val in ((6, len(c["ents"]) + 1), (7, len(c["ents"])), (6, K.M64)):
        bad = dict(c, ready=c["ready"].copy())
        bad["ready"][0, col] = np.uint64(val)
        assert K.validate_scan(bad) == K.E_INVAL                                          # a committed range outside
    for col, val in ((2, 99), (3, 99), (2, K.M64), (4, 1 | 3 << 32)):
        bad = dict(c, ents=c["ents"].copy())
        bad["ents"][int(c["ready"][0, 6]), col] = np.uint64(val)
        assert K.validate_scan(bad) == K.E_INVAL                                          # a Data range, data_nil
        assert K.validate_scan(bad, 0) == K.E_INVAL
    a = K.arrays_of([K.group(id=1, removed=(4, 1)), K.group(id=2)])
    recs = np.array([[0, 5, 4, 0, 0, 0, 0, 0], [1, 5, 4, 0, 0, 0, 0, 0], [0, 5, 1, 0, 0, 0, 0, 0]], dtype=np.uint64)
    x = K.expected_gate(a["groups"], a["cstate"], recs, 2)
    assert x["actions"] == [K.G_DENIED, K.G_PASS, K.G_DROPPED]
    assert K.validate_gate(a["groups"], a["cstate"], recs, 64, 2) == K.OK
    assert K.validate_gate(a["groups"], a["cstate"], recs, 64, 2, 1, 1) == K.OK
    assert K.validate_gate(a["groups"], a["cstate"], recs, 64, 2, 0, 1) == K.E_NOMEM
    assert K.validate_gate(a["groups"], a["cstate"], recs, 64, 2, 1, 0) == K.E_NOMEM
    assert K.validate_gate(a["groups"], a["cstate"], recs, 64, 2, 1, None) == K.E_INVAL
    for rb, fw in ((32, 1), (56, 1), (64, 0), (64, 8), (48, 6)):
        assert K.validate_gate(a["groups"], a["cstate"], recs, rb, fw) == K.E_INVAL
    assert K.validate_gate(a["groups"], a["cstate"], recs, 64, K.FROM_SELF) == K.OK
    bad = recs.copy()
    bad[1, 0] = 2
    assert K.validate_gate(a["groups"], a["cstate"], bad, 64, 2) == K.E_INVAL
    for col, val in ((0, 15), (15, 1)):
        c2 = a["cstate"].copy()
        c2[0, col] = val
        assert K.validate_gate(a["groups"], c2, recs, 64, 2) == K.E_INVAL


# ---- the generators' mix ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def restated_digest():
    return K.digest(7, RUNS)


def test_generator_mix(restated_digest):
    """Every action of the three calls occurs, from the restatement alone, and
    NOT_STEPPED plus panicked / unsupported requests stay under a quarter of
    the random requests."""
    _, acts, sts, gates = restated_digest
    assert acts[K.NOT_STEPPED] == 0 and all(acts[1:]) and all(gates[1:])
    assert acts[K.PANICKED] < sum(acts) / 4, acts
    assert {K.OK, K.ERR_EOF, K.ERR_WRONG_TYPE} <= set(sts)
    for seed in (1, 2, 3):
        a, reqs = K.random_batch(seed, 2048, 1500)
        assert K.validate_batch(a, reqs) == K.OK
        x = K.expected_batch(a, reqs)
        counts = [sum(1 for _, act in x["outcomes"] if act == k) for k in range(7)]
        assert all(counts), counts
        assert counts[K.NOT_STEPPED] + counts[K.PANICKED] < len(reqs) / 4, counts
        assert {st for st, _ in x["outcomes"]} == {K.OK, K.PANIC_CONF_TYPE, K.UNSUPPORTED}
        assert x["n_msgs"] > 0 and any(j - i >= 9 for i, j in K.runs_of(reqs))
    c = K.random_scan(5, 600)
    assert K.validate_scan(c) == K.OK
    x = K.expected_scan(c)
    assert {K.OK, K.ERR_EOF, K.ERR_WRONG_TYPE, K.ERR_ENTRY_TYPE} <= set(x["statuses"]) and x["n_reqs"] > 600
    for words, fw in ((6, 1), (8, 2), (12, 2), (6, K.FROM_SELF)):
        a, recs = K.random_gate(9, 64, 500, words, fw)
        acts = K.expected_gate(a["groups"], a["cstate"], recs, fw)["actions"]
        want = {K.G_PASS, K.G_DROPPED} if fw == K.FROM_SELF else {K.G_PASS, K.G_DENIED, K.G_DROPPED}
        assert set(acts) == want


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1"] + SAN], ids=["plain", "asan_ubsan"])
def test_conf_forms(tmp_path, flags, restated_digest):
    exe = str(tmp_path / "conf_forms")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "etcd_amd", "csrc"), "-o",
                    exe, os.path.join(ROOT, "tests", "host", "conf_forms.cpp")], check=True)
    out = subprocess.run([exe, "7", str(RUNS)], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "ok", out.stdout + out.stderr
    want, acts, sts, gates = restated_digest
    assert lines[0] == "runs %d" % RUNS
    assert [int(v) for _, v in re.findall(r"(\w+)=(\d+)", lines[1])] == acts
    assert [int(v) for _, v in re.findall(r"(\w+)=(\d+)", lines[2])] == \
        [sts.get(k, 0) for k in (K.OK, K.ERR_EOF, K.ERR_WRONG_TYPE, K.PANIC_BOUNDS, K.NONTERMINATING)]
    assert [int(v) for _, v in re.findall(r"(\w+)=(\d+)", lines[3])] == gates[1:]
    assert lines[4] == "digest %d" % want
