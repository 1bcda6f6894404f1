"""CPU tests of the batched leader msgProp / msgBeat step: the ABI, the
restatement in lead_prop_cases.py against the reference's own tables and its
edges, the scenario builders' class mixes, and the host program
(tests/host/lead_prop_forms.cpp) that checks the closed form the kernels use
against the serial step -- and the serial step against the restatement --
plain and under ASan + UBSan.  The GPU parity suite is test_gpu_lead_prop.py."""
import collections
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from etcd_amd import _lib as L
from etcd_amd import raftprop as P

import lead_prop_cases as K

M64 = K.M64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
THREE = [(1, 2, 3), (2, 0, 3), (3, 0, 3)]


def test_abi_sizes_and_symbols():
    assert C.sizeof(L.LeadPropState) == L.lib.elead_prop_state_size() == 32
    assert C.sizeof(L.LeadLocal) == L.lib.elead_local_size() == 48
    assert C.sizeof(L.LeadLocalResult) == L.lib.elead_local_result_size() == 48
    for name in ("elead_local_batch_device", "elead_prop_state_size", "elead_local_size", "elead_local_result_size"):
        assert name in L.header_symbols() and hasattr(L.lib, name), name
    assert (P.STATE_WORDS, P.LOCAL_WORDS, P.RESULT_WORDS) == (4, 6, 6)
    assert (L.LEAD_L_NOT_STEPPED, L.LEAD_L_BEAT, L.LEAD_L_APPENDED, L.LEAD_L_DROPPED, L.LEAD_L_PANICKED) == \
        (K.NOT_STEPPED, K.BEAT, K.APPENDED, K.DROPPED, K.PANICKED) == (0, 1, 2, 3, 4)
    assert (L.LEAD_L_MSG_BEAT, L.LEAD_L_MSG_PROP) == (K.MSG_BEAT, K.MSG_PROP) == (1, 2)
    import etcd_amd
    assert etcd_amd.local_batch is P.local_batch and etcd_amd.local_batch_device is P.local_batch_device


def test_null_ctx_is_inval():
    nm, na = C.c_uint64(7), C.c_uint64(7)
    assert L.lib.elead_local_batch_device(None, None, None, 0, None, None, 0, 0, None, 0, None, None, 0, C.byref(nm),
                                          C.byref(na)) == L.E_INVAL
    assert (nm.value, na.value) == (0, 0)


def test_packers():
    rows = P.pack_locals([dict(group=3, kind="beat"), dict(group=4, kind="prop", etype=1, data_off=5, data_len=6),
                          dict(group=M64, kind=2, data_nil=True)])
    m = L.LeadLocal.from_buffer_copy(rows[1].tobytes())
    assert (m.group, m.kind, m.etype, m.data_nil, m.data_off, m.data_len, m.pad) == (4, 2, 1, 0, 5, 6, 0)
    m = L.LeadLocal.from_buffer_copy(rows[2].tobytes())
    assert (m.group, m.kind, m.etype, m.data_nil) == (M64, 2, 0, 1)
    assert int(rows[0, 1]) == 1
    st = P.pack_state([dict(ents_cap=9, unstable=4, pending_conf=True), dict()])
    s = L.LeadPropState.from_buffer_copy(st[0].tobytes())
    assert (s.ents_cap, s.unstable, s.pending_conf, s.reserved) == (9, 4, 1, 0)
    assert P.unpack_state(st)[0] == dict(ents_cap=9, unstable=4, pending_conf=1)
    grows, erows = P.pack_logs([dict(id=1, term=1, prs=[]), dict(id=2, term=1, prs=[])], [[1, 2], [3]],
                               [dict(ents_cap=4), dict(ents_cap=1)])
    assert erows.shape == (5, 5) and [int(x) for x in grows[:, 5]] == [0, 4] and int(erows[4, 0]) == 3
    r = L.LeadLocalResult.from_buffer_copy(np.array([2 << 32 | 39, 1, 2, 3, 4, 5], dtype=np.uint64).tobytes())
    assert (r.status, r.action, r.msg_first, r.n_msgs, r.index, r.ent_pos, r.committed) == (39, 2, 1, 2, 3, 4, 5)
    with pytest.raises(ValueError):
        P.pack_logs([dict(id=1, prs=[])], [[1, 2]], [dict(ents_cap=1)])


def test_restatement_passes_the_reference_tables():
    sc, named = K.kat_scenario()
    assert [n for n, _ in named] == ["TestStepConfig", "TestStepIgnoreConfig", "TestSingleNodeCommit",
                                     "TestProposal_case0_leader", "TestBcastBeat", "TestRecvMsgBeat_leader"]
    K.check_kats(sc, named)
    # TestProposal in full: the entry as the leader's log holds it
    _, grows, _, erows, _ = sc.expected()
    g = named[3][1]
    o = sc.outcomes[dict(sc.runs)[g]]
    assert [int(x) for x in erows[o["ent_pos"]][:2]] == [1, 2] and o["ent_pos"] == int(grows[g, 5]) + 2


def _one(terms, prs, what, **kw):
    sc = K.Scenario()
    sc.add_run(sc.add_group(terms, prs, **kw), what)
    res, grows, strows, erows, msgs = sc.expected()
    return sc, grows, strows, erows


def test_restatement_edges():
    # the nil-slice append at nlog == 0: the log becomes the one new entry, at index offset (lastIndex() + 1)
    sc, grows, strows, erows = _one([], [(1, 0, 1), (2, 0, 6)], "P", gid=1, term=3, log_offset=5, unstable=9)
    o = sc.outcomes[0]
    assert (o["status"], o["action"], o["index"], o["pos"], o["n_msgs"]) == (0, K.APPENDED, 5, 0, 1)
    assert int(grows[0, 4]) == 1 and [int(x) for x in erows[0][:2]] == [3, 5] and int(strows[0, 1]) == 5
    assert [int(x) for x in grows[0, 14:16]] == [5, 0] and int(grows[0, 21]) == 6
    # ... and at offset 0: lastIndex() is 2^64 - 1, the entry's Index wraps to 0
    sc, grows, strows, erows = _one([], [(1, 0, 1), (2, 0, 1)], "P", gid=1, term=3)
    assert (sc.outcomes[0]["index"], int(grows[0, 4]), int(strows[0, 1])) == (0, 1, 0)
    # a wrapped lastIndex: 3 entries at offset 2^64 - 2 -- slice(offset, 1) is nil, the 3 entries are dropped
    off = M64 - 1
    sc, grows, strows, erows = _one([1, 1, 1], [(1, 0, 1), (2, 0, M64)], "PP", gid=1, term=3, log_offset=off,
                                    unstable=M64)
    assert [(o["action"], o["index"], o["pos"]) for o in sc.outcomes] == [(K.APPENDED, 1, 0), (K.APPENDED, M64, 1)]
    assert int(grows[0, 4]) == 2 and int(strows[0, 1]) == 1
    assert [int(x) for x in erows[0][:2]] == [3, 1] and [int(x) for x in erows[1][:2]] == [3, M64]
    # update(2^64 - 1): next wraps to 0; lastIndex() + 1 then wraps and the next append is a nil slice again
    sc, grows, strows, erows = _one([1], [(1, 0, 1)], "PP", gid=1, term=3, log_offset=off, room=3)
    assert [(o["index"], o["pos"]) for o in sc.outcomes] == [(M64, 1), (0, 0)]
    assert [int(grows[0, 14]), int(grows[0, 21])] == [off, M64]     # the log is the one new entry at offset
    r = K.Raft(1, 3, K.K.LeaderLog([1], off), [(1, 0, 1)])
    assert K.step(r, K.MSG_PROP)[:2] == (0, K.APPENDED) and (r.prs[0][1].match, r.prs[0][1].next) == (M64, 0)
    # id not among the peers: prs[r.id] is nil; the proposal changes nothing, a beat still goes to every slot
    sc, grows, strows, erows = _one([1, 1], THREE, "BCP", gid=9, term=3)
    assert [(o["status"], o["action"], o["n_msgs"]) for o in sc.outcomes] == \
        [(0, K.BEAT, 3), (K.PANIC_NIL_PROGRESS, K.PANICKED, 0), (0, K.NOT_STEPPED, 0)]
    pk = sc.pack()
    assert np.array_equal(grows, pk[0]) and np.array_equal(strows, pk[1]) and np.array_equal(erows, pk[3])
    # n_peers 0 (nil progress, a beat sends nothing), 1 (commits alone), 8 (unsupported)
    sc, *_ = _one([1, 1], [], "BP", gid=1, term=3)
    assert [(o["status"], o["action"], o["n_msgs"]) for o in sc.outcomes] == [(0, K.BEAT, 0), (39, K.PANICKED, 0)]
    sc, grows, *_ = _one([1, 3], [(1, 1, 2)], "PB", gid=1, term=3, committed=1)
    assert [(o["action"], o["committed"], o["n_msgs"]) for o in sc.outcomes] == [(K.APPENDED, 2, 0), (K.BEAT, 2, 0)]
    sc, *_ = _one([1, 1], THREE + [(4, 0, 1), (5, 0, 1), (6, 0, 1), (7, 0, 1)], "BP", gid=1, term=3, n_peers=8)
    assert [(o["status"], o["action"]) for o in sc.outcomes] == [(K.UNSUPPORTED, K.PANICKED), (0, K.NOT_STEPPED)]
    # a ConfChange at both values of pending_conf
    sc, _, strows, _ = _one([1, 1], THREE, "C", gid=1, term=3, pending_conf=0)
    assert sc.outcomes[0]["action"] == K.APPENDED and int(strows[0, 2]) == 1
    sc, grows, strows, erows = _one([1, 1], THREE, "C", gid=1, term=3, pending_conf=1)
    assert (sc.outcomes[0]["action"], sc.outcomes[0]["n_msgs"], int(strows[0, 2])) == (K.DROPPED, 0, 1)
    assert np.array_equal(grows, sc.pack()[0]) and np.array_equal(erows, sc.pack()[3])
    # a panic in the broadcast's second message (peer 3's next is the offset 0): record, state and log as they were
    sc, grows, strows, erows = _one([0, 1, 1], [(1, 2, 3), (2, 0, 3), (3, 0, 0)], "CP", gid=1, term=1, unstable=7)
    assert [(o["status"], o["action"], o["n_msgs"]) for o in sc.outcomes] == \
        [(K.PANIC_FIRST_ENTRY, K.PANICKED, 0), (0, K.NOT_STEPPED, 0)]
    pk = sc.pack()
    assert np.array_equal(grows, pk[0]) and np.array_equal(strows, pk[1]) and np.array_equal(erows, pk[3])
    assert sc.n_msgs == 0
    # needSnapshot without a snapshot; with one the message is a msgSnap
    sc, *_ = _one([1, 1], [(1, 6, 7), (2, 0, 4)], "P", gid=1, term=1, log_offset=5)
    assert sc.outcomes[0]["status"] == K.PANIC_NEED_SNAPSHOT
    sc, *_ = _one([1, 1], [(1, 6, 7), (2, 0, 4)], "P", gid=1, term=1, log_offset=5, snap=dict(index=5, term=1))
    assert sc.outcomes[0]["status"] == 0 and sc.messages[0]["type"] == K.MSG_SNAP
    # unstable above and below the new index
    for unstable, want in ((9, 3), (2, 2), (3, 3)):
        _, _, strows, _ = _one([1, 1, 1], THREE, "P", gid=1, term=3, unstable=unstable)
        assert int(strows[0, 1]) == want
    # a follower whose next is past the old log gets log_term = Term of the entries appended before
    sc, *_ = _one([1, 1], [(1, 1, 2), (2, 0, 3)], "PP", gid=1, term=4)
    assert [(m["index"], m["log_term"], m["ents"]) for m in sc.messages] == [(2, 4, None), (2, 4, (3, 1))]


def test_builders_reach_every_class():
    sc = K.lattice_scenario()
    assert len(sc.groups) == 4 * 2 * 6 * 2 * 3 + 4
    sc.expected()
    acts = collections.Counter(o["action"] for o in sc.outcomes)
    assert all(acts[a] for a in range(5)), acts
    # BOUNDS cannot occur: after an append the log is never empty, and a wrapped lastIndex puts every index out of bounds
    stats = collections.Counter(o["status"] for o in sc.outcomes)
    assert all(stats[s] for s in (K.PANIC_NIL_PROGRESS, K.PANIC_NEED_SNAPSHOT, K.PANIC_FIRST_ENTRY, K.UNSUPPORTED)), stats
    assert any(m["type"] == K.MSG_SNAP for m in sc.messages)
    for n in (1, 63, 64, 65, 255, 256, 257, 1025):
        b = K.boundary_scenario(n)
        assert len(b.locals) == n
        b.expected()
        heads = [i for _, i in b.runs]
        for seam in (64, 256, 1024):
            if n > seam + 3:
                assert seam - 3 in heads and not any(seam - 3 < h <= seam + 2 for h in heads)
    for seed in (1, 2):
        sc = K.random_scenario(seed)
        sc.expected()
        acts = collections.Counter(o["action"] for o in sc.outcomes)
        assert all(acts[a] >= 300 for a in (K.BEAT, K.APPENDED, K.DROPPED)) and acts[K.PANICKED] >= 30, acts


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1"] + SAN], ids=["plain", "asan_ubsan"])
def test_lead_prop_forms(tmp_path, flags):
    exe = str(tmp_path / "lead_prop_forms")
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-I", os.path.join(ROOT, "etcd_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "host", "lead_prop_forms.cpp")], check=True)
    files = []
    for name, sc in (("kats", K.kat_scenario()[0]), ("lattice", K.lattice_scenario()), ("random", K.random_scenario(1)),
                     ("long", K.long_scenario([70, 300], lead_in=60))):
        files.append(str(tmp_path / (name + ".txt")))
        sc.case_file(files[-1])
    out = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "ok", out.stdout + out.stderr
    runs = re.match(r"runs (\d+) closed (\d+)$", lines[0])
    assert int(runs.group(1)) >= 100000 and int(runs.group(2)) >= 50000
    classes = dict((k, int(v)) for k, v in re.findall(r"(\w+)=(\d+)", lines[-2]))
    assert set(classes) == {"not_stepped", "beat", "appended", "dropped", "panicked"}
    assert all(v >= 1000 for v in classes.values()), classes
    assert sum(1 for ln in lines if ln.endswith(" cases")) == 4
