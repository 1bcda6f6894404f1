"""CPU tests of the batched Ready: the ABI, the packers, the restatement in
ready_cases.py against the reference's own tables and its edges, the random
generator's class mix, and the host program (tests/host/ready_forms.cpp) that
runs the kernels' own decision (etcd_amd/csrc/ready_step.h) over 100 000 random
groups, plain and under ASan + UBSan, and prints a digest the restatement must
reproduce.  The GPU parity suite is test_gpu_ready.py."""
import collections
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from etcd_amd import _lib as L

import ready_cases as K

M64 = K.M64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
GROUPS = 100000


def test_abi_sizes_and_symbols():
    assert C.sizeof(L.ReadyState) == L.lib.eready_state_size() == 64
    assert C.sizeof(L.ReadyResult) == L.lib.eready_result_size() == 96
    for name in ("eready_batch_device", "eready_state_size", "eready_result_size"):
        assert name in L.header_symbols() and hasattr(L.lib, name), name
    from etcd_amd import raftready as R
    assert (R.RSTATE_WORDS, R.RESULT_WORDS, R.SAVE_WORDS) == (K.RSTATE_WORDS, K.RESULT_WORDS, K.SAVE_WORDS) == (8, 12, 7)
    assert (L.READY_SOFT, L.READY_HARD, L.READY_SNAP, L.READY_UPDATES) == (K.SOFT, K.HARD, K.SNAP, K.UPDATES) == \
        (1, 2, 4, 8)
    assert (R.SAVE_ENTRY, R.SAVE_STATE, R.SAVE_CUT) == (K.SAVE_ENTRY, K.SAVE_STATE, K.SAVE_CUT) == (2, 3, 4)
    assert (L.PANIC_BOUNDS, L.UNSUPPORTED_ENCODING, L.E_INVAL, L.E_NOMEM) == \
        (K.PANIC_BOUNDS, K.UNSUPPORTED, K.E_INVAL, K.E_NOMEM)
    import etcd_amd
    assert etcd_amd.ready_batch is R.ready_batch and etcd_amd.ready_batch_device is R.ready_batch_device


def test_null_ctx_is_inval():
    ns, nr = C.c_uint64(7), C.c_uint64(7)
    assert L.lib.eready_batch_device(None, None, None, None, None, 0, None, None, 0, None, 0, None, None, 0,
                                     C.byref(ns), C.byref(nr)) == L.E_INVAL
    assert (ns.value, nr.value) == (0, 0)


def test_packers():
    from etcd_amd import raftready as R
    rows = R.pack_rstate([dict(hs_term=1, hs_vote=2, hs_commit=3, lead=4, state="leader", snapi=6, applied=7,
                               soft_dirty=1), dict(), dict(state=1, applied=M64)])
    s = L.ReadyState.from_buffer_copy(rows[0].tobytes())
    assert (s.hs_term, s.hs_vote, s.hs_commit, s.lead, s.state, s.snapi, s.applied, s.soft_dirty) == \
        (1, 2, 3, 4, 2, 6, 7, 1)
    assert not rows[1].any() and (int(rows[2, 4]), int(rows[2, 6])) == (1, M64)
    assert R.unpack_rstate(rows)[0] == dict(hs_term=1, hs_vote=2, hs_commit=3, lead=4, state=2, snapi=6, applied=7,
                                           soft_dirty=1)
    raw = np.array([(K.HARD | K.UPDATES) << 32 | 33, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 2], dtype=np.uint64).tobytes()
    r = L.ReadyResult.from_buffer_copy(raw)
    assert (r.status, r.flags, r.term, r.vote, r.commit, r.ents_first, r.n_ents, r.committed_first, r.n_committed,
            r.save_first, r.n_save, r.lead, r.state, r.pad) == (33, 10, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 2, 0)
    assert R.results_from(raw, 1)[0] == dict(status=33, flags=10, term=1, vote=2, commit=3, ents_first=4, n_ents=5,
                                             committed_first=6, n_committed=7, save_first=8, n_save=9, lead=10, state=2)
    # an ewal_save_rec row is the C struct
    sc = K.Scenario()
    sc.add_group([K.entry(3, 9, 1, 11, 5, 0)], term=3, vote=2, committed=0, hs_term=1)
    _, srec, _, _, _ = sc.expected()
    assert R.saves_from(srec.tobytes(), 2) == [
        dict(kind=3, etype=0, a=3, b=2, c=0, data_off=0, data_len=0, data_nil=0),
        dict(kind=2, etype=1, a=3, b=9, c=0, data_off=11, data_len=5, data_nil=0)]
    assert srec.nbytes == 2 * 56


def test_restatement_passes_the_reference_tables():
    sc, named, data = K.kat_scenario()
    names = collections.Counter(n for n, _, _, _ in named)
    assert names == dict(TestReadyContainUpdates=7, TestNode=3, TestNodeRestart=2, TestNodeCompact=3,
                         TestSoftStateEqual=5, TestIsHardStateEqual=4, TestUnstableEnts=2)
    K.check_kats(sc, named)
    assert len(data) == 3 * 8 + 7 * 3 and data.count(bytes.fromhex("0800100018012200")) == 3 and data.count(b"foo") == 7
    # TestNode's first Ready saves the HardState, then the dummy entry, the ConfChange and the empty entry
    res, srec, srows, rrows, n_ready = sc.expected()
    g = [g for n, j, g, _ in named if (n, j) == ("TestNode", 0)][0]
    first, count = int(res[g, 8]), int(res[g, 9])
    assert count == 4 and [[int(x) for x in r] for r in srec[first:first + 4]] == [
        [3, 1, 0, 2, 0, 0, 0], [2, 0, 0, 0, 0, 0, 1], [2 | 1 << 32, 1, 1, 0, 0, 8, 0], [2, 1, 2, 0, 0, 0, 1]]
    # ... and the "no third Ready" leaves every word as it was
    g = [g for n, j, g, _ in named if (n, j) == ("TestNode", 2)][0]
    pk = sc.pack()
    assert int(res[g, 0]) == 0 and np.array_equal(rrows[g], pk[3][g]) and np.array_equal(srows[g], pk[1][g])


def test_restatement_edges():
    def one(log, **kw):
        sc = K.Scenario()
        sc.add_group(log, **kw)
        out = sc.expected()
        return sc.outcomes[0], out
    two = [K.entry(1, 0), K.entry(1, 1)]
    # lastIndex + 1 wraps to 0: lo >= hi, nil -- and resetUnstable stores the wrapped 0
    o, _ = one([K.entry(1, M64)], log_offset=M64, unstable=M64)
    assert (o["status"], o["n_ents"], o["unstable"]) == (0, 0, 0)
    # an empty log at offset 0: lastIndex is 2^64 - 1, nothing is out of bounds, nextEnts indexes past ents
    o, (res, srec, srows, rrows, n_ready) = one([], committed=1, unstable=5, hs_term=9)
    assert (o["status"], o["flags"], o["n_save"], n_ready) == (K.PANIC_BOUNDS, 0, 0, 0)
    assert [int(x) for x in res[0]] == [K.PANIC_BOUNDS] + [0] * 11 and int(srows[0, 1]) == 5 and int(rrows[0, 0]) == 9
    # ... with nothing newly committed it is fine: unstableEnts' hi wraps to 0
    o, _ = one([], unstable=5)
    assert (o["status"], o["n_ents"], o["unstable"]) == (0, 0, 0)
    # an empty log at a non-zero offset: everything is out of bounds
    o, _ = one([], log_offset=7, committed=9, applied=7, unstable=7)
    assert (o["status"], o["n_ents"], o["n_committed"], o["applied"], o["unstable"]) == (0, 0, 0, 9, 7)
    # resetNextEnts applies although the slice came out nil (committed past lastIndex)
    o, _ = one(two, committed=5, applied=0, unstable=2)
    assert (o["n_committed"], o["applied"]) == (0, 5)
    # the differing all-zero HardState: no update, not accepted
    o, (_, srec, _, rrows, _) = one(two, unstable=2, hs_term=3)
    assert (o["flags"], o["n_save"], int(rrows[0, 0])) == (0, 0, 3) and len(srec) == 0
    # unstable == 0 saves the dummy entry
    o, (_, srec, _, _, _) = one(two, unstable=0)
    assert o["n_ents"] == 2 and [int(x) for x in srec[0]] == [2, 1, 0, 0, 0, 0, 1]
    # data_nil == 2 among the unstable entries only
    bad = [K.entry(1, 0), K.entry(1, 1, data_nil=2), K.entry(1, 2)]
    assert one(bad, unstable=1)[0]["status"] == K.UNSUPPORTED and one(bad, unstable=2)[0]["status"] == 0
    # a snapshot index of 0 against a non-zero snapi is no snapshot
    assert one(two, unstable=2, snapi=4)[0]["flags"] == 0
    o, (_, _, _, rrows, _) = one(two, unstable=2, snapi=4, snap_index=6)
    assert o["flags"] == K.SNAP | K.UPDATES and int(rrows[0, 5]) == 6


def test_generators_reach_every_class():
    sc = K.lattice_scenario()
    sc.expected()
    stats = collections.Counter(o["status"] for o in sc.outcomes)
    assert stats[K.PANIC_BOUNDS] >= 3 and stats[K.UNSUPPORTED] >= 5 and stats[K.OK] >= 300, stats
    tot = np.sum([K.classes_of(o) for o in sc.outcomes], axis=0)
    assert all(int(t) >= 3 for t in tot), tot
    # the class mix of the random generator: at most 10 % panicking or unsupported, every flag and both the nil
    # and the non-nil form of each view in at least 5 % of the groups
    for seed in (1, 2):
        sc = K.random_scenario(seed)
        sc.expected()
        n = len(sc.outcomes)
        tot = dict(zip(K.CLASSES, (int(t) for t in np.sum([K.classes_of(o) for o in sc.outcomes], axis=0))))
        assert tot["void"] * 10 <= n, tot
        assert all(v * 20 >= n for k, v in tot.items() if k != "void"), tot
        stats = collections.Counter(o["status"] for o in sc.outcomes)
        assert stats[K.PANIC_BOUNDS] >= 10 and stats[K.UNSUPPORTED] >= 10, stats


@pytest.fixture(scope="module")
def restated_digest():
    return K.digest(7, GROUPS)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1"] + SAN], ids=["plain", "asan_ubsan"])
def test_ready_forms(tmp_path, flags, restated_digest):
    exe = str(tmp_path / "ready_forms")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "etcd_amd", "csrc"), "-o",
                    exe, os.path.join(ROOT, "tests", "host", "ready_forms.cpp")], check=True)
    out = subprocess.run([exe, "7", str(GROUPS)], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "ok", out.stdout + out.stderr
    assert re.match(r"groups %d records \d+$" % GROUPS, lines[0])
    classes = [int(v) for _, v in re.findall(r"(\w+)=(\d+)", lines[1])]
    want, counts = restated_digest
    assert classes == counts and all(c >= 1000 for c in classes), (classes, counts)
    assert lines[2] == "digest %d" % want
