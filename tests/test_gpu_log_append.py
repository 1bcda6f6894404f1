"""GPU parity of the batched follower append (elog_append_batch_device) with
the restatement of raftLog.maybeAppend / handleAppendEntries in
log_append_cases.py (raft/log.go:49-84, raft/raft.go:410-416).  Every call
compares d_res, the complete d_groups array, the complete d_terms array
(pre-filled with a canary in every word no log owns) and d_resp; d_res and
d_resp start as 0xA5 bytes, so a failing call must leave all four as they
were."""
import collections
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from etcd_amd import _lib as L
from etcd_amd import raftcommit as RC
from etcd_amd import raftlog as R
from etcd_amd import raftmsg as M
from etcd_amd import wal as W

import log_append_cases as K

pytestmark = pytest.mark.gpu

U64 = K.M64


class Dev:
    """One call's arrays on the device."""

    def __init__(self, ctx, arrays):
        self.ctx = ctx
        self.grows, self.terms, self.arows, self.erows = arrays
        self.G, self.nt, self.n, self.ne = len(self.grows), len(self.terms), len(self.arows), len(self.erows)
        self.fill_res = np.frombuffer(b"\xa5" * (self.n * 48), dtype=np.uint64).reshape(self.n, R.RESULT_WORDS)
        self.fill_resp = np.frombuffer(b"\xa5" * (self.n * 144), dtype=np.uint64).reshape(self.n, R.RESP_WORDS)
        self.bufs = [R._up(ctx, a) for a in (self.grows, self.terms, self.arows, self.erows, self.fill_res,
                                             self.fill_resp)]

    def call(self, G=None, n=None, ne=None, nt=None, resp=True):
        acc, app = C.c_uint64(99), C.c_uint64(99)
        b = self.bufs
        rc = L.lib.elog_append_batch_device(self.ctx.handle, b[0].ptr, self.G if G is None else G, b[1].ptr,
                                            self.nt if nt is None else nt, b[2].ptr, self.n if n is None else n,
                                            b[3].ptr, self.ne if ne is None else ne, b[4].ptr,
                                            b[5].ptr if resp else None, C.byref(acc), C.byref(app))
        return rc, acc.value, app.value

    def state(self):
        b = self.bufs

        def get(buf, like):
            return np.frombuffer(buf.download(like.nbytes), dtype=np.uint64).reshape(like.shape)
        return get(b[4], self.fill_res), get(b[0], self.grows), get(b[1], self.terms), get(b[5], self.fill_resp)

    def free(self):
        for b in self.bufs:
            b.free()


def same(got, want):
    for name, g, w in zip(("d_res", "d_groups", "d_terms", "d_resp"), got, want):
        if not np.array_equal(g, w):
            at = tuple(int(x) for x in np.argwhere(g != w)[0])
            raise AssertionError("%s differs at %r: got %#x, want %#x" % (name, at, int(g[at]), int(w[at])))


def check(ctx, sc, resp=True):
    """The call on sc equals the restatement; returns the outcomes."""
    want = sc.expected()
    dv = Dev(ctx, sc.pack())
    try:
        rc, acc, app = dv.call(resp=resp)
        got = dv.state()
    finally:
        dv.free()
    assert rc == L.OK
    same(got, want if resp else want[:3] + (dv.fill_resp,))
    assert acc == sum(o["accepted"] for o in sc.outcomes) and app == sum(o["n_app"] for o in sc.outcomes)
    return sc.outcomes


def check_fails(ctx, arrays, want_rc, **kw):
    """The call fails with want_rc and leaves all four arrays as they were."""
    dv = Dev(ctx, arrays)
    try:
        before = dv.state()
        rc, acc, app = dv.call(**kw)
        after = dv.state()
    finally:
        dv.free()
    assert (rc, acc, app) == (want_rc, 0, 0)
    same(after, before)


def test_kats(ctx):
    sc = K.kat_scenario()
    outs = check(ctx, sc)
    assert len(outs) == 15 and [o["accepted"] for o in outs[:2]] == [0, 0]


def test_kats_between_idle_groups(ctx):
    sc = K.kat_scenario(idle=50)
    assert len(sc.groups) == 65 and len(sc.apps) == 15
    check(ctx, sc)


def test_length_lattice(ctx):
    ls = K.lattice_lengths(R.LANE_MAX)
    assert ls[0] < R.LANE_MAX < ls[-1]
    sc = K.lattice_scenario(ls)
    outs = check(ctx, sc)
    mix = collections.Counter(K.classify(o) for o in outs)
    assert mix["noop"] >= len(ls) and mix["conflict"] >= 2 * (len(ls) - 1) and mix["extension"] >= len(ls) - 1
    assert set(mix) == {"noop", "conflict", "extension"}
    check(ctx, sc, resp=False)


def test_log_window_edges(ctx):
    sc = K.Scenario()
    big = (1 << 63) - 5
    # index == log_offset: matches on ents[0]; then extends / conflicts right after it
    sc.add_app(sc.add_group([7, 8, 8], log_offset=100, committed=100, unstable=103), 100, 7, 101, [8, 9, 9])
    sc.add_app(sc.add_group([7], log_offset=100, committed=100, unstable=101), 100, 7, 0, [])
    # index == lastIndex
    sc.add_app(sc.add_group([1, 2, 3], log_offset=40, committed=41, unstable=43), 42, 3, 50, [3] * 20)
    sc.add_app(sc.add_group([1, 2, 3], log_offset=40, committed=41, unstable=43), 42, 3, 50, [])
    # index == lastIndex + 1 and beyond: rejects
    sc.add_app(sc.add_group([1, 2, 3], log_offset=40), 43, 3, 50, [4])
    sc.add_app(sc.add_group([1, 2, 3], log_offset=40), U64, 3, 50, [4] * 12)
    # index < log_offset: rejects, the heartbeat index = log_term = 0 on a compacted log included
    sc.add_app(sc.add_group([1, 2, 3], log_offset=40), 39, 1, 50, [2])
    sc.add_app(sc.add_group([0, 0, 0], log_offset=40, committed=41), 0, 0, 41, [])
    sc.add_app(sc.add_group([1, 2, 3], log_offset=40), 0, 0, 50, [1] * 9)
    # a log_offset near 2^63, lane and wave paths
    sc.add_app(sc.add_group([5, 5, 6, 6], log_offset=big, committed=big + 1, unstable=big + 4), big + 1, 5, big + 9,
               [6, 7, 7])
    sc.add_app(sc.add_group([5] * 40, log_offset=big, committed=big + 1, unstable=big + 40), big + 1, 5, big + 9,
               [5] * 30 + [6] * 30)
    # index = 2^64 - 1 on a log that ends there: from wraps to 0, ci == 0 is "no conflict"
    sc.add_app(sc.add_group([3, 3], log_offset=U64 - 1, committed=U64 - 1, unstable=0), U64, 3, U64, [9, 9])
    sc.add_app(sc.add_group([3, 3], log_offset=U64 - 1, committed=U64 - 1, unstable=0), U64, 3, U64, [9] * 11)
    # ... and one before the end: the entries run up to 2^64 - 1 and past it
    sc.add_app(sc.add_group([3, 3, 3], log_offset=U64 - 2, committed=U64 - 2, unstable=U64), U64 - 1, 3, U64, [3])
    sc.add_app(sc.add_group([3, 3, 4], log_offset=U64 - 2, committed=U64 - 2, unstable=U64), U64 - 1, 3, U64, [3, 9, 9])
    outs = check(ctx, sc)
    want = ["conflict", "noop", "extension", "noop", "reject", "reject", "reject", "reject", "reject", "conflict",
            "conflict", "noop", "noop", "noop", "conflict"]
    assert [K.classify(o) for o in outs] == want
    assert outs[11]["last_index"] == U64 and outs[14]["conflict"] == U64


def test_commit_rule(ctx):
    sc = K.Scenario()
    for ents in ([], [2, 2], [2] * 12):
        lastnewi = 3 + len(ents)
        # commit < lastnewi; commit > lastnewi; commit < committed
        for commit, committed in ((lastnewi - 1 if ents else 2, 1), (lastnewi + 5, 1), (1, 2)):
            g = sc.add_group([1, 1, 1, 2], log_offset=0, committed=committed, unstable=4)
            sc.add_app(g, 3, 2, commit, ents)
    outs = check(ctx, sc)
    got = [o["committed"] for o in outs]
    assert got == [2, 3, 2, 4, 5, 2, 14, 15, 2]


def test_panics_leave_their_group_alone(ctx):
    sc = K.Scenario()
    sc.add_app(sc.add_group([1, 1, 1, 1], committed=2, unstable=4), 1, 1, 9, [2])             # ci = 2 <= committed
    sc.add_app(sc.add_group([1, 1, 1, 1], committed=2, unstable=4), 2, 1, 9, [2])             # ci = 3: proceeds
    sc.add_app(sc.add_group([1] * 30, committed=20, unstable=30), 1, 1, 9, [1] * 18 + [2] * 4)   # ci = 20, wave path
    sc.add_app(sc.add_group([1] * 30, committed=20, unstable=30), 1, 1, 9, [1] * 19 + [2] * 4)   # ci = 21: proceeds
    sc.add_app(sc.add_group([], cap=4), 0, 0, 0, [])                                          # nlog == 0, offset 0
    sc.add_app(sc.add_group([], cap=12), 5, 0, 0, [1] * 10)
    sc.add_app(sc.add_group([], log_offset=3, cap=4), 3, 0, 0, [1])                           # nlog == 0: rejects
    outs = check(ctx, sc)
    assert [o["status"] for o in outs] == [38, 0, 38, 0, 33, 33, 0]
    assert [o["accepted"] for o in outs] == [0, 1, 0, 1, 0, 0, 0]
    check(ctx, sc, resp=False)


def _thousand():
    sc = K.Scenario()
    for g in range(1000):
        sc.add_group([1, 2], log_offset=g, committed=g, unstable=g + 2, room=2)
        sc.add_app(g, g + 1, 2, g + 2, [3] if g % 3 else [])
    return sc


def test_whole_call_failures(ctx):
    sc = _thousand()
    check(ctx, sc)
    # a duplicate group as the first and last messages of a 1000-message call
    grows, terms, arows, erows = sc.pack()
    arows[999, 0] = arows[0, 0]
    check_fails(ctx, (grows, terms, arows, erows), L.E_INVAL)
    # group == G
    grows, terms, arows, erows = sc.pack()
    arows[500, 0] = 1000
    check_fails(ctx, (grows, terms, arows, erows), L.E_INVAL)
    check_fails(ctx, sc.pack(), L.E_INVAL, G=999)
    # an entry range one past n_ents_total; a wrapping range
    check_fails(ctx, sc.pack(), L.E_INVAL, ne=len(erows) - 1)
    grows, terms, arows, erows = sc.pack()
    arows[998, 5], arows[998, 6] = len(erows), 1
    check_fails(ctx, (grows, terms, arows, erows), L.E_INVAL)
    arows[998, 5], arows[998, 6] = np.uint64(U64), 2
    check_fails(ctx, (grows, terms, arows, erows), L.E_INVAL)
    # a term window outside n_terms, and one that wraps
    check_fails(ctx, sc.pack(), L.E_INVAL, nt=len(terms) - 1)
    grows, terms, arows, erows = sc.pack()
    grows[7, 6] = np.uint64(U64 - 1)
    check_fails(ctx, (grows, terms, arows, erows), L.E_INVAL)
    # nlog > terms_cap
    grows, terms, arows, erows = sc.pack()
    grows[3, 5] = grows[3, 7] + np.uint64(1)
    check_fails(ctx, (grows, terms, arows, erows), L.E_INVAL)
    # the host's own checks
    check_fails(ctx, sc.pack(), L.E_INVAL, n=(1 << 31) - 1)
    check_fails(ctx, sc.pack(), L.E_INVAL, G=(1 << 31) - 1)
    check(ctx, sc)


def test_nomem_is_exact(ctx):
    def build(cap):
        sc = K.Scenario()
        for g in range(70):
            sc.add_group([1, 2, 3], log_offset=5, committed=5, unstable=8, room=4)
            sc.add_app(g, 7, 3, 0, [4])
        g = sc.add_group([1, 2, 3], log_offset=5, committed=5, unstable=8, cap=cap)
        sc.add_app(g, 5, 1, 0, [2, 9], grow=False)    # conflict at 7: leaves 4 entries, the bound is nlog + n_ents = 5
        g = sc.add_group([1] * 20, log_offset=5, committed=5, unstable=8, cap=20 + cap + 6)
        sc.add_app(g, 24, 1, 0, [2] * (cap + 6), grow=False)
        return sc
    check_fails(ctx, build(4).pack(), L.E_NOMEM)      # nlog + n_ents == terms_cap + 1
    check(ctx, build(5))


@pytest.mark.parametrize("seed", [1, 2])
def test_random(ctx, seed):
    sc = K.random_scenario(seed)
    outs = check(ctx, sc)
    mix = collections.Counter(K.classify(o) for o in outs)
    for cls in ("reject", "noop", "extension", "conflict"):
        assert mix[cls] >= 150, mix


def test_shared_entry_range(ctx):
    """A leader's fan-out: several followers' messages name one entry range."""
    sc = K.Scenario()
    shared = [4, 4, 5] + [5] * 17
    logs = ([1, 4], [1, 4, 4, 4], [1, 4, 3, 3, 3], [1, 3], [1, 4, 4, 4, 5] + [5] * 20)
    first = None
    for k, terms in enumerate(logs):
        g = sc.add_group(terms, log_offset=10, committed=11, unstable=10 + len(terms), room=len(shared))
        if first is None:
            first = sc.add_app(g, 11, 4, 30, shared)
        else:
            sc.add_app(g, 11, 4, 30, ents_at=(0, len(shared)), grow=False)
            sc.add_app(sc.add_group(terms, log_offset=10, committed=11, unstable=10 + len(terms), room=3), 11, 4, 30,
                       ents_at=(0, 3), grow=False)
    outs = check(ctx, sc)
    assert [K.classify(o) for o in outs] == ["extension", "extension", "extension", "conflict", "conflict", "reject",
                                             "reject", "noop", "noop"]
    assert first == 0 and [o["n_app"] for o in outs] == [20, 18, 1, 20, 3, 0, 0, 0, 0]


def test_egress_pipeline(ctx):
    """d_resp goes through a size query and emsg_encode_batch_device as it is."""
    sc = K.random_scenario(7, G=300, n=200)
    res, _, _, resp = sc.expected()
    dv = Dev(ctx, sc.pack())
    out = None
    try:
        assert dv.call()[0] == L.OK
        args = (ctx, None, 0, dv.bufs[5], dv.n, dv.bufs[3], dv.ne, None, 0)
        offs, lens, total = M.encode_messages_device(*args, None, 0)
        out = ctx.alloc(total + 64)
        offs2, lens2, total2 = M.encode_messages_device(*args, out, total)
        raw = out.download(total)
    finally:
        dv.free()
        if out:
            out.free()
    assert (offs, lens, total) == (offs2, lens2, total2)
    snap = O.snapshot_marshal()
    npanic = 0
    for i, (o, k) in enumerate(zip(offs, lens)):
        r = resp[i]
        if sc.outcomes[i]["status"] != K.OK:      # 144 zero bytes: Message{}
            want = O.message_marshal(snapshot=snap)
            npanic += 1
        else:
            want = O.message_marshal(type_=4, to=int(r[1]), from_=int(r[2]), term=int(r[3]), index=int(r[5]),
                                     snapshot=snap, reject=bool(int(r[17])))
        assert raw[o:o + k] == want, i
    assert 0 < npanic < 50 and sum(1 for r in resp if int(r[17])) > 10


def _commit_records(groups, seed):
    """ecommit_group records over the followers' logs: three voters whose
    Match lie around the log's end, so the quorum index's term is one of the
    terms the append wrote."""
    rng = np.random.default_rng(seed)
    G = len(groups)
    nlog = np.array([len(g["terms"]) for g in groups], dtype=np.uint64)
    off = np.array([g["log_offset"] for g in groups], dtype=np.uint64)
    ptr = np.concatenate([[0], np.cumsum(nlog)]).astype(np.uint64)
    lt = np.array([t for g in groups for t in g["terms"]], dtype=np.uint64)
    last = off + nlog - np.uint64(1)
    match = np.stack([last - np.minimum(nlog - np.uint64(1), rng.integers(0, 3, size=G, dtype=np.uint64))
                      for _ in range(3)])
    term = np.array([g["terms"][-1] for g in groups], dtype=np.uint64)
    comm = np.array([g["committed"] for g in groups], dtype=np.uint64)
    return RC.pack_groups(match, np.full(G, 3, np.uint8), comm, term, off, ptr, lt), ptr, lt


def _run_commit(ctx, rec, ptr, lt):
    G = len(rec)
    bufs = [R._up(ctx, rec), R._up(ctx, ptr), R._up(ctx, lt), ctx.alloc(8 * G), ctx.alloc(G), ctx.alloc(G)]
    try:
        assert L.lib.ecommit_batch_rec_device(ctx.handle, G, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr,
                                              bufs[4].ptr, bufs[5].ptr, None) == 0
        return bufs[3].download(8 * G), bufs[4].download(G), bufs[5].download(G)
    finally:
        for b in bufs:
            b.free()


def test_commit_pipeline(ctx):
    """ecommit_batch_rec_device over the windows the append updated in place
    equals the same over the restatement's logs."""
    sc = K.random_scenario(11, G=600, n=500)
    _, g_want, t_want, _ = sc.expected()
    dv = Dev(ctx, sc.pack())
    try:
        assert dv.call()[0] == L.OK
        _, g_got, t_got, _ = dv.state()
    finally:
        dv.free()
    keep = [i for i, g in enumerate(R.unpack_groups(g_want, t_want)) if g["terms"]]
    got = [g for i, g in enumerate(R.unpack_groups(g_got, t_got)) if i in set(keep)]
    want = [g for i, g in enumerate(R.unpack_groups(g_want, t_want)) if i in set(keep)]
    a = _run_commit(ctx, *_commit_records(got, 3))
    b = _run_commit(ctx, *_commit_records(want, 3))
    assert a == b
    assert sum(a[1]) > 100 and not any(a[2])


def test_repeat_calls_and_set_stream(ctx):
    import torch
    big, small = K.random_scenario(5, G=2000, n=1500), K.kat_scenario(idle=3)
    check(ctx, big)
    check(ctx, small)
    check(ctx, big)
    c2 = W.Context(0)
    stream = torch.cuda.Stream()
    try:
        check(c2, small)
        c2.set_stream(stream.cuda_stream)
        check(c2, big)
        check(c2, small)
    finally:
        c2.close()
    del stream


def test_empty_call(ctx):
    sc = K.kat_scenario()
    check_fails(ctx, sc.pack(), L.OK, n=0)
    acc, app = C.c_uint64(5), C.c_uint64(5)
    assert L.lib.elog_append_batch_device(ctx.handle, None, 0, None, 0, None, 0, None, 0, None, None, C.byref(acc),
                                          C.byref(app)) == L.OK
    assert (acc.value, app.value) == (0, 0)
    assert R.append_batch(ctx, [dict(id=1, term=2)], [[0, 1, 2]], [])[0] == []


def test_append_batch_dicts(ctx):
    groups = [dict(id=11, term=2, committed=0, unstable=3, log_offset=0), dict(id=12, term=2, log_offset=0)]
    logs = [[0, 1, 2], [0, 1, 2]]
    apps = [dict(group=1, from_=5, index=3, log_term=3, commit=3),
            dict(group=0, from_=5, index=1, log_term=1, commit=3, ents=[3, 3])]
    res, new, resp = R.append_batch(ctx, groups, logs, apps)
    assert [(r["status"], r["accepted"], r["conflict"], r["n_app"], r["last_index"], r["committed"]) for r in res] == \
        [(0, 0, 0, 0, 2, 0), (0, 1, 2, 2, 3, 3)]
    assert new[0]["terms"] == [0, 1, 3, 3] and new[0]["unstable"] == 2 and new[1]["terms"] == [0, 1, 2]
    assert resp[0] == dict(type=4, to=5, from_=12, term=2, log_term=0, index=3, commit=0, reject=True, rest=[0] * 10)
    assert (resp[1]["from_"], resp[1]["index"], resp[1]["reject"]) == (11, 3, False)
