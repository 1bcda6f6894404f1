"""GPU parity of the batched Ready (eready_batch_device) with the restatement
of newReady, node.run's accept branch and wal.Save's record order in
ready_cases.py (raft/node.go:239-255, 332-348; wal/wal.go:281-288).  Every call
compares d_res, the complete d_save array and the two written arrays (d_pstate,
d_rstate) bit for bit, and the bytes of the arrays the call may not write
(d_groups, d_vstate, d_snaps, d_ents, d_sel); d_res starts as 0xA5 bytes and
d_save as a canary in every word, SLACK records longer than the call may fill,
so a failing call must leave everything as it was and a successful one the
canary after its last record."""
import ctypes as C

import numpy as np
import pytest

from etcd_amd import _lib as L
from etcd_amd import raftlead as R
from etcd_amd import raftprop as P
from etcd_amd import raftready as RD
from etcd_amd import wal as W

import ready_cases as K
import vote_step_cases as KV

pytestmark = pytest.mark.gpu

SLACK = 3
CANARY = 0xC0FFEE0DDEADBEEF
NAMES = ("d_res", "d_save", "d_pstate", "d_rstate", "d_groups", "d_vstate", "d_snaps", "d_ents", "d_sel")


class Dev:
    """One call's arrays on the device."""

    def __init__(self, ctx, arrays, sel=None, cap=0):
        self.ctx = ctx
        self.grows, self.srows, self.vrows, self.rrows, self.nrows, self.erows = arrays
        self.sel = None if sel is None else np.array(sel, dtype=np.uint64)
        self.G, self.ne = len(self.grows), len(self.erows)
        self.n = self.G if sel is None else len(self.sel)
        self.cap = cap
        self.fill_res = np.frombuffer(b"\xa5" * (self.n * 96), dtype=np.uint64).reshape(self.n, K.RESULT_WORDS)
        self.fill_save = np.full((cap + SLACK, K.SAVE_WORDS), CANARY, dtype=np.uint64)
        self.host = (self.fill_res, self.fill_save, self.srows, self.rrows, self.grows, self.vrows, self.nrows,
                     self.erows, self.sel)
        self.bufs = [R._up(ctx, a) if a is not None else None for a in self.host]

    def call(self, save=True, **kw):
        ns, nr = C.c_uint64(99), C.c_uint64(99)
        b = self.bufs
        a = dict(G=self.G, ne=self.ne, n=self.n, cap=self.cap, sel=b[8].ptr if b[8] else None,
                 snaps=b[6].ptr if b[6] else None)
        a.update(kw)
        rc = L.lib.eready_batch_device(self.ctx.handle, b[4].ptr, b[2].ptr, b[5].ptr, b[3].ptr, a["G"], a["snaps"],
                                       b[7].ptr, a["ne"], a["sel"], a["n"], b[0].ptr, b[1].ptr if save else None,
                                       a["cap"], C.byref(ns), C.byref(nr))
        return rc, ns.value, nr.value

    def state(self):
        def get(buf, like):
            if like is None or not like.nbytes:
                return like
            return np.frombuffer(buf.download(like.nbytes), dtype=np.uint64).reshape(like.shape)
        return tuple(get(b, h) for b, h in zip(self.bufs, self.host))

    def free(self):
        for b in self.bufs:
            if b is not None:
                b.free()


def same(got, want):
    for name, g, w in zip(NAMES, got, want):
        if g is None and w is None:
            continue
        if not np.array_equal(g, w):
            at = tuple(int(x) for x in np.argwhere(g != w)[0])
            raise AssertionError("%s differs at %r: got %#x, want %#x" % (name, at, int(g[at]), int(w[at])))


def want_of(sc, sel=None, emit=True):
    """(the arrays as the device must hold them after the call, n_save, n_ready)."""
    res, srec, srows, rrows, n_ready = sc.expected(sel, emit)
    grows, srows0, vrows, rrows0, nrows, erows = sc.pack()
    full = np.full((len(srec) + SLACK, K.SAVE_WORDS), CANARY, dtype=np.uint64)
    if emit:
        full[:len(srec)] = srec
    return (res, full, srows, rrows, grows, vrows, nrows, erows,
            None if sel is None else np.array(sel, dtype=np.uint64)), len(srec), n_ready


def check(ctx, sc, sel=None):
    """The peek equals the emitting call's results and modifies nothing; the
    emitting call with save_cap == the exact total equals the restatement."""
    want, n_save, n_ready = want_of(sc, sel)
    peek, _, _ = want_of(sc, sel, emit=False)
    dv = Dev(ctx, sc.pack(), sel, n_save)
    try:
        assert dv.call(save=False) == (L.OK, n_save, n_ready)
        same(dv.state(), peek)
        assert dv.call() == (L.OK, n_save, n_ready)
        got = dv.state()
    finally:
        dv.free()
    same(got, want)
    assert np.array_equal(peek[0], want[0])
    return sc.outcomes


def check_fails(ctx, arrays, want_rc, sel=None, cap=8192, **kw):
    """The call fails with want_rc and leaves every array as it was."""
    dv = Dev(ctx, arrays, sel, 8192)
    try:
        before = dv.state()
        got = dv.call(cap=cap, **kw)
        after = dv.state()
    finally:
        dv.free()
    assert got == (want_rc, 0, 0)
    same(after, before)


def test_kats(ctx):
    sc, named, _ = K.kat_scenario()
    outs = check(ctx, sc)
    K.check_kats(sc, named, {g: outs[g] for _, _, g, _ in named})
    assert len(named) == 26


def test_kats_between_idle_groups(ctx):
    sc, named, _ = K.kat_scenario(idle=3)
    assert len(sc.groups) == 4 * 26
    outs = check(ctx, sc)
    K.check_kats(sc, named, {g: outs[g] for _, _, g, _ in named})
    assert sum(1 for o in outs if o["flags"] == 0 and o["n_save"] == 0) >= 3 * 26


def test_lattice(ctx):
    sc = K.lattice_scenario()
    outs = check(ctx, sc)
    assert {o["status"] for o in outs} == {K.OK, K.PANIC_BOUNDS, K.UNSUPPORTED}
    sc.with_snaps = False                                  # d_snaps == NULL: every snapshot index is 0
    outs = check(ctx, sc)
    assert not any(o["flags"] & K.SNAP for o in outs)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_selection_sizes(ctx, n):
    sc = K.random_scenario(3, groups=n)
    check(ctx, sc)
    check(ctx, sc, sel=list(range(n))[::-1])


def test_run_lengths(ctx):
    lengths = [0, 1, 2, 63, 64, 65, 300]
    outs = check(ctx, K.run_scenario(lengths))
    assert [o["n_ents"] for o in outs] == lengths
    outs = check(ctx, K.run_scenario(lengths[::-1], idle_between=70))
    assert sorted(o["n_ents"] for o in outs if o["n_ents"]) == lengths[1:]


def test_one_long_run_among_idle_groups(ctx):
    """5 000 unstable entries in one group, 300 idle groups around it: its records span 20 workgroups of the emit
    pass, which is wider than the counting pass's grid."""
    sc = K.Scenario()
    sc.add_idle(170)
    log = [K.entry(1 + i % 4, i, i % 2, 8 * i, i % 9, 0) for i in range(5001)]
    g = sc.add_group(log, term=4, vote=2, committed=5000, applied=17, unstable=1, hs_term=3)
    sc.add_idle(130)
    outs = check(ctx, sc)
    assert (outs[g]["n_ents"], outs[g]["n_save"], outs[g]["n_committed"]) == (5000, 5001, 4983)
    assert sum(o["n_save"] for o in outs) == 5001
    check(ctx, sc, sel=[g])
    # an entry whose Data is outside d_data, deep in the run: the wave's scan finds it
    sc.logs[g][4321][4] |= 2 << 32
    outs = check(ctx, sc)
    assert outs[g]["status"] == K.UNSUPPORTED and sum(o["n_save"] for o in outs) == 0


def test_selections(ctx):
    sc = K.random_scenario(4, groups=700)
    rng = np.random.default_rng(4)
    perm = [int(x) for x in rng.permutation(700)]
    check(ctx, sc)
    check(ctx, sc, sel=perm)
    subset = perm[:300]
    outs = check(ctx, sc, sel=subset)
    assert len(outs) == 300
    check(ctx, sc, sel=[699])
    check(ctx, sc, sel=sorted(subset))


@pytest.mark.parametrize("seed", [1, 2])
def test_random(ctx, seed):
    sc = K.random_scenario(seed)
    outs = check(ctx, sc)
    assert {o["status"] for o in outs} == {K.OK, K.PANIC_BOUNDS, K.UNSUPPORTED}


def test_nomem_is_exact(ctx):
    sc = K.random_scenario(5, groups=600)
    want, n_save, n_ready = want_of(sc)
    assert n_save > 300
    check_fails(ctx, sc.pack(), L.E_NOMEM, cap=n_save - 1)
    check_fails(ctx, sc.pack(), L.E_NOMEM, cap=0)
    dv = Dev(ctx, sc.pack(), None, n_save)
    try:
        assert dv.call(cap=n_save) == (L.OK, n_save, n_ready)
        same(dv.state(), want)
    finally:
        dv.free()
    # the peek needs no room
    dv = Dev(ctx, sc.pack(), None, n_save)
    try:
        assert dv.call(save=False, cap=0) == (L.OK, n_save, n_ready)
    finally:
        dv.free()


def _thousand():
    sc = K.Scenario()
    sc.add_idle(400)
    sc.add_group([K.entry(1, 0), K.entry(1, 1), K.entry(2, 2)], term=2, vote=1, committed=2, unstable=1)
    sc.add_idle(599)
    return sc


def test_whole_call_failures(ctx):
    sc = _thousand()
    base = sc.pack()
    sel = list(range(1000))

    def broken(which, row, word, value):
        arrays = [a.copy() if a is not None else None for a in base]
        arrays[which][row, word] = np.uint64(value)
        return tuple(arrays)
    GROUPS, PSTATE, VSTATE, RSTATE = 0, 1, 2, 3
    causes = [
        ("vstate.state > 2", broken(VSTATE, 3, 0, 3)),
        ("rstate.state > 2", broken(RSTATE, 999, 4, 3)),
        ("soft_dirty > 1", broken(RSTATE, 400, 7, 2)),
        ("group.reserved[0]", broken(GROUPS, 300, 28, 1)),
        ("group.reserved[3]", broken(GROUPS, 0, 31, 1 << 63)),
        ("pstate.reserved", broken(PSTATE, 700, 3, 9)),
        ("vstate.reserved[0]", broken(VSTATE, 256, 6, 1)),
        ("vstate.reserved[1]", broken(VSTATE, 255, 7, 1)),
        ("nlog past n_ents_total", broken(GROUPS, 999, 4, 3)),
        ("ents_first past n_ents_total", broken(GROUPS, 5, 5, len(base[5]) - 1)),
        ("ents_first + nlog wraps", broken(GROUPS, 400, 5, K.M64)),
        ("nlog wraps", broken(GROUPS, 400, 4, K.M64)),
    ]
    for name, arrays in causes:
        check_fails(ctx, arrays, L.E_INVAL)
        check_fails(ctx, arrays, L.E_INVAL, save=False)
        check_fails(ctx, arrays, L.E_INVAL, cap=0)              # INVAL wins over NOMEM
    # a selected group >= G; a group selected twice (in one wave, in two workgroups)
    check_fails(ctx, base, L.E_INVAL, sel=sel[:500] + [1000])
    check_fails(ctx, base, L.E_INVAL, sel=[K.M64] + sel[:10])
    check_fails(ctx, base, L.E_INVAL, sel=sel[:20] + [7])
    check_fails(ctx, base, L.E_INVAL, sel=sel + [0])
    check_fails(ctx, base, L.E_INVAL, sel=[400, 400], cap=0)
    # a broken group that is not selected is not looked at
    sub = [g for g in sel if g != 300]
    want, n_save, n_ready = want_of(sc, sub)
    arrays = causes[3][1]
    dv = Dev(ctx, arrays, sub, n_save)
    try:
        assert dv.call() == (L.OK, n_save, n_ready)
        got = dv.state()
    finally:
        dv.free()
    same(got, want[:4] + (arrays[0],) + want[5:])
    # the host's checks: d_sel == NULL needs n == G; sizes; alignment
    check_fails(ctx, base, L.E_INVAL, n=999)
    check_fails(ctx, base, L.E_INVAL, G=1001)
    check_fails(ctx, base, L.E_INVAL, sel=sel, n=(1 << 31) - 1)
    check_fails(ctx, base, L.E_INVAL, sel=sel, G=(1 << 31) - 1)
    dv = Dev(ctx, base, sel, 64)
    try:
        before = dv.state()
        for k in (0, 1, 2, 3, 4, 5, 6):
            ptrs = [b.ptr if isinstance(b.ptr, int) else b.ptr.value for b in dv.bufs]
            ptrs[k] += 8
            ns, nr = C.c_uint64(9), C.c_uint64(9)
            rc = L.lib.eready_batch_device(ctx.handle, ptrs[4], ptrs[2], ptrs[5], ptrs[3], 1000, ptrs[6], ptrs[7], dv.ne,
                                           ptrs[8], 1000, ptrs[0], ptrs[1], 64, C.byref(ns), C.byref(nr))
            assert (rc, ns.value, nr.value) == (L.E_INVAL, 0, 0), k
        for k in (7, 8):
            ptrs = [b.ptr if isinstance(b.ptr, int) else b.ptr.value for b in dv.bufs]
            ptrs[k] += 4
            ns, nr = C.c_uint64(9), C.c_uint64(9)
            rc = L.lib.eready_batch_device(ctx.handle, ptrs[4], ptrs[2], ptrs[5], ptrs[3], 1000, ptrs[6], ptrs[7], dv.ne,
                                           ptrs[8], 1000, ptrs[0], ptrs[1], 64, C.byref(ns), C.byref(nr))
            assert (rc, ns.value, nr.value) == (L.E_INVAL, 0, 0), k
        for null in (0, 2, 3, 4, 5):
            ptrs = [b.ptr if isinstance(b.ptr, int) else b.ptr.value for b in dv.bufs]
            ptrs[null] = None
            ns, nr = C.c_uint64(9), C.c_uint64(9)
            rc = L.lib.eready_batch_device(ctx.handle, ptrs[4], ptrs[2], ptrs[5], ptrs[3], 1000, ptrs[6], ptrs[7], dv.ne,
                                           ptrs[8], 1000, ptrs[0], ptrs[1], 64, C.byref(ns), C.byref(nr))
            assert (rc, ns.value, nr.value) == (L.E_INVAL, 0, 0), null
        same(dv.state(), before)
    finally:
        dv.free()


def test_empty_call(ctx):
    sc = _thousand()
    dv = Dev(ctx, sc.pack(), [], 8)
    try:
        before = dv.state()
        assert dv.call(sel=None, n=0, G=0) == (L.OK, 0, 0)
        assert dv.call(sel=dv.bufs[0].ptr, n=0) == (L.OK, 0, 0)
        same(dv.state(), before)
    finally:
        dv.free()


def test_second_call_has_nothing(ctx):
    """Straight after an accepting call no group has updates and no record is written -- except where Go itself
    reports again: a differing all-zero HardState is never accepted but never reported either."""
    sc = K.random_scenario(6, groups=1500)
    want, n_save, n_ready = want_of(sc)
    assert n_ready > 1000
    dv = Dev(ctx, sc.pack(), None, n_save)
    try:
        assert dv.call() == (L.OK, n_save, n_ready)
        first = dv.state()
        same(first, want)
        dv.bufs[1].upload(dv.fill_save.tobytes())
        assert dv.call() == (L.OK, 0, 0)
        second = dv.state()
    finally:
        dv.free()
    res = second[0]
    ok = np.array([o["status"] == K.OK for o in sc.outcomes])
    assert not (res[ok, 0] >> np.uint64(32)).any() and not res[:, 9].any() and not res[ok, 5].any()
    assert np.array_equal(second[1], dv.fill_save)
    same((None, None) + second[2:], (None, None) + first[2:])   # nothing more to accept
    again = first[0][~ok].copy()                           # the panicking and unsupported groups answer as before,
    again[:, 8] = 0                                        # with no records before them
    assert np.array_equal(res[~ok], again) and not res[:, 8].any()


def test_host_convenience(ctx):
    groups = [dict(id=1, term=1, committed=2, prs=[(1, 2, 3)]), dict(id=1, term=1, committed=1, prs=[(1, 2, 3)])]
    logs = [[0, dict(term=1, index=1, type=1), 1], [0, 1, 1]]
    state = [dict(ents_cap=3, unstable=0), dict(ents_cap=3, unstable=3)]
    vstate = [dict(state="leader", lead=1), dict()]
    rstate = [dict(soft_dirty=1), dict(hs_term=1, hs_commit=1, applied=1)]
    for peek in (True, False):
        res, saves, s2, r2, n_ready = RD.ready_batch(ctx, groups, logs, state, vstate, rstate, sel=[1, 0], peek=peek)
        assert n_ready == 1 and [r["flags"] for r in res] == [0, L.READY_SOFT | L.READY_HARD | L.READY_UPDATES]
        assert (res[1]["term"], res[1]["vote"], res[1]["commit"], res[1]["ents_first"], res[1]["n_ents"],
                res[1]["committed_first"], res[1]["n_committed"], res[1]["n_save"]) == (1, 0, 2, 0, 3, 1, 2, 4)
        if peek:
            assert saves == [] and s2[0]["unstable"] == 0 and r2[0]["soft_dirty"] == 1
        else:
            assert [(s["kind"], s["etype"], s["a"], s["b"], s["c"]) for s in saves] == \
                [(3, 0, 1, 0, 2), (2, 0, 0, 0, 0), (2, 1, 1, 1, 0), (2, 0, 1, 2, 0)]
            assert s2[0]["unstable"] == 3 and r2[0] == dict(hs_term=1, hs_vote=0, hs_commit=2, lead=1, state=2,
                                                            snapi=0, applied=2, soft_dirty=0)
            assert r2[1] == dict(hs_term=1, hs_vote=0, hs_commit=1, lead=0, state=0, snapi=0, applied=1, soft_dirty=0)


def test_repeat_calls_and_set_stream(ctx):
    import torch
    big, small = K.random_scenario(7, groups=2000), K.kat_scenario(idle=1)[0]
    check(ctx, big)
    check(ctx, small)
    check(ctx, K.random_scenario(8, groups=2000))          # the same shape on a fresh scenario: no state is kept
    check(ctx, big, sel=list(range(0, 2000, 3)))
    c2 = W.Context(0)
    stream = torch.cuda.Stream()
    try:
        check(c2, small)
        c2.set_stream(stream.cuda_stream)
        check(c2, big)
        assert L.lib.ewal_last_device_ms(c2.handle) > 0
        check(c2, small)
    finally:
        c2.close()
    del stream


@pytest.mark.parametrize("nodes", [3, 5])
def test_step_ready_save_readall_on_the_device(ctx, nodes):
    """The loop this call exists for.  12 clusters, one group per node: the election of
    test_full_election_on_the_device with the existing calls, two proposals per leader
    (elead_local_batch_device), then Ready over every group, then per group ewal_save_device over its save
    records behind one EWAL_SAVE_CUT record with prev_crc 0 (Create's file head), then ewal_readall_device over
    those bytes: it returns rd.HardState and rd.Entries of the group."""
    from test_gpu_vote_step import gpu_call
    clusters = 12
    rng = np.random.default_rng(nodes)
    rows = [dict(peers=[[1] * int(rng.integers(1, 5))] * nodes) for _ in range(clusters)]
    states, sc, arrays, _ = KV.play_election(rows, gpu_call(ctx))
    assert states == [(KV.LEADER, 1)] * clusters
    grows, strows, vrows, erows = (a.copy() for a in arrays)
    erows[erows == np.uint64(KV.CANARY)] = 0               # the free slots
    heads = sorted(set(sc.cluster))
    G = len(grows)
    data = b"".join(b"proposal %d of group %d;" % (k, g) for g in heads for k in range(2))
    locs, off = [], 0
    for g in heads:
        for k in range(2):
            ln = len(b"proposal %d of group %d;" % (k, g))
            locs.append(dict(group=g, kind="prop", data_off=off, data_len=ln))
            off += ln
    lrows = P.pack_locals(locs)
    rrows = np.zeros((G, K.RSTATE_WORDS), dtype=np.uint64)  # node.run's start: the empty states, nothing applied
    bufs = [R._up(ctx, a) for a in (grows, strows, vrows, rrows, erows, lrows)]
    bufs += [R._up(ctx, np.frombuffer(data + b"\0" * (-len(data) % 8), dtype=np.uint64)), ctx.alloc(len(locs) * 48 + 64),
             ctx.alloc(G * 96 + 64)]
    try:
        args = (ctx, bufs[0], bufs[1], G, None, bufs[4], len(erows), len(data), bufs[5], len(locs), bufs[7])
        total, napp = P.local_batch_device(*args)
        assert napp == 2 * clusters
        bufs.append(ctx.alloc(total * 144 + 64))
        P.local_batch_device(*args, bufs[9], total)
        rargs = (ctx, bufs[0], bufs[1], bufs[2], bufs[3], G, None, bufs[4], len(erows), None, G, bufs[8])
        n_save, n_ready = RD.ready_batch_device(*rargs)
        assert n_ready == G and n_save == G + 3 * clusters  # every node's HardState; a leader's three new entries
        bufs.append(ctx.alloc((n_save + 1) * 56 + 64))
        assert RD.ready_batch_device(*rargs, bufs[10], n_save) == (n_save, n_ready)
        res = RD.results_from(bufs[8].download(G * 96), G)
        saves = np.frombuffer(bufs[10].download(n_save * 56), dtype=np.uint64).reshape(n_save, K.SAVE_WORDS)
        ents = np.frombuffer(bufs[4].download(erows.nbytes), dtype=np.uint64).reshape(-1, K.ENTRY_WORDS)
        g2 = np.frombuffer(bufs[0].download(grows.nbytes), dtype=np.uint64).reshape(-1, 32)
        v2 = np.frombuffer(bufs[2].download(vrows.nbytes), dtype=np.uint64).reshape(-1, 8)
        cut = np.array([[K.SAVE_CUT, 0, 0, 0, 0, 0, 1]], dtype=np.uint64)
        dout = ctx.alloc(1 << 16)
        bufs.append(dout)
        for g in range(G):
            r = res[g]
            assert r["status"] == L.OK and r["flags"] & L.READY_HARD
            assert (r["term"], r["vote"], r["commit"]) == (int(g2[g, 1]), int(v2[g, 1]), int(g2[g, 2]))
            assert r["n_ents"] == (3 if g in heads else 0) and r["n_save"] == r["n_ents"] + 1
            recs = np.concatenate([cut, saves[r["save_first"]:r["save_first"] + r["n_save"]]])
            drec = R._up(ctx, recs)
            try:
                out_len, crc = C.c_uint64(), C.c_uint32()
                L.check(L.lib.ewal_save_device(ctx.handle, bufs[6].ptr, len(data), drec.ptr, len(recs), 0, dout.ptr,
                                               1 << 16, C.byref(out_len), C.byref(crc), None))
            finally:
                drec.free()
            raw = dout.download(out_len.value)
            view = ents[r["ents_first"]:r["ents_first"] + r["n_ents"]]
            ri = int(view[0, 1]) if len(view) else 0
            back = W.readall_device(dout, out_len.value, ri, host_view=memoryview(raw), with_ents=True)
            assert back.status == L.OK and back.metadata is None and back.last_crc == crc.value
            assert (back.state.Term, back.state.Vote, back.state.Commit) == (r["term"], r["vote"], r["commit"])
            assert [(e.Term, e.Index, e.Type, e.Data or b"") for e in back.ents] == \
                [(int(e[0]), int(e[1]), int(e[4]) & 0xFFFFFFFF, data[int(e[2]):int(e[2]) + int(e[3])]) for e in view]
            if g in heads:
                assert [bytes(e.Data or b"") for e in back.ents[1:]] == \
                    [b"proposal %d of group %d;" % (k, g) for k in range(2)]
        # the second Ready: everything was persisted and accepted
        assert RD.ready_batch_device(*rargs, bufs[10], n_save) == (0, 0)
    finally:
        for b in bufs:
            b.free()
