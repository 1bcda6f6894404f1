"""GPU parity of the batched Tick (etick_batch_device) with the restatement of
tickElection / tickHeartbeat in tick_cases.py (raft/raft.go:287-307, 590-595,
608-617).  Every call compares d_res, the complete d_hups and d_beats arrays
and d_vstate bit for bit, and the bytes of the arrays the call may not write
(d_groups, d_sel, d_draws) -- the canary groups between the selected ones
included; d_res starts as 0xA5 bytes and the two outputs as a canary in every
word, SLACK records longer than the call may fill, so a failing call must leave
everything as it was and a successful one the canary after its last record."""
import ctypes as C

import numpy as np
import pytest

from etcd_amd import _lib as L
from etcd_amd import raftlead as R
from etcd_amd import rafttick as RT
from etcd_amd import wal as W

import tick_cases as K
import lead_prop_cases as KP
import vote_step_cases as KV
import test_gpu_lead_prop as TP
import test_gpu_vote_step as TV

pytestmark = pytest.mark.gpu

SLACK = 3
CANARY = 0xC0FFEE0DDEADBEEF
NAMES = ("d_res", "d_hups", "d_beats", "d_vstate", "d_groups", "d_sel", "d_draws")
SIZES = (1, 65, 257)    # 257: two workgroups, the second holding one record -- the cross-workgroup offsets


class Dev:
    """One call's arrays on the device."""

    def __init__(self, ctx, a, hups_cap=0, beats_cap=0):
        self.ctx, self.a = ctx, a
        self.sel = None if a["sel"] is None else np.array(a["sel"], dtype=np.uint64)
        self.draws = None if a["draws"] is None else np.array(a["draws"], dtype=np.uint64)
        self.caps = (hups_cap, beats_cap)
        self.fill_res = np.frombuffer(b"\xa5" * (a["n"] * 32), dtype=np.uint64).reshape(a["n"], K.RESULT_WORDS)
        self.fill_hups = np.full((hups_cap + SLACK, K.HUP_WORDS), CANARY, dtype=np.uint64)
        self.fill_beats = np.full((beats_cap + SLACK, K.BEAT_WORDS), CANARY, dtype=np.uint64)
        self.host = (self.fill_res, self.fill_hups, self.fill_beats, a["vstate"], a["groups"], self.sel, self.draws)
        self.bufs = [R._up(ctx, x) if x is not None else None for x in self.host]

    def call(self, emit=True, **kw):
        nh, nb = C.c_uint64(99), C.c_uint64(99)
        b, a = self.bufs, self.a
        p = dict(G=a["G"], n=a["n"], election=a["election"], heartbeat=a["heartbeat"], seed=a["seed"],
                 hups_cap=self.caps[0], beats_cap=self.caps[1], groups=b[4].ptr, vstate=b[3].ptr, res=b[0].ptr,
                 sel=b[5].ptr if b[5] else None, draws=b[6].ptr if b[6] else None,
                 hups=b[1].ptr if emit else None, beats=b[2].ptr if emit else None)
        p.update(kw)
        rc = L.lib.etick_batch_device(self.ctx.handle, p["groups"], p["vstate"], p["G"], p["sel"], p["n"],
                                      p["election"], p["heartbeat"], p["draws"], p["seed"], p["res"], p["hups"],
                                      p["hups_cap"], p["beats"], p["beats_cap"], C.byref(nh), C.byref(nb))
        return rc, nh.value, nb.value

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


def want_of(a, x, emit=True):
    """The arrays as the device must hold them after the call: the canary past the last record of either output."""
    hups = np.full((x["n_hups"] + SLACK, K.HUP_WORDS), CANARY, dtype=np.uint64)
    beats = np.full((x["n_beats"] + SLACK, K.BEAT_WORDS), CANARY, dtype=np.uint64)
    if emit:
        hups[:x["n_hups"]] = x["hups"]
        beats[:x["n_beats"]] = x["beats"]
    return (x["res_rows"], hups, beats, x["vstate"] if emit else a["vstate"], a["groups"],
            None if a["sel"] is None else np.array(a["sel"], dtype=np.uint64),
            None if a["draws"] is None else np.array(a["draws"], dtype=np.uint64))


def check(ctx, a):
    """The peek fills d_res and the counters as the real call does and modifies
    nothing else; the real call with both capacities exact equals the
    restatement.  Returns the outcomes."""
    assert K.validate(a) == K.OK
    x = K.expected(a)
    dv = Dev(ctx, a, x["n_hups"], x["n_beats"])
    try:
        assert dv.call(emit=False, hups_cap=0, beats_cap=0) == (L.OK, x["n_hups"], x["n_beats"])
        same(dv.state(), want_of(a, x, emit=False))
        assert dv.call() == (L.OK, x["n_hups"], x["n_beats"])
        got = dv.state()
    finally:
        dv.free()
    same(got, want_of(a, x))
    return x["outcomes"]


def check_fails(ctx, a, want_rc, hups_cap=8192, beats_cap=8192, **kw):
    """The call fails with want_rc and leaves every array as it was."""
    dv = Dev(ctx, a, hups_cap, beats_cap)
    try:
        before = dv.state()
        got = dv.call(**kw)
        after = dv.state()
    finally:
        dv.free()
    assert got == (want_rc, 0, 0)
    same(after, before)


@pytest.mark.parametrize("pair", range(len(K.lattice_pairs())))
def test_lattice(ctx, pair):
    acts = [0] * 7
    for a in K.lattice_calls()[4 * pair:4 * pair + 4]:
        for k, v in enumerate(K.mix_of(check(ctx, a))):
            acts[k] += v
    assert all(acts[1:]), acts


@pytest.mark.parametrize("n", SIZES)
def test_lattice_chunks(ctx, n):
    for a in K.lattice_calls(chunk=n):
        assert a["n"] == n
        check(ctx, a)


@pytest.mark.parametrize("n", SIZES + (1025,))
@pytest.mark.parametrize("seed", [3, 4])
def test_random(ctx, seed, n):
    for with_sel in (False, True):
        for with_draws in (False, True):
            outs = check(ctx, K.random_scenario(seed, n, with_sel, with_draws))
            if n >= 257:
                assert all(K.mix_of(outs)[1:])


@pytest.mark.parametrize("with_sel", [False, True])
def test_all_hup_and_all_beat(ctx, with_sel):
    """Each list in turn dense while the other is empty."""
    n, G = 257, 300 if with_sel else 257
    sel = K.permuted(n, G, 5) if with_sel else None
    filler = K.canaries(G, 5) if with_sel else None
    hup = [K.group(id=7 + i, term=i % 3, peers=(1, 7 + i, 2), elapsed=19) for i in range(n)]
    outs = check(ctx, K.call_of(hup, sel=sel, G=G, filler=filler))
    assert K.mix_of(outs)[K.HUP] == n and [o["out_pos"] for o in outs] == list(range(n))
    beat = [K.group(id=7 + i, peers=(7 + i, 1, 2), state=K.LEADER, elapsed=1) for i in range(n)]
    outs = check(ctx, K.call_of(beat, sel=sel, G=G, filler=filler))
    assert K.mix_of(outs)[K.BEAT] == n and [o["out_pos"] for o in outs] == list(range(n))


def test_nomem_is_exact(ctx):
    a = K.random_scenario(6, 257, True, True)
    x = K.expected(a)
    nh, nb = x["n_hups"], x["n_beats"]
    assert nh > 10 and nb > 10
    check_fails(ctx, a, L.E_NOMEM, hups_cap=nh - 1, beats_cap=nb)
    check_fails(ctx, a, L.E_NOMEM, hups_cap=nh, beats_cap=nb - 1)
    check_fails(ctx, a, L.E_NOMEM, hups_cap=0, beats_cap=0)
    assert K.validate(a, nh - 1, nb) == K.validate(a, nh, nb - 1) == K.E_NOMEM and K.validate(a, nh, nb) == K.OK
    dv = Dev(ctx, a, nh, nb)
    try:
        assert dv.call() == (L.OK, nh, nb)
        same(dv.state(), want_of(a, x))
    finally:
        dv.free()


def test_device_inval_classes(ctx):
    def broken(edit, n=257, with_sel=True, with_draws=True):
        a = K.random_scenario(8, n, with_sel, with_draws)
        edit(a)
        assert K.validate(a, 8192, 8192) == K.E_INVAL
        return a

    def word(name, sel_pos, col, val):
        def f(a):
            g = sel_pos if a["sel"] is None else a["sel"][sel_pos]
            a[name][g, col] = np.uint64(val)
        return f

    def sel_at(i, val):
        def f(a):
            a["sel"][i] = val(a) if callable(val) else val
        return f

    def draw_at(i, val):
        def f(a):
            a["draws"][i] = val
        return f
    check_fails(ctx, broken(sel_at(3, lambda a: a["G"])), L.E_INVAL)              # a selected group >= G
    check_fails(ctx, broken(sel_at(256, K.M64)), L.E_INVAL)
    check_fails(ctx, broken(sel_at(256, lambda a: a["sel"][0])), L.E_INVAL)       # twice, across the workgroups
    check_fails(ctx, broken(sel_at(1, lambda a: a["sel"][0])), L.E_INVAL)         # ... and side by side
    for with_sel in (False, True):
        check_fails(ctx, broken(word("vstate", 70, 0, 3), with_sel=with_sel), L.E_INVAL)      # state > 2
        for col in (28, 29, 30, 31):
            check_fails(ctx, broken(word("groups", 256, col, 1), with_sel=with_sel), L.E_INVAL)   # reserved
        for col in (6, 7):
            check_fails(ctx, broken(word("vstate", 0, col, 1 << 63), with_sel=with_sel), L.E_INVAL)

        def dup(a):
            for i in range(a["n"]):
                g = i if a["sel"] is None else a["sel"][i]
                if int(a["groups"][g, 6]) >= 3:
                    a["groups"][g, 9] = a["groups"][g, 7]
                    return
        check_fails(ctx, broken(dup, with_sel=with_sel), L.E_INVAL)                # two equal peer ids
    check_fails(ctx, broken(draw_at(200, 1 << 63)), L.E_INVAL)                     # a draw >= 2^63
    check_fails(ctx, broken(draw_at(0, K.M64), n=1, with_sel=False), L.E_INVAL)
    # INVAL wins over NOMEM
    check_fails(ctx, broken(word("vstate", 5, 0, 3)), L.E_INVAL, hups_cap=0, beats_cap=0)
    # a peek fails the same way
    check_fails(ctx, broken(word("vstate", 5, 0, 3)), L.E_INVAL, emit=False)


def test_host_argument_classes(ctx):
    a = K.random_scenario(9, 65, True, True)
    dv = Dev(ctx, a, 64, 64)
    try:
        before = dv.state()
        b = dv.bufs
        for kw in (dict(groups=None), dict(vstate=None), dict(res=None), dict(hups=None), dict(beats=None),
                   dict(sel=None),                                               # d_sel NULL with n != G
                   dict(groups=b[4].ptr.value + 8), dict(vstate=b[3].ptr.value + 8), dict(res=b[0].ptr.value + 8),
                   dict(hups=b[1].ptr.value + 8), dict(beats=b[2].ptr.value + 8), dict(sel=b[5].ptr.value + 4),
                   dict(draws=b[6].ptr.value + 4), dict(n=(1 << 31) - 1), dict(G=(1 << 31) - 1), dict(election=0),
                   dict(election=-1), dict(election=1 << 31), dict(heartbeat=-1), dict(heartbeat=1 << 31)):
            assert dv.call(**kw) == (L.E_INVAL, 0, 0), kw
        nh, nb = C.c_uint64(9), C.c_uint64(9)
        assert L.lib.etick_batch_device(None, b[4].ptr, b[3].ptr, a["G"], b[5].ptr, a["n"], 10, 1, None, 0, b[0].ptr,
                                        None, 0, None, 0, C.byref(nh), C.byref(nb)) == L.E_INVAL
        assert (nh.value, nb.value) == (0, 0)
        same(dv.state(), before)
        # n == 0: EWAL_OK with both counters 0, with and without d_sel; the counters are nullable
        assert dv.call(n=0) == (L.OK, 0, 0) and dv.call(n=0, G=0, sel=None) == (L.OK, 0, 0)
        same(dv.state(), before)
        assert L.lib.etick_batch_device(ctx.handle, b[4].ptr, b[3].ptr, a["G"], b[5].ptr, a["n"], 10, 1, b[6].ptr, 0,
                                        b[0].ptr, None, 0, None, 0, None, None) == L.OK
    finally:
        dv.free()


def test_host_convenience_and_timing(ctx):
    groups = [dict(id=1, term=2, prs=[(1, 0, 1), (2, 0, 1), (3, 0, 1)]), dict(id=2, term=2, prs=[(1, 0, 1), (2, 0, 1)]),
              dict(id=9, term=2, prs=[(1, 0, 1)]), dict(id=3, term=2, prs=[(3, 0, 1)])]
    grows, _ = R.pack_groups(groups, [[0]] * 4)
    from etcd_amd import raftvote as V
    vrows = V.pack_vstate([dict(state="leader", elapsed=1), dict(elapsed=19), dict(elapsed=4), dict(elapsed=3)])
    for peek in (True, False):
        res, v2, hups, beats, nh, nb = RT.tick_batch(ctx, grows, vrows, 10, 1, sel=[3, 2, 1, 0], seed=5, peek=peek)
        assert [RT.ACTIONS[r["action"]] for r in res] == ["idle", "not_promotable", "hup", "beat"] and (nh, nb) == (1, 1)
        assert res[2]["draw"] == RT.draw(5, 2, 2, 20) and [r["elapsed"] for r in res] == [4, 0, 0, 0]
        if peek:
            assert np.array_equal(v2, vrows) and len(hups) == len(beats) == 0
        else:
            assert [int(v) for v in v2[:, 3]] == [0, 0, 0, 4]
            assert [int(v) for v in hups[0]] == [1, 0, 2, 0, 0, 0, 0, 0] and [int(v) for v in beats[0]] == [0, 1, 0, 0, 0, 0]
    assert L.lib.ewal_last_device_ms(ctx.handle) > 0
    assert RT.tick_batch(ctx, grows[:0], vrows[:0], 10, 1)[4:] == (0, 0)
    res = RT.tick_batch(ctx, grows, vrows, 10, 1, draws=[0, 9, 0, 0])[0]
    assert [RT.ACTIONS[r["action"]] for r in res] == ["beat", "hup", "not_promotable", "idle"] and res[1]["draw"] == 9


def test_repeat_calls_and_set_stream(ctx):
    import torch
    big, small = K.random_scenario(12, 2000, True, False), K.random_scenario(13, 65, False, True)
    check(ctx, big)
    check(ctx, small)
    check(ctx, K.random_scenario(14, 2000, True, False))   # the same shape on a fresh scenario: no state is kept
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


def _handed(monkeypatch, T, slot, buf):
    """T.check's Dev takes the device array `buf` as its input records (bufs[slot]) as it lies."""
    class Handed(T.Dev):
        def __init__(self, *args):
            super().__init__(*args)
            self.bufs[slot].free()
            self.bufs[slot] = buf
    monkeypatch.setattr(T, "Dev", Handed)


@pytest.mark.parametrize("n", [65, 257])
def test_hups_go_to_the_election_step_as_they_lie(ctx, monkeypatch, n):
    """Followers past the election timeout: the tick's d_hups, not downloaded,
    is evote_step_batch_device's d_in, checked with that suite's own check()."""
    def scenario(ticked):
        sc = KV.Scenario()
        for g in range(n):
            peers = [(10 * g + k, 0, 3) for k in (1, 2, 3)][:1 + g % 3]
            fires = g % 5 != 4
            sc.add_group([0, 1, 1], peers, gid=peers[g % len(peers)][0], term=1 + g % 2, committed=1,
                         elapsed=(0 if fires else 4) if ticked else (19 if fires else 3),
                         vote=peers[0][0] if g % 2 else 0)
            if ticked and fires:
                sc.add_hup(g)
        return sc
    before, after = scenario(False), scenario(True)
    grows, _, vrows, _, _, _ = before.pack()
    _, _, vrows2, _, _, mrows = after.pack()
    a = dict(groups=grows, vstate=vrows, G=n, n=n, sel=None, draws=None, seed=77, election=10, heartbeat=1)
    x = K.expected(a)
    assert x["n_hups"] == len(mrows) > n // 2 and np.array_equal(x["hups"], mrows) and np.array_equal(x["vstate"], vrows2)
    dv = Dev(ctx, a, x["n_hups"], 0)
    try:
        assert dv.call() == (L.OK, x["n_hups"], 0)
        same(dv.state(), want_of(a, x))
        hups = dv.bufs[1]
        dv.bufs[1] = None
    finally:
        dv.free()
    # the election step starts on the vote state the tick left: after's rows are exactly those
    _handed(monkeypatch, TV, 5, hups)
    outs = TV.check(ctx, after)
    assert {o["action"] for o in outs} <= {KV.CAMPAIGNED, KV.WON} and after.n_won > 0


@pytest.mark.parametrize("n", [65, 257])
def test_beats_go_to_the_leader_step_as_they_lie(ctx, monkeypatch, n):
    """Leaders past the heartbeat timeout: the tick's d_beats is
    elead_local_batch_device's d_locals, checked with that suite's own check()."""
    sc = KP.Scenario()
    fires = [g % 4 != 3 for g in range(n)]
    for g in range(n):
        sc.add_group([1, 1, 2, 2], [(1, 3, 4), (2, 0, 3), (3, 0, 4)][:1 + g % 3], gid=1, term=2, committed=2)
        if fires[g]:
            sc.add_beat(g)
    grows, _, _, _, lrows = sc.pack()
    vrows = np.zeros((n, K.VSTATE_WORDS), dtype=np.uint64)
    vrows[:, 0], vrows[:, 2] = K.LEADER, 1
    vrows[:, 3] = np.array([1 if f else 0 for f in fires], dtype=np.uint64)
    a = dict(groups=grows, vstate=vrows, G=n, n=n, sel=None, draws=None, seed=0, election=10, heartbeat=1)
    x = K.expected(a)
    assert x["n_beats"] == len(lrows) and np.array_equal(x["beats"], lrows)
    dv = Dev(ctx, a, 0, x["n_beats"])
    try:
        assert dv.call() == (L.OK, 0, x["n_beats"])
        same(dv.state(), want_of(a, x))
        beats = dv.bufs[2]
        dv.bufs[2] = None
    finally:
        dv.free()
    _handed(monkeypatch, TP, 4, beats)
    outs = TP.check(ctx, sc)
    assert {o["action"] for o in outs} == {KP.BEAT}
