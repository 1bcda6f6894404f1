"""CPU tests of the batched Tick: the ABI, etick_draw's pins, the restatement in
tick_cases.py against the reference's table (TestIsElectionTimeout) and its
edges, every validate class, the generators' mix, and the host program
(tests/host/tick_forms.cpp) that runs the kernels' own decision
(etcd_amd/csrc/tick_step.h) over 100 000 random ticks -- the modulo shortcut
against the plain form included -- plain and under ASan + UBSan, and prints a
digest the restatement must reproduce.  The GPU parity suite is
test_gpu_tick.py."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from etcd_amd import _lib as L
from etcd_amd import rafttick as RT

import tick_cases as K

M64, M63 = K.M64, K.M63
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
RUNS = 100000
PINS = (((0, 0, 0, 0), 0), ((1, 2, 3, 4), 0x5a86a12931d3dfc7), ((M64, M64, M64, M64), 0x343596642af3c78e))


def test_abi_sizes_and_symbols():
    assert C.sizeof(L.TickResult) == L.lib.etick_result_size() == 32
    for name in ("etick_batch_device", "etick_draw", "etick_result_size"):
        assert name in L.header_symbols() and hasattr(L.lib, name), name
    assert RT.RESULT_WORDS == K.RESULT_WORDS == 4
    assert (L.TICK_IDLE, L.TICK_HELD, L.TICK_HUP, L.TICK_BEAT, L.TICK_NOT_PROMOTABLE, L.TICK_PANICKED) == \
        (K.IDLE, K.HELD, K.HUP, K.BEAT, K.NOT_PROMOTABLE, K.PANICKED) == \
        (RT.IDLE, RT.HELD, RT.HUP, RT.BEAT, RT.NOT_PROMOTABLE, RT.PANICKED) == tuple(range(1, 7))
    assert RT.ACTIONS == K.ACTION_NAMES and len(RT.ACTIONS) == 7
    hdr = open(L.HEADER).read()
    for k, name in enumerate(("IDLE", "HELD", "HUP", "BEAT", "NOT_PROMOTABLE", "PANICKED")):
        assert "ETICK_%s = %d" % (name, k + 1) in hdr
    import etcd_amd
    assert etcd_amd.tick_batch is RT.tick_batch and etcd_amd.tick_batch_device is RT.tick_batch_device
    raw = np.array([(K.HUP << 32) | 48, 7, 3, 9], dtype=np.uint64).tobytes()
    r = L.TickResult.from_buffer_copy(raw)
    assert (r.status, r.action, r.elapsed, r.out_pos, r.draw) == (48, K.HUP, 7, 3, 9)
    assert RT.results_from(raw, 1)[0] == dict(status=48, action=K.HUP, elapsed=7, out_pos=3, draw=9)


def test_null_ctx_is_inval():
    nh, nb = C.c_uint64(7), C.c_uint64(7)
    assert L.lib.etick_batch_device(None, None, None, 0, None, 0, 10, 1, None, 0, None, None, 0, None, 0, C.byref(nh),
                                    C.byref(nb)) == L.E_INVAL
    assert (nh.value, nb.value) == (0, 0)


def test_draw_pins():
    for args, want in PINS:
        assert L.lib.etick_draw(*args) == want, args
        assert RT.draw(*args) == want and K.draw(*args) == want, args
    r = K.SplitMix(5, 0)
    for _ in range(2000):
        args = tuple(r.next() >> r.rnd(64) for _ in range(4))
        v = L.lib.etick_draw(*args)
        assert v == RT.draw(*args) == K.draw(*args) and v <= M63


def _kat_groups(elapse, ids):
    return [K.group(id=i, peers=(i,), elapsed=elapse - 1, draw=k % 10) for k, i in enumerate(ids)]


def test_restatement_passes_the_reference_table():
    """TestIsElectionTimeout: the table's elapse is the value AFTER the
    increment, so the groups start at elapse - 1."""
    kat = K.load_kats()
    t = kat["TestIsElectionTimeout"]
    assert (t["election"], t["heartbeat"]) == (kat["server"]["election"], kat["server"]["heartbeat"]) == (10, 1)
    assert [(x["elapse"], x["wprobability"]) for x in t["tests"]] == [(5, 0), (13, 0.3), (15, 0.5), (18, 0.8), (20, 1)]
    for x in t["tests"]:
        # the draws 0 .. 9, each once: the count is exact
        a = K.call_of(_kat_groups(x["elapse"], [t["id"]] * 10), t["election"], t["heartbeat"], with_draws=True)
        assert K.validate(a) == K.OK
        out = K.expected(a)
        assert out["n_hups"] == round(x["wprobability"] * 10) and out["n_beats"] == 0
        assert all(o["elapsed"] == (0 if o["action"] == K.HUP else x["elapse"]) for o in out["outcomes"])
        # the library's own draw over 10 000 nodes: the fired share rounds to the table's
        for seed, term in ((0, 0), (1, 1), (7, 5), (0xdeadbeef, 0)):
            groups = _kat_groups(x["elapse"], range(1, t["trials"] + 1))
            for g in groups:
                g["term"] = term
            out = K.expected(K.call_of(groups, t["election"], t["heartbeat"], seed=seed))
            got = out["n_hups"] / t["trials"]
            if x["round"]:
                got = math.floor(got * 10 + 0.5) / 10.0
            assert got == x["wprobability"], (x, seed, term, out["n_hups"])


def _one(election=10, heartbeat=1, with_draws=True, **kw):
    a = K.call_of([K.group(**kw)], election, heartbeat, with_draws=with_draws)
    assert K.validate(a) == K.OK
    x = K.expected(a)
    return a, x, x["outcomes"][0]


def test_restatement_edges():
    # d < 0: no draw is consumed, whatever d_draws holds
    a, x, o = _one(elapsed=8, draw=0)
    assert (o["action"], o["elapsed"], o["draw"]) == (K.IDLE, 9, 0) and x["n_hups"] == 0
    # d == 0 never fires (0 > r % election is false) but consumes the draw
    a, x, o = _one(elapsed=9, draw=M63)
    assert (o["action"], o["elapsed"], o["draw"]) == (K.HELD, 10, M63)
    a, x, o = _one(elapsed=9, draw=0)
    assert (o["action"], o["elapsed"], o["draw"]) == (K.HELD, 10, 0)
    # d == 1 fires on a draw that is 0 mod election only
    assert _one(elapsed=10, draw=20)[2]["action"] == K.HUP and _one(elapsed=10, draw=21)[2]["action"] == K.HELD
    a, x, o = _one(elapsed=10, draw=20, id=5, peers=(4, 5), term=3)
    assert [int(v) for v in x["hups"][0]] == [0, 0, 5, 0, 0, 0, 0, 0] and int(x["vstate"][0, 3]) == 0
    # d == election - 1 fires unless r % election == election - 1; d >= election always fires
    assert _one(elapsed=18, draw=9)[2]["action"] == K.HELD and _one(elapsed=18, draw=8)[2]["action"] == K.HUP
    assert _one(elapsed=19, draw=9)[2]["action"] == K.HUP and _one(elapsed=19, draw=M63)[2]["action"] == K.HUP
    # not promotable: elapsed = 0 WITHOUT the increment, at a follower and a candidate, whatever elapsed was
    for state in (K.FOLLOWER, K.CANDIDATE):
        for el in (0, 5, 19, M63, M64):
            a, x, o = _one(elapsed=el, id=9, peers=(1, 2, 3), state=state)
            assert (o["action"], o["elapsed"], o["draw"]) == (K.NOT_PROMOTABLE, 0, 0)
    assert _one(elapsed=3, id=9, peers=(), state=K.FOLLOWER)[2]["action"] == K.NOT_PROMOTABLE
    assert _one(elapsed=3, id=4, peers=(1, 2, 3, 4), n_peers=3)[2]["action"] == K.NOT_PROMOTABLE
    # ... but a leader that is not among its peers still heartbeats
    assert _one(elapsed=1, id=9, peers=(1, 2, 3), state=K.LEADER)[2]["action"] == K.BEAT
    # the 2^63 - 1 wrap: e is the most negative int.  At a leader it is not > heartbeat; at a follower d = e -
    # election wraps to a huge positive number and fires
    a, x, o = _one(elapsed=M63, state=K.LEADER)
    assert (o["action"], o["elapsed"]) == (K.IDLE, M63 + 1)
    a, x, o = _one(elapsed=M63, draw=9)
    assert (o["action"], o["elapsed"], o["draw"]) == (K.HUP, 0, 9)
    a, x, o = _one(elapsed=M63 + 1, draw=9)                # e = -(2^63 - 1): d wraps too, at election >= 2
    assert o["action"] == K.HUP
    a, x, o = _one(elapsed=M64)                            # elapsed -1: e = 0
    assert (o["action"], o["elapsed"]) == (K.IDLE, 0)
    a, x, o = _one(elapsed=M64, state=K.LEADER, heartbeat=0)
    assert (o["action"], o["elapsed"]) == (K.IDLE, 0)
    # heartbeat 0 fires every tick; heartbeat 1 every second one
    for el in (0, 1, 5):
        a, x, o = _one(elapsed=el, state=K.LEADER, heartbeat=0)
        assert (o["action"], o["elapsed"]) == (K.BEAT, 0) and [int(v) for v in x["beats"][0]] == [0, 1, 0, 0, 0, 0]
    assert _one(elapsed=0, state=K.LEADER)[2]["action"] == K.IDLE and _one(elapsed=1, state=K.LEADER)[2]["action"] == K.BEAT
    # election 1: every promotable tick reaches the draw; d == 0 holds, d >= 1 fires
    assert _one(election=1, elapsed=0, draw=5)[2]["action"] == K.HELD
    assert _one(election=1, elapsed=1, draw=5)[2]["action"] == K.HUP
    # n_peers > 7: unsupported, left as it was
    a, x, o = _one(elapsed=5, id=1, peers=(1, 2, 3, 4, 5, 6, 7), n_peers=8)
    assert (o["status"], o["action"], o["elapsed"]) == (K.UNSUPPORTED, K.PANICKED, 5)
    assert np.array_equal(x["vstate"], a["vstate"])
    # d_draws NULL: the draw is etick_draw(seed, id, term, e), and the peek agrees with the call
    a = K.call_of([K.group(id=7, term=3, peers=(7,), elapsed=14)], seed=99)
    o = K.expected(a)["outcomes"][0]
    assert o["draw"] == K.draw(99, 7, 3, 15) and o["action"] == (K.HUP if 5 > o["draw"] % 10 else K.HELD)
    assert np.array_equal(K.expected(a, emit=False)["res_rows"], K.expected(a)["res_rows"])
    assert np.array_equal(K.expected(a, emit=False)["vstate"], a["vstate"])


def test_validate_classes():
    def call(edit=None, **kw):
        groups = [K.group(id=1, peers=(1, 2, 3), elapsed=12, draw=3), K.group(id=2, peers=(1, 2, 3), state=K.LEADER, elapsed=1),
                  K.group(id=3, peers=(1, 2, 3), elapsed=3)]
        a = K.call_of(groups, with_draws=True, **kw)
        if edit:
            edit(a)
        return a

    def word(name, row, col, val):
        def f(a):
            a[name][row, col] = np.uint64(val & M64)
        return f

    def key(name, val):
        def f(a):
            a[name] = val
        return f
    assert K.validate(call()) == K.OK
    sel = dict(sel=[4, 0, 2], G=5)
    assert K.validate(call(**sel)) == K.OK
    # on the device
    assert K.validate(call(key("sel", [4, 5, 2]), **sel)) == K.E_INVAL       # a selected group >= G
    assert K.validate(call(key("sel", [4, 2, 4]), **sel)) == K.E_INVAL       # a group selected twice
    assert K.validate(call(word("vstate", 1, 0, 3))) == K.E_INVAL            # state > 2
    for col in (28, 31):
        assert K.validate(call(word("groups", 2, col, 1))) == K.E_INVAL      # elead_group.reserved
    for col in (6, 7):
        assert K.validate(call(word("vstate", 0, col, 1))) == K.E_INVAL      # evote_state.reserved
    assert K.validate(call(word("groups", 0, 9, 1))) == K.E_INVAL            # two equal peer ids
    assert K.validate(call(word("groups", 0, 10, 1))) == K.OK                # ... past n_peers: not looked at
    assert K.validate(call(key("draws", [0, 1 << 63, 0]))) == K.E_INVAL      # a draw >= 2^63, consumed or not
    assert K.validate(call(key("draws", [0, M63, 0]))) == K.OK
    assert K.validate(call(word("vstate", 1, 0, 3), **sel)) == K.OK          # a group no selection names
    # capacity: one msgHup (d = 3 > 3 % 10 is false -> held; make it fire) and one msgBeat
    a = call(key("draws", [2, 0, 0]))
    x = K.expected(a)
    assert (x["n_hups"], x["n_beats"]) == (1, 1)
    assert K.validate(a, 1, 1) == K.OK and K.validate(a, 0, 1) == K.E_NOMEM and K.validate(a, 1, 0) == K.E_NOMEM
    assert K.validate(call(word("vstate", 1, 0, 3)), 0, 0) == K.E_INVAL      # INVAL wins
    # on the host
    assert K.validate(a, 1, None) == K.E_INVAL and K.validate(a, None, 1) == K.E_INVAL
    assert K.validate(call(key("n", 2))) == K.E_INVAL                        # d_sel NULL with n != G
    for e in (0, -1, 1 << 31):
        assert K.validate(call(election=e)) == K.E_INVAL
    for h in (-1, 1 << 31):
        assert K.validate(call(heartbeat=h)) == K.E_INVAL
    assert K.validate(call(election=K.INT_MAX, heartbeat=K.INT_MAX)) == K.OK
    assert K.validate(call(lambda a: a.update(G=K.INT_MAX, n=K.INT_MAX))) == K.E_INVAL


def test_lattice_reaches_every_edge():
    acts = [0] * 7
    n_calls = 0
    for a in K.lattice_calls():
        assert K.validate(a) == K.OK
        x = K.expected(a)
        for k, v in enumerate(K.mix_of(x["outcomes"])):
            acts[k] += v
        assert x["n_hups"] == len(x["hups"]) and x["n_beats"] == len(x["beats"])
        n_calls += 1
    assert n_calls == 4 * len(K.lattice_pairs()) and all(acts[1:]), acts
    for n in (1, 65, 257):
        calls = K.lattice_calls(chunk=n)
        assert all(a["n"] == n and K.validate(a) == K.OK for a in calls)


@pytest.fixture(scope="module")
def restated_digest():
    return K.digest(7, RUNS)


def test_generator_mix(restated_digest):
    """The condition on the generators, from the restatement alone: every
    action in at least 2 % of the selections, and both forms of the timeout
    test in at least 2 % of the ticks."""
    _, acts, forms = restated_digest
    assert acts[0] == 0 and sum(acts) == RUNS
    assert all(v >= RUNS * 0.02 for v in acts[1:]), acts
    assert all(v >= RUNS * 0.02 for v in forms), forms
    for with_sel in (False, True):
        for with_draws in (False, True):
            a = K.random_scenario(11, 4000, with_sel, with_draws)
            assert K.validate(a) == K.OK
            acts = K.mix_of(K.expected(a)["outcomes"])
            assert all(v >= 4000 * 0.02 for v in acts[1:]), acts


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1"] + SAN], ids=["plain", "asan_ubsan"])
def test_tick_forms(tmp_path, flags, restated_digest):
    exe = str(tmp_path / "tick_forms")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "etcd_amd", "csrc"), "-o",
                    exe, os.path.join(ROOT, "tests", "host", "tick_forms.cpp")], check=True)
    out = subprocess.run([exe, "7", str(RUNS)], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "ok", out.stdout + out.stderr
    want, acts, forms = restated_digest
    assert lines[0] == "runs %d" % RUNS
    assert [int(v) for _, v in re.findall(r"(\w+)=(\d+)", lines[1])] == acts[1:]
    assert [int(v) for _, v in re.findall(r"(\w+)=(\d+)", lines[2])] == forms
    assert lines[3] == "pins ok"
    assert lines[4] == "digest %d" % want
