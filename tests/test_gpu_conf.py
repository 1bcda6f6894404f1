"""GPU parity of the three membership calls (econf_batch_device,
econf_scan_committed_device, econf_gate_batch_device) with the restatement in
conf_cases.py, bit for bit on every record and every output.  Every call
compares the result rows, the complete output arrays and the five group
records, and the bytes of the arrays the call may not write; d_res starts as
0xA5 bytes and an output as a canary in every word, SLACK records longer than
the call may fill, so a failing call must leave everything as it was and a
successful one the canary after its last record."""
import ctypes as C

import numpy as np
import pytest

from etcd_amd import _lib as L
from etcd_amd import raftconf as RC
from etcd_amd import raftlead as RL
from etcd_amd import raftprop as RP
from etcd_amd import raftvote as RV
from etcd_amd import wal as W

import conf_cases as K
import raft_model as R

pytestmark = pytest.mark.gpu

SLACK = 3
CANARY = 0xC0FFEE0DDEADBEEF


class Bufs:
    """Named host arrays on the device (None stays None)."""

    def __init__(self, ctx, **host):
        self.ctx, self.host = ctx, host
        self.bufs = {k: (None if v is None else RL._up(ctx, v)) for k, v in host.items()}

    def p(self, name):
        b = self.bufs[name]
        return None if b is None else b.ptr

    def state(self):
        out = {}
        for k, v in self.host.items():
            if v is None or not v.nbytes:
                out[k] = v
            else:
                out[k] = np.frombuffer(self.bufs[k].download(v.nbytes), dtype=v.dtype).reshape(v.shape)
        return out

    def free(self):
        for b in self.bufs.values():
            if b is not None:
                b.free()


def same(got, want):
    assert set(got) == set(want)
    for name in want:
        g, w = got[name], want[name]
        if g is None and w is None:
            continue
        if not np.array_equal(g, w):
            at = tuple(int(x) for x in np.argwhere(g != w)[0])
            raise AssertionError("%s differs at %r: got %#x, want %#x" % (name, at, int(g[at]), int(w[at])))


def fill(rows, words, val=None):
    if val is None:
        return np.frombuffer(b"\xa5" * (rows * words * 8), dtype=np.uint64).reshape(rows, words).copy()
    return np.full((rows, words), val, dtype=np.uint64)


# ---- econf_batch_device ---------------------------------------------------------------------------

def batch_bufs(ctx, a, reqs, cap):
    return Bufs(ctx, groups=a["groups"], pstate=a["pstate"], vstate=a["vstate"], rstate=a["rstate"],
                cstate=a["cstate"], snaps=a["snaps"], u64=a["u64"], reqs=reqs, res=fill(len(reqs), 6),
                msgs=fill(cap + SLACK, 18, CANARY))


def batch_call(b, a, rq, cap, emit=True, **kw):
    nm, nc = C.c_uint64(99), C.c_uint64(99)
    p = dict(G=len(a["groups"]), n=len(rq), n_u64=len(a["u64"]), cap=cap, msgs=b.p("msgs") if emit else None)
    for k in ("groups", "pstate", "vstate", "rstate", "cstate", "snaps", "u64", "reqs", "res"):
        p[k] = b.p(k)
    p.update(kw)
    rc = L.lib.econf_batch_device(b.ctx.handle, p["groups"], p["pstate"], p["vstate"], p["rstate"], p["cstate"], p["G"],
                                  p["snaps"], p["u64"], p["n_u64"], p["reqs"], p["n"], p["res"], p["msgs"], p["cap"],
                                  C.byref(nm), C.byref(nc))
    return rc, nm.value, nc.value


def batch_want(a, reqs, x, emit):
    msgs = fill(x["n_msgs"] + SLACK, 18, CANARY)
    if emit:
        msgs[:x["n_msgs"]] = x["msg_rows"]
    o = x["arrays"] if emit else a
    return dict(groups=o["groups"], pstate=o["pstate"], vstate=o["vstate"], rstate=o["rstate"], cstate=o["cstate"],
                snaps=a["snaps"], u64=a["u64"], reqs=reqs, res=x["res_rows"], msgs=msgs)


def check_batch(ctx, a, reqs):
    """The size query fills d_res and the counters and modifies nothing else;
    the call with the exact capacity equals the restatement.  Returns it."""
    assert K.validate_batch(a, reqs) == K.OK
    x = K.expected_batch(a, reqs)
    b = batch_bufs(ctx, a, reqs, x["n_msgs"])
    try:
        assert batch_call(b, a, reqs, 0, emit=False) == (L.OK, x["n_msgs"], x["n_changed"])
        same(b.state(), batch_want(a, reqs, x, False))
        assert batch_call(b, a, reqs, x["n_msgs"]) == (L.OK, x["n_msgs"], x["n_changed"])
        got = b.state()
    finally:
        b.free()
    same(got, batch_want(a, reqs, x, True))
    return x


def check_batch_fails(ctx, a, rq, want_rc, cap=64, **kw):
    assert kw or K.validate_batch(a, rq, cap) == want_rc
    b = batch_bufs(ctx, a, rq, cap)
    try:
        before = b.state()
        got = batch_call(b, a, rq, cap, **kw)
        after = b.state()
    finally:
        b.free()
    assert got == (want_rc, 0, 0)
    same(after, before)


def _peers(n):
    return tuple(10 + 3 * k for k in range(n))


def test_add_lattice(ctx):
    """n_peers {0, 1, 6, 7} x node {new, slot 0, last slot, own id, a removed id}: one group per pair."""
    groups, reqs, want = [], [], []
    for np_ in (0, 1, 6, 7):
        peers = _peers(np_)
        own = peers[np_ // 2] if np_ else 77
        for node in ("new", "slot0", "last", "own", "removed"):
            if node in ("slot0", "last") and not np_:
                continue
            v = dict(new=500, slot0=peers[0] if np_ else 0, last=peers[-1] if np_ else 0, own=own, removed=600)[node]
            groups.append(K.group(id=own, peers=peers, off=5, nlog=3, pending=1, state=R.LEADER, removed=(600, 601)))
            reqs.append((len(groups) - 1, K.ADD, v))
            new = v not in peers
            want.append((K.UNSUPPORTED, K.PANICKED) if new and np_ == 7 else (K.OK, K.ADDED))
    x = check_batch(ctx, K.arrays_of(groups), K.reqs_of(reqs))
    assert x["outcomes"] == want and (K.UNSUPPORTED, K.PANICKED) in want
    # the leader's own id keeps its slot and loses its match: Go's quirk
    g = [k for k, r in enumerate(reqs) if groups[r[0]]["n_peers"] == 6 and r[2] == groups[r[0]]["id"]][0]
    row = [int(v) for v in x["arrays"]["groups"][g]]
    assert row[6] == 6 and row[14 + 3] == 0 and row[21 + 3] == 8 and int(x["arrays"]["rstate"][g, 7]) == 0
    assert RC.unpack_cstate(x["arrays"]["cstate"])[g] == [600, 601]        # removed[] is not cleared


def test_remove_lattice(ctx):
    """slot (first, middle, last, own id, absent) x state {0, 1, 2} x the slot's voted bit."""
    groups, reqs, want = [], [], []
    peers = _peers(5)
    for slot in (0, 2, 4, "own", "absent"):
        for state in (0, 1, 2):
            for bit in (0, 1):
                own = peers[3] if slot == "own" else peers[1]
                k = 3 if slot == "own" else slot
                node = 900 if slot == "absent" else peers[k]
                voted = 0b10010 | ((bit << k) if slot != "absent" else 0) | (bit << 1)
                groups.append(K.group(id=own, peers=peers, pending=1, state=state, voted=voted, granted=voted & 0b10111))
                reqs.append((len(groups) - 1, K.REMOVE, node))
                hit = slot != "absent" and state == 1 and (voted >> k) & 1
                want.append((K.UNSUPPORTED, K.PANICKED) if hit else (K.OK, K.REMOVED))
    x = check_batch(ctx, K.arrays_of(groups), K.reqs_of(reqs))
    assert x["outcomes"] == want and want.count((K.UNSUPPORTED, K.PANICKED)) >= 4


def test_removed_capacity_lattice(ctx):
    """n_removed {0, 13, 14} with a new id and with a duplicate, for kinds 2 and 3."""
    groups, reqs, want = [], [], []
    for nrem in (0, 13, 14):
        rem = tuple(100 + k for k in range(nrem))
        for kind in (K.REMOVE, K.DENIED):
            for dup in (False, True):
                if dup and not nrem:
                    continue
                if kind == K.REMOVE:
                    node, own = (rem[-1] if dup else 13), 10
                else:                      # a msgDenied stores the group's own id: already there, or new
                    node, own = 10, (rem[-1] if dup else 10)
                groups.append(K.group(id=own, peers=_peers(3), removed=rem))
                reqs.append((len(groups) - 1, kind, node))
                full = nrem == 14 and not dup
                want.append((K.UNSUPPORTED, K.PANICKED) if full else
                            (K.OK, K.REMOVED if kind == K.REMOVE else K.STOPPED))
    x = check_batch(ctx, K.arrays_of(groups), K.reqs_of(reqs))
    assert x["outcomes"] == want and want.count((K.UNSUPPORTED, K.PANICKED)) == 2


@pytest.mark.parametrize("length", (1, 2, 9, 65))
def test_runs_with_a_panic_in_the_middle(ctx, length):
    """Runs of one length, scattered over the groups, each with a bad kind half way: the requests before it keep
    their effect, the rest is NOT_STEPPED."""
    groups = [K.group(id=10, peers=_peers(3), removed=(13,)) for _ in range(7)]
    reqs = []
    for g in (5, 0, 3):
        for k in range(length):
            kind, node = ((K.ADD, 500 + k % 3), (K.REMOVE, 500 + k % 3), (K.DENIED, 13), (K.DENIED, 10))[k % 4]
            if k == length // 2 and g != 3:
                kind = 9 if g == 5 else 0
            reqs.append((g, kind, node))
    x = check_batch(ctx, K.arrays_of(groups), K.reqs_of(reqs))
    acts = [act for _, act in x["outcomes"]]
    assert acts.count(K.PANICKED) == 2 and acts.count(K.NOT_STEPPED) == 2 * (length - length // 2 - 1)
    assert x["outcomes"][length // 2] == (K.PANIC_CONF_TYPE, K.PANICKED)


def test_denied_and_reload(ctx):
    """Kind 3 from a removed sender, a live sender and self; kind 4 with 0, 14 and 15 ids and with duplicates."""
    ids14, ids15 = list(range(200, 214)), list(range(200, 215))
    dups = [7, 7, 8, 7, 9, 8] * 4
    u64 = ids14 + ids15 + dups + [10]
    snaps = [(0, 0), (0, 14), (14, 15), (29, len(dups)), (29 + len(dups), 1), (0, 14)]
    groups = [K.group(id=10, peers=_peers(3), removed=(13, 10, 55)) for _ in range(6)]
    groups[4] = K.group(id=10, peers=_peers(3), removed=())
    reqs = [(0, K.DENIED, 13), (0, K.DENIED, 16), (0, K.DENIED, 10), (0, K.RELOAD, 0), (0, K.DENIED, 13),
            (1, K.RELOAD, 0), (2, K.RELOAD, 0), (2, K.ADD, 1), (3, K.RELOAD, 0), (4, K.RELOAD, 0), (5, K.DENIED, 16)]
    x = check_batch(ctx, K.arrays_of(groups, snaps=snaps, u64=u64), K.reqs_of(reqs))
    assert x["outcomes"] == [(0, K.DENIED_BACK), (0, K.STOPPED), (0, K.DENIED_BACK), (0, K.RELOADED), (0, K.STOPPED),
                             (0, K.RELOADED), (K.UNSUPPORTED, K.PANICKED), (0, K.NOT_STEPPED), (0, K.RELOADED),
                             (0, K.RELOADED), (0, K.STOPPED)]
    assert x["n_msgs"] == 1 and [int(v) for v in x["msg_rows"][0, :4]] == [8, 13, 10, 1]
    rem = RC.unpack_cstate(x["arrays"]["cstate"])
    assert rem[0] == [10] and rem[1] == ids14 and rem[2] == [13, 10, 55] and rem[3] == [7, 8, 9] and rem[4] == [10]
    assert [int(v) for v in x["arrays"]["rstate"][:, 7]] == [1, 1, 0, 1, 1, 0]


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_random_mix(ctx, seed):
    a, reqs = K.random_batch(seed, 2048, 1500)
    x = check_batch(ctx, a, reqs)
    assert len({act for _, act in x["outcomes"]}) == 7


def test_batch_nomem_inval_and_host_classes(ctx):
    def call(edit=None, reqs=((0, K.ADD, 9), (0, K.REMOVE, 2), (2, K.DENIED, 5), (2, K.DENIED, 5), (2, K.RELOAD, 0))):
        a = K.arrays_of([K.group(id=1), K.group(id=2), K.group(id=3, removed=(5,))], snaps=[None, None, (1, 2)],
                        u64=(7, 8, 9))
        if edit:
            edit(a)
        return a, K.reqs_of(reqs)

    def word(name, row, col, val):
        def f(a):
            a[name][row, col] = np.uint64(val & K.M64)
        return f
    a, reqs = call()
    assert check_batch(ctx, a, reqs)["n_msgs"] == 2
    check_batch_fails(ctx, a, reqs, L.E_NOMEM, cap=1)                       # exact: one below
    for edit in (word("groups", 0, 28, 1), word("groups", 0, 31, 1), word("pstate", 0, 3, 1), word("vstate", 2, 6, 1),
                 word("vstate", 2, 7, 1), word("cstate", 2, 15, 1), word("cstate", 0, 0, 15), word("groups", 0, 8, 1),
                 word("pstate", 2, 2, 2), word("rstate", 0, 7, 2), word("vstate", 0, 0, 3), word("vstate", 0, 4, 8),
                 word("vstate", 0, 5, 1), word("snaps", 2, 7, 3), word("snaps", 2, 6, K.M64)):
        check_batch_fails(ctx, *call(edit), L.E_INVAL)
        check_batch_fails(ctx, *call(edit), L.E_INVAL, cap=0)               # INVAL wins
    for bad in (((3, K.ADD, 1),), ((0, 1, 1), (1, 1, 1), (0, 1, 2)), ((0, 1, 1, 1),), ((0, 1, 1), (0, 1, 2, 1 << 63))):
        check_batch_fails(ctx, *call(reqs=bad), L.E_INVAL)
    check_batch_fails(ctx, a, reqs, L.E_INVAL, snaps=None)                  # kind 4 without d_snaps
    check_batch(ctx, *call(word("pstate", 1, 3, 1)))                        # a group no request names
    # on the host
    for kw in (dict(groups=None), dict(pstate=None), dict(vstate=None), dict(rstate=None), dict(cstate=None),
               dict(reqs=None), dict(res=None), dict(u64=None), dict(n=K.INT_MAX), dict(G=K.INT_MAX)):
        check_batch_fails(ctx, a, reqs, L.E_INVAL, **kw)
    b = batch_bufs(ctx, a, reqs, 4)
    try:
        for name in ("groups", "pstate", "vstate", "rstate", "cstate", "snaps", "reqs", "res", "msgs", "u64"):
            off = 4 if name == "u64" else 8
            assert batch_call(b, a, reqs, 4, **{name: C.c_void_p(b.p(name).value + off)})[0] == L.E_INVAL, name
        assert batch_call(b, a, reqs, 4, n=0) == (L.OK, 0, 0)
    finally:
        b.free()


def test_batch_host_convenience_and_repeat_calls(ctx):
    import torch
    a = K.arrays_of([K.group(id=1, peers=()), K.group(id=2, peers=(1, 2, 3), removed=(3,))])
    out = RC.conf_batch(ctx, a["groups"], a["pstate"], a["vstate"], a["rstate"], a["cstate"],
                        [(0, K.ADD, 1), (0, K.ADD, 2), (0, K.ADD, 3), dict(group=1, kind=K.DENIED, node=3)])
    assert [RC.ACTIONS[r["action"]] for r in out["res"]] == ["added", "added", "added", "denied_back"]
    assert [int(v) for v in out["groups"][0, 6:10]] == [3, 1, 2, 3] and out["n_msgs"] == 1 and out["n_changed"] == 3
    assert out["msgs"][0]["type"] == RC.MSG_DENIED and out["msgs"][0]["to"] == 3 and out["msgs"][0]["from_"] == 2
    assert L.lib.ewal_last_device_ms(ctx.handle) > 0
    assert RC.conf_batch(ctx, a["groups"], a["pstate"], a["vstate"], a["rstate"], a["cstate"], [])["n_msgs"] == 0
    big, small = K.random_batch(11, 2048, 1500), K.random_batch(12, 65, 40)
    check_batch(ctx, *big)
    check_batch(ctx, *small)
    check_batch(ctx, *K.random_batch(13, 2048, 1500))    # the same shape on fresh groups: no state is kept
    c2 = W.Context(0)
    stream = torch.cuda.Stream()
    try:
        check_batch(c2, *small)
        c2.set_stream(stream.cuda_stream)
        check_batch(c2, *big)
        check_scan(c2, K.random_scan(3, 300))
        a, recs = K.random_gate(4, 64, 300, 8, 2)
        check_gate(c2, a, recs, 2)
        assert L.lib.ewal_last_device_ms(c2.handle) > 0
        check_batch(c2, *small)
    finally:
        c2.close()
    del stream


# ---- econf_scan_committed_device ------------------------------------------------------------------

def scan_bufs(ctx, c, cap):
    return Bufs(ctx, ready=c["ready"], sel=None if c["sel"] is None else np.array(c["sel"], dtype=np.uint64),
                ents=c["ents"], data=np.frombuffer(c["data"] + b"\0" * 8, dtype=np.uint8), scan=fill(c["n"], 6),
                reqs=fill(cap + SLACK, 4, CANARY), applied=fill(cap + SLACK, 4, CANARY))


def scan_call(b, c, cap, emit=True, **kw):
    nr, ne = C.c_uint64(99), C.c_uint64(99)
    p = dict(n=c["n"], G=c["G"], n_ents=len(c["ents"]), n_data=len(c["data"]), cap=cap,
             reqs=b.p("reqs") if emit else None, applied=b.p("applied") if emit else None)
    for k in ("ready", "sel", "ents", "data", "scan"):
        p[k] = b.p(k)
    p.update(kw)
    rc = L.lib.econf_scan_committed_device(b.ctx.handle, p["ready"], p["sel"], p["n"], p["G"], p["ents"], p["n_ents"],
                                           p["data"], p["n_data"], p["scan"], p["reqs"], p["applied"], p["cap"],
                                           C.byref(nr), C.byref(ne))
    return rc, nr.value, ne.value


def scan_want(b, x, emit):
    reqs, applied = fill(x["n_reqs"] + SLACK, 4, CANARY), fill(x["n_reqs"] + SLACK, 4, CANARY)
    if emit:
        reqs[:x["n_reqs"]] = x["req_rows"]
        applied[:x["n_reqs"]] = x["applied_rows"]
    return dict(b.host, scan=x["scan_rows"], reqs=reqs, applied=applied)


def check_scan(ctx, c):
    assert K.validate_scan(c) == K.OK
    x = K.expected_scan(c)
    b = scan_bufs(ctx, c, x["n_reqs"])
    try:
        assert scan_call(b, c, 0, emit=False) == (L.OK, x["n_reqs"], x["n_entries"])
        same(b.state(), scan_want(b, x, False))
        assert scan_call(b, c, x["n_reqs"]) == (L.OK, x["n_reqs"], x["n_entries"])
        got = b.state()
    finally:
        b.free()
    same(got, scan_want(b, x, True))
    return x


def check_scan_fails(ctx, c, want_rc, cap=4096, **kw):
    b = scan_bufs(ctx, c, cap)
    try:
        before = b.state()
        got = scan_call(b, c, cap, **kw)
        after = b.state()
    finally:
        b.free()
    assert got == (want_rc, 0, 0)
    same(after, before)


def test_scan_decode_edges(ctx):
    """Every decode edge as a selection of its own, between two good entries."""
    good = K.conf_change_marshal(5, 1, 3)
    bodies = K.scan_edge_bodies()
    per = [[(1, good), (1, body), (0, b"app"), (1, good)] for _, body in bodies]
    x = check_scan(ctx, K.scan_case(per))
    st = dict(zip([name for name, _ in bodies], x["statuses"]))
    assert st["empty"] == st["nil"] == st["ten_byte_varint"] == st["repeated_field"] == st["group_depth_16"] == K.OK
    assert st["group_depth_17"] == K.UNSUPPORTED and st["context_negative"] == K.PANIC_BOUNDS
    assert st["wrong_wire_f1"] == st["wrong_wire_f4"] == K.ERR_WRONG_TYPE and st["cut_4"] == K.ERR_EOF
    rows = {name: x["scan_rows"][k] for k, (name, _) in enumerate(bodies)}
    assert int(rows["plain"][2]) == 3 and int(rows["cut_4"][2]) == 1 and int(rows["cut_4"][4]) == 1
    first = int(rows["empty"][1])
    assert [int(v) for v in x["req_rows"][first + 1]] == [0, K.ADD, 0, 0]       # ConfChange{}: addNode(0)


def test_scan_shapes(ctx):
    """n_committed of 0, 1 and 70 (a group's entries cross a wave and a workgroup), entry type 2, a bad entry in
    the middle, data_nil == 2, a selection list."""
    good = [K.conf_change_marshal(k, k & 1, k % 7, b"x" * (k % 5)) for k in range(70)]
    long_ = [(1, good[k]) if k % 3 else (0, b"kv") for k in range(70)]
    bad_mid = list(long_)
    bad_mid[35] = (1, b"\x08")
    per = [[], [(1, good[1])], long_, [], bad_mid, [(1, good[2]), (2, b""), (1, good[3])], [(0, None)],
           [(1, good[4]), (1, good[5], 2), (1, good[6])], long_, [(-1 & 0xFFFFFFFF, b"")], [(1, good[9])] * 70,
           [(1, good[7])] * 200, []]
    x = check_scan(ctx, K.scan_case(per))
    assert x["statuses"] == [0, 0, 0, 0, K.ERR_EOF, K.ERR_ENTRY_TYPE, 0, K.UNSUPPORTED, 0, K.ERR_ENTRY_TYPE, 0, 0, 0]
    assert int(x["scan_rows"][5][0]) >> 32 == 2 and int(x["scan_rows"][9][0]) >> 32 == 0xFFFFFFFF
    assert int(x["scan_rows"][4][4]) == 35 and x["n_entries"] == sum(len(p) for p in per)
    sel = [40, 3, 17, 0, 9, 22, 1, 2, 39, 5, 6, 7, 8]
    y = check_scan(ctx, K.scan_case(per, G=41, sel=sel))
    assert [int(v) for v in y["req_rows"][:, 0]] == [sel[g] for g in (int(v) for v in x["req_rows"][:, 0])]
    check_scan(ctx, K.scan_case([[], [], []]))                                    # no entry at all
    check_scan(ctx, K.scan_case([[(0, b"a")] * 3] * 300))                         # entries, no request


def test_scan_feeds_conf_batch(ctx):
    """The bootstrap: three committed ConfChangeAddNode entries per group give n_peers == 3 everywhere."""
    G = 300
    per = [[(1, K.conf_change_marshal(7 * g + k, 0, k)) for k in (1, 2, 3)] for g in range(G)]
    c = K.scan_case(per)
    out = RC.scan_committed(ctx, c["ready"], c["ents"], c["data"])
    assert out["n_reqs"] == 3 * G == out["n_entries"] and all(s["status"] == 0 and s["n_reqs"] == 3 for s in out["scan"])
    a = K.arrays_of([K.group(id=1 + g % 3, peers=()) for g in range(G)])
    x = check_batch(ctx, a, out["req_rows"])
    assert all(int(v) == 3 for v in x["arrays"]["groups"][:, 6]) and x["n_changed"] == 3 * G
    assert [int(v) for v in out["applied_rows"][4]] == [7 * 1 + 2, 100 * 1 + 2, 3, int(c["ready"][1, 6]) + 1]


@pytest.mark.parametrize("seed", (1, 2))
def test_scan_random(ctx, seed):
    x = check_scan(ctx, K.random_scan(seed, 700))
    assert {K.OK, K.ERR_EOF, K.ERR_WRONG_TYPE} <= set(x["statuses"])


def test_scan_nomem_inval_and_host_classes(ctx):
    c = K.scan_case([[(1, b"\x18\x02")], [], [(0, b"zz"), (1, None), (1, b"\x10\x01")]])
    assert check_scan(ctx, c)["n_reqs"] == 3
    check_scan_fails(ctx, c, L.E_NOMEM, cap=2)
    check_scan_fails(ctx, dict(c, sel=[0, 3, 1]), L.E_INVAL)
    check_scan_fails(ctx, dict(c, G=5), L.E_INVAL)
    for col, val in ((6, len(c["ents"]) + 1), (7, len(c["ents"])), (6, K.M64)):
        bad = dict(c, ready=c["ready"].copy())
        bad["ready"][0, col] = np.uint64(val)
        check_scan_fails(ctx, bad, L.E_INVAL)
    for col, val in ((2, 99), (3, 99), (2, K.M64), (4, 1 | 3 << 32)):
        bad = dict(c, ents=c["ents"].copy())
        bad["ents"][int(c["ready"][0, 6]), col] = np.uint64(val)
        assert K.validate_scan(bad) == K.E_INVAL
        check_scan_fails(ctx, bad, L.E_INVAL)
        check_scan_fails(ctx, bad, L.E_INVAL, cap=0)
    b = scan_bufs(ctx, c, 8)
    try:
        for kw in (dict(ready=None), dict(scan=None), dict(ents=None), dict(data=None), dict(reqs=None),
                   dict(applied=None), dict(n=K.INT_MAX, G=K.INT_MAX), dict(n_ents=K.INT_MAX)):
            assert scan_call(b, c, 8, **kw) == (L.E_INVAL, 0, 0), kw
        for name in ("ready", "scan", "reqs", "applied", "ents"):
            off = 4 if name == "ents" else 8
            assert scan_call(b, c, 8, **{name: C.c_void_p(b.p(name).value + off)})[0] == L.E_INVAL, name
        assert scan_call(b, c, 8, n=0, G=0) == (L.OK, 0, 0)
    finally:
        b.free()


# ---- econf_gate_batch_device --------------------------------------------------------------------

def gate_bufs(ctx, a, recs, pass_cap, msgs_cap):
    return Bufs(ctx, groups=a["groups"], cstate=a["cstate"], recs=recs, res=fill(len(recs), 4),
                passed=fill(pass_cap + SLACK, recs.shape[1], CANARY), msgs=fill(msgs_cap + SLACK, 18, CANARY))


def gate_call(b, a, rows, from_word, pass_cap, msgs_cap, emit=True, **kw):
    np_, nm = C.c_uint64(99), C.c_uint64(99)
    p = dict(G=len(a["groups"]), n=len(rows), rec_bytes=rows.shape[1] * 8, from_word=from_word, pass_cap=pass_cap,
             msgs_cap=msgs_cap, passed=b.p("passed") if emit else None, msgs=b.p("msgs") if emit else None)
    for k in ("groups", "cstate", "recs", "res"):
        p[k] = b.p(k)
    p.update(kw)
    rc = L.lib.econf_gate_batch_device(b.ctx.handle, p["groups"], p["cstate"], p["G"], p["recs"], p["n"],
                                       p["rec_bytes"], p["from_word"], p["res"], p["passed"], p["pass_cap"], p["msgs"],
                                       p["msgs_cap"], C.byref(np_), C.byref(nm))
    return rc, np_.value, nm.value


def gate_want(b, x, emit):
    passed = fill(x["n_pass"] + SLACK, b.host["recs"].shape[1], CANARY)
    msgs = fill(x["n_msgs"] + SLACK, 18, CANARY)
    if emit:
        passed[:x["n_pass"]] = x["pass_rows"]
        msgs[:x["n_msgs"]] = x["msg_rows"]
    return dict(b.host, res=x["res_rows"], passed=passed, msgs=msgs)


def check_gate(ctx, a, recs, from_word):
    assert K.validate_gate(a["groups"], a["cstate"], recs, recs.shape[1] * 8, from_word) == K.OK
    x = K.expected_gate(a["groups"], a["cstate"], recs, from_word)
    b = gate_bufs(ctx, a, recs, x["n_pass"], x["n_msgs"])
    try:
        assert gate_call(b, a, recs, from_word, 0, 0, emit=False) == (L.OK, x["n_pass"], x["n_msgs"])
        same(b.state(), gate_want(b, x, False))
        assert gate_call(b, a, recs, from_word, x["n_pass"], x["n_msgs"]) == (L.OK, x["n_pass"], x["n_msgs"])
        got = b.state()
    finally:
        b.free()
    same(got, gate_want(b, x, True))
    return x


def _gate_case(n, words, from_word, pattern):
    """n records over 9 groups, each with removed ids {40, its own id}; From by the pattern."""
    a = K.arrays_of([K.group(id=10 + g, term=3 + g, peers=_peers(3), removed=(40, 10 + g, 41)) for g in range(9)])
    recs = np.zeros((n, words), np.uint64)
    for i in range(n):
        g = (i * 5) % 9
        recs[i] = [g] + [(i << 8) | w for w in range(1, words)]
        if from_word != K.FROM_SELF:
            live = pattern == "all" or (pattern == "alt" and i % 2 == 0)
            recs[i, from_word] = 999 if live else (40, 41, 10 + g)[i % 3]
    if from_word == K.FROM_SELF and pattern != "none":
        a["cstate"][::(1 if pattern == "all" else 2), 0] = 1          # the own id is forgotten: the record passes
    return a, recs


@pytest.mark.parametrize("words,from_word", ((6, 1), (6, K.FROM_SELF), (8, 2), (8, K.FROM_SELF), (12, 2)))
def test_gate_pairings(ctx, words, from_word):
    for pattern in ("all", "none", "alt"):
        for n in (1, 63, 64, 65, 4097):
            a, recs = _gate_case(n, words, from_word, pattern)
            x = check_gate(ctx, a, recs, from_word)
            if pattern == "all":
                assert x["n_pass"] == n and x["n_msgs"] == 0
            if pattern == "none":
                assert x["n_pass"] == 0 and (x["n_msgs"] > 0 or from_word == K.FROM_SELF or n == 1)
    a, recs = K.random_gate(7, 64, 1000, words, from_word)
    check_gate(ctx, a, recs, from_word)


def test_gate_feeds_vote_step(ctx):
    """msgVote records through the gate; d_pass goes to evote_step_batch_device as it lies."""
    G = 70
    groups = [dict(id=1, term=2, committed=0, log_offset=0, prs=[(1, 0, 1), (2, 0, 1), (3, 0, 1)]) for _ in range(G)]
    logs = [[0] for _ in range(G)]
    state = [dict(ents_cap=4, unstable=1) for _ in range(G)]
    grows, erows = RP.pack_logs(groups, logs, state)
    srows, vrows = RP.pack_state(state), RV.pack_vstate([dict(state=0) for _ in range(G)])
    crows = RC.pack_cstate([[3] if g % 3 == 0 else [] for g in range(G)])
    msgs = []
    for g in range(G):                       # two candidates per group: runs of two, one of them removed in a third
        msgs += [dict(group=g, kind=5, from_=3, term=3, index=0, log_term=0),
                 dict(group=g, kind=5, from_=2, term=3, index=0, log_term=0)]
    recs = RV.pack_msgs(msgs)
    x = K.expected_gate(grows, crows, recs, 2)
    n_denied = len(range(0, G, 3))
    assert (x["n_pass"], x["n_msgs"]) == (2 * G - n_denied, n_denied)
    want = RV.vote_batch(ctx, groups, logs, state, [dict(state=0) for _ in range(G)],
                         [m for m, act in zip(msgs, x["actions"]) if act == K.G_PASS])
    b = Bufs(ctx, groups=grows, cstate=crows, recs=recs, res=fill(len(recs), 4), passed=fill(x["n_pass"], 8, CANARY),
             msgs=fill(x["n_msgs"], 18, CANARY), pstate=srows, vstate=vrows, ents=erows, vres=fill(x["n_pass"], 6))
    try:
        a = dict(groups=grows, cstate=crows)
        assert gate_call(b, a, recs, 2, x["n_pass"], x["n_msgs"]) == (L.OK, x["n_pass"], x["n_msgs"])
        args = (ctx, b.bufs["groups"], b.bufs["pstate"], b.bufs["vstate"], G, None, b.bufs["ents"], len(erows),
                b.bufs["passed"], x["n_pass"], b.bufs["vres"])
        total, _ = RV.vote_batch_device(*args)
        out = ctx.alloc(total * 144 + 64)
        try:
            RV.vote_batch_device(*args, out, total)
            got_msgs = RL.messages_from(out.download(total * 144), total)
        finally:
            out.free()
        got = b.state()
    finally:
        b.free()
    same(dict(passed=got["passed"], msgs=got["msgs"], res=got["res"]),
         dict(passed=x["pass_rows"], msgs=x["msg_rows"], res=x["res_rows"]))
    assert RV.results_from(got["vres"].tobytes(), x["n_pass"]) == want[0] and got_msgs == want[5]
    assert RV.unpack_vstate(got["vstate"]) == want[3]
    assert [int(v) for v in x["msg_rows"][0, :4]] == [8, 3, 1, 2]


def test_gate_nomem_inval_and_host_classes(ctx):
    a, recs = _gate_case(300, 8, 2, "alt")
    x = check_gate(ctx, a, recs, 2)

    def fails(want_rc, use_a=a, use_recs=recs, pass_cap=x["n_pass"], msgs_cap=x["n_msgs"], **kw):
        b = gate_bufs(ctx, use_a, use_recs, pass_cap, msgs_cap)
        try:
            before = b.state()
            got = gate_call(b, use_a, use_recs, kw.pop("from_word", 2), pass_cap, msgs_cap, **kw)
            after = b.state()
        finally:
            b.free()
        assert got == (want_rc, 0, 0), (got, kw)
        same(after, before)
    fails(L.E_NOMEM, pass_cap=x["n_pass"] - 1)
    fails(L.E_NOMEM, msgs_cap=x["n_msgs"] - 1)
    bad = recs.copy()
    bad[150, 0] = 9
    fails(L.E_INVAL, use_recs=bad)
    fails(L.E_INVAL, use_recs=bad, pass_cap=0, msgs_cap=0)                  # INVAL wins
    for col, val in ((0, 15), (15, 1)):
        a2 = dict(a, cstate=a["cstate"].copy())
        a2["cstate"][4, col] = val
        fails(L.E_INVAL, use_a=a2)
    for kw in (dict(rec_bytes=32), dict(rec_bytes=56), dict(rec_bytes=128), dict(from_word=0), dict(from_word=8),
               dict(groups=None), dict(cstate=None), dict(recs=None), dict(res=None), dict(passed=None),
               dict(msgs=None), dict(n=K.INT_MAX), dict(G=K.INT_MAX)):
        fails(L.E_INVAL, **kw)
    b = gate_bufs(ctx, a, recs, 300, 300)
    try:
        for name in ("groups", "cstate", "recs", "res", "passed", "msgs"):
            assert gate_call(b, a, recs, 2, 300, 300, **{name: C.c_void_p(b.p(name).value + 8)})[0] == L.E_INVAL, name
        assert gate_call(b, a, recs, 2, 300, 300, passed=C.c_void_p(b.p("recs").value + 64))[0] == L.E_INVAL
        assert gate_call(b, a, recs, 2, 300, 300, n=0) == (L.OK, 0, 0)
    finally:
        b.free()
    out = RC.gate_batch(ctx, a["groups"], a["cstate"], recs, 2)
    assert np.array_equal(out["pass_rows"], x["pass_rows"]) and out["n_msgs"] == x["n_msgs"]
    assert [r["action"] for r in out["res"]] == x["actions"]
