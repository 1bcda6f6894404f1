"""The seven batched raft step calls share one scratch buffer on the ctx
(step_api.hip's lstep).  On a single ctx all seven entry points run
interleaved, in three rounds, each at 257 records (two workgroups, the second
nearly empty), at 1 and at 65, so consecutive calls carve the same bytes
differently and meet each other's leftovers.  Every call is checked with its
own suite's check() against the Python restatement, bit for bit.  Every round
also holds a call that fails whole (a group claimed twice) and a size query
followed by the real call, each followed by another step on the same ctx."""
import pytest

from etcd_amd import _lib as L

import compact_cases as KC
import lead_prop_cases as KP
import lead_step_cases as KL
import log_append_cases as KA
import ready_cases as KR
import vote_step_cases as KV
import test_gpu_compact as TC
import test_gpu_follow as TF
import test_gpu_lead_prop as TP
import test_gpu_lead_step as TL
import test_gpu_log_append as TA
import test_gpu_ready as TR
import test_gpu_vote_step as TV

pytestmark = pytest.mark.gpu

SIZES = (257, 1, 65)


def _ready(ctx, n, seed):
    # with d_sel (the claim words are carved and used) in two rounds, without it in the middle one
    sc = KR.random_scenario(seed, groups=n)
    TR.check(ctx, sc, sel=list(range(n))[::-1] if seed != 4 else None)


# (name, the call on n records checked against its restatement)
STEPS = (
    ("log_append", lambda ctx, n, seed: TA.check(ctx, KA.random_scenario(seed, G=n + 3, n=n))),
    ("lead_step", lambda ctx, n, seed: TL.check(ctx, KL.boundary_scenario(n))),
    ("lead_prop", lambda ctx, n, seed: TP.check(ctx, KP.boundary_scenario(n))),
    ("vote_step", lambda ctx, n, seed: TV.check(ctx, KV.boundary_scenario(n))),
    ("ready", _ready),
    ("follow", lambda ctx, n, seed: TF.check(ctx, TF.boundary_scenario(n).pack())),
    ("compact", lambda ctx, n, seed: TC.check(ctx, KC.random_scenario(seed, n + 3, n))),
)


def _lead_step_twice(ctx):
    sc = KL.boundary_scenario(65)
    arrays = sc.pack()
    resps = arrays[3]
    assert resps[-1, 0] != resps[0, 0] and resps[-2, 0] != resps[0, 0]
    resps[-1, 0] = resps[0, 0]                           # a second run of the first response's group
    TL.check_fails(ctx, arrays, L.E_INVAL)


def _log_append_twice(ctx):
    arrays = KA.random_scenario(5, G=260, n=257).pack()
    apps = arrays[2]
    apps[-1, 0] = apps[0, 0]                             # in the second workgroup, claimed in the first
    TA.check_fails(ctx, arrays, L.E_INVAL)


def _compact_twice(ctx):
    a = KC.random_scenario(6, 68, 65)
    a["reqs"][-1, 0] = a["reqs"][0, 0]
    assert KC.validate(a) == KC.E_INVAL
    TC.check_fails(ctx, a, L.E_INVAL)


def _size_query(T, ctx, sc, *extra):
    """d_msgs NULL gives the totals and d_res and leaves the records alone; the real call agrees."""
    want = T.want_of(sc)
    dv = T.Dev(ctx, sc.pack(), sc.n_msgs, *extra)
    try:
        before = dv.state()
        got = dv.call(msgs=False, cap=0)
        assert got[:2] == (L.OK, sc.n_msgs)
        T.same(dv.state(), (want[0],) + tuple(before[1:]))
        assert dv.call() == got
        T.same(dv.state(), want)
    finally:
        dv.free()


def _lead_step_query(ctx):
    _size_query(TL, ctx, KL.boundary_scenario(257))


def _lead_prop_query(ctx):
    sc = KP.boundary_scenario(65)
    _size_query(TP, ctx, sc, sc.data_len_total)


def _vote_step_query(ctx):
    _size_query(TV, ctx, KV.boundary_scenario(257))


FAILS = (_lead_step_twice, _log_append_twice, _compact_twice)
QUERIES = (_lead_prop_query, _vote_step_query, _lead_step_query)


@pytest.mark.parametrize("rnd", [0, 1, 2])
def test_interleaved_steps_share_the_scratch(ctx, rnd):
    """Round rnd: the seven steps in a rotated order, step s at SIZES[(s + rnd) % 3],
    so every step meets every size over the three rounds; the failing call
    after the second step and the size query after the fifth, each with the
    remaining steps behind it."""
    for j in range(len(STEPS)):
        s = (j + 2 * rnd) % len(STEPS)
        STEPS[s][1](ctx, SIZES[(s + rnd) % 3], 3 + rnd)
        if j == 1:
            FAILS[rnd](ctx)
        if j == 4:
            QUERIES[rnd](ctx)
