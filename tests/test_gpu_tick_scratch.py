"""The batched Tick carves the step scratch of the ctx (step_api.hip's lstep) as
the other step calls do.  On a single ctx the tick runs interleaved with four of
them -- the election step, the leader's local step, Ready and the compaction --
in three rounds, each call at 257 records (two workgroups, the second nearly
empty), at 1 and at 65, so consecutive calls carve the same bytes differently
and meet each other's leftovers: the claim words of a call with d_sel under the
scratch records of one without, a head record where a partial sum was.  Every
call is checked with its own suite's check() against the Python restatement,
bit for bit.  Every round also holds a tick that fails whole (a group selected
twice) and a peek, each with further steps behind it."""
import pytest

from etcd_amd import _lib as L

import compact_cases as KC
import lead_prop_cases as KP
import ready_cases as KR
import tick_cases as K
import vote_step_cases as KV
import test_gpu_compact as TC
import test_gpu_lead_prop as TP
import test_gpu_ready as TR
import test_gpu_tick as TT
import test_gpu_vote_step as TV

pytestmark = pytest.mark.gpu

SIZES = (257, 1, 65)


def _tick(with_sel, with_draws):
    return lambda ctx, n, seed: TT.check(ctx, K.random_scenario(seed, n, with_sel, with_draws))


# (name, the call on n records checked against its restatement)
STEPS = (
    ("tick", _tick(True, False)),
    ("vote_step", lambda ctx, n, seed: TV.check(ctx, KV.boundary_scenario(n))),
    ("tick_dense", _tick(False, True)),
    ("lead_prop", lambda ctx, n, seed: TP.check(ctx, KP.boundary_scenario(n))),
    ("ready", lambda ctx, n, seed: TR.check(ctx, KR.random_scenario(seed, groups=n), sel=list(range(n))[::-1])),
    ("tick_sel_draws", _tick(True, True)),
    ("compact", lambda ctx, n, seed: TC.check(ctx, KC.random_scenario(seed, n + 3, n))),
)


def _tick_twice(ctx, n):
    a = K.random_scenario(5, max(n, 2), True, False)
    a["sel"][-1] = a["sel"][0]                             # in the last workgroup, claimed in the first
    assert K.validate(a) == K.E_INVAL
    TT.check_fails(ctx, a, L.E_INVAL)


def _tick_peek(ctx, n):
    """The peek gives the totals and d_res and leaves the records alone; the real call agrees."""
    a = K.random_scenario(6, n, False, False)
    x = K.expected(a)
    dv = TT.Dev(ctx, a, x["n_hups"], x["n_beats"])
    try:
        got = dv.call(emit=False)
        assert got == (L.OK, x["n_hups"], x["n_beats"])
        TT.same(dv.state(), TT.want_of(a, x, emit=False))
        assert dv.call() == got
        TT.same(dv.state(), TT.want_of(a, x))
    finally:
        dv.free()


@pytest.mark.parametrize("rnd", [0, 1, 2])
def test_tick_shares_the_scratch(ctx, rnd):
    """Round rnd: the steps in a rotated order, step s at SIZES[(s + rnd) % 3], so
    every step meets every size over the three rounds; the failing tick after
    the second step and the peek after the fifth, each with the remaining steps
    behind it."""
    for j in range(len(STEPS)):
        s = (j + 2 * rnd) % len(STEPS)
        STEPS[s][1](ctx, SIZES[(s + rnd) % 3], 3 + rnd)
        if j == 1:
            _tick_twice(ctx, SIZES[rnd])
        if j == 4:
            _tick_peek(ctx, SIZES[(rnd + 1) % 3])
