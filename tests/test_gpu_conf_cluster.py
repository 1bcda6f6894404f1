"""Membership end to end on the device: conf_cluster_cases' scenario with every
existing call made by the real entry points and compared with raft_model after
every call, and every membership call compared bit for bit with conf_cases'
restatement (test_gpu_conf's check functions: the size query first, which must
modify nothing, then the call with exact capacities).  Every message travels
as bytes."""
import pytest

import cluster_cases as C
import conf_cluster_cases as CC
import test_gpu_conf as TG
import tick_cluster_cases as T

pytestmark = pytest.mark.gpu


class DeviceChecks:
    def __init__(self, ctx):
        self.ctx = ctx

    def check_batch(self, a, reqs):
        return TG.check_batch(self.ctx, a, reqs)

    def check_scan(self, c):
        return TG.check_scan(self.ctx, c)

    def check_gate(self, a, recs, from_word):
        return TG.check_gate(self.ctx, a, recs, from_word)


def test_membership_end_to_end(ctx):
    CC.play(CC.ConfCluster(DeviceChecks(ctx), T.DeviceBackend(ctx), C.DeviceWire(ctx)))
