"""Clusters driven by time alone, on the device: the runs of
test_tick_cluster_host.py with every call made by the real entry points -- the
tick peeked first, which must modify nothing -- and after every call every
array, result row and output row compared bit for bit with raft_model's.  Every
msgHup the election call steps and every msgBeat the leader call steps is a row
of etick_batch_device's output; the coverage conditions hold on the model and
so, by construction, on the device.  Every message travels as bytes."""
import pytest

import cluster_cases as C
import tick_cluster_cases as T
from test_tick_cluster_host import TIMED

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nodes,clusters,seed,intervals", TIMED)
def test_timed_clusters(ctx, nodes, clusters, seed, intervals):
    cl = T.play_timed(nodes, clusters, T.DeviceBackend(ctx), intervals, seed, wire=C.DeviceWire(ctx))
    T.timed_conditions(cl)
    assert cl.needed == intervals
