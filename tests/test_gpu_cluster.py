"""The cluster tests on the device: the reference's network scenarios and the
lossy-network fuzz of test_cluster_host.py with every call made by the real
entry points (sized by the size query first, which must modify nothing), and
after every call every array, result row and emsg_out row compared bit for bit
with raft_model's, the canaries of idle groups and free window slots
included.  Every message travels as bytes: emsg_encode_batch_device after the
emitting call, emsg_decode_batch_device at the receiver, both compared with the
oracle's Marshal and Unmarshal."""
import pytest

import cluster_cases as C
from test_cluster_host import LOSSY, check_wal_sample, lossy_conditions, network_scenarios

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("copies", [1, 65])
def test_network_scenarios(ctx, copies):
    """Every call of a scenario holds one record per copy: 65 cross a wave.  The
    single copy has no idle groups around it, so its Ready is the d_sel == NULL one."""
    for sc in network_scenarios():
        cl = C.play_network(sc, C.DeviceBackend(ctx), copies=copies, wire=C.DeviceWire(ctx),
                            idle=0 if copies == 1 else 2)
        assert (cl.tally.get("ready_without_sel") == 1) == (copies == 1)


@pytest.mark.parametrize("nodes,clusters,seed,ticks,cap", LOSSY)
def test_lossy_network(ctx, nodes, clusters, seed, ticks, cap):
    cl = C.play_lossy(nodes, clusters, C.DeviceBackend(ctx), ticks, seed, cap, wire=C.DeviceWire(ctx))
    lossy_conditions(cl)
    check_wal_sample(cl, ctx)
