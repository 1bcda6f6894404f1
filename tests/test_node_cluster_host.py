"""StartNode -> a played cluster -> per-group WALs -> replay -> RestartNode ->
re-election, on the CPU: raft_model for every existing call, conf_cases' and
node_cases' restatements, the oracle for the WALs -- the run
test_gpu_node_cluster.py repeats on the device."""
import conf_cluster_cases as CC
import node_cluster_cases as NC
import tick_cluster_cases as T


def test_start_crash_restart_restated():
    NC.play(NC.NodeCluster(CC.RestatedChecks(), T.ModelBackend()), NC.RestatedHost())
