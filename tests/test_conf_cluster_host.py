"""Membership end to end on the CPU: conf_cluster_cases' scenario with raft_model
for every existing call and conf_cases' restatement for the three membership
calls -- the run test_gpu_conf_cluster.py repeats on the device."""
import conf_cluster_cases as CC
import tick_cluster_cases as T


def test_membership_end_to_end_restated():
    CC.play(CC.ConfCluster(CC.RestatedChecks(), T.ModelBackend()))
