"""etcd_amd -- MI355X-native engine for etcd's WAL replay-and-verify path.

Product layout:
  csrc/        HIP kernels (gfx950) + host C++ behind the C ABI in include/ewal.h
  libewal.so   built in-tree by build.sh
  wal.py       mirror of the reference `wal` package (OpenAtIndex/ReadAll/Create/...)
  snap.py      mirror of `snap.Snapshotter` (Load / snapNames / batch verify; SaveSnap / batched save)
  raftcommit.py batched `raft.maybeCommit` (SoA arrays or 192-B group records)
  raftlog.py   batched `raft.handleAppendEntries` / `raftLog.maybeAppend` (the follower's append)
  raftlead.py  batched `stepLeader` msgAppResp case (the leader's progress, commit and next fan-out)
  raftprop.py  batched `stepLeader` msgProp / msgBeat cases (the leader's append and the round's first fan-out)
  raftvote.py  batched election step: msgHup / msgVote / msgVoteResp (campaign, the vote, poll, becomeLeader)
  raftready.py batched Ready: newReady, the accept branch and Storage.Save's records (steps -> write side)
  raftfollow.py batched follower step: msgApp / msgSnap (the term switch, maybeAppend, restore, the msgAppResp)
  raftcompact.py batched log compaction: node.Compact (raft.compact, raftLog.snap, the window's slide)
  rafttick.py  batched Tick: tickElection / tickHeartbeat (elapsed, the msgHup and msgBeat that start the steps)
  raftconf.py  batched membership: ApplyConfChange (addNode / removeNode), the removed[] gate, the ConfChange scan
  raftnode.py  batched StartNode / RestartNode: a replay's result (or a peer list) into the groups' records
  crc.py       `pkg/crc` digest (chained CRC-32C) over host or device buffers
  raftmsg.py   batched `raftpb.Message` decode (the /raft ingress) and Marshal (the egress)
  shard.py     per-rank shard assignment, the RCCL summary all-reduce and the
               torch.distributed exchange of ONE WAL's split ranges (C join)
  _lib.py      ctypes bindings of include/ewal.h
"""
from . import _lib  # noqa: F401  (fails loudly if libewal.so is missing)
from .wal import Context, OpenAtIndex, Create, Encoder, readall_bytes, synth_wal  # noqa: F401
from .snap import save_packed, save_dir, snap_name  # noqa: F401
from .raftlog import append_batch, append_batch_device  # noqa: F401
from .raftlead import lead_step_batch, lead_step_batch_device  # noqa: F401
from .raftprop import local_batch, local_batch_device  # noqa: F401
from .raftvote import vote_batch, vote_batch_device  # noqa: F401
from .raftready import ready_batch, ready_batch_device  # noqa: F401
from .raftfollow import follow_batch, follow_batch_device  # noqa: F401
from .raftcompact import compact_batch, compact_batch_device  # noqa: F401
from .rafttick import tick_batch, tick_batch_device  # noqa: F401
from .raftconf import (conf_batch, conf_batch_device, scan_committed, scan_committed_device, gate_batch,  # noqa: F401
                       gate_batch_device, pack_cstate, unpack_cstate, removed_u64)
from .raftnode import node_batch, node_batch_device, reqs_from_batch, entries_device  # noqa: F401

__all__ = ["Context", "OpenAtIndex", "Create", "Encoder", "readall_bytes", "synth_wal", "save_packed", "save_dir",
           "snap_name", "append_batch", "append_batch_device", "lead_step_batch", "lead_step_batch_device",
           "local_batch", "local_batch_device", "vote_batch", "vote_batch_device", "ready_batch",
           "ready_batch_device", "follow_batch", "follow_batch_device",
           "compact_batch", "compact_batch_device", "tick_batch", "tick_batch_device",
           "conf_batch", "conf_batch_device", "scan_committed", "scan_committed_device", "gate_batch",
           "gate_batch_device", "pack_cstate", "unpack_cstate", "removed_u64",
           "node_batch", "node_batch_device", "reqs_from_batch", "entries_device"]
