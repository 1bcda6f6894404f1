"""Batched election step on the GPU (evote_step_batch_device, include/ewal.h):
`raft.Step` for msgHup, msgVote and msgVoteResp (raft/raft.go:372-408) --
campaign, the vote, poll, becomeFollower / becomeCandidate / becomeLeader --
for runs of election messages per raft group.  The groups are raftlead's
elead_group records with raftprop's state records and one more side record
(evote_state); the msgVote / msgVoteResp fan-out and the winner's first
broadcast come back as emsg_out records that `raftmsg.encode_messages_device`
takes directly, and the winner's empty entry is appended to the device log."""
import ctypes as C

import numpy as np

from ._lib import lib, check
from .raftlead import GROUP_WORDS, ENTRY_WORDS, _u64, _up, messages_from, pack_snaps, unpack_groups  # noqa: F401
from .raftprop import STATE_WORDS, pack_logs, pack_state, unpack_state  # noqa: F401
from .raftmsg import _ptr

VSTATE_WORDS = 8   # evote_state, 64 B
MSG_IN_WORDS = 8   # evote_msg, 64 B (word 6: reject | pad << 32)
RESULT_WORDS = 6   # evote_result, 48 B (word 0: status | action << 32, word 5: state | flags << 32)
MSG_HUP, MSG_VOTE, MSG_VOTE_RESP = 0, 5, 6       # raft.msgHup, raft.msgVote, raft.msgVoteResp
FOLLOWER, CANDIDATE, LEADER = 0, 1, 2            # raft.StateType
ACTIONS = ("not_stepped", "ignored", "granted", "rejected", "campaigned", "won", "lost", "polled", "no_case",
           "panicked")
_KINDS = {"hup": MSG_HUP, "vote": MSG_VOTE, "vote_resp": MSG_VOTE_RESP}
_STATES = {"follower": FOLLOWER, "candidate": CANDIDATE, "leader": LEADER}


def pack_vstate(vstate):
    """evote_state rows: one dict (state -- 0 / 1 / 2 or its name --, vote,
    lead, elapsed, voted, granted) per group."""
    return _u64([[_STATES.get(s.get("state"), s.get("state", 0)), s.get("vote", 0), s.get("lead", 0),
                  s.get("elapsed", 0), s.get("voted", 0), s.get("granted", 0), 0, 0] for s in vstate], VSTATE_WORDS)


def unpack_vstate(rows):
    return [dict(state=int(r[0]), vote=int(r[1]), lead=int(r[2]), elapsed=int(r[3]), voted=int(r[4]),
                 granted=int(r[5])) for r in np.asarray(rows, dtype=np.uint64).reshape(-1, VSTATE_WORDS)]


def pack_msgs(msgs):
    """evote_msg rows of message dicts: group, kind ("hup" / "vote" /
    "vote_resp" or 0 / 5 / 6), from_, term, index, log_term, reject."""
    return _u64([[m.get("group", 0), _KINDS.get(m.get("kind"), m.get("kind", 0)), m.get("from_", 0), m.get("term", 0),
                  m.get("index", 0), m.get("log_term", 0), 1 if m.get("reject") else 0, 0] for m in msgs],
                MSG_IN_WORDS)


def results_from(raw, n):
    """evote_result rows (bytes) as dicts."""
    out = []
    for r in np.frombuffer(raw, dtype=np.uint64, count=n * RESULT_WORDS).reshape(n, RESULT_WORDS):
        w0, w5 = int(r[0]), int(r[5])
        out.append(dict(status=w0 & 0xFFFFFFFF, action=w0 >> 32, msg_first=int(r[1]), n_msgs=int(r[2]),
                        term=int(r[3]), vote=int(r[4]), state=w5 & 0xFFFFFFFF, flags=w5 >> 32))
    return out


def vote_batch_device(ctx, d_groups, d_pstate, d_vstate, G, d_snaps, d_ents, n_ents_total, d_in, n, d_res,
                      d_msgs=None, msgs_cap=0):
    """evote_step_batch_device over device arrays (elead_group[G],
    elead_prop_state[G], evote_state[G], elead_snap[G] or None,
    ewal_entry[n_ents_total], evote_msg[n], evote_result[n], emsg_out[msgs_cap]
    or None for the size query).  Returns (n_msgs, n_won)."""
    nm, nw = C.c_uint64(0), C.c_uint64(0)
    check(lib.evote_step_batch_device(ctx.handle, _ptr(d_groups), _ptr(d_pstate), _ptr(d_vstate), G, _ptr(d_snaps),
                                      _ptr(d_ents), n_ents_total, _ptr(d_in), n, _ptr(d_res), _ptr(d_msgs), msgs_cap,
                                      C.byref(nm), C.byref(nw)))
    return nm.value, nw.value


def vote_batch(ctx, groups, logs, state, vstate, msgs_in, snaps=None):
    """Host convenience: groups and logs as raftlead.pack_groups takes them,
    state as raftprop.pack_state, vstate as pack_vstate, msgs_in as pack_msgs,
    snaps as raftlead.pack_snaps.  Packs, uploads, asks for the size, calls,
    downloads.  Returns (results, new groups as unpack_groups gives them, new
    state, new vstate, entry rows (n_ents, 5) uint64, messages) -- the results,
    groups, states and messages as lists of dicts."""
    n, G = len(msgs_in), len(groups)
    grows, erows = pack_logs(groups, logs, state)
    srows, vrows = pack_state(state), pack_vstate(vstate)
    if n == 0:
        return [], unpack_groups(grows), unpack_state(srows), unpack_vstate(vrows), erows, []
    bufs = [_up(ctx, grows), _up(ctx, srows), _up(ctx, vrows), _up(ctx, pack_snaps(snaps)) if snaps is not None else None,
            _up(ctx, erows), _up(ctx, pack_msgs(msgs_in)), ctx.alloc(n * 48 + 64)]
    try:
        args = (ctx, bufs[0], bufs[1], bufs[2], G, bufs[3], bufs[4], len(erows), bufs[5], n, bufs[6])
        total, _ = vote_batch_device(*args)
        bufs.append(ctx.alloc(total * 144 + 64))
        vote_batch_device(*args, bufs[7], total)
        res = results_from(bufs[6].download(n * 48), n)
        msgs = messages_from(bufs[7].download(total * 144), total) if total else []
        g2 = np.frombuffer(bufs[0].download(grows.nbytes), dtype=np.uint64).reshape(-1, GROUP_WORDS)
        s2 = np.frombuffer(bufs[1].download(srows.nbytes), dtype=np.uint64).reshape(-1, STATE_WORDS)
        v2 = np.frombuffer(bufs[2].download(vrows.nbytes), dtype=np.uint64).reshape(-1, VSTATE_WORDS)
        e2 = np.frombuffer(bufs[4].download(erows.nbytes), dtype=np.uint64).reshape(-1, ENTRY_WORDS) if len(erows) \
            else erows
    finally:
        for b in bufs:
            if b is not None:
                b.free()
    return res, unpack_groups(g2), unpack_state(s2), unpack_vstate(v2), e2.copy(), msgs
