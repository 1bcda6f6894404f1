// follow_step.hip -- the follower's half of a replication round on the shared
// group records: raft.Step for msgApp and msgSnap over n messages, with
// handleAppendEntries, handleSnapshot and raft.restore.  The decisions are
// follow_step.h's (shared with the host check); this file is the assignment of
// work and the memory traffic.
//
// Assignment: ONE LANE PER RUN HEAD for the decisions, vote_step.hip's: a
// record's case depends on the state its predecessors left, and runs are short
// (a follower gets a msgApp or two and a heartbeat a round).  ONE LANE PER
// COPIED ENTRY for the entries: a run appends at most one suffix (the run rule
// defers a second one), so a run is one copy descriptor, and one long catch-up
// spreads over many workgroups.
//
//   k_follow_count  one lane per record, nothing of the caller's modified: the
//                   checks of a record (group, kind, padding, the source range,
//                   the snapshot and its Nodes range) and, by a run's head, of
//                   its group (the claim, lead_prop.hip's group and window
//                   checks, vote_step.hip's evote_state checks), then a replay
//                   of the run that only counts: the run's messages into
//                   run_msgs[head], its copy descriptor into cp[head], the room
//                   its records need against ents_cap (NOMEM), the workgroup's
//                   sums of messages / RESTORED records into partial[] and of
//                   copied entries into cpart[].  A later record of the run
//                   that fails its checks ends the replay before any of its
//                   ranges is read.
//   k_lead_scan     step_common.hip's, twice: the workgroups' message offsets and
//                   copy offsets and the totals.  The host reads the flag word
//                   and the totals here -- the one decision point.
//   k_follow_apply  one lane per record again: a workgroup-wide exclusive scan
//                   of run_msgs plus the workgroup's offset places each run's
//                   messages; the head replays the run, writes d_res, the
//                   responses, and of the four records only the words that
//                   changed; a restore's entry and d_snaps[g] at the run's end.
//                   It reads d_ents as the call found it: the appended suffix
//                   is seen through the overlay, as in the counting pass.
//                   <false> writes d_res alone.
//   k_follow_copy   one lane per copied entry: it finds its run by a search in
//                   the scanned offsets (the workgroups' in cpart[], then the
//                   256 descriptors of that workgroup, as ready_step.hip's emit
//                   pass does) and moves one 40-B ewal_entry, data_off rebased.
//                   A launch of its own: every read of the apply pass is done.
//
// Uses step_common.hip, lead_prop.hip's and vote_step.hip's group loaders and
// checks and ready_step.hip's offset search.
#include "ewal_device.h"
#include "ewal_internal.h"
#include "follow_step.h"

namespace fs = follow_step;

struct EfollowCopy {                // 48 bytes per record; cnt == 0 unless the record heads a run that appends
  unsigned long long cnt, loc;      // the run's copied entries; their offset within its workgroup
  unsigned long long src, dst;      // d_src / d_ents positions of the first one
  unsigned long long delta, pad;    // added to data_off where data_nil == 0
};

struct EfollowArgs {
  EpropArgs p;                      // groups, state, G, ents, n_ents_total, msgs, claim, partial, head
  evote_state *vstate;
  eready_state *rstate;             // nullable
  elead_snap *snaps;                // nullable; written by a restore
  const ewal_entry *src;
  uint64_t n_src_total;
  const elead_snap *in_snaps;
  uint64_t n_in_snaps;
  const uint64_t *u64;
  uint64_t n_u64;
  const efollow_msg *in;
  uint64_t n;
  efollow_result *res;
  unsigned long long *run_msgs;     // n
  EfollowCopy *cp;                  // n
  unsigned long long *cpart;        // 2 per workgroup: the copied entries
  EleadHead *chead;                 // their total
  uint64_t n_copy;                  // the copy pass: the total
  uint32_t blocks;                  // the counting pass's workgroups
};

// one message's words
struct EfollowRec {
  uint64_t group, kind, from, term, index, log_term, commit, ents_first, n_ents, data_delta, snap, pad;
};

__device__ __forceinline__ EfollowRec efollow_unpack(const el_v2 (&u)[6]) {
  return EfollowRec{u[0].x, u[0].y, u[1].x, u[1].y, u[2].x, u[2].y, u[3].x, u[3].y, u[4].x, u[4].y, u[5].x, u[5].y};
}

// the wave's 64 records: lane l gets record r0 + l
__device__ __forceinline__ EfollowRec efollow_load_wave(const efollow_msg *__restrict__ in, uint64_t n, el_v2 *s_wave,
                                                        uint64_t r0, uint32_t lane) {
  el_v2 u[6];
  step_load_wave(in, n, s_wave, r0, lane, u);
  return efollow_unpack(u);
}

// One record at an arbitrary place (a run's later records).
__device__ __forceinline__ EfollowRec efollow_load_rec(const efollow_msg *p) {
  el_v2 u[6];
  step_load_rec(p, u);
  return efollow_unpack(u);
}

// The checks of one record (group < G included); a msgSnap's Snapshot comes back in *sn.
__device__ __forceinline__ bool efollow_rec_ok(const EfollowArgs &a, const EfollowRec &r, fs::Snap *sn,
                                               uint64_t *nodes_off) {
  sn->index = sn->term = sn->n_nodes = 0;
  *nodes_off = 0;
  if (r.group >= a.p.G || r.pad != 0) return false;
  if (r.kind != fs::KIND_APP && r.kind != fs::KIND_SNAP) return false;
  if (r.n_ents > a.n_src_total || r.ents_first > a.n_src_total - r.n_ents) return false;
  if (r.kind == fs::KIND_SNAP) {
    if (!a.rstate || !a.snaps || r.snap >= a.n_in_snaps) return false;
    const el_v2 *q = (const el_v2 *)(a.in_snaps + r.snap);
    const el_v2 q0 = q[0], q2 = q[2];                // index, term | nodes_off, n_nodes
    if (q2.y > a.n_u64 || q2.x > a.n_u64 - q2.y) return false;
    sn->index = q0.x;
    sn->term = q0.y;
    sn->n_nodes = q2.y;
    *nodes_off = q2.x;
  }
  return true;
}

// the group's four records as a run's start state
__device__ __forceinline__ uint64_t efollow_load_group(const EfollowArgs &a, uint64_t g, lp::State &s, vs::Vote &v,
                                                       fs::Ready &rd, uint64_t *cap, uint64_t *vreserved) {
  const uint64_t reserved = eprop_load_group(a.p, g, s, cap);
  *vreserved = evote_load_state(a.vstate + g, v);
  rd.applied = rd.soft_dirty = 0;
  if (a.rstate) {
    const el_v2 x = ((const el_v2 *)(a.rstate + g))[3];
    rd.applied = x.x;
    rd.soft_dirty = x.y;
  }
  return reserved;
}

// The run of group g headed at record i (r0) on the start state: steps it in
// order.  write_res: d_res; EMIT: the responses from msg_first on and the
// records' changed words.  Returns false when a later record of the run fails
// its checks (the counting pass; nothing past it has been read).  COUNT: the
// counting pass's outputs (the copy descriptor, the room, whether a snapshot came).
template <bool EMIT, bool COUNT>
__device__ __forceinline__ bool efollow_run(const EfollowArgs &a, uint64_t i, const EfollowRec &r0, lp::State s,
                                            vs::Vote v, fs::Ready rd, bool write_res, uint64_t msg_first,
                                            unsigned long long &tot, unsigned long long &nrest, EfollowCopy &cp,
                                            uint64_t &room, bool &snap_seen) {
  const uint64_t g = r0.group;
  const lp::State s0 = s;
  const vs::Vote v0 = v;
  const fs::Ready rd0 = rd;
  const ewal_entry *win = a.p.ents + s.efirst;
  fs::Run run = fs::run_start();
  uint64_t restored_from = 0;
  EfollowRec r = r0;
  for (uint64_t k = i;;) {
    fs::Snap sn;
    uint64_t nodes_off = 0;
    if (!efollow_rec_ok(a, r, &sn, &nodes_off)) return false;
    const fs::Rec rec{r.kind, r.from, r.term, r.index, r.log_term, r.commit, r.n_ents};
    const fs::Overlay ov = run.ov;
    const ewal_entry *src = a.src;
    const auto log_at = [&](uint64_t pos) { return win[pos].term; };
    const auto src_at = [&](uint64_t q) { return src[q].term; };
    const auto term_at = [&](uint64_t pos) { return fs::overlay_term(ov, pos, log_at, src_at); };
    const auto src_term = [&](uint64_t j) { return src[r.ents_first + j].term; };
    const auto node_at = [&](uint64_t j) { return a.u64[nodes_off + j]; };
    const fs::Out o = fs::run_step(run, s, v, rd, rec, r.ents_first, sn, term_at, src_term, node_at);
    if (COUNT && r.kind == fs::KIND_APP) room = r.n_ents > room ? r.n_ents : room;
    if (COUNT) snap_seen = snap_seen || r.kind == fs::KIND_SNAP;
    if (COUNT && o.n_app != 0) {
      cp.cnt = o.n_app;
      cp.src = r.ents_first + o.app_k;
      cp.dst = s.efirst + o.dst_pos;
      cp.delta = r.data_delta;
    }
    if (o.restored) restored_from = r.snap;
    if (write_res) {
      el_v2 *rq = (el_v2 *)(a.res + k);
      rq[0] = el_v2{(uint64_t)(uint32_t)o.status | ((uint64_t)(uint32_t)o.action << 32), msg_first};
      rq[1] = el_v2{o.n_msgs, o.conflict};
      rq[2] = el_v2{o.n_app ? r.ents_first + o.app_k : 0, o.n_app};
      rq[3] = el_v2{o.n_app ? s.efirst + o.dst_pos : 0, s.nlog - 1 + s.off};
      rq[4] = el_v2{s.committed, s.term};
      rq[5] = el_v2{v.state | ((uint64_t)(uint32_t)o.flags << 32), 0};
    }
    if (EMIT && o.n_msgs != 0) {                     // the msgAppResp after send (raft.go:190-199)
      el_v2 *q = (el_v2 *)(a.p.msgs + msg_first);
      q[0] = el_v2{fs::MSG_APP_RESP, r.from};
      q[1] = el_v2{s.id, s.term};
      q[2] = el_v2{0, o.resp_index};
#pragma unroll
      for (uint32_t w = 3; w < 8; ++w) q[w] = el_v2{0, 0};
      q[8] = el_v2{0, o.resp_reject ? 1ull : 0ull};
    }
    msg_first += o.n_msgs;
    tot += o.n_msgs;
    nrest += o.restored ? 1 : 0;
    ++k;
    if (k >= a.n) break;
    r = efollow_load_rec(a.in + k);
    if (r.group != g) break;
  }
  if (EMIT) {
    lp_store_changed(a.p.groups, a.p.state, g, s0, s);
    vs_store_changed(a.vstate, g, v0, v);
    if (run.ov.restored) {                           // efollow_rec_ok: rstate and snaps are there
      uint64_t *rw = (uint64_t *)(a.rstate + g);
      if (rd.applied != rd0.applied) rw[6] = rd.applied;
      if (rd.soft_dirty != rd0.soft_dirty) rw[7] = rd.soft_dirty;
      const el_v2 *from = (const el_v2 *)(a.in_snaps + restored_from);
      el_v2 *to = (el_v2 *)(a.snaps + g);
      const el_v2 x0 = from[0], x1 = from[1], x2 = from[2], x3 = from[3];
      to[0] = x0, to[1] = x1, to[2] = x2, to[3] = x3;
      uint64_t *e = (uint64_t *)(a.p.ents + s.efirst);   // ents = []Entry{{Term: s.Term}}
      e[0] = run.ov.term;
      e[1] = e[2] = e[3] = 0;
      e[4] = 1ull << 32;
    }
  }
  return true;
}

__global__ __launch_bounds__(256) void k_follow_count(const EfollowArgs a) {
  __shared__ el_v2 s_rec[4][384];
  const auto [lane, wave, r0, i] = step_lane();
  const EfollowRec r = efollow_load_wave(a.in, a.n, s_rec[wave], r0, lane);
  const bool valid = i < a.n;
  const bool head = step_is_head(a.in, a.n, i, r.group, lane);
  uint32_t err = 0;
  unsigned long long tot = 0, nrest = 0;
  EfollowCopy cp{0, 0, 0, 0, 0, 0};
  if (valid) {
    fs::Snap sn;
    uint64_t nodes_off = 0;
    if (!efollow_rec_ok(a, r, &sn, &nodes_off)) err = STEP_ERR_INVAL;
  }
  if (head && !err) {
    lp::State s;
    vs::Vote v;
    fs::Ready rd;
    uint64_t cap = 0, vreserved = 0;
    const uint64_t reserved = efollow_load_group(a, r.group, s, v, rd, &cap, &vreserved);
    // the group's claim: the head of a second run finds the word taken
    if (!step_claim(a.p.claim, r.group, i)) err = STEP_ERR_INVAL;
    if (!eprop_group_ok(a.p, s, cap, reserved) || !evote_state_ok(s, v, vreserved)) err = STEP_ERR_INVAL;
    if (!err) {
      uint64_t room = 0;
      bool snap_seen = false;
      if (!efollow_run<false, true>(a, i, r, s, v, rd, false, 0, tot, nrest, cp, room, snap_seen)) {
        err = STEP_ERR_INVAL;
        tot = nrest = 0;
        cp.cnt = 0;
      } else if (cap - s.nlog < room || (snap_seen && cap == 0)) {
        err = STEP_ERR_NOMEM;
      }
    }
  }
  step_flag(a.p.head, err);
  unsigned long long total = 0;
  cp.loc = step_block_scan(cp.cnt, &total);
  if (valid) {
    a.run_msgs[i] = tot;
    el_v2 *q = (el_v2 *)(a.cp + i);
    q[0] = el_v2{cp.cnt, cp.loc};
    q[1] = el_v2{cp.src, cp.dst};
    q[2] = el_v2{cp.delta, 0};
  }
  step_block_sums(tot, nrest, a.p.partial, blockIdx.x);
  __syncthreads();                                   // the sums' staging words are reused
  step_block_sums(cp.cnt, 0, a.cpart, blockIdx.x);
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_follow_apply(const EfollowArgs a) {
  __shared__ el_v2 s_rec[4][384];
  const auto [lane, wave, r0, i] = step_lane();
  const EfollowRec r = efollow_load_wave(a.in, a.n, s_rec[wave], r0, lane);
  const bool head = step_is_head(a.in, a.n, i, r.group, lane);
  unsigned long long total = 0;
  const unsigned long long before = step_block_scan(i < a.n ? a.run_msgs[i] : 0, &total);
  if (head) {
    lp::State s;
    vs::Vote v;
    fs::Ready rd;
    uint64_t cap = 0, vreserved = 0, room = 0;
    bool snap_seen = false;
    (void)efollow_load_group(a, r.group, s, v, rd, &cap, &vreserved);
    unsigned long long tot = 0, nrest = 0;
    EfollowCopy cp{0, 0, 0, 0, 0, 0};
    (void)efollow_run<EMIT, false>(a, i, r, s, v, rd, true, a.p.partial[2 * (uint64_t)blockIdx.x] + before, tot, nrest, cp,
                            room, snap_seen);
  }
}

__global__ __launch_bounds__(256) void k_follow_copy(const EfollowArgs a) {
  __shared__ unsigned long long s_loc[256];
  __shared__ uint32_t s_b0;
  const uint64_t R0 = (uint64_t)blockIdx.x * 256;
  if (R0 >= a.n_copy) return;
  const auto wg_at = [&](uint32_t b) { return a.cpart[2 * (uint64_t)b]; };
  if (threadIdx.x == 0) s_b0 = eready_last_le(a.blocks, R0, wg_at);
  __syncthreads();
  const uint32_t b0 = s_b0;
  {
    const uint64_t p = (uint64_t)b0 * 256 + threadIdx.x;
    s_loc[threadIdx.x] = p < a.n ? a.cp[p].loc : ~0ull;
  }
  __syncthreads();
  const uint64_t r = R0 + threadIdx.x;
  if (r >= a.n_copy) return;
  uint32_t b = b0, idx;
  if (b0 + 1 < a.blocks && r >= wg_at(b0 + 1)) {
    const auto later_at = [&](uint32_t k) { return a.cpart[2 * (uint64_t)(b0 + 1 + k)]; };
    b = b0 + 1 + eready_last_le(a.blocks - b0 - 1, r, later_at);
  }
  const unsigned long long x = r - wg_at(b);
  if (b == b0) {
    idx = eready_last_le(256, x, [&](uint32_t k) { return s_loc[k]; });
  } else {
    const uint64_t left = a.n - (uint64_t)b * 256;
    const EfollowCopy *base = a.cp + (uint64_t)b * 256;
    idx = eready_last_le(left < 256 ? (uint32_t)left : 256u, x, [&](uint32_t k) { return base[k].loc; });
  }
  const el_v2 *cq = (const el_v2 *)(a.cp + (uint64_t)b * 256 + idx);
  const el_v2 c0 = cq[0], c1 = cq[1], c2 = cq[2];
  const uint64_t k = x - c0.y;
  if (k >= c0.x) return;                             // cannot happen: the offsets are the counts' scan
  const uint64_t *e = (const uint64_t *)(a.src + c1.x + k);
  uint64_t t[5];
#pragma unroll
  for (uint32_t w = 0; w < 5; ++w) t[w] = e[w];
  if ((uint32_t)(t[4] >> 32) == 0) t[2] += c2.x;     // data_nil == 0: Data is a range of the ingress buffer
  uint64_t *d = (uint64_t *)(a.p.ents + c1.y + k);
#pragma unroll
  for (uint32_t w = 0; w < 5; ++w) d[w] = t[w];
}
