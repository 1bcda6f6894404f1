// ready_step.hip -- the joint between raft.Step and the write side of a
// multi-raft host: newReady (raft/node.go:332-348), node.run's accept branch
// (:239-255) and Storage.Save's record order (wal/wal.go:281-288) over n
// selected groups.  The decisions are ready_step.h's (shared with the host
// check); this file is the assignment of work and the memory traffic.
//
//   k_ready_count  ONE LANE PER SELECTED GROUP, nothing of the caller's
//                  modified.  The lane loads what the decision needs as aligned
//                  16-B pieces -- the first 48 B of the elead_group and its
//                  reserved words, the elead_prop_state, state / vote / lead
//                  and the reserved words of the evote_state, the eready_state,
//                  the snapshot's index -- claims the group (step_common.hip's
//                  claim word; skipped without d_sel, where no group can be
//                  named twice), runs the whole-call checks and the decision,
//                  and looks at data_nil of the unstable entries: the first few
//                  by itself, a longer run by the whole wave, 64 entries a
//                  step, so one restarted follower does not hold its wave for
//                  thousands of serial loads.  It leaves the group's save
//                  record count, its exclusive offset within the workgroup,
//                  where its unstable entries start in d_ents and its status in
//                  rec[p], and the workgroup's sums (records, groups with
//                  updates) in partial[].
//   k_lead_scan    step_common.hip's: the workgroups' record offsets and the
//                  totals.  The host reads the flag word and the totals here --
//                  the one decision point (INVAL, NOMEM, the peek).
//   k_ready_emit   two parts in one launch.  Thread i < n owns selection i: it
//                  decides again (nothing has changed), stores the result and,
//                  with EMIT, the accepted words that changed.  Thread r <
//                  *n_save owns SAVE RECORD r -- the work is balanced by output
//                  record, not by group: it finds its group by a search in the
//                  scanned offsets (first the workgroups' in partial[], then
//                  the 256 groups' of that workgroup, staged in LDS for the
//                  one the launch's workgroup starts in) and converts one 40-B
//                  ewal_entry into one 56-B ewal_save_rec, or builds the
//                  group's EWAL_SAVE_STATE record.  The record part reads only
//                  what no owner writes: rec[], partial[], d_ents and the const
//                  arrays.  <false> is the peek: results alone.
//
// Uses step_common.hip.
#include "ewal_device.h"
#include "ewal_internal.h"
#include "ready_step.h"

namespace rs = ready_step;

#define EREADY_LANE_SCAN 4u          // unstable entries a lane looks at by itself

struct EreadyRec {                   // 32 bytes per selection
  unsigned long long cnt, loc;       // its save records; their offset within its workgroup
  unsigned long long src;            // d_ents position of its first unstable entry
  unsigned long long meta;           // status | (EREADY_HARD ? 1 << 32 : 0)
};

struct EreadyArgs {
  const elead_group *groups;
  elead_prop_state *pstate;
  const evote_state *vstate;
  eready_state *rstate;
  uint64_t G;
  const elead_snap *snaps;           // nullable
  const ewal_entry *ents;
  uint64_t n_ents_total;
  const uint64_t *sel;               // nullable
  uint64_t n;
  eready_result *res;
  ewal_save_rec *save;               // NULL: the peek
  uint64_t n_save;                   // the records' total (the emit pass)
  uint32_t blocks;                   // the counting pass's workgroups
  uint32_t *claim;                   // G
  EreadyRec *rec;                    // n
  unsigned long long *partial;       // 2 per workgroup
  EleadHead *head;
};

// The words of group g the decision reads.  CHECK: the reserved words too;
// returns their OR.
template <bool CHECK>
__device__ __forceinline__ uint64_t eready_load(const EreadyArgs &a, uint64_t g, rs::In &in, uint64_t *efirst) {
  const el_v2 *gp = (const el_v2 *)(a.groups + g);
  const el_v2 *sp = (const el_v2 *)(a.pstate + g);
  const el_v2 *vp = (const el_v2 *)(a.vstate + g);
  const el_v2 *rp = (const el_v2 *)(a.rstate + g);
  const el_v2 g0 = gp[0], g1 = gp[1], g2 = gp[2];
  const el_v2 s0 = sp[0];
  const el_v2 v0 = vp[0], v1 = vp[1];
  const el_v2 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3];
  in.snap_index = a.snaps ? ((const el_v2 *)(a.snaps + g))[0].x : 0;
  uint64_t reserved = 0;
  if (CHECK) {
    const el_v2 g14 = gp[14], g15 = gp[15], s1 = sp[1], v3 = vp[3];
    reserved = g14.x | g14.y | g15.x | g15.y | s1.y | v3.x | v3.y;
  }
  in.term = g0.y;
  in.committed = g1.x;
  in.off = g1.y;
  in.nlog = g2.x;
  *efirst = g2.y;
  in.unstable = s0.y;
  in.state = v0.x;
  in.vote = v0.y;
  in.lead = v1.x;
  in.hs_term = r0.x;
  in.hs_vote = r0.y;
  in.hs_commit = r1.x;
  in.plead = r1.y;
  in.pstate = r2.x;
  in.snapi = r2.y;
  in.applied = r3.x;
  in.soft_dirty = r3.y;
  return reserved;
}

// a panicking or unsupported group: the status alone
__device__ __forceinline__ void eready_void(rs::Out &o, int32_t status, const rs::In &in) {
  o.status = status;
  o.flags = 0;
  o.term = o.vote = o.commit = 0;
  o.ents_pos = o.n_ents = o.committed_pos = o.n_committed = o.n_save = 0;
  o.lead = o.state = 0;
  o.applied = in.applied;
  o.unstable = in.unstable;
}

__global__ __launch_bounds__(256) void k_ready_count(const EreadyArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < a.n;
  const uint64_t g = valid ? (a.sel ? a.sel[i] : i) : 0;
  uint32_t err = 0;
  rs::In in;
  rs::Out o;
  uint64_t efirst = 0;
  bool decided = false;
  if (valid && g >= a.G) err = STEP_ERR_INVAL;
  if (valid && !err) {
    const uint64_t reserved = eready_load<true>(a, g, in, &efirst);
    // the group's claim: a second selection of the group finds the word taken
    if (a.sel && !step_claim(a.claim, g, i)) err = STEP_ERR_INVAL;
    if (reserved != 0 || in.state > 2 || in.pstate > 2 || in.soft_dirty > 1) err = STEP_ERR_INVAL;
    if (in.nlog > a.n_ents_total || efirst > a.n_ents_total - in.nlog) err = STEP_ERR_INVAL;
    if (!err) {
      o = rs::decide(in);
      if (o.status != lp::ST_OK) eready_void(o, o.status, in);
      decided = true;
    }
  }
  step_flag(a.head, err);
  // data_nil == 2 among the unstable entries: their bytes are not in d_data
  const uint64_t scan_first = decided ? efirst + o.ents_pos : 0, scan_n = decided ? o.n_ents : 0;
  bool outside = false;
  for (uint64_t k = 0; k < scan_n && k < EREADY_LANE_SCAN; ++k) outside |= rs::data_outside(a.ents[scan_first + k].data_nil);
  unsigned long long todo = __ballot(scan_n > EREADY_LANE_SCAN);
  while (todo) {
    const int src = __ffsll(todo) - 1;
    todo &= todo - 1;
    const uint64_t f = __shfl(scan_first, src), m = __shfl(scan_n, src);
    bool mine = false;
    for (uint64_t k = EREADY_LANE_SCAN + lane; k < m; k += 64) mine |= rs::data_outside(a.ents[f + k].data_nil);
    if (__ballot(mine) && (int)lane == src) outside = true;
  }
  if (outside) eready_void(o, lp::ST_UNSUPPORTED, in);
  const unsigned long long cnt = decided ? o.n_save : 0;
  unsigned long long total = 0;
  const unsigned long long loc = step_block_scan(cnt, &total);
  if (valid) {
    el_v2 *q = (el_v2 *)(a.rec + i);
    const uint64_t status = decided ? (uint64_t)(uint32_t)o.status : 0;
    q[0] = el_v2{cnt, loc};
    q[1] = el_v2{scan_first, status | ((decided && (o.flags & rs::HARD)) ? 1ull << 32 : 0ull)};
  }
  step_block_sums(cnt, (decided && (o.flags & rs::UPDATES)) ? 1 : 0, a.partial, blockIdx.x);
}

// the last k in [0, m) with at(k) <= x; at(0) <= x is the caller's
template <class At>
__device__ __forceinline__ uint32_t eready_last_le(uint32_t m, unsigned long long x, const At &at) {
  uint32_t lo = 0, hi = m;           // at(lo) <= x; every k >= hi has at(k) > x
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (at(mid) <= x)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_ready_emit(const EreadyArgs a) {
  __shared__ unsigned long long s_loc[256];
  __shared__ uint32_t s_b0;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  // the owner of selection i
  if (i < a.n) {
    const uint64_t g = a.sel ? a.sel[i] : i;
    rs::In in;
    uint64_t efirst = 0;
    (void)eready_load<false>(a, g, in, &efirst);
    const el_v2 *rq = (const el_v2 *)(a.rec + i);
    const el_v2 r0 = rq[0], r1 = rq[1];
    const int32_t status = (int32_t)(uint32_t)r1.y;
    rs::Out o = rs::decide(in);
    if (status != lp::ST_OK) eready_void(o, status, in);
    const uint64_t save_first = a.partial[2 * (uint64_t)blockIdx.x] + r0.y;
    el_v2 *q = (el_v2 *)(a.res + i);
    q[0] = el_v2{(uint64_t)(uint32_t)o.status | ((uint64_t)(uint32_t)o.flags << 32), o.term};
    q[1] = el_v2{o.vote, o.commit};
    q[2] = el_v2{o.n_ents ? efirst + o.ents_pos : 0, o.n_ents};
    q[3] = el_v2{o.n_committed ? efirst + o.committed_pos : 0, o.n_committed};
    q[4] = el_v2{save_first, o.n_save};
    q[5] = el_v2{o.lead, o.state};
    if (EMIT && status == lp::ST_OK) {
      uint64_t *rw = (uint64_t *)(a.rstate + g);
      uint64_t *sw = (uint64_t *)(a.pstate + g);
      if (o.flags & rs::SOFT) {
        if (in.lead != in.plead) rw[3] = in.lead;
        if (in.state != in.pstate) rw[4] = in.state;
        if (in.soft_dirty != 0) rw[7] = 0;
      }
      if (o.flags & rs::HARD) {
        if (o.term != in.hs_term) rw[0] = o.term;
        if (o.vote != in.hs_vote) rw[1] = o.vote;
        if (o.commit != in.hs_commit) rw[2] = o.commit;
      }
      if (o.flags & rs::SNAP) rw[5] = in.snap_index;
      if (o.applied != in.applied) rw[6] = o.applied;
      if (o.unstable != in.unstable) sw[1] = o.unstable;
    }
  }
  if (!EMIT) return;
  // the owner of save record r
  const uint64_t R0 = (uint64_t)blockIdx.x * 256;
  if (R0 >= a.n_save) return;
  const auto wg_at = [&](uint32_t b) { return a.partial[2 * (uint64_t)b]; };
  if (threadIdx.x == 0) s_b0 = eready_last_le(a.blocks, R0, wg_at);
  __syncthreads();
  const uint32_t b0 = s_b0;
  {
    const uint64_t p = (uint64_t)b0 * 256 + threadIdx.x;
    s_loc[threadIdx.x] = p < a.n ? a.rec[p].loc : ~0ull;
  }
  __syncthreads();
  const uint64_t r = R0 + threadIdx.x;
  if (r >= a.n_save) return;
  uint32_t b = b0, idx;
  if (b0 + 1 < a.blocks && r >= wg_at(b0 + 1)) {
    const auto later_at = [&](uint32_t k) { return a.partial[2 * (uint64_t)(b0 + 1 + k)]; };
    b = b0 + 1 + eready_last_le(a.blocks - b0 - 1, r, later_at);
  }
  const unsigned long long x = r - wg_at(b);
  if (b == b0) {
    idx = eready_last_le(256, x, [&](uint32_t k) { return s_loc[k]; });
  } else {
    const uint64_t left = a.n - (uint64_t)b * 256;
    const EreadyRec *base = a.rec + (uint64_t)b * 256;
    idx = eready_last_le(left < 256 ? (uint32_t)left : 256u, x, [&](uint32_t k) { return base[k].loc; });
  }
  const uint64_t p = (uint64_t)b * 256 + idx;
  const el_v2 *rq = (const el_v2 *)(a.rec + p);
  const el_v2 r0 = rq[0], r1 = rq[1];
  const uint64_t hard = (r1.y >> 32) & 1, k = x - r0.y;
  uint64_t w[7];
  if (hard && k == 0) {
    const uint64_t g = a.sel ? a.sel[p] : p;
    const el_v2 g0 = ((const el_v2 *)(a.groups + g))[0], g1 = ((const el_v2 *)(a.groups + g))[1];
    const el_v2 v0 = ((const el_v2 *)(a.vstate + g))[0];
    rs::save_of_state(w, g0.y, v0.y, g1.x);
  } else {
    const uint64_t *e = (const uint64_t *)(a.ents + r1.x + (k - hard));
    uint64_t t[5];
    if (((uintptr_t)e & 15) == 0) {
      const el_v2 x0 = ((const el_v2 *)e)[0], x1 = ((const el_v2 *)e)[1];
      t[0] = x0.x, t[1] = x0.y, t[2] = x1.x, t[3] = x1.y, t[4] = e[4];
    } else {
      const el_v2 x0 = *(const el_v2 *)(e + 1), x1 = *(const el_v2 *)(e + 3);
      t[0] = e[0], t[1] = x0.x, t[2] = x0.y, t[3] = x1.x, t[4] = x1.y;
    }
    rs::save_of_entry(w, t);
  }
  uint64_t *d = (uint64_t *)(a.save + r);
  if ((r & 1) == 0) {                                // 56 r is a multiple of 16
    ((el_v2 *)d)[0] = el_v2{w[0], w[1]};
    ((el_v2 *)d)[1] = el_v2{w[2], w[3]};
    ((el_v2 *)d)[2] = el_v2{w[4], w[5]};
    d[6] = w[6];
  } else {
    d[0] = w[0];
    *(el_v2 *)(d + 1) = el_v2{w[1], w[2]};
    *(el_v2 *)(d + 3) = el_v2{w[3], w[4]};
    *(el_v2 *)(d + 5) = el_v2{w[5], w[6]};
  }
}
