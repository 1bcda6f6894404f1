// compact_step.hip -- node.Compact on the shared group records: raft.compact,
// raftLog.snap and raftLog.compact over n requests, one per raft group.  The
// decision is compact_step.h's (shared with the host check); this file is the
// assignment of work and the memory traffic.
//
// A fixed window cannot reslice as Go does: the survivors of a compaction are
// MOVED to the window's base, or the room would never come back.  Assignment:
// ONE LANE PER REQUEST for the decisions (a request is independent of every
// other one: a group is named once), ONE LANE PER MOVED ENTRY for the slide, so
// one group that keeps a million entries spreads over many workgroups.
//
//   k_compact_count  one lane per request, nothing of the caller's modified:
//                    the checks of the request (group, flags, padding, the Data,
//                    Nodes and RemovedNodes ranges) and of its group (the claim,
//                    lead_prop.hip's group and window checks), the decision, and
//                    the move descriptor into mv[i]: the survivors' count, where
//                    they lie and go, and the class -- none (shift == 0),
//                    disjoint (shift >= n_left), overlapping (0 < shift <
//                    n_left).  The moved entries are block-scanned per class;
//                    the workgroup's sums go to dpart[] (with the COMPACTED
//                    requests) and opart[].
//   k_lead_scan      step_common.hip's, twice: the workgroups' offsets of both
//                    classes and the totals.  The host reads the flag word and
//                    the totals here -- the one decision point.
//   k_compact_apply  one lane per request again: d_res, and of a COMPACTED
//                    group log_offset, nlog, unstable (only where they changed)
//                    and d_snaps[g].  It reads the snapshot's term from d_ents
//                    as the call found it, so it runs before any move.  <false>
//                    is the peek and writes d_res alone.
//   k_compact_move   one lane per moved entry of one class: it finds its
//                    descriptor by a search in the scanned offsets (the
//                    workgroups', then the 256 descriptors of that workgroup,
//                    as k_follow_copy does) and moves one 40-B ewal_entry.
//                    <MV_DIRECT>: the disjoint class, in place -- no lane reads
//                    what another one writes.  The overlapping class cannot be
//                    moved in place by independent lanes: <MV_GATHER> copies
//                    every entry of the class into the ctx's staging buffer,
//                    <MV_SCATTER>, a launch of its own, stores them at their
//                    targets.  A launch with no work is skipped.
//
// Uses step_common.hip, lead_prop.hip's group loader and checks and
// ready_step.hip's offset search.
#include "ewal_device.h"
#include "ewal_internal.h"
#include "compact_step.h"

namespace cs = compact_step;

#define MV_DIRECT 0
#define MV_GATHER 1
#define MV_SCATTER 2

struct EcompactMove {               // 48 bytes per request; cnt == 0 unless the request moves entries
  unsigned long long cnt, cls;      // the survivors; cs::MOVE_*
  unsigned long long src, dst;      // their d_ents positions before and after
  unsigned long long loc_d, loc_o;  // the workgroup's exclusive scans of the disjoint / overlapping counts
};

struct EcompactArgs {
  EpropArgs p;                      // groups, state, G, ents, n_ents_total, data_len_total, claim, head
  const eready_state *rstate;
  elead_snap *snaps;
  uint64_t n_u64;
  const ecompact_req *in;
  uint64_t n;
  ecompact_result *res;
  EcompactMove *mv;                 // n
  unsigned long long *dpart;        // 2 per workgroup: the disjoint entries, the COMPACTED requests
  unsigned long long *opart;        // 2 per workgroup: the overlapping entries
  EleadHead *ohead;                 // their total
  ewal_entry *stage;                // the overlapping class in flight
  uint64_t n_move;                  // the move pass: its class's total
  uint32_t blocks;                  // the counting pass's workgroups
};

// one request's words
struct EcompactRec {
  uint64_t group, flags, index, threshold, data_off, data_len, nodes_off, n_nodes, removed_off, n_removed, pad0, pad1;
};

// the wave's 64 requests: lane l gets request r0 + l
__device__ __forceinline__ EcompactRec ecompact_load_wave(const ecompact_req *__restrict__ in, uint64_t n, el_v2 *s_wave,
                                                          uint64_t r0, uint32_t lane) {
  el_v2 u[6];
  step_load_wave(in, n, s_wave, r0, lane, u);
  return EcompactRec{u[0].x, u[0].y, u[1].x, u[1].y, u[2].x, u[2].y, u[3].x, u[3].y, u[4].x, u[4].y, u[5].x, u[5].y};
}

__device__ __forceinline__ bool ecompact_range_ok(uint64_t off, uint64_t len, uint64_t total) {
  return len <= total && off <= total - len;
}

// the checks of one request (group < G included)
__device__ __forceinline__ bool ecompact_rec_ok(const EcompactArgs &a, const EcompactRec &r) {
  if (r.group >= a.p.G || (r.flags & ~cs::AT_APPLIED) != 0 || (r.pad0 | r.pad1) != 0) return false;
  if ((r.flags & cs::AT_APPLIED) && r.index != 0) return false;
  return ecompact_range_ok(r.data_off, r.data_len, a.p.data_len_total) &&
         ecompact_range_ok(r.nodes_off, r.n_nodes, a.n_u64) && ecompact_range_ok(r.removed_off, r.n_removed, a.n_u64);
}

// The request on its group as the call found it; the group's window checks are
// the caller's (the term is read only from a checked window).
__device__ __forceinline__ cs::Out ecompact_decide(const EcompactArgs &a, const EcompactRec &r, const lp::State &s) {
  const uint64_t applied = ((const uint64_t *)(a.rstate + r.group))[6];
  const ewal_entry *win = a.p.ents + s.efirst;
  return cs::decide(s, applied, cs::Req{r.flags, r.index, r.threshold}, [&](uint64_t pos) { return win[pos].term; });
}

__global__ __launch_bounds__(256) void k_compact_count(const EcompactArgs a) {
  __shared__ el_v2 s_rec[4][384];
  const auto [lane, wave, r0, i] = step_lane();
  const EcompactRec r = ecompact_load_wave(a.in, a.n, s_rec[wave], r0, lane);
  const bool valid = i < a.n;
  uint32_t err = 0;
  unsigned long long ncompacted = 0;
  EcompactMove mv{0, cs::MOVE_NONE, 0, 0, 0, 0};
  if (valid && !ecompact_rec_ok(a, r)) err = STEP_ERR_INVAL;
  if (valid && !err) {
    lp::State s;
    uint64_t cap = 0;
    const uint64_t reserved = eprop_load_group(a.p, r.group, s, &cap);
    // the group's claim: a second request for the group finds the word taken
    if (!step_claim(a.p.claim, r.group, i)) err = STEP_ERR_INVAL;
    if (!eprop_group_ok(a.p, s, cap, reserved)) err = STEP_ERR_INVAL;
    if (!err) {
      const cs::Out o = ecompact_decide(a, r, s);
      if (o.action == cs::COMPACTED) {
        ncompacted = 1;
        mv.cls = cs::move_class(o.n_left, o.shift);
        mv.cnt = mv.cls == cs::MOVE_NONE ? 0 : o.n_left;
        mv.src = s.efirst + o.shift;
        mv.dst = s.efirst;
      }
    }
  }
  step_flag(a.p.head, err);
  const unsigned long long nd = mv.cls == cs::MOVE_DISJOINT ? mv.cnt : 0;
  const unsigned long long no = mv.cls == cs::MOVE_OVERLAP ? mv.cnt : 0;
  unsigned long long total = 0;
  mv.loc_d = step_block_scan(nd, &total);
  mv.loc_o = step_block_scan(no, &total);
  if (valid) {
    el_v2 *q = (el_v2 *)(a.mv + i);
    q[0] = el_v2{mv.cnt, mv.cls};
    q[1] = el_v2{mv.src, mv.dst};
    q[2] = el_v2{mv.loc_d, mv.loc_o};
  }
  step_block_sums(nd, ncompacted, a.dpart, blockIdx.x);
  __syncthreads();                                   // the sums' staging words are reused
  step_block_sums(no, 0, a.opart, blockIdx.x);
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_compact_apply(const EcompactArgs a) {
  __shared__ el_v2 s_rec[4][384];
  const auto [lane, wave, r0, i] = step_lane();
  const EcompactRec r = ecompact_load_wave(a.in, a.n, s_rec[wave], r0, lane);
  if (i >= a.n) return;
  lp::State s;
  uint64_t cap = 0;
  (void)eprop_load_group(a.p, r.group, s, &cap);
  const cs::Out o = ecompact_decide(a, r, s);
  const bool done = o.action == cs::COMPACTED;
  el_v2 *rq = (el_v2 *)(a.res + i);
  rq[0] = el_v2{(uint64_t)(uint32_t)o.status | ((uint64_t)(uint32_t)o.action << 32), o.index};
  rq[1] = el_v2{o.term, o.n_left};
  rq[2] = el_v2{o.shift, done ? s.efirst + o.shift : 0};
  rq[3] = el_v2{done ? s.efirst : 0, o.unstable};
  if (EMIT && done) {
    uint64_t *gw = (uint64_t *)(a.p.groups + r.group);
    uint64_t *sw = (uint64_t *)(a.p.state + r.group);
    if (o.index != s.off) gw[3] = o.index;
    if (o.n_left != s.nlog) gw[4] = o.n_left;
    if (o.unstable != s.unstable) sw[1] = o.unstable;
    el_v2 *to = (el_v2 *)(a.snaps + r.group);        // raftLog.snap
    to[0] = el_v2{o.index, o.term};
    to[1] = el_v2{r.data_off, r.data_len};
    to[2] = el_v2{r.nodes_off, r.n_nodes};
    to[3] = el_v2{r.removed_off, r.n_removed};
  }
}

// Lane r moves entry r of the launch's class (MV_DIRECT: the disjoint one,
// else the overlapping one); the staging slot of an overlapping entry is r itself.
template <int MODE>
__global__ __launch_bounds__(256) void k_compact_move(const EcompactArgs a) {
  constexpr bool OV = MODE != MV_DIRECT;
  __shared__ unsigned long long s_loc[256];
  __shared__ uint32_t s_b0;
  const unsigned long long *part = OV ? a.opart : a.dpart;
  const uint64_t R0 = (uint64_t)blockIdx.x * 256;
  if (R0 >= a.n_move) return;
  const auto wg_at = [&](uint32_t b) { return part[2 * (uint64_t)b]; };
  const auto loc_of = [&](const EcompactMove *m) { return OV ? m->loc_o : m->loc_d; };
  if (threadIdx.x == 0) s_b0 = eready_last_le(a.blocks, R0, wg_at);
  __syncthreads();
  const uint32_t b0 = s_b0;
  {
    const uint64_t p = (uint64_t)b0 * 256 + threadIdx.x;
    s_loc[threadIdx.x] = p < a.n ? loc_of(a.mv + p) : ~0ull;
  }
  __syncthreads();
  const uint64_t r = R0 + threadIdx.x;
  if (r >= a.n_move) return;
  uint32_t b = b0, idx;
  if (b0 + 1 < a.blocks && r >= wg_at(b0 + 1)) {
    const auto later_at = [&](uint32_t k) { return part[2 * (uint64_t)(b0 + 1 + k)]; };
    b = b0 + 1 + eready_last_le(a.blocks - b0 - 1, r, later_at);
  }
  const unsigned long long x = r - wg_at(b);
  if (b == b0) {
    idx = eready_last_le(256, x, [&](uint32_t k) { return s_loc[k]; });
  } else {
    const uint64_t left = a.n - (uint64_t)b * 256;
    const EcompactMove *base = a.mv + (uint64_t)b * 256;
    idx = eready_last_le(left < 256 ? (uint32_t)left : 256u, x, [&](uint32_t k) { return loc_of(base + k); });
  }
  const el_v2 *mq = (const el_v2 *)(a.mv + (uint64_t)b * 256 + idx);
  const el_v2 m0 = mq[0], m1 = mq[1], m2 = mq[2];
  const uint64_t k = x - (OV ? m2.y : m2.x);
  // cannot happen: the offsets are the scan of this class's counts
  if (k >= m0.x || m0.y != (OV ? cs::MOVE_OVERLAP : cs::MOVE_DISJOINT)) return;
  const uint64_t *e = MODE == MV_SCATTER ? (const uint64_t *)(a.stage + r) : (const uint64_t *)(a.p.ents + m1.x + k);
  uint64_t *d = MODE == MV_GATHER ? (uint64_t *)(a.stage + r) : (uint64_t *)(a.p.ents + m1.y + k);
  uint64_t t[5];
#pragma unroll
  for (uint32_t w = 0; w < 5; ++w) t[w] = e[w];
#pragma unroll
  for (uint32_t w = 0; w < 5; ++w) d[w] = t[w];
}
