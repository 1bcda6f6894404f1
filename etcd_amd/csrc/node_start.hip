// node_start.hip -- raft.StartNode / raft.RestartNode over n requests on the
// shared group records: what turns a batch replay's result (or a list of peers)
// into the records the step calls run on.  The decisions are node_start.h's
// (shared with the host check); this file is the assignment of work and the
// memory traffic.
//
// Assignment: ONE LANE PER REQUEST validates, decides and writes the five
// records; ONE LANE PER COPIED ENTRY moves RestartNode's entries (the only part
// with real traffic: 40 bytes read, 40 written); ONE LANE PER PEER marshals a
// StartNode entry's ConfChange.
//
//   k_node_count    one lane per request, nothing of the caller's modified: the
//                   request's checks (group, kind, padding, the claim, the
//                   window, the source range, the snapshot and its two ranges,
//                   the peers and their Context ranges), the room (NOMEM), the
//                   decision, and into rec[i] the request's copied entries,
//                   peers and ConfChange bytes with their offsets within the
//                   workgroup; the workgroup's sums into cpart[] (entries, built
//                   requests), dpart[] (bytes) and ppart[] (peers).
//   k_lead_scan     step_common.hip's, three times.  The host reads the flag
//                   word and the totals here -- the one decision point.
//   k_node_apply    one lane per request again: d_res, and with <true> every
//                   word of the five records, d_snaps[g] and, of a StartNode,
//                   the dummy entry and the peers' entry rows (data_off is the
//                   scanned position).  <false> (the size query) writes d_res
//                   alone.
//   k_node_copy     one lane per copied entry: it finds its request by a search
//                   in the scanned offsets, as follow_step.hip's copy pass does,
//                   and moves one ewal_entry, data_off rebased.
//   k_node_marshal  one lane per peer, found the same way: the ConfChange head
//                   and the Context bytes at the place its entry row names.  A
//                   launch after the apply pass: the rows are there.
//
// Uses step_common.hip and ready_step.hip's offset search.
#include "ewal_device.h"
#include "ewal_internal.h"
#include "node_start.h"

namespace ns = node_start;

struct EnodeRec {                   // 48 bytes per request; all 0 unless the request builds a node
  unsigned long long ccnt, cloc;    // kind 1: the copied entries; their offset within the workgroup
  unsigned long long pcnt, ploc;    // kind 2: the peers, likewise
  unsigned long long bytes, dloc;   // kind 2: the ConfChange bytes, likewise
};

struct EnodeArgs {
  elead_group *groups;
  elead_prop_state *pstate;
  evote_state *vstate;
  eready_state *rstate;
  econf_state *cstate;
  elead_snap *snaps;
  uint64_t G;
  ewal_entry *ents;
  uint64_t n_ents_total;
  const ewal_entry *src;
  uint64_t n_src_total;
  const elead_snap *in_snaps;
  uint64_t n_in_snaps;
  const uint64_t *u64;
  uint64_t n_u64;
  const enode_peer *peers;
  uint64_t n_peers_total;
  const uint8_t *ctx;
  uint64_t ctx_len;
  uint8_t *data;
  uint64_t data_base;
  const enode_req *in;
  uint64_t n;
  enode_result *res;
  EleadHead *head, *dhead, *phead;  // copied entries / built requests; bytes; peers
  uint32_t *claim;
  EnodeRec *rec;                    // n
  unsigned long long *cpart, *dpart, *ppart;   // 2 per workgroup each
  uint64_t n_work;                  // the copy and marshal passes: their lanes
  uint32_t blocks;                  // the counting pass's workgroups
};

// one request's words
struct EnodeReq {
  uint64_t group, kind, id, ents_first, ents_cap, src_first, n_src, data_delta, hs_term, hs_vote, hs_commit, snap;
  uint64_t pad;                     // the four padding words OR-ed
};

__device__ __forceinline__ EnodeReq enode_unpack(const el_v2 (&u)[8]) {
  return EnodeReq{u[0].x, u[0].y, u[1].x, u[1].y, u[2].x, u[2].y, u[3].x, u[3].y,
                  u[4].x, u[4].y, u[5].x, u[5].y, u[6].x | u[6].y | u[7].x | u[7].y};
}

// The checks of one request but the claim; a kind-1 request's Snapshot comes
// back in *sn with the places of its two ranges, a kind-2 request's ConfChange
// bytes in *bytes.  0, STEP_ERR_INVAL or STEP_ERR_NOMEM.
__device__ __forceinline__ uint32_t enode_req_check(const EnodeArgs &a, const EnodeReq &r, ns::Snap *sn,
                                                    uint64_t *nodes_off, uint64_t *removed_off, uint64_t *bytes) {
  sn->index = sn->term = sn->n_nodes = sn->n_removed = 0;
  *nodes_off = *removed_off = *bytes = 0;
  if (r.group >= a.G || r.kind > ns::KIND_START || r.pad != 0) return STEP_ERR_INVAL;
  if (r.kind == ns::KIND_NONE) return 0;
  if (r.ents_cap > a.n_ents_total || r.ents_first > a.n_ents_total - r.ents_cap) return STEP_ERR_INVAL;
  if (r.kind == ns::KIND_RESTART) {
    if (r.n_src > a.n_src_total || r.src_first > a.n_src_total - r.n_src) return STEP_ERR_INVAL;
    if (r.snap != ns::NO_SNAP) {
      if (r.snap >= a.n_in_snaps) return STEP_ERR_INVAL;
      const el_v2 *q = (const el_v2 *)(a.in_snaps + r.snap);
      const el_v2 q0 = q[0], q2 = q[2], q3 = q[3];    // index, term | nodes_off, n_nodes | removed_off, n_removed
      if (q2.y > a.n_u64 || q2.x > a.n_u64 - q2.y) return STEP_ERR_INVAL;
      if (q3.y > a.n_u64 || q3.x > a.n_u64 - q3.y) return STEP_ERR_INVAL;
      sn->index = q0.x;
      sn->term = q0.y;
      sn->n_nodes = q2.y;
      sn->n_removed = q3.y;
      *nodes_off = q2.x;
      *removed_off = q3.x;
    }
    return r.n_src > r.ents_cap ? STEP_ERR_NOMEM : 0;
  }
  if (r.n_src > a.n_peers_total || r.src_first > a.n_peers_total - r.n_src) return STEP_ERR_INVAL;
  uint64_t total = 0;
  for (uint64_t j = 0; j < r.n_src; ++j) {
    const el_v2 *q = (const el_v2 *)(a.peers + r.src_first + j);
    const el_v2 q0 = q[0], q1 = q[1];                 // id, ctx_off | ctx_len, pad
    if (q1.y != 0 || q1.x > a.ctx_len || q0.y > a.ctx_len - q1.x) return STEP_ERR_INVAL;
    total += ns::conf_change_size(q0.x, q1.x);
  }
  *bytes = total;
  return r.n_src >= r.ents_cap ? STEP_ERR_NOMEM : 0;   // 1 + n_src > ents_cap
}

// the decision of a request that passed its checks
__device__ __forceinline__ ns::Out enode_build(const EnodeArgs &a, const EnodeReq &r, const ns::Snap &sn,
                                               uint64_t nodes_off, uint64_t removed_off, ns::Node &node) {
  const ns::Req rq{r.kind, r.id, r.n_src, r.hs_term, r.hs_vote, r.hs_commit, r.snap != ns::NO_SNAP};
  const auto node_at = [&](uint64_t j) { return a.u64[nodes_off + j]; };
  const auto rem_at = [&](uint64_t j) { return a.u64[removed_off + j]; };
  return ns::build(node, rq, sn, node_at, rem_at);
}

__global__ __launch_bounds__(256) void k_node_count(const EnodeArgs a) {
  __shared__ el_v2 s_rec[4][512];
  const auto [lane, wave, r0, i] = step_lane();
  el_v2 u[8];
  step_load_wave(a.in, a.n, s_rec[wave], r0, lane, u);
  const EnodeReq r = enode_unpack(u);
  const bool valid = i < a.n;
  uint32_t err = 0;
  EnodeRec rec{0, 0, 0, 0, 0, 0};
  unsigned long long built = 0;
  if (valid) {
    ns::Snap sn;
    uint64_t nodes_off = 0, removed_off = 0, bytes = 0;
    err = enode_req_check(a, r, &sn, &nodes_off, &removed_off, &bytes);
    // the group's claim: a second request finds the word taken
    if (r.group < a.G && !step_claim(a.claim, r.group, i)) err |= STEP_ERR_INVAL;
    if (!err && r.kind != ns::KIND_NONE) {
      ns::Node node;
      if (enode_build(a, r, sn, nodes_off, removed_off, node).status == ns::ST_OK) {
        built = 1;
        if (r.kind == ns::KIND_RESTART) rec.ccnt = r.n_src;
        if (r.kind == ns::KIND_START) rec.pcnt = r.n_src, rec.bytes = bytes;
      }
    }
  }
  step_flag(a.head, err);
  unsigned long long total = 0;
  rec.cloc = step_block_scan(rec.ccnt, &total);
  rec.ploc = step_block_scan(rec.pcnt, &total);
  rec.dloc = step_block_scan(rec.bytes, &total);
  if (valid) {
    el_v2 *q = (el_v2 *)(a.rec + i);
    q[0] = el_v2{rec.ccnt, rec.cloc};
    q[1] = el_v2{rec.pcnt, rec.ploc};
    q[2] = el_v2{rec.bytes, rec.dloc};
  }
  step_block_sums(rec.ccnt, built, a.cpart, blockIdx.x);
  __syncthreads();                                   // the sums' staging words are reused
  step_block_sums(rec.bytes, 0, a.dpart, blockIdx.x);
  __syncthreads();
  step_block_sums(rec.pcnt, 0, a.ppart, blockIdx.x);
}

template <uint32_t W>
__device__ __forceinline__ void enode_store(void *dst, const uint64_t (&w)[W]) {
  el_v2 *q = (el_v2 *)dst;
#pragma unroll
  for (uint32_t k = 0; k < W / 2; ++k) q[k] = el_v2{w[2 * k], w[2 * k + 1]};
}

template <bool WRITE>
__global__ __launch_bounds__(256) void k_node_apply(const EnodeArgs a) {
  __shared__ el_v2 s_rec[4][512];
  const auto [lane, wave, r0, i] = step_lane();
  el_v2 u[8];
  step_load_wave(a.in, a.n, s_rec[wave], r0, lane, u);
  const EnodeReq r = enode_unpack(u);
  if (i >= a.n) return;
  ns::Snap sn;
  uint64_t nodes_off = 0, removed_off = 0, bytes = 0;
  (void)enode_req_check(a, r, &sn, &nodes_off, &removed_off, &bytes);
  ns::Node node;
  const ns::Out o = enode_build(a, r, sn, nodes_off, removed_off, node);
  const bool built = r.kind != ns::KIND_NONE && o.status == ns::ST_OK;
  const uint64_t data_first = built && r.kind == ns::KIND_START ? a.dpart[2 * (uint64_t)blockIdx.x] + a.rec[i].dloc : 0;
  el_v2 *rq = (el_v2 *)(a.res + i);
  rq[0] = el_v2{(uint64_t)(uint32_t)o.status | ((uint64_t)(uint32_t)o.action << 32), built ? node.nlog : 0};
  rq[1] = el_v2{built ? node.committed : 0, built ? node.off : 0};
  rq[2] = el_v2{built ? node.np : 0, data_first};
  if (!WRITE || !built) return;
  const uint64_t g = r.group;
  uint64_t gw[32], pw[4], vw[8], rw[8], cw[16];
  ns::words(node, r.ents_first, r.ents_cap, gw, pw, vw, rw, cw);
  enode_store(a.groups + g, gw);
  enode_store(a.pstate + g, pw);
  enode_store(a.vstate + g, vw);
  enode_store(a.rstate + g, rw);
  enode_store(a.cstate + g, cw);
  el_v2 *to = (el_v2 *)(a.snaps + g);
  if (node.restored) {                               // raftLog.snapshot = s
    const el_v2 *from = (const el_v2 *)(a.in_snaps + r.snap);
    const el_v2 x0 = from[0], x1 = from[1], x2 = from[2], x3 = from[3];
    to[0] = x0, to[1] = x1, to[2] = x2, to[3] = x3;
  } else {
    to[0] = to[1] = to[2] = to[3] = el_v2{0, 0};
  }
  if (r.kind == ns::KIND_START) {                    // the dummy entry, then one EntryConfChange per peer
    uint64_t *e = (uint64_t *)(a.ents + r.ents_first);
    e[0] = e[1] = e[2] = e[3] = 0;
    e[4] = 1ull << 32;
    uint64_t at = a.data_base + data_first;
    for (uint64_t j = 0; j < r.n_src; ++j) {
      const el_v2 *q = (const el_v2 *)(a.peers + r.src_first + j);
      const uint64_t sz = ns::conf_change_size(q[0].x, q[1].x);
      e += 5;
      e[0] = 1, e[1] = j + 1, e[2] = at, e[3] = sz, e[4] = 1;
      at += sz;
    }
  }
}

// The request a lane of the copy or marshal pass works for, and its ordinal
// within it: part[] holds the workgroups' scanned offsets, loc_at(p) request
// p's offset within its workgroup.  Every thread of the workgroup calls it.
template <class LocAt>
__device__ __forceinline__ uint64_t enode_locate(const EnodeArgs &a, const unsigned long long *part, uint64_t r,
                                                 const LocAt &loc_at, uint64_t *k) {
  __shared__ unsigned long long s_loc[256];
  __shared__ uint32_t s_b0;
  const uint64_t R0 = (uint64_t)blockIdx.x * 256;
  const auto wg_at = [&](uint32_t b) { return part[2 * (uint64_t)b]; };
  if (threadIdx.x == 0) s_b0 = eready_last_le(a.blocks, R0, wg_at);
  __syncthreads();
  const uint32_t b0 = s_b0;
  {
    const uint64_t p = (uint64_t)b0 * 256 + threadIdx.x;
    s_loc[threadIdx.x] = p < a.n ? loc_at(p) : ~0ull;
  }
  __syncthreads();
  uint32_t b = b0, idx;
  if (b0 + 1 < a.blocks && r >= wg_at(b0 + 1)) {
    const auto later_at = [&](uint32_t j) { return part[2 * (uint64_t)(b0 + 1 + j)]; };
    b = b0 + 1 + eready_last_le(a.blocks - b0 - 1, r, later_at);
  }
  const unsigned long long x = r - wg_at(b);
  if (b == b0) {
    idx = eready_last_le(256, x, [&](uint32_t j) { return s_loc[j]; });
  } else {
    const uint64_t left = a.n - (uint64_t)b * 256;
    const uint64_t base = (uint64_t)b * 256;
    idx = eready_last_le(left < 256 ? (uint32_t)left : 256u, x, [&](uint32_t j) { return loc_at(base + j); });
  }
  const uint64_t p = (uint64_t)b * 256 + idx;
  *k = x - loc_at(p);
  return p;
}

__global__ __launch_bounds__(256) void k_node_copy(const EnodeArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t k = 0;
  const uint64_t p = enode_locate(a, a.cpart, r < a.n_work ? r : a.n_work - 1, [&](uint64_t q) { return a.rec[q].cloc; }, &k);
  if (r >= a.n_work || k >= a.rec[p].ccnt) return;   // the second cannot happen: the offsets are the counts' scan
  const el_v2 *rq = (const el_v2 *)(a.in + p);
  const el_v2 q1 = rq[1], q2 = rq[2], q3 = rq[3];    // id, ents_first | ents_cap, src_first | n_src, data_delta
  const uint64_t *e = (const uint64_t *)(a.src + q2.y + k);
  uint64_t t[5];
#pragma unroll
  for (uint32_t w = 0; w < 5; ++w) t[w] = e[w];
  if ((uint32_t)(t[4] >> 32) == 0) t[2] += q3.y;     // data_nil == 0: Data is a range of the WAL buffer
  uint64_t *d = (uint64_t *)(a.ents + q1.y + k);
#pragma unroll
  for (uint32_t w = 0; w < 5; ++w) d[w] = t[w];
}

__global__ __launch_bounds__(256) void k_node_marshal(const EnodeArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t k = 0;
  const uint64_t p = enode_locate(a, a.ppart, r < a.n_work ? r : a.n_work - 1, [&](uint64_t q) { return a.rec[q].ploc; }, &k);
  if (r >= a.n_work || k >= a.rec[p].pcnt) return;
  const el_v2 *rq = (const el_v2 *)(a.in + p);
  const el_v2 q1 = rq[1], q2 = rq[2];                // id, ents_first | ents_cap, src_first
  const el_v2 *pq = (const el_v2 *)(a.peers + q2.y + k);
  const el_v2 p0 = pq[0], p1 = pq[1];                // id, ctx_off | ctx_len, pad
  const uint64_t at = ((const uint64_t *)(a.ents + q1.y + 1 + k))[2] - a.data_base;   // the row the apply pass wrote
  uint8_t head[ns::CONF_HEAD_MAX];
  const uint32_t hl = (uint32_t)(ns::conf_change_head(head, p0.x, p1.x) - head);
  uint8_t *o = a.data + at;
  for (uint32_t b = 0; b < hl; ++b) o[b] = head[b];
  const uint8_t *c = a.ctx + p0.y;
  for (uint64_t b = 0; b < p1.x; ++b) o[hl + b] = c[b];
}
