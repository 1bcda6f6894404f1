// log_append.hip -- the follower's half of a multi-raft replication round:
// handleAppendEntries (raft/raft.go:410-416) over n msgApp, one per raft group,
// with raftLog.maybeAppend, matchTerm, findConflict, append, at, isOutOfBounds
// and lastIndex (raft/log.go:49-84, 115-117, 141-146, 194-217) restated on
// uint64 arithmetic that wraps as Go's does.
//
//   k_lapp_check  one lane per message, nothing modified: the range checks of
//                 the whole call, the claim of the message's group (atomicMin
//                 of the ordinal into claim[G]; whoever finds the word taken
//                 is a second message for that group), and the compact work
//                 list of the messages longer than ELOG_LANE_MAX entries
//                 (one atomicAdd per wave).  The host reads the flag word and
//                 the list's length before anything else is launched.
//   k_lapp_lane   one lane per message of <= ELOG_LANE_MAX entries (heartbeats,
//                 single-entry appends).  Three levels of loads: the app record
//                 (coalesced, transposed through LDS); then the group record and
//                 the entries' terms, which do not depend on each other; then
//                 the matchTerm word and the log terms findConflict compares.
//                 Messages on the work list are skipped, not walked.
//   k_lapp_wave   one wave per message of the work list: lanes take position
//                 from + lane + 64 r, a ballot gives the first mismatch and the
//                 rounds stop at the first one that has any; the appended
//                 suffix's terms are written back 64 a round.
//   k_lapp_sum    n_accepted / n_appended from the per-workgroup partial sums
//                 the two deciding kernels leave (no atomics on one address).
// A message reads its group's window before it writes it (the lane in program
// order, the wave after its last ballot), and different groups' windows do not
// overlap (the caller's contract), so no read sees an append of the same call.
#include "ewal_device.h"
#include "ewal_internal.h"

#define ELOG_LANE_MAX 8u          // entries per message the lane-per-message kernel takes
#define ELOG_MSGAPPRESP 4u        // raft.msgAppResp (raft/raft.go:22-34)

struct ElogHead {
  uint32_t errflag, nlong;
  unsigned long long accepted, appended;
};

struct ElogArgs {
  elog_group *groups;
  uint64_t G;
  uint64_t *terms;
  uint64_t n_terms;
  const elog_app *apps;
  uint64_t n;
  const ewal_entry *ents;
  uint64_t n_ents_total;
  elog_app_result *res;
  emsg_out *resp;                 // nullable
  uint32_t *claim;                // G
  uint32_t *wlist;                // n
  ElogHead *head;
  unsigned long long *partial;    // 2 per workgroup: the lane kernel's, then the wave kernel's
  uint32_t lane_blocks;
};

struct ElogRec {
  uint64_t w[8];
};

// the wave's 64 app records: lane l gets record r0 + l
__device__ __forceinline__ ElogRec load_app(const elog_app *__restrict__ apps, uint64_t n, el_v2 *s_wave,
                                            uint64_t r0, uint32_t lane) {
  el_v2 u[4];
  step_load_wave(apps, n, s_wave, r0, lane, u);
  ElogRec r;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    r.w[2 * k] = u[k].x;
    r.w[2 * k + 1] = u[k].y;
  }
  return r;
}

// One 64-B record at an arbitrary place (a group, or an app in the wave kernel).
__host__ __device__ __forceinline__ ElogRec load_rec(const void *p) {
  const el_v2 *src = (const el_v2 *)p;
  ElogRec r;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const el_v2 v = src[k];
    r.w[2 * k] = v.x;
    r.w[2 * k + 1] = v.y;
  }
  return r;
}

// elog_app's words: group, from, index, log_term, commit, ents_first, n_ents, pad
// elog_group's:     id, term, committed, unstable, log_offset, nlog, terms_off, terms_cap
#define A_GROUP 0
#define A_FROM 1
#define A_INDEX 2
#define A_LOGTERM 3
#define A_COMMIT 4
#define A_FIRST 5
#define A_NENTS 6
#define G_ID 0
#define G_TERM 1
#define G_COMMITTED 2
#define G_UNSTABLE 3
#define G_OFFSET 4
#define G_NLOG 5
#define G_TOFF 6
#define G_TCAP 7

__global__ __launch_bounds__(256) void k_lapp_check(const ElogArgs a) {
  __shared__ el_v2 s_app[4][256];
  const auto [lane, wave, r0, i] = step_lane();
  const ElogRec A = load_app(a.apps, a.n, s_app[wave], r0, lane);
  uint32_t err = 0;
  bool lng = false;
  if (i < a.n) {
    const uint64_t ne = A.w[A_NENTS];
    if (A.w[A_GROUP] >= a.G || ne > a.n_ents_total || A.w[A_FIRST] > a.n_ents_total - ne) {
      err = STEP_ERR_INVAL;
    } else {
      const ElogRec g = load_rec(a.groups + A.w[A_GROUP]);
      const uint64_t cap = g.w[G_TCAP], nlog = g.w[G_NLOG];
      if (cap > a.n_terms || g.w[G_TOFF] > a.n_terms - cap || nlog > cap) err = STEP_ERR_INVAL;
      else if (ne > cap - nlog) err = STEP_ERR_NOMEM;
      // the group's claim: a second message for it finds the word taken
      if (!step_claim(a.claim, A.w[A_GROUP], i)) err |= STEP_ERR_INVAL;
      lng = ne > ELOG_LANE_MAX;
    }
  }
  const unsigned long long mb = __ballot(err != 0), ml = __ballot(lng);
  if (mb) {
    if (err) atomicOr(&a.head->errflag, err);   // one atomic a wave (the compiler folds the active lanes)
  }
  if (ml) {
    const uint32_t first = (uint32_t)__builtin_ctzll(ml);
    uint32_t base = 0;
    if (lane == first) base = atomicAdd(&a.head->nlong, (uint32_t)__popcll(ml));
    base = (uint32_t)__shfl((int)base, (int)first);
    if (lng) a.wlist[base + (uint32_t)__popcll(ml & ((1ull << lane) - 1ull))] = (uint32_t)i;
  }
}

// The per-message functions below are __host__ __device__: a plain C++
// program can call them on host arrays to check the decision logic.
__host__ __device__ __forceinline__ void elog_zero_resp(emsg_out *resp) {
  el_v2 *q = (el_v2 *)resp;
#pragma unroll
  for (uint32_t k = 0; k < 9; ++k) q[k] = el_v2{0, 0};
}

// raftLog.at(index) for matchTerm: 0 nil (reject), 1 an entry (*pos = its place in ents), 2 Go indexes past ents
__host__ __device__ __forceinline__ int elog_at(const ElogRec &g, uint64_t index, uint64_t *pos) {
  const uint64_t off = g.w[G_OFFSET], nlog = g.w[G_NLOG];
  const uint64_t last = nlog - 1 + off;          // lastIndex(), uint64 wrap
  if (index < off || index > last) return 0;     // isOutOfBounds
  *pos = index - off;
  return *pos < nlog ? 1 : 2;
}

// What maybeAppend decided, from the first mismatching position kc among the
// nm entries that lie inside the log (kc == nm: none): the stores to the
// group, d_res[i] and d_resp[i].  The terms' write-back is the caller's, over
// the entries [*kc_out, n_ents) when *n_app_out != 0.
__host__ __device__ __forceinline__ void elog_finish(const ElogArgs &a, uint64_t i, const ElogRec &A,
                                                     const ElogRec &g, int at, bool match, uint64_t kc,
                                                     unsigned long long &acc, unsigned long long &napp,
                                                     uint64_t *kc_out, uint64_t *n_app_out) {
  const uint64_t off = g.w[G_OFFSET], nlog = g.w[G_NLOG], ne = A.w[A_NENTS], index = A.w[A_INDEX];
  const uint64_t last = nlog - 1 + off;
  int32_t status = EWAL_OK, accepted = 0;
  uint64_t ci = 0, n_app = 0, app_first = 0, last_after = last, committed = g.w[G_COMMITTED];
  *kc_out = 0;
  *n_app_out = 0;
  if (at == 2) {
    status = EWAL_PANIC_BOUNDS;
  } else if (at == 1 && match) {
    const uint64_t from = index + 1;
    ci = kc < ne ? from + kc : 0;               // findConflict's return; 0 also when from + kc wrapped to 0
    if (ci != 0 && ci <= committed) {
      status = EWAL_PANIC_COMMITTED_CONFLICT;
      ci = 0;
    } else {
      accepted = 1;
      uint64_t new_nlog = nlog, unstable = g.w[G_UNSTABLE];
      if (ci != 0) {                            // l.append(ci - 1, ents[ci - from:]...)
        n_app = ne - kc;
        app_first = A.w[A_FIRST] + kc;
        new_nlog = ci - off + n_app;
        unstable = unstable < ci ? unstable : ci;
        *kc_out = kc;
        *n_app_out = n_app;
      }
      const uint64_t lastnewi = index + ne;
      const uint64_t tocommit = A.w[A_COMMIT] < lastnewi ? A.w[A_COMMIT] : lastnewi;
      if (committed < tocommit) committed = tocommit;
      last_after = new_nlog - 1 + off;
      el_v2 *gq = (el_v2 *)(a.groups + A.w[A_GROUP]);
      gq[1] = el_v2{committed, unstable};
      ((uint64_t *)gq)[G_NLOG] = new_nlog;
    }
  }
  el_v2 *rq = (el_v2 *)(a.res + i);
  rq[0] = el_v2{(uint64_t)(uint32_t)status | ((uint64_t)(uint32_t)accepted << 32), ci};
  rq[1] = el_v2{app_first, n_app};
  rq[2] = el_v2{last_after, committed};
  if (a.resp) {
    if (status != EWAL_OK) {
      elog_zero_resp(a.resp + i);               // Go panics: nothing is sent
    } else {
      el_v2 *q = (el_v2 *)(a.resp + i);
      q[0] = el_v2{ELOG_MSGAPPRESP, A.w[A_FROM]};
      q[1] = el_v2{g.w[G_ID], g.w[G_TERM]};
      q[2] = el_v2{0, accepted ? last_after : index};
#pragma unroll
      for (uint32_t k = 3; k < 8; ++k) q[k] = el_v2{0, 0};
      q[8] = el_v2{0, accepted ? 0ull : 1ull};   // reject (int32) and pad
    }
  }
  acc += (unsigned long long)accepted;
  napp += n_app;
}

// One message of at most ELOG_LANE_MAX entries, start to finish, in one lane.
__host__ __device__ __forceinline__ void elog_lane_message(const ElogArgs &a, uint64_t i, const ElogRec &A,
                                                           unsigned long long &acc, unsigned long long &napp) {
  const uint64_t ne = A.w[A_NENTS];
  // level 2: the group record and the entries' terms (strided 8-B reads of the 40-B ewal_entry)
  const ElogRec g = load_rec(a.groups + A.w[A_GROUP]);
  uint64_t et[ELOG_LANE_MAX];
#pragma unroll
  for (uint32_t k = 0; k < ELOG_LANE_MAX; ++k) et[k] = k < ne ? a.ents[A.w[A_FIRST] + k].term : 0;
  // level 3: the matchTerm word and the log terms at from + k
  uint64_t pos = 0;
  const int at = elog_at(g, A.w[A_INDEX], &pos);
  const uint64_t *win = a.terms + g.w[G_TOFF];
  const uint64_t after = at == 1 ? g.w[G_NLOG] - 1 - pos : 0;   // lastIndex - index: the positions after index
  const uint64_t nm = ne < after ? ne : after;
  const uint64_t mt = at == 1 ? win[pos] : 0;
  uint64_t lt[ELOG_LANE_MAX];
#pragma unroll
  for (uint32_t k = 0; k < ELOG_LANE_MAX; ++k) lt[k] = k < nm ? win[pos + 1 + k] : 0;
  const bool match = at == 1 && mt == A.w[A_LOGTERM];
  uint64_t kc = nm;
#pragma unroll
  for (int k = (int)ELOG_LANE_MAX - 1; k >= 0; --k)
    if ((uint64_t)k < nm && lt[k] != et[k]) kc = (uint64_t)k;
  uint64_t wk = 0, wn = 0;
  elog_finish(a, i, A, g, at, match, kc, acc, napp, &wk, &wn);
  if (wn) {
    uint64_t *dst = a.terms + g.w[G_TOFF] + pos + 1;
#pragma unroll
    for (uint32_t k = 0; k < ELOG_LANE_MAX; ++k)
      if (k >= wk && k < ne) dst[k] = et[k];
  }
}

__global__ __launch_bounds__(256) void k_lapp_lane(const ElogArgs a) {
  __shared__ el_v2 s_app[4][256];
  const auto [lane, wave, r0, i] = step_lane();
  const ElogRec A = load_app(a.apps, a.n, s_app[wave], r0, lane);
  unsigned long long acc = 0, napp = 0;
  const uint64_t ne = A.w[A_NENTS];
  if (i < a.n && ne <= ELOG_LANE_MAX) elog_lane_message(a, i, A, acc, napp);
  step_block_sums(acc, napp, a.partial, blockIdx.x);
}

__global__ __launch_bounds__(256) void k_lapp_wave(const ElogArgs a, uint32_t nlong) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long acc = 0, napp = 0;
  for (uint64_t w = (uint64_t)blockIdx.x * 4 + wave; w < nlong; w += (uint64_t)gridDim.x * 4) {
    const uint64_t i = a.wlist[w];
    // every lane reads the same two records (one request each)
    const ElogRec A = load_rec(a.apps + i);
    const ElogRec g = load_rec(a.groups + A.w[A_GROUP]);
    const uint64_t ne = A.w[A_NENTS];
    uint64_t pos = 0;
    const int at = elog_at(g, A.w[A_INDEX], &pos);
    uint64_t *win = a.terms + g.w[G_TOFF];
    const bool match = at == 1 && win[pos] == A.w[A_LOGTERM];
    const uint64_t after = at == 1 ? g.w[G_NLOG] - 1 - pos : 0;
    const uint64_t nm = ne < after ? ne : after;
    const ewal_entry *es = a.ents + A.w[A_FIRST];
    uint64_t kc = nm;
    if (match) {
      for (uint64_t k0 = 0; k0 < nm; k0 += 64) {
        const uint64_t k = k0 + lane;
        const bool differ = k < nm && win[pos + 1 + k] != es[k].term;
        const unsigned long long m = __ballot(differ);
        if (m) {
          kc = k0 + (uint64_t)__builtin_ctzll(m);
          break;
        }
      }
    }
    uint64_t wk = 0, wn = 0;
    unsigned long long acc1 = 0, napp1 = 0;
    if (lane == 0) elog_finish(a, i, A, g, at, match, kc, acc1, napp1, &wk, &wn);
    wk = __shfl(wk, 0);
    wn = __shfl(wn, 0);
    acc += acc1;
    napp += napp1;
    if (wn)
      for (uint64_t k = wk + lane; k < ne; k += 64) win[pos + 1 + k] = es[k].term;
  }
  step_block_sums(acc, napp, a.partial, a.lane_blocks + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_lapp_sum(const unsigned long long *__restrict__ partial, uint32_t nslots,
                                                  ElogHead *head) {
  unsigned long long acc = 0, napp = 0;
  for (uint32_t s = threadIdx.x; s < nslots; s += 256) {
    acc += partial[2 * (uint64_t)s];
    napp += partial[2 * (uint64_t)s + 1];
  }
  step_block_sums(acc, napp, &head->accepted, 0);   // accepted, appended: adjacent words
}
