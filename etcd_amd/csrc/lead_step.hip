// lead_step.hip -- the leader's half of a multi-raft replication round:
// stepLeader's msgAppResp case (raft/raft.go:456-466) over n msgAppResp, with
// the term switch of Step (:393-405), progress.update / maybeDecrTo (:71-90),
// raft.maybeCommit (:248-258, raft/log.go:148-154), sendAppend / bcastAppend
// (:202-236), needSnapshot (:556-564) and raftLog.term / entries / at / slice /
// isOutOfBounds / lastIndex (log.go:115-134, 194-217) restated on uint64
// arithmetic that wraps as Go's does.
//
// Assignment: ONE LANE PER RUN HEAD.  The responses of one group are adjacent
// (the caller's contract, checked); response i is a run head when i == 0 or
// d_resps[i - 1] names another group.  The head's lane loads the group's
// 256-B record once, keeps id, term, committed, the log window and the seven
// (peer_id, match, next) triples in registers, and steps its run in array
// order, reading the run's later responses from global memory, wherever the
// run ends: a run may straddle any wave or workgroup boundary, no lane but
// its head looks at it.  The other lanes only load their own response (to
// tell whether they are heads) and take part in the sums.
//
//   k_lead_count  one lane per response, nothing of the caller's modified: the
//                 checks of the whole call (group < G, the group's claim --
//                 atomicMin of the head's ordinal into claim[G]; a head that
//                 finds the word taken is a second run of that group --, the
//                 entry window, distinct peer ids, reserved words), then a
//                 replay of the run in registers that only counts: the
//                 messages of the run into run_msgs[head] (0 at the other
//                 responses) and the workgroup's sums of messages and of
//                 committing responses into partial[2 b], [2 b + 1].
//   k_lead_scan   step_common.hip's, one workgroup: the exclusive prefix sum of
//                 the workgroups' message counts in place, the two totals
//                 into the head words.
//                 The host reads the flag word and the totals here -- the one
//                 decision point (INVAL, NOMEM, the size query's answer).
//   k_lead_apply  one lane per response again: a workgroup-wide exclusive scan
//                 of run_msgs plus the workgroup's offset places each run's
//                 messages (dense, by response, then by peer slot); the head
//                 replays the run, writes d_res, the messages, and of its
//                 record only the words that changed.  <false> writes d_res
//                 alone (the size query).
// The counters are per-workgroup partial sums (no atomics on one address).
// The response records are loaded coalesced and transposed through LDS, as
// log_append.hip's app records are; a group record is sixteen 16-B loads of
// its head's lane (256 contiguous bytes, all in flight together).  A run's
// loads depend on each other (response -> record -> the quorum index's term ->
// the next response), so the run loop keeps the next response's load in flight
// during a step, whether a send would panic is decided by arithmetic alone (no
// load), and the counting pass reads no entry but the quorum index's.  The
// results and messages are stored by the head's lane, 16 B a store (not
// coalesced across lanes): DESIGN.md has what that costs.
#include "ewal_device.h"
#include "ewal_internal.h"

#define ELEAD_PEERS 7u
#define ELEAD_MSGAPP 3u           // raft.msgApp (raft/raft.go:22-34)
#define ELEAD_MSGSNAP 7u          // raft.msgSnap

struct EleadArgs {
  elead_group *groups;
  uint64_t G;
  const elead_snap *snaps;        // nullable
  const ewal_entry *ents;
  uint64_t n_ents_total;
  const elead_resp *resps;
  uint64_t n;
  elead_result *res;
  emsg_out *msgs;                 // NULL: the size query
  uint32_t *claim;                // G
  unsigned long long *run_msgs;   // n
  unsigned long long *partial;    // 2 per workgroup
  EleadHead *head;
};

// one response's words: group, from, term, index, reject | pad << 32, pad2
struct EleadResp {
  uint64_t group, from, term, index;
  bool reject;
};

// a group record in registers; every access to the arrays is by a constant
// index of an unrolled loop, so they stay in registers
struct EleadState {
  uint64_t id, term, committed, off, nlog, efirst, np;
  uint64_t pid[ELEAD_PEERS], match[ELEAD_PEERS], next[ELEAD_PEERS];
};

struct EleadMsg {
  uint64_t type, index, log_term, efirst, nents;
};

// the wave's 64 response records: lane l gets record r0 + l
__device__ __forceinline__ EleadResp elead_load_resp_wave(const elead_resp *__restrict__ resps, uint64_t n,
                                                          el_v2 *s_wave, uint64_t r0, uint32_t lane) {
  el_v2 u[3];
  step_load_wave(resps, n, s_wave, r0, lane, u);
  const el_v2 a = u[0], b = u[1], c = u[2];
  EleadResp r;
  r.group = a.x;
  r.from = a.y;
  r.term = b.x;
  r.index = b.y;
  r.reject = (uint32_t)c.x != 0;
  return r;
}

// One response at an arbitrary place (a run's later responses).
__host__ __device__ __forceinline__ EleadResp elead_load_resp(const elead_resp *p) {
  const el_v2 *src = (const el_v2 *)p;
  const el_v2 a = src[0], b = src[1];
  EleadResp r;
  r.group = a.x;
  r.from = a.y;
  r.term = b.x;
  r.index = b.y;
  r.reject = p->reject != 0;
  return r;
}

// The group's record; returns the OR of its reserved words.
__host__ __device__ __forceinline__ uint64_t elead_load_group(const elead_group *p, EleadState &s) {
  const el_v2 *src = (const el_v2 *)p;
  uint64_t w[32];
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k) {
    const el_v2 v = src[k];
    w[2 * k] = v.x;
    w[2 * k + 1] = v.y;
  }
  s.id = w[0];
  s.term = w[1];
  s.committed = w[2];
  s.off = w[3];
  s.nlog = w[4];
  s.efirst = w[5];
  s.np = w[6];
#pragma unroll
  for (uint32_t k = 0; k < ELEAD_PEERS; ++k) {
    s.pid[k] = w[7 + k];
    s.match[k] = w[14 + k];
    s.next[k] = w[21 + k];
  }
  return w[28] | w[29] | w[30] | w[31];
}

// raftLog.term(i): 0 where at(i) is nil; EWAL_PANIC_BOUNDS where Go indexes past ents.
// LOAD false: only the status (it does not depend on the entry), *t = 0, no memory is read.
template <bool LOAD>
__host__ __device__ __forceinline__ int elead_term(const EleadArgs &a, const EleadState &s, uint64_t i, uint64_t *t) {
  const uint64_t last = s.nlog - 1 + s.off;        // lastIndex(), uint64 wrap
  *t = 0;
  if (i < s.off || i > last) return EWAL_OK;       // isOutOfBounds
  const uint64_t pos = i - s.off;
  if (pos >= s.nlog) return EWAL_PANIC_BOUNDS;
  if (LOAD) *t = a.ents[s.efirst + pos].term;
  return EWAL_OK;
}

// sendAppend for a peer whose Progress.next is `next`: the message's fields, or
// the class of Go's panic.  Nothing is stored.  LOAD false: the class alone,
// without the read of log_term's entry (no class depends on it).
template <bool LOAD>
__host__ __device__ __forceinline__ int elead_send(const EleadArgs &a, const EleadState &s, uint64_t g, uint64_t next,
                                                   EleadMsg *m) {
  const uint64_t index = next - 1;
  m->index = index;
  m->log_term = 0;
  m->efirst = 0;
  m->nents = 0;
  if (index < s.off) {                             // needSnapshot
    m->type = ELEAD_MSGSNAP;
    if (!a.snaps || a.snaps[g].term == 0) return EWAL_PANIC_NEED_SNAPSHOT;
    return EWAL_OK;
  }
  m->type = ELEAD_MSGAPP;
  const int st = elead_term<LOAD>(a, s, index, &m->log_term);
  if (st != EWAL_OK) return st;
  if (next == s.off) return EWAL_PANIC_FIRST_ENTRY;   // entries(i) with i == offset
  // slice(next, lastIndex() + 1)
  const uint64_t last = s.nlog - 1 + s.off, hi = last + 1;
  if (next >= hi) return EWAL_OK;                  // nil
  if (next < s.off || next > last) return EWAL_OK; // isOutOfBounds(lo); that of hi - 1 = lastIndex is last < off, which makes this one true
  const uint64_t lo_p = next - s.off, hi_p = hi - s.off;
  if (lo_p > hi_p || hi_p > s.nlog) return EWAL_PANIC_BOUNDS;
  m->efirst = s.efirst + lo_p;
  m->nents = hi_p - lo_p;
  return EWAL_OK;
}

// the emsg_out of one sendAppend, after send (raft.go:190-199)
__host__ __device__ __forceinline__ void elead_store_msg(const EleadArgs &a, emsg_out *dst, const EleadState &s,
                                                         uint64_t g, uint64_t to, const EleadMsg &m) {
  el_v2 *q = (el_v2 *)dst;
  q[0] = el_v2{m.type, to};
  q[1] = el_v2{s.id, s.term};
  q[2] = el_v2{m.log_term, m.index};
  if (m.type == ELEAD_MSGSNAP) {
    const el_v2 *sn = (const el_v2 *)(a.snaps + g);
    const el_v2 s0 = sn[0], s1 = sn[1], s2 = sn[2], s3 = sn[3];
    q[3] = el_v2{0, 0};
    q[4] = el_v2{0, s0.x};
    q[5] = el_v2{s0.y, s1.x};
    q[6] = el_v2{s1.y, s2.x};
    q[7] = el_v2{s2.y, s3.x};
    q[8] = el_v2{s3.y, 0};
  } else {
    q[3] = el_v2{s.committed, m.efirst};
    q[4] = el_v2{m.nents, 0};
#pragma unroll
    for (uint32_t k = 5; k < 9; ++k) q[k] = el_v2{0, 0};
  }
}

// r.prs[from]: its slot among the first n_peers (-1: nil) and its match / next (0, 0)
__host__ __device__ __forceinline__ int elead_lookup(const EleadState &s, uint64_t from, uint64_t *match,
                                                     uint64_t *next) {
  int slot = -1;
  *match = 0;
  *next = 0;
#pragma unroll
  for (int k = (int)ELEAD_PEERS - 1; k >= 0; --k)
    if ((uint64_t)k < s.np && s.pid[k] == from) {
      slot = k;
      *match = s.match[k];
      *next = s.next[k];
    }
  return slot;
}

struct EleadOut {
  int32_t status, action;
  uint64_t n_msgs, match, next;   // prs[from] after the response
};

// One response on the state s its predecessors left.  On a panic s is as it
// was.  EMIT: the messages go to a.msgs[msg_first ...]; `dirty` collects the
// peer slots whose match / next changed.
template <bool EMIT>
__host__ __device__ __forceinline__ EleadOut elead_step(const EleadArgs &a, EleadState &s, uint64_t g,
                                                        const EleadResp &r, uint64_t msg_first, uint32_t &dirty) {
  EleadOut o;
  o.status = EWAL_OK;
  o.action = ELEAD_NOT_STEPPED;
  o.n_msgs = 0;
  uint64_t cm = 0, cn = 0;
  const int slot = elead_lookup(s, r.from, &cm, &cn);
  o.match = cm;
  o.next = cn;
  if (r.term != 0 && r.term < s.term) {
    o.action = ELEAD_IGNORED;
    return o;
  }
  if (r.term > s.term) {
    o.action = ELEAD_STEP_DOWN;
    return o;
  }
  o.action = ELEAD_PANICKED;
  if (slot < 0) {
    o.status = EWAL_PANIC_NIL_PROGRESS;
    return o;
  }
  if (r.reject) {
    if (cm != 0 || cn - 1 != r.index) {            // maybeDecrTo
      o.action = ELEAD_STALE;
      return o;
    }
    uint64_t nn = cn - 1;
    if (nn < 1) nn = 1;
    EleadMsg m;
    o.status = elead_send<EMIT>(a, s, g, nn, &m);
    if (o.status != EWAL_OK) return o;
#pragma unroll
    for (int k = 0; k < (int)ELEAD_PEERS; ++k)
      if (k == slot) s.next[k] = nn;
    dirty |= 1u << slot;
    if (EMIT) elead_store_msg(a, a.msgs + msg_first, s, g, r.from, m);
    o.action = ELEAD_PROBE;
    o.n_msgs = 1;
    o.next = nn;
    return o;
  }
  // update(index), then maybeCommit on the match values it leaves
  const uint64_t nm = r.index, nn = r.index + 1;
  uint64_t mt[ELEAD_PEERS], nx[ELEAD_PEERS];
#pragma unroll
  for (int k = 0; k < (int)ELEAD_PEERS; ++k) {
    mt[k] = k == slot ? nm : s.match[k];
    nx[k] = k == slot ? nn : s.next[k];
  }
  const uint64_t q = s.np / 2 + 1;
  uint64_t mci = 0;
#pragma unroll
  for (int k = 0; k < (int)ELEAD_PEERS; ++k) {
    uint64_t above = 0, same = 0;
#pragma unroll
    for (int j = 0; j < (int)ELEAD_PEERS; ++j) {
      above += ((uint64_t)j < s.np && mt[j] > mt[k]) ? 1 : 0;
      same += ((uint64_t)j < s.np && mt[j] == mt[k]) ? 1 : 0;
    }
    if ((uint64_t)k < s.np && above < q && q <= above + same) mci = mt[k];   // the q-th largest
  }
  bool commit = false;
  if (mci > s.committed) {
    uint64_t t = 0;
    o.status = elead_term<true>(a, s, mci, &t);
    if (o.status != EWAL_OK) return o;
    commit = t == s.term;
  }
  if (commit) {
    // bcastAppend would panic at its k-th message: find that out (arithmetic alone) before anything is stored
    uint64_t cnt = 0;
#pragma unroll
    for (int k = 0; k < (int)ELEAD_PEERS; ++k)
      if ((uint64_t)k < s.np && s.pid[k] != s.id && o.status == EWAL_OK) {
        EleadMsg m;
        o.status = elead_send<false>(a, s, g, nx[k], &m);
        ++cnt;
      }
    if (o.status != EWAL_OK) return o;
    s.committed = mci;
    o.n_msgs = cnt;
    if (EMIT) {
      uint64_t j = 0;
#pragma unroll
      for (int k = 0; k < (int)ELEAD_PEERS; ++k)
        if ((uint64_t)k < s.np && s.pid[k] != s.id) {
          EleadMsg m;
          (void)elead_send<true>(a, s, g, nx[k], &m);
          elead_store_msg(a, a.msgs + msg_first + j, s, g, s.pid[k], m);
          ++j;
        }
    }
  }
#pragma unroll
  for (int k = 0; k < (int)ELEAD_PEERS; ++k) {
    s.match[k] = mt[k];
    s.next[k] = nx[k];
  }
  dirty |= 1u << slot;
  o.action = commit ? ELEAD_COMMITTED : ELEAD_UPDATED;
  o.match = nm;
  o.next = nn;
  return o;
}

// The run of group g headed at response i (r0), on the record as it stands:
// steps it in order, writes d_res when write_res, and with EMIT the messages
// from msg_first on and the record's changed words.  Adds the run's messages
// and committing responses to tot / ncommit.
template <bool EMIT>
__host__ __device__ __forceinline__ void elead_run(const EleadArgs &a, uint64_t i, const EleadResp &r0,
                                                   EleadState s, bool write_res, uint64_t msg_first,
                                                   unsigned long long &tot, unsigned long long &ncommit) {
  const uint64_t g = r0.group, committed0 = s.committed;
  const bool unsupported = s.np > ELEAD_PEERS;
  if (unsupported) s.np = 0;                       // no peer is looked up: match / next are reported as 0
  bool stopped = false;
  uint32_t dirty = 0;
  EleadResp r = r0, ahead = r0;
  bool more = i + 1 < a.n;
  if (more) ahead = elead_load_resp(a.resps + i + 1);   // one response ahead: its load is in flight during the step
  for (uint64_t k = i;;) {
    EleadOut o;
    if (stopped || unsupported) {
      (void)elead_lookup(s, r.from, &o.match, &o.next);
      o.n_msgs = 0;
      o.action = stopped ? ELEAD_NOT_STEPPED : ELEAD_PANICKED;
      o.status = stopped ? EWAL_OK : EWAL_UNSUPPORTED_ENCODING;
      stopped = true;
    } else {
      o = elead_step<EMIT>(a, s, g, r, msg_first, dirty);
      stopped = o.action == ELEAD_STEP_DOWN || o.status != EWAL_OK;
    }
    if (write_res) {
      el_v2 *rq = (el_v2 *)(a.res + k);
      rq[0] = el_v2{(uint64_t)(uint32_t)o.status | ((uint64_t)(uint32_t)o.action << 32), msg_first};
      rq[1] = el_v2{o.n_msgs, s.committed};
      rq[2] = el_v2{o.match, o.next};
    }
    msg_first += o.n_msgs;
    tot += o.n_msgs;
    ncommit += o.action == ELEAD_COMMITTED ? 1 : 0;
    ++k;
    if (!more || ahead.group != g) break;
    r = ahead;
    more = k + 1 < a.n;
    if (more) ahead = elead_load_resp(a.resps + k + 1);
  }
  if (EMIT) {
    uint64_t *gw = (uint64_t *)(a.groups + g);
    if (s.committed != committed0) gw[2] = s.committed;
#pragma unroll
    for (uint32_t k = 0; k < ELEAD_PEERS; ++k)
      if (dirty & (1u << k)) {
        gw[14 + k] = s.match[k];
        gw[21 + k] = s.next[k];
      }
  }
}

// The checks of a run head's record (group < G is its caller's).
__host__ __device__ __forceinline__ bool elead_group_ok(const EleadArgs &a, const EleadState &s, uint64_t reserved) {
  if (reserved != 0) return false;
  if (s.nlog > a.n_ents_total || s.efirst > a.n_ents_total - s.nlog) return false;
  bool dup = false;
#pragma unroll
  for (uint32_t k = 0; k < ELEAD_PEERS; ++k)
#pragma unroll
    for (uint32_t j = k + 1; j < ELEAD_PEERS; ++j)
      dup |= j < s.np && s.pid[j] == s.pid[k];
  return !dup;
}

__global__ __launch_bounds__(256) void k_lead_count(const EleadArgs a) {
  __shared__ el_v2 s_resp[4][192];
  const auto [lane, wave, r0, i] = step_lane();
  const EleadResp r = elead_load_resp_wave(a.resps, a.n, s_resp[wave], r0, lane);
  const bool head = step_is_head(a.resps, a.n, i, r.group, lane);
  uint32_t err = 0;
  unsigned long long tot = 0, ncommit = 0;
  if (i < a.n && r.group >= a.G) err = STEP_ERR_INVAL;
  if (head && !err) {
    EleadState s;
    const uint64_t reserved = elead_load_group(a.groups + r.group, s);
    // the group's claim: the head of a second run finds the word taken
    if (!step_claim(a.claim, r.group, i)) err = STEP_ERR_INVAL;
    if (!elead_group_ok(a, s, reserved)) err = STEP_ERR_INVAL;
    if (!err) elead_run<false>(a, i, r, s, false, 0, tot, ncommit);
  }
  step_flag(a.head, err);
  if (i < a.n) a.run_msgs[i] = tot;
  step_block_sums(tot, ncommit, a.partial, blockIdx.x);
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_lead_apply(const EleadArgs a) {
  __shared__ el_v2 s_resp[4][192];
  const auto [lane, wave, r0, i] = step_lane();
  const EleadResp r = elead_load_resp_wave(a.resps, a.n, s_resp[wave], r0, lane);
  const bool head = step_is_head(a.resps, a.n, i, r.group, lane);
  unsigned long long total = 0;
  const unsigned long long before = step_block_scan(i < a.n ? a.run_msgs[i] : 0, &total);
  if (head) {
    EleadState s;
    (void)elead_load_group(a.groups + r.group, s);
    unsigned long long tot = 0, ncommit = 0;
    elead_run<EMIT>(a, i, r, s, true, a.partial[2 * (uint64_t)blockIdx.x] + before, tot, ncommit);
  }
}
