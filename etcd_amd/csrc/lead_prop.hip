// lead_prop.hip -- the start of a multi-raft replication round: stepLeader's
// msgProp and msgBeat cases (raft/raft.go:441-455) over n local messages.  The
// decisions are lead_prop_step.h's (shared with the host check); this file is
// the assignment of work and the memory traffic.
//
// Assignment: ONE LANE PER RECORD.  The records of one group are adjacent (the
// caller's contract, checked); a run's record j needs of its predecessors only
// two counts -- the proposals and the ConfChange proposals among the run's
// records <= j -- and the run's start state, which every lane of the run reads
// for itself (the group's 256-B record and its 32-B state record; the lanes of
// a run read the same lines).  The counts are one segmented inclusive scan,
// keyed on "record j - 1 names another group", of a packed word (proposals in
// the low half, ConfChanges in the high half):
//
//   k_prop_check  one lane per record, nothing of the caller's modified: the
//                 checks of a record (group < G, kind, data_nil, the Data
//                 range) and, by a run's head, of its group (the claim as in
//                 lead_step.hip, the entry window, distinct peer ids, reserved
//                 words, pending_conf).  The segmented scan within the wave
//                 (cross-lane) and the workgroup (LDS): seg[i] = the counts
//                 since the run's head or the workgroup's first record, bit 63:
//                 the run started in an earlier workgroup; agg[b] = the
//                 workgroup's trailing segment and whether it holds a head.
//   k_prop_carry  one workgroup: the segmented exclusive scan of agg in place
//                 (a thread owns a contiguous chunk) -- agg[b] becomes what a
//                 run that enters workgroup b brings along.  No workgroup ever
//                 waits for another.
//   k_prop_count  one lane per record: its counts, its group's start state,
//                 the run's mode and the record's messages into cnt[i]; the
//                 run's last record checks the room for the run's proposals
//                 (NOMEM).  Per-workgroup sums of messages and appended
//                 entries into partial[] (no atomics on one address).
//   k_lead_scan   step_common.hip's: the workgroups' message offsets and the
//                 totals.  The host reads the flag word and the totals here --
//                 the one decision point (INVAL, NOMEM, the size query).
//   k_prop_apply  one lane per record: d_res, and with EMIT the record's own
//                 entry and its own messages.  <false> writes d_res alone.
//   k_prop_commit one lane per record: a closed run's last record writes the
//                 group's and the state record's changed words.  It is a kernel
//                 of its own because the lanes of a run read the start state
//                 throughout k_prop_apply.
//
// A run outside the closed form's domain (lead_prop::prepare: a wrap, an empty
// log, term 0, id not among the peers, more than 7 peers, a peer whose
// sendAppend panics) is SERIAL: its head's lane replays it with the shared
// serial step, in k_prop_count (counting), in k_prop_apply (writing, the
// group's words included: no other lane of a serial run reads the group there
// -- cnt[i] carries the mode).  Correctness first; such runs are rare.
#include "ewal_device.h"
#include "ewal_internal.h"
#include "lead_prop_step.h"

#define EPROP_SERIAL (1ull << 63)   // cnt[i]: the record's run is serial
#define EPROP_OPEN (1ull << 63)     // seg[i]: the run started in an earlier workgroup
#define EPROP_LOW 0xFFFFFFFFull

struct EpropAgg {
  unsigned long long val, head;     // the trailing segment's counts; whether the workgroup holds a run head
};

struct EpropArgs {
  elead_group *groups;
  elead_prop_state *state;
  uint64_t G;
  const elead_snap *snaps;          // nullable
  ewal_entry *ents;
  uint64_t n_ents_total, data_len_total;
  const elead_local *locals;
  uint64_t n;
  elead_local_result *res;
  emsg_out *msgs;                   // NULL: the size query
  uint32_t *claim;                  // G
  unsigned long long *seg;          // n
  unsigned long long *cnt;          // n
  EpropAgg *agg;                    // per workgroup
  unsigned long long *partial;      // 2 per workgroup
  EleadHead *head;
};

// one local message's words: group, kind, etype | data_nil << 32, data_off, data_len, pad
struct EpropRec {
  uint64_t group, kind, tn, data_off, data_len;
};

__device__ __forceinline__ EpropRec eprop_unpack(const el_v2 (&u)[3]) {
  return EpropRec{u[0].x, u[0].y, u[1].x, u[1].y, u[2].x};
}

// the wave's 64 records: lane l gets record r0 + l
__device__ __forceinline__ EpropRec eprop_load_wave(const elead_local *__restrict__ locals, uint64_t n, el_v2 *s_wave,
                                                    uint64_t r0, uint32_t lane) {
  el_v2 u[3];
  step_load_wave(locals, n, s_wave, r0, lane, u);
  return eprop_unpack(u);
}

// One record at an arbitrary place (a serial run's later records).
__device__ __forceinline__ EpropRec eprop_load_rec(const elead_local *p) {
  el_v2 u[3];
  step_load_rec(p, u);
  return eprop_unpack(u);
}

// The group's record and its state record; returns the OR of the reserved words.
__device__ __forceinline__ uint64_t eprop_load_group(const EpropArgs &a, uint64_t g, lp::State &s, uint64_t *cap) {
  const el_v2 *src = (const el_v2 *)(a.groups + g);
  uint64_t w[32];
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k) {
    const el_v2 v = src[k];
    w[2 * k] = v.x;
    w[2 * k + 1] = v.y;
  }
  const el_v2 *sp = (const el_v2 *)(a.state + g);
  const el_v2 s0 = sp[0], s1 = sp[1];
  s.id = w[0];
  s.term = w[1];
  s.committed = w[2];
  s.off = w[3];
  s.nlog = w[4];
  s.efirst = w[5];
  s.np = w[6];
#pragma unroll
  for (uint32_t k = 0; k < lp::PEERS; ++k) {
    s.pid[k] = w[7 + k];
    s.match[k] = w[14 + k];
    s.next[k] = w[21 + k];
  }
  *cap = s0.x;
  s.unstable = s0.y;
  s.pending = s1.x;
  s.fresh = s.nlog;
  s.snap_ok = false;
  return w[28] | w[29] | w[30] | w[31] | s1.y;
}

// raftLog.snapshot.Term != 0, read only for a group that would look at it
__device__ __forceinline__ void eprop_load_snap(const EpropArgs &a, uint64_t g, lp::State &s) {
  if (a.snaps && s.np <= lp::PEERS && lp::wants_snapshot(s)) s.snap_ok = a.snaps[g].term != 0;
}

// the checks of a run head's group (group < G is its caller's)
__device__ __forceinline__ bool eprop_group_ok(const EpropArgs &a, const lp::State &s, uint64_t cap, uint64_t reserved) {
  if (reserved != 0 || s.pending > 1) return false;
  if (cap > a.n_ents_total || s.efirst > a.n_ents_total - cap || s.nlog > cap) return false;
  bool dup = false;
#pragma unroll
  for (uint32_t k = 0; k < lp::PEERS; ++k)
#pragma unroll
    for (uint32_t j = k + 1; j < lp::PEERS; ++j) dup |= j < s.np && s.pid[j] == s.pid[k];
  return !dup;
}

// whether record i ends a run (step_is_head's mirror): lane 63 looks at the record after its wave's
__device__ __forceinline__ bool eprop_is_tail(const EpropArgs &a, uint64_t i, uint64_t group, uint32_t lane) {
  uint64_t nxt = __shfl_down(group, 1);
  if (lane == 63 && i + 1 < a.n) nxt = a.locals[i + 1].group;
  return i < a.n && (i + 1 == a.n || nxt != group);
}

// The workgroup's segmented inclusive scan: a set flag starts a segment.
// Returns the sum since the last flag at or before this thread (or since the
// workgroup's first thread), *seen: there is such a flag.  *wg_val / *wg_seen:
// the last thread's values.
__device__ __forceinline__ unsigned long long eprop_seg_scan(unsigned long long v, bool flag, bool *seen,
                                                             unsigned long long *wg_val, bool *wg_seen) {
  __shared__ unsigned long long s_v[4];
  __shared__ uint32_t s_f[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t f = flag ? 1u : 0u;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long tv = __shfl_up(v, d);
    const uint32_t tf = __shfl_up(f, d);
    if ((int)lane >= d) {
      if (!f) v += tv;
      f |= tf;
    }
  }
  if (lane == 63) {
    s_v[wave] = v;
    s_f[wave] = f;
  }
  __syncthreads();
  unsigned long long cv = 0, av = 0;
  uint32_t cf = 0, af = 0;
#pragma unroll
  for (uint32_t w = 0; w < 4; ++w) {
    const unsigned long long x = s_v[w];
    const uint32_t xf = s_f[w];
    if (w < wave) {
      cv = xf ? x : cv + x;
      cf |= xf;
    }
    av = xf ? x : av + x;
    af |= xf;
  }
  __syncthreads();                                   // s_v / s_f are free for the next call
  *wg_val = av;
  *wg_seen = af != 0;
  *seen = (f | cf) != 0;
  return f ? v : cv + v;
}

__global__ __launch_bounds__(256) void k_prop_check(const EpropArgs a) {
  __shared__ el_v2 s_rec[4][192];
  const auto [lane, wave, r0, i] = step_lane();
  const EpropRec r = eprop_load_wave(a.locals, a.n, s_rec[wave], r0, lane);
  const bool valid = i < a.n;
  const bool head = step_is_head(a.locals, a.n, i, r.group, lane);
  const bool prop = r.kind == lp::KIND_PROP;
  uint32_t err = 0;
  if (valid) {
    if (r.group >= a.G) err = STEP_ERR_INVAL;
    if (r.kind != lp::KIND_BEAT && !prop) err = STEP_ERR_INVAL;
    if ((r.tn >> 32) > 1) err = STEP_ERR_INVAL;     // data_nil
    if (prop && (r.data_len > a.data_len_total || r.data_off > a.data_len_total - r.data_len)) err = STEP_ERR_INVAL;
  }
  if (head && r.group < a.G) {
    lp::State s;
    uint64_t cap = 0;
    const uint64_t reserved = eprop_load_group(a, r.group, s, &cap);
    // the group's claim: the head of a second run finds the word taken
    if (!step_claim(a.claim, r.group, i)) err = STEP_ERR_INVAL;
    if (!eprop_group_ok(a, s, cap, reserved)) err = STEP_ERR_INVAL;
  }
  step_flag(a.head, err);
  const unsigned long long v =
      (valid && prop) ? 1ull | ((uint32_t)r.tn == (uint32_t)lp::ENTRY_CONF_CHANGE ? 1ull << 32 : 0ull) : 0ull;
  bool seen = false, wg_seen = false;
  unsigned long long wg_val = 0;
  const unsigned long long incl = eprop_seg_scan(v, head, &seen, &wg_val, &wg_seen);
  if (valid) a.seg[i] = incl | (seen ? 0ull : EPROP_OPEN);
  if (threadIdx.x == 0) {
    a.agg[blockIdx.x].val = wg_val;
    a.agg[blockIdx.x].head = wg_seen ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void k_prop_carry(EpropAgg *__restrict__ agg, uint32_t nslots) {
  __shared__ unsigned long long s_v[256];
  // thread t owns the workgroups [t * chunk, (t + 1) * chunk)
  const uint32_t chunk = (nslots + 255u) / 256u;
  const uint64_t lo = (uint64_t)threadIdx.x * chunk;
  const uint64_t hi = lo + chunk < nslots ? lo + chunk : nslots;
  unsigned long long v = 0;
  bool f = false;
  for (uint64_t s = lo; s < hi; ++s) {
    const EpropAgg x = agg[s];
    v = x.head ? x.val : v + x.val;
    f = f || x.head != 0;
  }
  bool seen = false, wg_seen = false;
  unsigned long long wg_val = 0;
  const unsigned long long incl = eprop_seg_scan(v, f, &seen, &wg_val, &wg_seen);
  s_v[threadIdx.x] = incl;
  __syncthreads();
  // what the threads before this one leave: the inclusive value of the thread before
  unsigned long long at = threadIdx.x ? s_v[threadIdx.x - 1] : 0;
  for (uint64_t s = lo; s < hi; ++s) {
    const EpropAgg x = agg[s];
    agg[s].val = at;
    at = x.head ? x.val : at + x.val;
  }
}

// the counts of record i: seg[i], plus what the run brought into the workgroup
__device__ __forceinline__ void eprop_counts(const EpropArgs &a, uint64_t i, uint64_t *nprops, uint64_t *ncc) {
  unsigned long long v = a.seg[i];
  if (v & EPROP_OPEN) v = (v & ~EPROP_OPEN) + a.agg[blockIdx.x].val;
  *nprops = v & EPROP_LOW;
  *ncc = v >> 32;
}

// the sinks of lead_prop_step.h's EMIT paths
struct EpropNoSink {
  __device__ __forceinline__ void entry(uint64_t, uint64_t, uint64_t) {}
  __device__ __forceinline__ void msg(uint64_t, const lp::State &, const lp::Msg &) {}
};
struct EpropSink {
  const EpropArgs &a;
  uint64_t g, msg_first, efirst;
  EpropRec r;
  // the new entry: {term, index, data_off, data_len, type | data_nil << 32}
  __device__ __forceinline__ void entry(uint64_t pos, uint64_t term, uint64_t index) {
    uint64_t *e = (uint64_t *)(a.ents + efirst + pos);
    e[0] = term;
    e[1] = index;
    e[2] = r.data_off;
    e[3] = r.data_len;
    e[4] = r.tn;
  }
  // the emsg_out of one sendAppend / sendHeartbeat, after send (raft.go:190-199)
  __device__ __forceinline__ void msg(uint64_t j, const lp::State &s, const lp::Msg &m) {
    el_v2 *q = (el_v2 *)(a.msgs + msg_first + j);
    q[0] = el_v2{m.type, m.to};
    q[1] = el_v2{s.id, s.term};
    q[2] = el_v2{m.log_term, m.index};
    if (m.type == lp::MSG_SNAP) {
      const el_v2 *sn = (const el_v2 *)(a.snaps + g);
      const el_v2 s0 = sn[0], s1 = sn[1], s2 = sn[2], s3 = sn[3];
      q[3] = el_v2{0, 0};
      q[4] = el_v2{0, s0.x};
      q[5] = el_v2{s0.y, s1.x};
      q[6] = el_v2{s1.y, s2.x};
      q[7] = el_v2{s2.y, s3.x};
      q[8] = el_v2{s3.y, 0};
    } else {
      q[3] = el_v2{m.commit, m.nents ? s.efirst + m.efirst : 0};
      q[4] = el_v2{m.nents, 0};
#pragma unroll
      for (uint32_t k = 5; k < 9; ++k) q[k] = el_v2{0, 0};
    }
  }
};

// the terms of the log as the call found it
struct EpropTermAt {
  const ewal_entry *ents;
  __device__ __forceinline__ uint64_t operator()(uint64_t pos) const { return ents[pos].term; }
};

__device__ __forceinline__ void eprop_store_res(elead_local_result *dst, const lp::Out &o, uint64_t msg_first,
                                                uint64_t efirst) {
  el_v2 *rq = (el_v2 *)dst;
  rq[0] = el_v2{(uint64_t)(uint32_t)o.status | ((uint64_t)(uint32_t)o.action << 32), msg_first};
  rq[1] = el_v2{o.n_msgs, o.index};
  rq[2] = el_v2{o.action == lp::APPENDED ? efirst + o.pos : 0, o.committed};
}

// The serial run of group g headed at record i (r0) on the start state s:
// steps it in order.  write_res: d_res; EMIT: the entries, the messages from
// msg_first on and the records' changed words.  Adds the run's messages and
// appended entries to tot / napp.
template <bool EMIT>
__device__ __forceinline__ void eprop_run(const EpropArgs &a, uint64_t i, const EpropRec &r0, lp::State s,
                                          bool write_res, uint64_t msg_first, unsigned long long &tot,
                                          unsigned long long &napp) {
  const uint64_t g = r0.group;
  const lp::State s0 = s;
  const bool unsupported = s.np > lp::PEERS;
  const EpropTermAt term_at{a.ents + s.efirst};
  bool stopped = false;
  EpropRec r = r0;
  for (uint64_t k = i;;) {
    lp::Out o;
    if (stopped || unsupported) {
      o.status = stopped ? lp::ST_OK : lp::ST_UNSUPPORTED;
      o.action = stopped ? lp::NOT_STEPPED : lp::PANICKED;
      o.n_msgs = o.index = o.pos = 0;
      o.committed = s.committed;
      stopped = true;
    } else if (EMIT) {
      EpropSink sink{a, g, msg_first, s.efirst, r};
      o = lp::step<true>(s, r.kind, (int32_t)(uint32_t)r.tn, term_at, sink);
    } else {
      EpropNoSink sink;
      o = lp::step<false>(s, r.kind, (int32_t)(uint32_t)r.tn, term_at, sink);
    }
    stopped = stopped || o.status != lp::ST_OK;
    if (write_res) eprop_store_res(a.res + k, o, msg_first, s.efirst);
    msg_first += o.n_msgs;
    tot += o.n_msgs;
    napp += o.action == lp::APPENDED ? 1 : 0;
    ++k;
    if (k >= a.n) break;
    r = eprop_load_rec(a.locals + k);
    if (r.group != g) break;
  }
  if (EMIT) {
    // lp_store_changed's words, but a peer's match and next go together here
    uint64_t *gw = (uint64_t *)(a.groups + g);
    uint64_t *sw = (uint64_t *)(a.state + g);
    if (s.committed != s0.committed) gw[2] = s.committed;
    if (s.nlog != s0.nlog) gw[4] = s.nlog;
#pragma unroll
    for (uint32_t k = 0; k < lp::PEERS; ++k)
      if (s.match[k] != s0.match[k] || s.next[k] != s0.next[k]) {
        gw[14 + k] = s.match[k];
        gw[21 + k] = s.next[k];
      }
    if (s.unstable != s0.unstable) sw[1] = s.unstable;
    if (s.pending != s0.pending) sw[2] = s.pending;
  }
}

__global__ __launch_bounds__(256) void k_prop_count(const EpropArgs a) {
  __shared__ el_v2 s_rec[4][192];
  if (a.head->errflag & STEP_ERR_INVAL) return;                       // an invalid call: nothing below may trust the records
  const auto [lane, wave, r0, i] = step_lane();
  const EpropRec r = eprop_load_wave(a.locals, a.n, s_rec[wave], r0, lane);
  const bool valid = i < a.n;
  const bool head = step_is_head(a.locals, a.n, i, r.group, lane);
  const bool tail = eprop_is_tail(a, i, r.group, lane);
  unsigned long long tot = 0, napp = 0, mode = 0;
  uint32_t err = 0;
  if (valid) {
    uint64_t nprops = 0, ncc = 0, cap = 0;
    eprop_counts(a, i, &nprops, &ncc);
    lp::State s;
    (void)eprop_load_group(a, r.group, s, &cap);
    eprop_load_snap(a, r.group, s);
    if (tail && cap - s.nlog < nprops) err = STEP_ERR_NOMEM;
    const lp::Run run = lp::prepare(s);
    if (run.closed) {
      if (r.kind == lp::KIND_BEAT) {
        tot = run.others;
      } else if (lp::accepted(s, (int32_t)(uint32_t)r.tn, ncc)) {
        tot = run.others;
        napp = 1;
      }
    } else {
      mode = EPROP_SERIAL;
      if (head) eprop_run<false>(a, i, r, s, false, 0, tot, napp);
    }
  }
  step_flag(a.head, err);
  if (valid) a.cnt[i] = tot | mode;
  step_block_sums(tot, napp, a.partial, blockIdx.x);
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_prop_apply(const EpropArgs a) {
  __shared__ el_v2 s_rec[4][192];
  const auto [lane, wave, r0, i] = step_lane();
  const EpropRec r = eprop_load_wave(a.locals, a.n, s_rec[wave], r0, lane);
  const bool valid = i < a.n;
  const bool head = step_is_head(a.locals, a.n, i, r.group, lane);
  const unsigned long long c = valid ? a.cnt[i] : 0;
  unsigned long long total = 0;
  const unsigned long long before = step_block_scan(c & ~EPROP_SERIAL, &total);
  const uint64_t msg_first = a.partial[2 * (uint64_t)blockIdx.x] + before;
  if (!valid) return;
  if (c & EPROP_SERIAL) {
    if (!head) return;                               // the head's lane writes this record's result
    lp::State s;
    uint64_t cap = 0;
    (void)eprop_load_group(a, r.group, s, &cap);
    eprop_load_snap(a, r.group, s);
    unsigned long long tot = 0, napp = 0;
    eprop_run<EMIT>(a, i, r, s, true, msg_first, tot, napp);
    return;
  }
  uint64_t nprops = 0, ncc = 0, cap = 0;
  eprop_counts(a, i, &nprops, &ncc);
  lp::State s;
  (void)eprop_load_group(a, r.group, s, &cap);
  eprop_load_snap(a, r.group, s);
  const lp::Run run = lp::prepare(s);
  const EpropTermAt term_at{a.ents + s.efirst};
  lp::Out o;
  if (EMIT) {
    EpropSink sink{a, r.group, msg_first, s.efirst, r};
    o = lp::closed_record<true>(s, run, r.kind, (int32_t)(uint32_t)r.tn, nprops, ncc, term_at, sink);
  } else {
    EpropNoSink sink;
    o = lp::closed_record<false>(s, run, r.kind, (int32_t)(uint32_t)r.tn, nprops, ncc, term_at, sink);
  }
  eprop_store_res(a.res + i, o, msg_first, s.efirst);
}

__global__ __launch_bounds__(256) void k_prop_commit(const EpropArgs a) {
  __shared__ el_v2 s_rec[4][192];
  const auto [lane, wave, r0, i] = step_lane();
  const EpropRec r = eprop_load_wave(a.locals, a.n, s_rec[wave], r0, lane);
  const bool tail = eprop_is_tail(a, i, r.group, lane);
  if (!tail || (a.cnt[i] & EPROP_SERIAL)) return;
  uint64_t nprops = 0, ncc = 0, cap = 0;
  eprop_counts(a, i, &nprops, &ncc);
  lp::State s;
  (void)eprop_load_group(a, r.group, s, &cap);
  const uint64_t acc = lp::accepted_upto(s, nprops, ncc);
  if (acc == 0) return;
  eprop_load_snap(a, r.group, s);
  const lp::Run run = lp::prepare(s);
  const EpropTermAt term_at{a.ents + s.efirst};
  const lp::State e = lp::closed_state(s, run, acc, ncc > 0, term_at);
  uint64_t *gw = (uint64_t *)(a.groups + r.group);
  uint64_t *sw = (uint64_t *)(a.state + r.group);
  if (e.committed != s.committed) gw[2] = e.committed;
  gw[4] = e.nlog;
#pragma unroll
  for (int k = 0; k < (int)lp::PEERS; ++k)
    if (k == run.self) {
      gw[14 + k] = e.match[k];
      gw[21 + k] = e.next[k];
    }
  if (e.unstable != s.unstable) sw[1] = e.unstable;
  if (e.pending != s.pending) sw[2] = e.pending;
}
