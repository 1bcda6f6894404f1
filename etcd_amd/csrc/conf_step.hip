// conf_step.hip -- membership on the shared group records: ApplyConfChange and
// the arrival of a msgDenied (econf_batch_device), the server loop's ConfChange
// half over rd.CommittedEntries (econf_scan_committed_device) and the
// removed[m.From] gate in front of the step calls (econf_gate_batch_device).
// The decisions are conf_step.h's (shared with the host check); this file is
// the assignment of work and the memory traffic.
//
// econf_batch_device: ONE LANE PER RUN HEAD, vote_step.hip's assignment.  A
// request's case depends on what its predecessors left (a remove moves slots, a
// 15th id stops the run) and runs are short -- a bootstrap applies three adds, a
// steady group one request -- so the head's lane loads the group's five records
// once (256 + 32 + 64 + 16 + 128 bytes), keeps them in registers and replays
// its run in array order.
//   k_conf_count   one lane per request, nothing of the caller's modified: the
//                  request's checks, and by a run's head the claim, the group's
//                  checks and a replay that only counts the msgDenied.
//   k_lead_scan    step_common.hip's; the host reads the head -- the one
//                  decision point.
//   k_conf_apply   the head replays the run, writes d_res, the messages and of
//                  the five records only the words that changed.  <false>
//                  writes d_res alone.
//
// econf_scan_committed_device: ONE LANE PER COMMITTED ENTRY, count -> scan ->
// emit twice over, because the number of lanes is itself a sum:
//   k_cscan_sel    one lane per selection: its range's checks, the selections'
//                  entry counts into selloc[] / spart[].
//   k_lead_scan    the selections' offsets; the host reads T, the entries of
//                  the call, and sizes the per-entry records.
//   k_cscan_decode one lane per entry: finds its selection by a binary search
//                  over the scanned counts, loads the 40-byte entry and, for an
//                  EntryConfChange, walks its Data -- a dependent chain d_ready
//                  -> d_ents -> d_data that no layout here can shorten; leaves
//                  the decoded request in erec[e] and the selection's first
//                  failing entry in selbad[] (atomicMin).
//   k_cscan_count  one lane per entry: whether it emits (a ConfChange before
//                  its selection's failing entry), the workgroups' sums.
//   k_lead_scan    the offsets; the host reads the head -- the decision point.
//   k_cscan_emit   one lane per entry: its place (a block scan), epos[e], and
//                  with EMIT the econf_req and econf_applied records.
//   k_cscan_rows   one lane per selection: d_scan from epos[] and selbad[].
//
// econf_gate_batch_device: ONE LANE PER RECORD, tick_step.hip's shape:
//   k_gate_count   reads the record's group and From words, the group's id and
//                  term and its econf_state; leaves the verdict in rec[i].
//   k_lead_scan    twice: the copies' and the messages' offsets.
//   k_gate_apply   d_res, and with EMIT the record's copy and the msgDenied.
//
// Uses step_common.hip.
#include "ewal_device.h"
#include "ewal_internal.h"
#include "conf_step.h"

namespace cf = conf_step;

// ---- econf_batch_device ---------------------------------------------------------
struct EconfArgs {
  elead_group *groups;
  elead_prop_state *pstate;
  evote_state *vstate;
  eready_state *rstate;
  econf_state *cstate;
  uint64_t G;
  const elead_snap *snaps;          // nullable
  const uint64_t *u64;
  uint64_t n_u64;
  const econf_req *in;
  uint64_t n;
  econf_result *res;
  emsg_out *msgs;                   // NULL: the size query
  EleadHead *head;
  uint32_t *claim;                  // G
  unsigned long long *run_msgs;     // n
  unsigned long long *partial;      // 2 per workgroup: messages, changed requests
};

struct EconfRec {
  uint64_t group, kind, node, pad;
};

struct EconfU64At {
  const uint64_t *p;
  __device__ __forceinline__ uint64_t operator()(uint64_t j) const { return p[j]; }
};

// word k of a record held as 16-B units
#define ECONF_W(u, k) (((k) & 1) ? (u)[(k) >> 1].y : (u)[(k) >> 1].x)

// The group's five records as a run's start state.  False: a whole-call check fails.
__device__ __forceinline__ bool econf_load_group(const EconfArgs &a, uint64_t g, cf::State &s) {
  el_v2 gu[16], cu[8];
  step_load_rec(a.groups + g, gu);
  step_load_rec(a.cstate + g, cu);
  const el_v2 *pp = (const el_v2 *)(a.pstate + g);
  const el_v2 *vp = (const el_v2 *)(a.vstate + g);
  const el_v2 p1 = pp[1], v0 = vp[0], v2 = vp[2], v3 = vp[3];
  const el_v2 r3 = ((const el_v2 *)(a.rstate + g))[3];
  s.id = gu[0].x;
  s.term = gu[0].y;
  s.off = gu[1].y;
  s.nlog = gu[2].x;
  s.np = gu[3].x;
#pragma unroll
  for (uint32_t k = 0; k < cf::PEERS; ++k) {
    s.pid[k] = ECONF_W(gu, 7 + k);
    s.match[k] = ECONF_W(gu, 14 + k);
    s.next[k] = ECONF_W(gu, 21 + k);
  }
  s.pending = p1.x;
  s.rstate = v0.x;
  s.voted = v2.x;
  s.granted = v2.y;
  s.dirty = r3.y;
  s.nrem = cu[0].x;
#pragma unroll
  for (uint32_t k = 0; k < cf::REMOVED; ++k) s.rem[k] = ECONF_W(cu, 1 + k);
  bool ok = (gu[14].x | gu[14].y | gu[15].x | gu[15].y | p1.y | v3.x | v3.y | cu[7].y) == 0;
  ok = ok && s.nrem <= cf::REMOVED && s.pending <= 1 && s.dirty <= 1 && s.rstate <= 2;
  const uint64_t slots = s.np < cf::PEERS ? s.np : cf::PEERS;
  const uint64_t mask = (1ull << (uint32_t)slots) - 1;
  ok = ok && ((s.voted | s.granted) & ~mask) == 0 && (s.granted & ~s.voted) == 0;
  bool dup = false;
#pragma unroll
  for (uint32_t j = 1; j < cf::PEERS; ++j)
#pragma unroll
    for (uint32_t k = 0; k < j; ++k) dup |= j < s.np && s.pid[j] == s.pid[k];
  return ok && !dup;
}

// of group g's five records, the words the run changed
__device__ __forceinline__ void econf_store_changed(const EconfArgs &a, uint64_t g, const cf::State &s0,
                                                    const cf::State &s) {
  uint64_t *gw = (uint64_t *)(a.groups + g);
  uint64_t *cw = (uint64_t *)(a.cstate + g);
  if (s.np != s0.np) gw[6] = s.np;
#pragma unroll
  for (uint32_t k = 0; k < cf::PEERS; ++k) {
    if (s.pid[k] != s0.pid[k]) gw[7 + k] = s.pid[k];
    if (s.match[k] != s0.match[k]) gw[14 + k] = s.match[k];
    if (s.next[k] != s0.next[k]) gw[21 + k] = s.next[k];
  }
  if (s.pending != s0.pending) ((uint64_t *)(a.pstate + g))[2] = s.pending;
  if (s.voted != s0.voted) ((uint64_t *)(a.vstate + g))[4] = s.voted;
  if (s.granted != s0.granted) ((uint64_t *)(a.vstate + g))[5] = s.granted;
  if (s.dirty != s0.dirty) ((uint64_t *)(a.rstate + g))[7] = s.dirty;
  if (s.nrem != s0.nrem) cw[0] = s.nrem;
#pragma unroll
  for (uint32_t k = 0; k < cf::REMOVED; ++k)
    if (s.rem[k] != s0.rem[k]) cw[1 + k] = s.rem[k];
}

// The run of group g headed at request i on the start state s, stepped in
// order.  write_res: d_res; EMIT: the messages from msg_first on and the
// records' changed words.
template <bool EMIT>
__device__ __forceinline__ void econf_run(const EconfArgs &a, uint64_t i, const EconfRec &r0, cf::State s,
                                          bool write_res, uint64_t msg_first, unsigned long long &tot,
                                          unsigned long long &nchg) {
  const uint64_t g = r0.group;
  const cf::State s0 = s;
  bool stopped = false;
  EconfRec r = r0;
  for (uint64_t k = i;;) {
    cf::Out o{cf::ST_OK, cf::NOT_STEPPED, 0};
    if (!stopped) {
      uint64_t roff = 0, rn = 0;
      bool range_ok = r.pad == 0;
      if (r.kind == cf::KIND_RELOAD) {
        range_ok = range_ok && a.snaps != nullptr;
        if (range_ok) {
          const el_v2 sn = ((const el_v2 *)(a.snaps + g))[3];
          roff = sn.x;
          rn = sn.y;
          range_ok = roff <= a.n_u64 && rn <= a.n_u64 - roff;
        }
      }
      // a request that fails its own lane's check makes the call INVAL: the replay stops in front of it
      if (range_ok) o = cf::step(s, r.kind, r.node, rn, EconfU64At{a.u64 + roff});
      else stopped = true;
    }
    stopped = stopped || o.status != cf::ST_OK;
    if (write_res) {
      el_v2 *rq = (el_v2 *)(a.res + k);
      rq[0] = el_v2{(uint64_t)(uint32_t)o.status | ((uint64_t)(uint32_t)o.action << 32), msg_first};
      rq[1] = el_v2{o.n_msgs, s.np};
      rq[2] = el_v2{s.nrem, 0};
    }
    if (EMIT && o.n_msgs) {                           // send(pb.Message{To: m.From, Type: msgDenied})
      el_v2 *q = (el_v2 *)(a.msgs + msg_first);
      q[0] = el_v2{cf::MSG_DENIED, r.node};
      q[1] = el_v2{s.id, s.term};
#pragma unroll
      for (uint32_t w = 2; w < 9; ++w) q[w] = el_v2{0, 0};
    }
    msg_first += o.n_msgs;
    tot += o.n_msgs;
    nchg += (o.status == cf::ST_OK && o.action != cf::NOT_STEPPED && o.action != cf::DENIED_BACK) ? 1 : 0;
    ++k;
    if (k >= a.n) break;
    el_v2 u[2];
    step_load_rec(a.in + k, u);
    if (u[0].x != g) break;
    r = EconfRec{u[0].x, u[0].y, u[1].x, u[1].y};
  }
  if (EMIT) econf_store_changed(a, g, s0, s);
}

__global__ __launch_bounds__(256) void k_conf_count(const EconfArgs a) {
  __shared__ el_v2 s_rec[4][128];
  const auto [lane, wave, r0, i] = step_lane();
  el_v2 u[2];
  step_load_wave(a.in, a.n, s_rec[wave], r0, lane, u);
  const EconfRec r{u[0].x, u[0].y, u[1].x, u[1].y};
  const bool valid = i < a.n;
  const bool head = step_is_head(a.in, a.n, i, r.group, lane);
  uint32_t err = 0;
  unsigned long long tot = 0, nchg = 0;
  if (valid) {
    if (r.group >= a.G || r.pad != 0) err = STEP_ERR_INVAL;
    if (!err && r.kind == cf::KIND_RELOAD) {
      if (!a.snaps) {
        err = STEP_ERR_INVAL;
      } else {
        const el_v2 sn = ((const el_v2 *)(a.snaps + r.group))[3];
        if (sn.x > a.n_u64 || sn.y > a.n_u64 - sn.x) err = STEP_ERR_INVAL;
      }
    }
  }
  if (head && r.group < a.G) {
    // the group's claim: the head of a second run finds the word taken
    if (!step_claim(a.claim, r.group, i)) err = STEP_ERR_INVAL;
    cf::State s;
    if (!econf_load_group(a, r.group, s)) err = STEP_ERR_INVAL;
    if (!err) econf_run<false>(a, i, r, s, false, 0, tot, nchg);
  }
  step_flag(a.head, err);
  if (valid) a.run_msgs[i] = tot;
  step_block_sums(tot, nchg, a.partial, blockIdx.x);
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_conf_apply(const EconfArgs a) {
  __shared__ el_v2 s_rec[4][128];
  const auto [lane, wave, r0, i] = step_lane();
  el_v2 u[2];
  step_load_wave(a.in, a.n, s_rec[wave], r0, lane, u);
  const EconfRec r{u[0].x, u[0].y, u[1].x, u[1].y};
  const bool head = step_is_head(a.in, a.n, i, r.group, lane);
  unsigned long long total = 0;
  const unsigned long long before = step_block_scan(i < a.n ? a.run_msgs[i] : 0, &total);
  if (head) {
    cf::State s;
    (void)econf_load_group(a, r.group, s);
    unsigned long long tot = 0, nchg = 0;
    econf_run<EMIT>(a, i, r, s, true, a.partial[2 * (uint64_t)blockIdx.x] + before, tot, nchg);
  }
}

// ---- econf_scan_committed_device ------------------------------------------------
#define ECSCAN_NONE 0xFFFFFFFFu     // selbad[i]: no entry of selection i fails
#define ECSCAN_CONF (1ull << 8)     // EcscanRec.meta: a decoded EntryConfChange

struct EcscanRec {                  // 48 bytes per committed entry
  unsigned long long meta;          // status | ECSCAN_CONF | selection << 32
  unsigned long long id;            // cc.ID; a failing entry: its type (the row's detail)
  unsigned long long node, kind;
  unsigned long long ent_pos;
  unsigned long long pad;
};

struct EcscanArgs {
  const eready_result *ready;
  const uint64_t *sel;              // nullable
  uint64_t n, G;
  const ewal_entry *ents;
  uint64_t n_ents_total;
  const uint8_t *data;
  uint64_t data_len_total;
  econf_scan_result *scan;
  econf_req *reqs;                  // NULL (with applied): the size query
  econf_applied *applied;
  EleadHead *head, *ehead;
  unsigned long long *selloc;       // n: the entries of the selections before i in its workgroup
  unsigned long long *spart;        // 2 per selection workgroup
  uint32_t *selbad;                 // n: the call-wide ordinal of selection i's first failing entry
  uint64_t T;                       // the committed entries of the call
  EcscanRec *erec;                  // T
  unsigned long long *epos;         // T: the requests before entry e
  unsigned long long *epart;        // 2 per entry workgroup
  uint64_t R;                       // the requests of the call
};

struct EcscanSkip {
  __device__ __forceinline__ int32_t operator()(const uint8_t *p, int64_t l, int64_t &out) const {
    return pb_skip(p, l, out);
  }
};

// the call-wide ordinal of selection i's first entry
__device__ __forceinline__ uint64_t ecscan_first(const EcscanArgs &a, uint64_t i) {
  return a.selloc[i] + a.spart[2 * (i >> 8)];
}

__global__ __launch_bounds__(256) void k_cscan_sel(const EcscanArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < a.n;
  uint32_t err = 0;
  unsigned long long nc = 0;
  if (valid) {
    const uint64_t g = a.sel ? a.sel[i] : i;
    const el_v2 c = ((const el_v2 *)(a.ready + i))[3];   // committed_first, n_committed
    if (g >= a.G) err = STEP_ERR_INVAL;
    if (c.y != 0 && (c.x > a.n_ents_total || c.y > a.n_ents_total - c.x)) err = STEP_ERR_INVAL;
    nc = err ? 0 : c.y;
    a.selbad[i] = ECSCAN_NONE;
  }
  step_flag(a.head, err);
  unsigned long long total = 0;
  const unsigned long long before = step_block_scan(nc, &total);
  if (valid) a.selloc[i] = before;
  step_block_sums(nc, 0, a.spart, blockIdx.x);
}

__global__ __launch_bounds__(256) void k_cscan_decode(const EcscanArgs a) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t err = 0;
  if (e < a.T) {
    // the last selection whose first entry is at or before e: the empty ones before it share its ordinal
    uint64_t lo = 0, hi = a.n;
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (ecscan_first(a, mid) <= e) lo = mid;
      else hi = mid;
    }
    const uint64_t pos = ((const uint64_t *)(a.ready + lo))[6] + (e - ecscan_first(a, lo));
    const uint64_t *ew = (const uint64_t *)(a.ents + pos);
    const uint64_t doff = ew[2], dlen = ew[3], tn = ew[4];
    const int32_t type = (int32_t)(uint32_t)tn, data_nil = (int32_t)(uint32_t)(tn >> 32);
    int32_t st = cf::ST_OK;
    cf::ConfChange cc{0, 0, 0};
    bool conf = false;
    if (type == 1) {
      if (data_nil < 0 || data_nil > 2) {
        err = STEP_ERR_INVAL;
      } else if (data_nil == 2) {
        st = cf::ST_UNSUPPORTED;                     // the bytes are outside d_data
      } else if (doff > a.data_len_total || dlen > a.data_len_total - doff) {
        err = STEP_ERR_INVAL;
      } else {
        st = cf::decode(a.data + doff, data_nil ? 0 : (int64_t)dlen, EcscanSkip{}, &cc);
        conf = st == cf::ST_OK;
      }
    } else if (type != 0) {
      st = cf::ST_ENTRY_TYPE;
      cc.id = (uint64_t)(uint32_t)type;
    }
    if (st != cf::ST_OK) atomicMin(a.selbad + lo, (uint32_t)e);
    el_v2 *q = (el_v2 *)(a.erec + e);
    q[0] = el_v2{(uint64_t)(uint32_t)st | (conf ? ECSCAN_CONF : 0ull) | (lo << 32), cc.id};
    q[1] = el_v2{cc.node, cf::kind_of(cc)};
    q[2] = el_v2{pos, 0};
  }
  step_flag(a.head, err);
}

// whether entry e emits a request; m: its record's first word
__device__ __forceinline__ bool ecscan_emits(const EcscanArgs &a, uint64_t e, uint64_t m) {
  return (m & ECSCAN_CONF) && e < a.selbad[m >> 32];
}

__global__ __launch_bounds__(256) void k_cscan_count(const EcscanArgs a) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned long long emit = 0;
  if (e < a.T) emit = ecscan_emits(a, e, a.erec[e].meta) ? 1 : 0;
  step_block_sums(emit, 0, a.epart, blockIdx.x);
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_cscan_emit(const EcscanArgs a) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = e < a.T;
  el_v2 r0{0, 0}, r1{0, 0}, r2{0, 0};
  if (valid) {
    const el_v2 *q = (const el_v2 *)(a.erec + e);
    r0 = q[0];
    r1 = q[1];
    r2 = q[2];
  }
  const bool emit = valid && ecscan_emits(a, e, r0.x);
  unsigned long long total = 0;
  const unsigned long long at = a.epart[2 * (uint64_t)blockIdx.x] + step_block_scan(emit ? 1 : 0, &total);
  if (!valid) return;
  a.epos[e] = at;
  if (!EMIT || !emit) return;
  const uint64_t i = r0.x >> 32;
  const uint64_t g = a.sel ? a.sel[i] : i;
  const uint64_t *ew = (const uint64_t *)(a.ents + r2.x);   // a 40-byte record: 8-byte loads
  const uint64_t term = ew[0], index = ew[1];
  el_v2 *rq = (el_v2 *)(a.reqs + at);
  rq[0] = el_v2{g, r1.y};
  rq[1] = el_v2{r1.x, 0};
  el_v2 *aq = (el_v2 *)(a.applied + at);
  aq[0] = el_v2{r0.y, index};
  aq[1] = el_v2{term, r2.x};
}

__global__ __launch_bounds__(256) void k_cscan_rows(const EcscanArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t nc = ((const uint64_t *)(a.ready + i))[7];
  const uint64_t e0 = ecscan_first(a, i), e1 = e0 + nc;
  const uint64_t first = e0 < a.T ? a.epos[e0] : a.R, end = e1 < a.T ? a.epos[e1] : a.R;
  const uint32_t bad = a.selbad[i];
  uint64_t st = 0, detail = 0, bad_pos = 0, scanned = nc;
  if (bad != ECSCAN_NONE) {
    const el_v2 *q = (const el_v2 *)(a.erec + bad);
    const el_v2 r0 = q[0];
    st = r0.x & 0xffu;
    detail = st == (uint64_t)cf::ST_ENTRY_TYPE ? r0.y & 0xffffffffull : 0;
    bad_pos = q[2].x;
    scanned = bad - e0;
  }
  el_v2 *o = (el_v2 *)(a.scan + i);
  o[0] = el_v2{st | (detail << 32), first};
  o[1] = el_v2{end - first, bad_pos};
  o[2] = el_v2{scanned, 0};
}

// ---- econf_gate_batch_device ----------------------------------------------------
struct EgateRec {                   // 32 bytes per record
  unsigned long long action, from, id, term;
};

struct EgateArgs {
  const elead_group *groups;
  const econf_state *cstate;
  uint64_t G;
  const uint8_t *recs;
  uint64_t n;
  uint32_t rec_bytes, from_word;
  econf_gate_result *res;
  uint8_t *pass;                    // NULL (with msgs): the size query
  emsg_out *msgs;
  EleadHead *head, *mhead;
  EgateRec *rec;                    // n
  unsigned long long *ppart;        // 2 per workgroup: copies, messages
  unsigned long long *mpart;        // 2 per workgroup: messages, 0
};

__global__ __launch_bounds__(256) void k_gate_count(const EgateArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < a.n;
  uint32_t err = 0;
  int32_t action = 0;
  if (valid) {
    const uint64_t *rw = (const uint64_t *)(a.recs + i * a.rec_bytes);
    const uint64_t g = rw[0];
    uint64_t from = 0, id = 0, term = 0;
    if (g >= a.G) {
      err = STEP_ERR_INVAL;
    } else {
      const el_v2 g0 = *(const el_v2 *)(a.groups + g);
      id = g0.x;
      term = g0.y;
      from = a.from_word == ECONF_FROM_SELF ? id : rw[a.from_word];
      el_v2 cu[8];
      step_load_rec(a.cstate + g, cu);
      if (cu[0].x > cf::REMOVED || cu[7].y != 0) {
        err = STEP_ERR_INVAL;
      } else {
        uint64_t w[1 + cf::REMOVED];
#pragma unroll
        for (uint32_t k = 0; k < 1 + cf::REMOVED; ++k) w[k] = ECONF_W(cu, k);
        action = cf::gate(w, id, from);
      }
    }
    el_v2 *q = (el_v2 *)(a.rec + i);
    q[0] = el_v2{(uint64_t)(uint32_t)action, from};
    q[1] = el_v2{id, term};
  }
  step_flag(a.head, err);
  const unsigned long long pass = action == cf::G_PASS ? 1 : 0, deny = action == cf::G_DENIED ? 1 : 0;
  step_block_sums(pass, deny, a.ppart, blockIdx.x);
  __syncthreads();                                   // the sums' staging words are reused
  step_block_sums(deny, 0, a.mpart, blockIdx.x);
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_gate_apply(const EgateArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < a.n;
  el_v2 r0{0, 0}, r1{0, 0};
  if (valid) {
    const el_v2 *rq = (const el_v2 *)(a.rec + i);
    r0 = rq[0];
    r1 = rq[1];
  }
  const int32_t action = (int32_t)(uint32_t)r0.x;
  const unsigned long long pass = action == cf::G_PASS ? 1 : 0, deny = action == cf::G_DENIED ? 1 : 0;
  unsigned long long total = 0;
  const unsigned long long pat = a.ppart[2 * (uint64_t)blockIdx.x] + step_block_scan(pass, &total);
  const unsigned long long mat = a.mpart[2 * (uint64_t)blockIdx.x] + step_block_scan(deny, &total);
  if (!valid) return;
  el_v2 *q = (el_v2 *)(a.res + i);
  q[0] = el_v2{(uint64_t)(uint32_t)action << 32, pass ? pat : 0};
  q[1] = el_v2{deny ? mat : 0, 0};
  if (!EMIT) return;
  if (pass) {
    const uint32_t units = a.rec_bytes / 16;
    const el_v2 *src = (const el_v2 *)(a.recs + i * a.rec_bytes);
    el_v2 *dst = (el_v2 *)(a.pass + pat * a.rec_bytes);
    for (uint32_t k = 0; k < units; ++k) dst[k] = src[k];
  }
  if (deny) {
    el_v2 *m = (el_v2 *)(a.msgs + mat);
    m[0] = el_v2{cf::MSG_DENIED, r0.y};
    m[1] = el_v2{r1.x, r1.y};
#pragma unroll
    for (uint32_t w = 2; w < 9; ++w) m[w] = el_v2{0, 0};
  }
}
