// vote_step.hip -- the election round of a multi-raft host: raft.Step for
// msgHup, msgVote and msgVoteResp (raft/raft.go:372-408) over n election
// messages, with campaign, poll, reset and the three become* transitions.  The
// decisions are vote_step.h's (shared with the host check); this file is the
// assignment of work and the memory traffic.
//
// Assignment: ONE LANE PER RUN HEAD, lead_step.hip's.  The step is a state
// machine with no closed form (a record's case depends on the state its
// predecessors left) and runs are short -- a candidate gets at most n_peers - 1
// answers, a voter one or two msgVote -- so the head's lane loads the group's
// three records once (256 + 32 + 64 bytes), keeps them in registers, and
// replays its run in array order, reading the later records from global memory
// wherever the run ends.  The other lanes load their own record (to check it
// and to tell whether they are heads) and take part in the sums.
//
//   k_vote_count  one lane per record, nothing of the caller's modified: the
//                 checks of a record (group < G, kind, reject, padding) and, by
//                 a run's head, of its group (the claim as in lead_step.hip,
//                 lead_prop.hip's group and window checks, the evote_state
//                 words), then a replay of the run that only counts: the run's
//                 messages into run_msgs[head], the room its msgHup and
//                 msgVoteResp records need against ents_cap (NOMEM), the
//                 workgroup's sums of messages and of WON records into
//                 partial[].
//   k_lead_scan   step_common.hip's: the workgroups' message offsets and the
//                 totals.  The host reads the flag word and the totals here --
//                 the one decision point (INVAL, NOMEM, the size query).
//   k_vote_apply  one lane per record again: a workgroup-wide exclusive scan of
//                 run_msgs plus the workgroup's offset places each run's
//                 messages; the head replays the run, writes d_res, the
//                 messages, becomeLeader's entries, and of the three records
//                 only the words that changed.  <false> writes d_res alone.
//
// A run's own entries: becomeLeader appends one entry whose term is the Term
// of that election.  A later record of the same run (a higher-term msgVote, a
// second msgHup) reads it back -- isUpToDate, campaign's term(lastIndex()), the
// next broadcast's log_term -- after Term has moved on, and the counting pass
// has not written d_ents.  Both passes therefore keep the terms of the run's
// own entries in scratch, fterm[head + k] for the run's k-th own entry (a run
// appends at most one entry per record, so the runs' ranges are disjoint), and
// read every older entry from d_ents.
//
// Uses step_common.hip, and lead_prop.hip's group loader, checks and message sink.
#include "ewal_device.h"
#include "ewal_internal.h"
#include "vote_step.h"

struct EvoteArgs {
  EpropArgs p;                      // groups, state, G, snaps, ents, n_ents_total, msgs, claim, partial, head
  evote_state *vstate;
  const evote_msg *in;
  uint64_t n;
  evote_result *res;
  unsigned long long *run_msgs;     // n
  unsigned long long *fterm;        // n: the terms of the runs' own entries
};

// one election message's words: group, kind, from, term, index, log_term, reject | pad << 32, pad2
struct EvoteRec {
  uint64_t group, kind, from, term, index, log_term, rj, pad2;
};

__device__ __forceinline__ EvoteRec evote_unpack(const el_v2 (&u)[4]) {
  return EvoteRec{u[0].x, u[0].y, u[1].x, u[1].y, u[2].x, u[2].y, u[3].x, u[3].y};
}

// the wave's 64 records: lane l gets record r0 + l
__device__ __forceinline__ EvoteRec evote_load_wave(const evote_msg *__restrict__ in, uint64_t n, el_v2 *s_wave,
                                                    uint64_t r0, uint32_t lane) {
  el_v2 u[4];
  step_load_wave(in, n, s_wave, r0, lane, u);
  return evote_unpack(u);
}

// One record at an arbitrary place (a run's later records).
__device__ __forceinline__ EvoteRec evote_load_rec(const evote_msg *p) {
  el_v2 u[4];
  step_load_rec(p, u);
  return evote_unpack(u);
}

// The group's evote_state; returns the OR of its reserved words.
__device__ __forceinline__ uint64_t evote_load_state(const evote_state *p, vs::Vote &v) {
  const el_v2 *src = (const el_v2 *)p;
  const el_v2 a = src[0], b = src[1], c = src[2], d = src[3];
  v.state = a.x;
  v.vote = a.y;
  v.lead = b.x;
  v.elapsed = b.y;
  v.voted = c.x;
  v.granted = c.y;
  return d.x | d.y;
}

// the checks of a run head's evote_state
__device__ __forceinline__ bool evote_state_ok(const lp::State &s, const vs::Vote &v, uint64_t reserved) {
  const uint64_t mask = (1ull << (uint32_t)lp::n_slots(s)) - 1;
  return reserved == 0 && v.state <= vs::LEADER && ((v.voted | v.granted) & ~mask) == 0 && (v.granted & ~v.voted) == 0;
}

// the log as the run sees it: its own entries from scratch, the older ones from d_ents
struct EvoteTermAt {
  const ewal_entry *ents;           // the group's window
  const unsigned long long *own;    // fterm + the run's head
  uint64_t first;
  __device__ __forceinline__ uint64_t operator()(uint64_t pos) const {
    return pos >= first ? own[pos - first] : ents[pos].term;
  }
};
struct EvoteTypeAt {
  const ewal_entry *ents;
  uint64_t first;
  __device__ __forceinline__ int32_t operator()(uint64_t pos) const { return pos >= first ? 0 : ents[pos].type; }
};

// the sinks of vote_step.h's EMIT path
struct EvoteNoSink {
  __device__ __forceinline__ void entry(uint64_t, uint64_t, uint64_t) {}
  __device__ __forceinline__ void msg(uint64_t, const lp::State &, const lp::Msg &) {}
  __device__ __forceinline__ void vote_resp(uint64_t, const lp::State &, uint64_t, bool) {}
};
struct EvoteSink {
  EpropSink p;                      // the entry {term, index, 0, 0, type 0, data_nil 1}; sendAppend's and msgVote's records
  __device__ __forceinline__ void entry(uint64_t pos, uint64_t term, uint64_t index) { p.entry(pos, term, index); }
  __device__ __forceinline__ void msg(uint64_t j, const lp::State &s, const lp::Msg &m) { p.msg(j, s, m); }
  // the msgVoteResp after send (raft.go:190-199)
  __device__ __forceinline__ void vote_resp(uint64_t j, const lp::State &s, uint64_t to, bool reject) {
    el_v2 *q = (el_v2 *)(p.a.msgs + p.msg_first + j);
    q[0] = el_v2{vs::KIND_VOTE_RESP, to};
    q[1] = el_v2{s.id, s.term};
#pragma unroll
    for (uint32_t k = 2; k < 8; ++k) q[k] = el_v2{0, 0};
    q[8] = el_v2{0, reject ? 1ull : 0ull};
  }
};

// The run of group g headed at record i (r0) on the start state (s, v): steps
// it in order.  write_res: d_res; EMIT: the entries, the messages from
// msg_first on and the records' changed words.  Adds the run's messages, WON
// records and the entries it may need room for to tot / nwon / nroom.
template <bool EMIT>
__device__ __forceinline__ void evote_run(const EvoteArgs &a, uint64_t i, const EvoteRec &r0, lp::State s, vs::Vote v,
                                          bool write_res, uint64_t msg_first, unsigned long long &tot,
                                          unsigned long long &nwon, uint64_t &nroom) {
  const uint64_t g = r0.group;
  const lp::State s0 = s;
  const vs::Vote v0 = v;
  const bool unsupported = s.np > lp::PEERS;
  const ewal_entry *win = a.p.ents + s.efirst;
  unsigned long long *own = a.fterm + i;
  vs::Run run{s.nlog};
  bool stopped = false;
  EvoteRec r = r0, ahead = r0;
  bool more = i + 1 < a.n;
  if (more) ahead = evote_load_rec(a.in + i + 1);    // one record ahead: its load is in flight during the step
  for (uint64_t k = i;;) {
    vs::Out o;
    if (stopped || unsupported) {
      o.status = stopped ? lp::ST_OK : lp::ST_UNSUPPORTED;
      o.action = stopped ? vs::NOT_STEPPED : vs::PANICKED;
      o.flags = 0;
      o.n_msgs = 0;
      o.appended = false;
      stopped = true;
    } else {
      const vs::Rec rec{r.kind, r.from, r.term, r.index, r.log_term, (uint32_t)r.rj != 0};
      const EvoteTermAt term_at{win, own, run.first};
      const EvoteTypeAt type_at{win, run.first};
      if (EMIT) {
        EvoteSink sink{EpropSink{a.p, g, msg_first, s.efirst, EpropRec{g, lp::KIND_PROP, 1ull << 32, 0, 0}}};
        o = vs::step<true>(s, v, rec, term_at, type_at, sink);
      } else {
        EvoteNoSink sink;
        o = vs::step<false>(s, v, rec, term_at, type_at, sink);
      }
      if (o.appended) {
        run.note(s, o);
        own[o.pos - run.first] = s.term;
      }
    }
    stopped = stopped || o.status != lp::ST_OK;
    nroom += (r.kind == vs::KIND_HUP || r.kind == vs::KIND_VOTE_RESP) ? 1 : 0;
    if (write_res) {
      el_v2 *rq = (el_v2 *)(a.res + k);
      rq[0] = el_v2{(uint64_t)(uint32_t)o.status | ((uint64_t)(uint32_t)o.action << 32), msg_first};
      rq[1] = el_v2{o.n_msgs, s.term};
      rq[2] = el_v2{v.vote, v.state | ((uint64_t)(uint32_t)o.flags << 32)};
    }
    msg_first += o.n_msgs;
    tot += o.n_msgs;
    nwon += o.action == vs::WON ? 1 : 0;
    ++k;
    if (!more || ahead.group != g) break;
    r = ahead;
    more = k + 1 < a.n;
    if (more) ahead = evote_load_rec(a.in + k + 1);
  }
  if (EMIT) {
    lp_store_changed(a.p.groups, a.p.state, g, s0, s);
    vs_store_changed(a.vstate, g, v0, v);
  }
}

// the group's three records as a run's start state
__device__ __forceinline__ uint64_t evote_load_group(const EvoteArgs &a, uint64_t g, lp::State &s, vs::Vote &v,
                                                     uint64_t *cap, uint64_t *vreserved) {
  const uint64_t reserved = eprop_load_group(a.p, g, s, cap);
  *vreserved = evote_load_state(a.vstate + g, v);
  // a reset moves every next: whether a sendAppend looks at the snapshot is not known from the start state
  s.snap_ok = a.p.snaps != nullptr && a.p.snaps[g].term != 0;
  return reserved;
}

__global__ __launch_bounds__(256) void k_vote_count(const EvoteArgs a) {
  __shared__ el_v2 s_rec[4][256];
  const auto [lane, wave, r0, i] = step_lane();
  const EvoteRec r = evote_load_wave(a.in, a.n, s_rec[wave], r0, lane);
  const bool valid = i < a.n;
  const bool head = step_is_head(a.in, a.n, i, r.group, lane);
  uint32_t err = 0;
  unsigned long long tot = 0, nwon = 0;
  if (valid) {
    if (r.group >= a.p.G) err = STEP_ERR_INVAL;
    if (r.kind != vs::KIND_HUP && r.kind != vs::KIND_VOTE && r.kind != vs::KIND_VOTE_RESP) err = STEP_ERR_INVAL;
    if (r.rj > 1 || r.pad2 != 0) err = STEP_ERR_INVAL;   // reject not 0 or 1, or the padding not 0
  }
  if (head && r.group < a.p.G) {
    lp::State s;
    vs::Vote v;
    uint64_t cap = 0, vreserved = 0;
    const uint64_t reserved = evote_load_group(a, r.group, s, v, &cap, &vreserved);
    // the group's claim: the head of a second run finds the word taken
    if (!step_claim(a.p.claim, r.group, i)) err = STEP_ERR_INVAL;
    if (!eprop_group_ok(a.p, s, cap, reserved) || !evote_state_ok(s, v, vreserved)) err = STEP_ERR_INVAL;
    if (!err) {
      uint64_t nroom = 0;
      evote_run<false>(a, i, r, s, v, false, 0, tot, nwon, nroom);
      if (cap - s.nlog < nroom) err = STEP_ERR_NOMEM;
    }
  }
  step_flag(a.p.head, err);
  if (valid) a.run_msgs[i] = tot;
  step_block_sums(tot, nwon, a.p.partial, blockIdx.x);
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_vote_apply(const EvoteArgs a) {
  __shared__ el_v2 s_rec[4][256];
  const auto [lane, wave, r0, i] = step_lane();
  const EvoteRec r = evote_load_wave(a.in, a.n, s_rec[wave], r0, lane);
  const bool head = step_is_head(a.in, a.n, i, r.group, lane);
  unsigned long long total = 0;
  const unsigned long long before = step_block_scan(i < a.n ? a.run_msgs[i] : 0, &total);
  if (head) {
    lp::State s;
    vs::Vote v;
    uint64_t cap = 0, vreserved = 0, nroom = 0;
    (void)evote_load_group(a, r.group, s, v, &cap, &vreserved);
    unsigned long long tot = 0, nwon = 0;
    evote_run<EMIT>(a, i, r, s, v, true, a.p.partial[2 * (uint64_t)blockIdx.x] + before, tot, nwon, nroom);
  }
}
