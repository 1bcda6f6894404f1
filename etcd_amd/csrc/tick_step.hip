// tick_step.hip -- node.Tick on the shared group records: tickElection or
// tickHeartbeat over n selected groups of G.  The decision is tick_step.h's
// (shared with the host check and etick_draw); this file is the assignment of
// work and the memory traffic.
//
// A tick reads 176 bytes of a group -- the first 112 of its 256-byte
// elead_group (id, term, n_peers, peer_id[7]) and its 64-byte evote_state --
// and mostly writes one word of it, so the whole call is the traffic.  ONE LANE
// PER SELECTION in both passes; match[] and next[] are never read.
//
//   k_tick_count   nothing of the caller's modified.  Without d_sel the wave's
//                  64 groups lie side by side: their 7-unit heads and their
//                  evote_state come in as coalesced 16-B loads (a load
//                  instruction covers nine whole heads, not 64 cache lines) and
//                  are transposed through the wave's LDS.  With d_sel a lane
//                  loads its own group's units.  The reserved words of the
//                  elead_group, which the whole-call check looks at, are the
//                  one piece past byte 112.  The lane claims the group (with
//                  d_sel), runs the checks and the decision and leaves it in
//                  rec[i]; the workgroup's sums go to hpart[] (msgHup, msgBeat)
//                  and bpart[] (msgBeat).
//   k_lead_scan    step_common.hip's, twice: the workgroups' offsets in both
//                  outputs; the first head has both totals (n_msgs the msgHup,
//                  n_committed the msgBeat).  The host reads it -- the one
//                  decision point.
//   k_tick_apply   reads rec[] and the scanned offsets, no group record: d_res,
//                  and with EMIT the elapsed words that changed, the evote_msg
//                  of a HUP and the elead_local of a BEAT, each placed by a
//                  block scan.  <false> is the peek.
//
// Only lanes with 0 <= d < election run the 64-bit modulo (tick_step.h's
// fires()): a wave with none of them skips the sequence.
//
// Uses step_common.hip.
#include "ewal_device.h"
#include "ewal_internal.h"
#include "tick_step.h"

namespace ts = tick_step;

#define ETICK_CHANGED (1ull << 48)  // EtickRec.meta: elapsed differs from what the call found

struct EtickRec {                   // 32 bytes per selection
  unsigned long long meta;          // status | action << 32 | ETICK_CHANGED
  unsigned long long elapsed;       // raft.elapsed after the tick
  unsigned long long draw;
  unsigned long long id;            // the msgHup's From
};

struct EtickArgs {
  const elead_group *groups;
  evote_state *vstate;
  uint64_t G;
  const uint64_t *sel;              // nullable
  uint64_t n;
  int64_t election, heartbeat;
  const uint64_t *draws;            // nullable
  uint64_t seed;
  etick_result *res;
  evote_msg *hups;                  // NULL (with beats): the peek
  elead_local *beats;
  uint32_t *claim;                  // G (with sel)
  EtickRec *rec;                    // n
  unsigned long long *hpart;        // 2 per workgroup: msgHup, msgBeat
  unsigned long long *bpart;        // 2 per workgroup: msgBeat, 0
  EleadHead *head, *bhead;
};

// The wave's 64 adjacent records of STRIDE 16-B units each, their first U units:
// U coalesced 16-B loads per lane, transposed through the wave's LDS.  Every
// thread of the workgroup calls it; records past n come back as zeros.
template <uint32_t U, uint32_t STRIDE>
__device__ __forceinline__ void etick_fetch_wave(const el_v2 *__restrict__ src, uint64_t n, uint64_t r0, uint32_t lane,
                                                 el_v2 (&x)[U]) {
  const uint32_t left = r0 < n ? (uint32_t)(n - r0 < 64 ? n - r0 : 64) * U : 0;
#pragma unroll
  for (uint32_t k = 0; k < U; ++k) {
    const uint32_t i = k * 64 + lane, rec = i / U, unit = i - rec * U;
    x[k] = i < left ? src[(r0 + rec) * STRIDE + unit] : el_v2{0, 0};
  }
}
template <uint32_t U>
__device__ __forceinline__ void etick_transpose(el_v2 *s_wave, uint32_t lane, el_v2 (&x)[U]) {
#pragma unroll
  for (uint32_t k = 0; k < U; ++k) s_wave[k * 64 + lane] = x[k];
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < U; ++k) x[k] = s_wave[lane * U + k];
  __syncthreads();                                   // the wave's words are free for the next record kind
}

__global__ __launch_bounds__(256) void k_tick_count(const EtickArgs a) {
  __shared__ el_v2 s_rec[4][448];
  const auto [lane, wave, r0, i] = step_lane();
  const bool valid = i < a.n;
  uint32_t err = 0;
  uint64_t g = i;
  el_v2 gu[7], vu[4];
  if (a.sel) {
    g = valid ? a.sel[i] : 0;
    if (valid && g >= a.G) err = STEP_ERR_INVAL;
    const bool ld = valid && !err;
    const el_v2 *gp = (const el_v2 *)(a.groups + (ld ? g : 0));
    const el_v2 *vp = (const el_v2 *)(a.vstate + (ld ? g : 0));
#pragma unroll
    for (uint32_t k = 0; k < 7; ++k) gu[k] = ld ? gp[k] : el_v2{0, 0};
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) vu[k] = ld ? vp[k] : el_v2{0, 0};
  } else {
    etick_fetch_wave<7, 16>((const el_v2 *)a.groups, a.n, r0, lane, gu);
    etick_fetch_wave<4, 4>((const el_v2 *)a.vstate, a.n, r0, lane, vu);
    etick_transpose(s_rec[wave], lane, gu);
    etick_transpose(s_rec[wave], lane, vu);
  }
  uint64_t dr = a.seed;
  if (a.draws && valid) {
    dr = a.draws[i];
    if (dr >> 63) err = STEP_ERR_INVAL;
  }
  ts::Out o{0, 0, 0, 0};
  ts::In in{};
  if (valid && !err) {
    const el_v2 *gp = (const el_v2 *)(a.groups + g);
    const el_v2 g14 = gp[14], g15 = gp[15];
    // the group's claim: a second selection of the group finds the word taken
    if (a.sel && !step_claim(a.claim, g, i)) err = STEP_ERR_INVAL;
    in.state = vu[0].x;
    in.elapsed = vu[1].y;
    in.id = gu[0].x;
    in.term = gu[0].y;
    in.np = gu[3].x;
    in.pid[0] = gu[3].y;
    in.pid[1] = gu[4].x, in.pid[2] = gu[4].y;
    in.pid[3] = gu[5].x, in.pid[4] = gu[5].y;
    in.pid[5] = gu[6].x, in.pid[6] = gu[6].y;
    if ((g14.x | g14.y | g15.x | g15.y | vu[3].x | vu[3].y) != 0 || in.state > 2) err = STEP_ERR_INVAL;
    bool dup = false;
#pragma unroll
    for (uint32_t j = 1; j < ts::PEERS; ++j)
#pragma unroll
      for (uint32_t k = 0; k < j; ++k) dup |= j < in.np && in.pid[j] == in.pid[k];
    if (dup) err = STEP_ERR_INVAL;
    if (!err) o = ts::decide(in, a.election, a.heartbeat, a.draws != nullptr, dr);
  }
  step_flag(a.head, err);
  if (valid) {
    const bool changed = !err && o.elapsed != in.elapsed;
    el_v2 *q = (el_v2 *)(a.rec + i);
    q[0] = el_v2{(uint64_t)(uint32_t)o.status | ((uint64_t)(uint32_t)o.action << 32) | (changed ? ETICK_CHANGED : 0ull),
                 o.elapsed};
    q[1] = el_v2{o.draw, in.id};
  }
  const unsigned long long hup = o.action == ts::HUP ? 1 : 0, beat = o.action == ts::BEAT ? 1 : 0;
  step_block_sums(hup, beat, a.hpart, blockIdx.x);
  __syncthreads();                                   // the sums' staging words are reused
  step_block_sums(beat, 0, a.bpart, blockIdx.x);
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_tick_apply(const EtickArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < a.n;
  el_v2 r0{0, 0}, r1{0, 0};
  if (valid) {
    const el_v2 *rq = (const el_v2 *)(a.rec + i);
    r0 = rq[0];
    r1 = rq[1];
  }
  const int32_t action = (int32_t)((r0.x >> 32) & 0xffffu);
  const unsigned long long hup = action == ts::HUP ? 1 : 0, beat = action == ts::BEAT ? 1 : 0;
  unsigned long long total = 0;
  const unsigned long long hat = a.hpart[2 * (uint64_t)blockIdx.x] + step_block_scan(hup, &total);
  const unsigned long long bat = a.bpart[2 * (uint64_t)blockIdx.x] + step_block_scan(beat, &total);
  if (!valid) return;
  el_v2 *q = (el_v2 *)(a.res + i);
  q[0] = el_v2{r0.x & 0xffffffffffffull, r0.y};
  q[1] = el_v2{hup ? hat : beat ? bat : 0, r1.x};
  if (!EMIT) return;
  const uint64_t g = a.sel ? a.sel[i] : i;
  if (r0.x & ETICK_CHANGED) ((uint64_t *)(a.vstate + g))[3] = r0.y;
  if (hup) {                                         // pb.Message{From: r.id, Type: msgHup}
    el_v2 *m = (el_v2 *)(a.hups + hat);
    m[0] = el_v2{g, 0};
    m[1] = el_v2{r1.y, 0};
    m[2] = el_v2{0, 0};
    m[3] = el_v2{0, 0};
  }
  if (beat) {                                        // pb.Message{From: r.id, Type: msgBeat}
    el_v2 *m = (el_v2 *)(a.beats + bat);
    m[0] = el_v2{g, 1};
    m[1] = el_v2{0, 0};
    m[2] = el_v2{0, 0};
  }
}
