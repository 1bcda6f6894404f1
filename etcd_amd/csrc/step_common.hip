// step_common.hip -- what the batched raft step files share (log_append.hip,
// lead_step.hip, lead_prop.hip, vote_step.hip, ready_step.hip, follow_step.hip,
// compact_step.hip, tick_step.hip, conf_step.hip, node_start.hip): the call's head record and error classes, the claim word,
// the workgroup sums and scan, k_lead_scan, the record loaders and the
// write-back of a group's changed words.  DESIGN.md, "The step calls' common
// skeleton", has how a step call is put together from them.
#include "ewal_device.h"
#include "ewal_internal.h"
#include "lead_prop_step.h"
#include "vote_step.h"

namespace lp = lead_prop;
namespace vs = vote_step;

typedef uint64_t el_v2 __attribute__((ext_vector_type(2)));   // 16 bytes

// the whole-call error classes a counting pass ORs into the head's errflag
#define STEP_ERR_INVAL 1u
#define STEP_ERR_NOMEM 2u
#define STEP_NOCLAIM 0xFFFFFFFFu    // claim[g]: no run has named group g yet

// The call's head record: the flag word and the two totals k_lead_scan leaves.
// The host reads it at the one decision point.
struct EleadHead {
  uint32_t errflag, pad;
  unsigned long long n_msgs, n_committed;
};

// lane / wave of the thread, the wave's first record and the thread's own, one lane per record
struct StepLane {
  uint32_t lane, wave;
  uint64_t r0, i;
};
__device__ __forceinline__ StepLane step_lane() {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t r0 = (uint64_t)blockIdx.x * 256 + wave * 64;
  return StepLane{lane, wave, r0, r0 + lane};
}

// The group's claim: atomicMin of the record's ordinal into claim[g].  False:
// the word was taken -- a second run (or record) names the group.
__device__ __forceinline__ bool step_claim(uint32_t *claim, uint64_t g, uint64_t i) {
  return atomicMin(claim + g, (uint32_t)i) == STEP_NOCLAIM;
}

// ORs the lanes' error classes into the head's flag word
__device__ __forceinline__ void step_flag(EleadHead *head, uint32_t err) {
  if (__ballot(err != 0)) {
    if (err) atomicOr(&head->errflag, err);          // one atomic a wave (the compiler folds the active lanes)
  }
}

// The wave's 64 records of U 16-B units each as U coalesced 16-B loads per
// lane, transposed through the wave's U KiB of LDS: lane l gets the units of
// record r0 + l.  Every thread of the workgroup calls it (records past n come
// back as zeros).
template <uint32_t U, class T>
__device__ __forceinline__ void step_load_wave(const T *__restrict__ in, uint64_t n, el_v2 *s_wave, uint64_t r0,
                                               uint32_t lane, el_v2 (&out)[U]) {
  static_assert(sizeof(T) == U * 16, "a record is U 16-B units");
  const el_v2 *src = (const el_v2 *)(in + r0);
  const uint64_t left = r0 < n ? (n - r0 < 64 ? n - r0 : 64) * U : 0;   // 16-B units of this wave
  el_v2 x[U];
#pragma unroll
  for (uint32_t k = 0; k < U; ++k) {
    const uint32_t i = k * 64 + lane;
    x[k] = i < left ? src[i] : el_v2{0, 0};
  }
#pragma unroll
  for (uint32_t k = 0; k < U; ++k) s_wave[k * 64 + lane] = x[k];
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < U; ++k) out[k] = s_wave[lane * U + k];
}

// One record at an arbitrary place (a run's later records).
template <uint32_t U, class T>
__device__ __forceinline__ void step_load_rec(const T *p, el_v2 (&out)[U]) {
  static_assert(sizeof(T) == U * 16, "a record is U 16-B units");
  const el_v2 *src = (const el_v2 *)p;
#pragma unroll
  for (uint32_t k = 0; k < U; ++k) out[k] = src[k];
}

// whether record i starts a run: lane 0 of a wave looks at the record before its wave's
template <class T>
__device__ __forceinline__ bool step_is_head(const T *in, uint64_t n, uint64_t i, uint64_t group, uint32_t lane) {
  uint64_t prev = __shfl_up(group, 1);
  if (lane == 0 && i > 0 && i < n) prev = in[i - 1].group;
  return i < n && (i == 0 || prev != group);
}

__device__ __forceinline__ unsigned long long step_wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// the workgroup's two sums into partial[2 * slot ..]
__device__ __forceinline__ void step_block_sums(unsigned long long acc, unsigned long long napp,
                                                unsigned long long *partial, uint32_t slot) {
  __shared__ unsigned long long s_sum[4][2];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  acc = step_wave_sum(acc);
  napp = step_wave_sum(napp);
  if (lane == 0) {
    s_sum[wave][0] = acc;
    s_sum[wave][1] = napp;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[2 * (uint64_t)slot] = s_sum[0][0] + s_sum[1][0] + s_sum[2][0] + s_sum[3][0];
    partial[2 * (uint64_t)slot + 1] = s_sum[0][1] + s_sum[1][1] + s_sum[2][1] + s_sum[3][1];
  }
}

// the workgroup's exclusive prefix sum of v; *total = the workgroup's sum
__device__ __forceinline__ unsigned long long step_block_scan(unsigned long long v, unsigned long long *total) {
  __shared__ unsigned long long s_wsum[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long t = __shfl_up(incl, d);
    if ((int)lane >= d) incl += t;
  }
  if (lane == 63) s_wsum[wave] = incl;
  __syncthreads();
  unsigned long long base = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < 4; ++w) {
    const unsigned long long x = s_wsum[w];
    base += w < wave ? x : 0;
    all += x;
  }
  __syncthreads();                                 // s_wsum is free for the next call
  *total = all;
  return base + incl - v;
}

// One workgroup: the exclusive prefix sum of the workgroups' first sums in
// place (a thread owns a contiguous chunk of them), the two totals into the
// head record.
__global__ __launch_bounds__(256) void k_lead_scan(unsigned long long *__restrict__ partial, uint32_t nslots,
                                                   EleadHead *head) {
  // thread t owns the workgroups [t * chunk, (t + 1) * chunk)
  const uint32_t chunk = (nslots + 255u) / 256u;
  const uint64_t lo = (uint64_t)threadIdx.x * chunk;
  const uint64_t hi = lo + chunk < nslots ? lo + chunk : nslots;
  unsigned long long sum = 0, ncommit = 0;
  for (uint64_t s = lo; s < hi; ++s) {
    sum += partial[2 * s];
    ncommit += partial[2 * s + 1];
  }
  unsigned long long total = 0, ctotal = 0;
  unsigned long long at = step_block_scan(sum, &total);
  (void)step_block_scan(ncommit, &ctotal);
  for (uint64_t s = lo; s < hi; ++s) {
    const unsigned long long v = partial[2 * s];
    partial[2 * s] = at;
    at += v;
  }
  if (threadIdx.x == 0) {
    head->n_msgs = total;
    head->n_committed = ctotal;
  }
}

// Of group g's elead_group and elead_prop_state, the words a step changed (s0:
// the state the run started on).  A field the step never assigns compares a
// value with itself and costs nothing.
__device__ __forceinline__ void lp_store_changed(elead_group *groups, elead_prop_state *state, uint64_t g,
                                                 const lp::State &s0, const lp::State &s) {
  uint64_t *gw = (uint64_t *)(groups + g);
  uint64_t *sw = (uint64_t *)(state + g);
  if (s.term != s0.term) gw[1] = s.term;
  if (s.committed != s0.committed) gw[2] = s.committed;
  if (s.off != s0.off) gw[3] = s.off;
  if (s.nlog != s0.nlog) gw[4] = s.nlog;
  if (s.np != s0.np) gw[6] = s.np;
#pragma unroll
  for (uint32_t k = 0; k < lp::PEERS; ++k) {
    if (s.pid[k] != s0.pid[k]) gw[7 + k] = s.pid[k];
    if (s.match[k] != s0.match[k]) gw[14 + k] = s.match[k];
    if (s.next[k] != s0.next[k]) gw[21 + k] = s.next[k];
  }
  if (s.unstable != s0.unstable) sw[1] = s.unstable;
  if (s.pending != s0.pending) sw[2] = s.pending;
}

// ... and of its evote_state
__device__ __forceinline__ void vs_store_changed(evote_state *vstate, uint64_t g, const vs::Vote &v0,
                                                 const vs::Vote &v) {
  uint64_t *vw = (uint64_t *)(vstate + g);
  if (v.state != v0.state) vw[0] = v.state;
  if (v.vote != v0.vote) vw[1] = v.vote;
  if (v.lead != v0.lead) vw[2] = v.lead;
  if (v.elapsed != v0.elapsed) vw[3] = v.elapsed;
  if (v.voted != v0.voted) vw[4] = v.voted;
  if (v.granted != v0.granted) vw[5] = v.granted;
}
