// tick_step.h -- the decision of the batched Tick (etick_batch_device), shared
// by its kernels (tick_step.hip), the exported host function etick_draw
// (step_api.hip) and the host check (tests/host/tick_forms.cpp).  Plain C++17,
// no HIP header.
//
// decide() is one node.Tick() on a raft group (raft/node.go:237-238, 262-269):
// r.tick() is tickHeartbeat at a leader and tickElection at a follower or a
// candidate (raft/raft.go:287-307, 317, 325, 339), with promotable (:590-595)
// and isElectionTimeout (:608-617).  raft.elapsed is Go's int: int64 that wraps,
// compared signed; the record holds its two's-complement bits.
//
// decide() writes nothing.  It says what elapsed becomes, whether a msgHup or a
// msgBeat leaves, and which rand.Int() value was consumed; the traffic is the
// caller's.
#pragma once
#include <cstdint>

#ifndef EWAL_HD
#ifdef __HIPCC__
#define EWAL_HD __host__ __device__
#else
#define EWAL_HD
#endif
#endif

namespace tick_step {

constexpr uint32_t PEERS = 7;
constexpr int32_t ST_OK = 0, ST_UNSUPPORTED = 48;    // include/ewal.h's codes
// etick_result.action
constexpr int32_t IDLE = 1, HELD = 2, HUP = 3, BEAT = 4, NOT_PROMOTABLE = 5, PANICKED = 6;
constexpr uint64_t LEADER = 2;                        // raft.StateLeader

struct In {
  uint64_t state, elapsed;         // evote_state.state, .elapsed
  uint64_t id, term, np;           // elead_group.id, .term, .n_peers
  uint64_t pid[PEERS];
};

struct Out {
  int32_t status, action;
  uint64_t elapsed;                // raft.elapsed afterwards
  uint64_t draw;                   // the rand.Int() value consumed (HELD, HUP), else 0
};

// The library's stand-in for the process-wide rand.Int(): a 63-bit value from
// the seed, the node's id and term and the incremented elapsed.
EWAL_HD inline uint64_t draw(uint64_t seed, uint64_t id, uint64_t term, uint64_t elapsed) {
  uint64_t x = seed ^ id * 0x9E3779B97F4A7C15ull ^ term * 0xBF58476D1CE4E5B9ull ^ elapsed * 0x94D049BB133111EBull;
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x >> 1;
}

// promotable: r.prs has the key r.id
EWAL_HD inline bool promotable(const In &in) {
  bool self = false;
  for (uint32_t k = 0; k < PEERS; ++k) self |= k < in.np && in.pid[k] == in.id;
  return self;
}

// isElectionTimeout's last line, d >= 0: d > int(r) % election, as written
EWAL_HD inline bool fires_plain(int64_t d, uint64_t r, int64_t election) {
  return d > (int64_t)(r % (uint64_t)election);
}

// ... and without the 64-bit modulo where it cannot matter: r % election <=
// election - 1, so d >= election fires whatever r is
EWAL_HD inline bool fires(int64_t d, uint64_t r, int64_t election) {
  if (d >= election) return true;
  return d > (int64_t)(r % (uint64_t)election);
}

// One tick of the group `in`.  election is in [1, 2^31 - 1], heartbeat in
// [0, 2^31 - 1].  have_draw: r is the draw itself (d_draws[i], < 2^63);
// otherwise r is the seed and the draw is draw(seed, id, term, e).
EWAL_HD inline Out decide(const In &in, int64_t election, int64_t heartbeat, bool have_draw, uint64_t r) {
  Out o;
  o.status = ST_OK;
  o.draw = 0;
  if (in.np > PEERS) {
    o.status = ST_UNSUPPORTED;
    o.action = PANICKED;
    o.elapsed = in.elapsed;
    return o;
  }
  const uint64_t e = in.elapsed + 1;                 // r.elapsed++, wrapping
  if (in.state == LEADER) {                          // tickHeartbeat
    const bool beat = (int64_t)e > heartbeat;
    o.action = beat ? BEAT : IDLE;
    o.elapsed = beat ? 0 : e;
    return o;
  }
  if (!promotable(in)) {                             // tickElection: elapsed = 0, return
    o.action = NOT_PROMOTABLE;
    o.elapsed = 0;
    return o;
  }
  const int64_t d = (int64_t)(e - (uint64_t)election);   // isElectionTimeout
  if (d < 0) {
    o.action = IDLE;
    o.elapsed = e;
    return o;
  }
  o.draw = have_draw ? r : draw(r, in.id, in.term, e);
  const bool hup = fires(d, o.draw, election);
  o.action = hup ? HUP : HELD;
  o.elapsed = hup ? 0 : e;
  return o;
}

}  // namespace tick_step
