// msg_encode.hip -- batched raftpb.Message.Marshal for the /raft egress
// (raft/raftpb/raft.pb.go:1000-1068, called per outgoing message by send,
// etcdserver/cluster_store.go:118-144), over messages whose Entries and
// Snapshot.Data are resident in HBM.
//
//   msg   = 08 v(Type) 10 v(To) 18 v(From) 20 v(Term) 28 v(LogTerm) 30 v(Index)
//           {3a v(|E|) E}* 40 v(Commit) 4a v(|S|) S 50 (00|01)
//   E     = 08 v(Type) 10 v(Term) 18 v(Index) 22 v(len Data) Data
//   S     = 0a v(len Data) Data {10 v(node)}* 18 v(Index) 20 v(Term) {28 v(removed)}*
//
// Sizes first, bytes second:
//   k_menc_esz   one thread per entry of d_ents: its framed size 1 + |v(|E|)| + |E|
//                and its range check; an exclusive sum gives X[].  A message's
//                entry bytes are X[first + n] - X[first], whichever other
//                messages share the range.
//   k_menc_usz   one thread per value of d_u64: 1 + |v(value)|; the exclusive
//                sum NX[] does for Nodes / RemovedNodes what X[] does for Entries.
//   k_menc_msz   one thread per message: its range checks and size; an
//                exclusive sum gives moff[].
//   k_menc_body  output-tile driven.  A wave owns EME_TILE bytes of d_out,
//                a lane EME_RUN contiguous bytes of them.  The wave finds the
//                messages its tile touches with two 64-ary searches in
//                moff[]; the lane finds its run's message among them, its
//                place inside the message from the region ends (msg_layout)
//                and, in the Entries or a node list, by a binary search in
//                X[] / NX[].  From there it walks forward, composing header
//                bytes in registers and taking payload bytes with 16-B
//                aligned loads (each loaded once) realigned in registers,
//                and puts every full 16 bytes into the wave's tile in LDS.
//                The wave then stores the tile to d_out, 1 KiB a store
//                instruction.  A header, varint or payload that straddles
//                two runs or two tiles is composed by both owners, each
//                keeping its own bytes.
// Every byte of d_out below the total has exactly one writer, every store is
// one aligned 16 bytes (the output's last, partial 16 bytes: byte stores),
// there are no atomics on d_out, and a wave's work is bounded by its tile
// whatever the batch looks like: one 256 MiB Snapshot is 32 Ki tiles, a
// million heartbeats ~340 messages per tile, 5 or 6 per lane.
#include "ewal_device.h"
#include "ewal_internal.h"
#include "ewal_wire.h"

#define EME_RUN 128u                           // contiguous output bytes per lane and tile
#define EME_TILE (64u * EME_RUN)               // bytes of d_out per wave
#define EME_WAVES 4u                           // waves per k_menc_body workgroup
#define EME_MIN_MSG 24u                        // Message{}: no message is shorter
#define EME_ERR_RANGE 1u                       // a range outside its array, data_nil == 2
#define EME_ERR_BIG 2u                         // sizes whose sum does not fit 64 bits

typedef unsigned __int128 eme_u128;

// saturating sum: the scans' operator (associative), ~0 = does not fit
struct EmeSatAdd {
  __host__ __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const {
    const uint64_t s = a + b;
    return s < a ? ~0ull : s;
  }
};

struct EmeArgs {
  const uint8_t *data;
  uint64_t data_len;
  const emsg_out *msgs;
  uint64_t n;
  const ewal_entry *ents;
  const uint64_t *u64;
  const uint64_t *X;      // n_ents_total + 1
  const uint64_t *NX;     // n_u64 + 1
  const uint64_t *moff;   // n + 1
  uint8_t *out;
  uint64_t total;
};

using ewal_wire::entry_size;
using ewal_wire::sov;

// fsz[i] = framed size of entry i, fsz[ne] = 0 (so that the exclusive sum's last element is the total)
__global__ __launch_bounds__(256) void k_menc_esz(const ewal_entry *__restrict__ ents, uint64_t ne, uint64_t data_len,
                                                  uint64_t *__restrict__ fsz, uint32_t *__restrict__ errflag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > ne) return;
  uint64_t z = 0;
  if (i < ne) {
    const ewal_entry e = ents[i];
    if (e.data_nil == 2 || e.data_len > data_len || e.data_off > data_len - e.data_len) {
      atomicOr(errflag, EME_ERR_RANGE);
    } else {
      const uint64_t E = entry_size(e.type, e.term, e.index, e.data_len);
      z = 1 + sov(E) + E;
    }
  }
  fsz[i] = z;
}

__global__ __launch_bounds__(256) void k_menc_usz(const uint64_t *__restrict__ u, uint64_t nu,
                                                  uint64_t *__restrict__ usz) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > nu) return;
  usz[i] = i < nu ? 1 + sov(u[i]) : 0;
}

// Message regions, by their ends relative to the message's first byte:
//   0 head   1 Entries   2 `40 v(Commit) 4a v(|S|) 0a v(len Data)`   3 Snapshot.Data
//   4 Nodes  5 `18 v(Index) 20 v(Term)`   6 RemovedNodes   7 `50 (00|01)`
struct MsgLay {
  uint64_t e[8];
  uint64_t S;   // |S|
};
// false: a size does not fit 64 bits.  The ranges of m are inside their arrays.
__device__ __forceinline__ bool msg_layout(const emsg_out &m, const uint64_t *__restrict__ X,
                                           const uint64_t *__restrict__ NX, MsgLay &L) {
  const uint64_t eb = X[m.ents_first + m.n_ents] - X[m.ents_first];
  const uint64_t nb = NX[m.snap_nodes_off + m.snap_n_nodes] - NX[m.snap_nodes_off];
  const uint64_t rb = NX[m.snap_removed_off + m.snap_n_removed] - NX[m.snap_removed_off];
  const uint64_t it = 2 + sov(m.snap_index) + sov(m.snap_term);
  bool ov = false;
  uint64_t S = 1 + sov(m.snap_data_len) + it;
  ov |= __builtin_add_overflow(S, m.snap_data_len, &S);
  ov |= __builtin_add_overflow(S, nb, &S);
  ov |= __builtin_add_overflow(S, rb, &S);
  L.S = S;
  L.e[0] = 6 + sov(m.type) + sov(m.to) + sov(m.from) + sov(m.term) + sov(m.log_term) + sov(m.index);
  ov |= __builtin_add_overflow(L.e[0], eb, &L.e[1]);
  ov |= __builtin_add_overflow(L.e[1], (uint64_t)(3 + sov(m.commit) + sov(S) + sov(m.snap_data_len)), &L.e[2]);
  ov |= __builtin_add_overflow(L.e[2], m.snap_data_len, &L.e[3]);
  ov |= __builtin_add_overflow(L.e[3], nb, &L.e[4]);
  ov |= __builtin_add_overflow(L.e[4], it, &L.e[5]);
  ov |= __builtin_add_overflow(L.e[5], rb, &L.e[6]);
  ov |= __builtin_add_overflow(L.e[6], (uint64_t)2, &L.e[7]);
  return !ov;
}

// msz[i] = Message i's Size(), msz[n] = 0
__global__ __launch_bounds__(256) void k_menc_msz(const emsg_out *__restrict__ msgs, uint64_t n, uint64_t ne,
                                                  uint64_t nu, uint64_t data_len, const uint64_t *__restrict__ X,
                                                  const uint64_t *__restrict__ NX, uint64_t *__restrict__ msz,
                                                  uint32_t *__restrict__ errflag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  if (i == n) {
    if (X[ne] == ~0ull || NX[nu] == ~0ull) atomicOr(errflag, EME_ERR_BIG);
    msz[i] = 0;
    return;
  }
  const emsg_out m = msgs[i];
  uint64_t z = 0;
  if (m.n_ents > ne || m.ents_first > ne - m.n_ents || m.snap_n_nodes > nu || m.snap_nodes_off > nu - m.snap_n_nodes ||
      m.snap_n_removed > nu || m.snap_removed_off > nu - m.snap_n_removed || m.snap_data_len > data_len ||
      m.snap_data_off > data_len - m.snap_data_len) {
    atomicOr(errflag, EME_ERR_RANGE);
  } else {
    MsgLay L;
    z = msg_layout(m, X, NX, L) ? L.e[7] : ~0ull;
  }
  msz[i] = z;
}

__global__ __launch_bounds__(256) void k_menc_pack(const uint64_t *__restrict__ moff, uint64_t n,
                                                   emsg_encoded *__restrict__ enc) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  emsg_encoded r;
  r.off = moff[i];
  r.len = moff[i + 1] - r.off;
  enc[i] = r;
}

// The last i in [lo, hi) with arr[i] <= key; arr ascending, arr[lo] <= key.
// The whole wave calls it with the same arguments: 64 probes a step.
__device__ __forceinline__ uint64_t wave_search(const uint64_t *__restrict__ arr, uint64_t lo, uint64_t hi,
                                                uint64_t key, uint32_t lane) {
  while (hi - lo > 1) {
    const uint64_t step = (hi - lo + 63) / 64;
    const uint64_t idx = lo + (uint64_t)lane * step;
    const bool ok = idx < hi && arr[idx] <= key;   // a prefix of the lanes, lane 0 among them
    const uint32_t c = (uint32_t)__popcll(__ballot(ok)) - 1u;
    lo += (uint64_t)c * step;
    hi = std::min(hi, lo + step);
  }
  return lo;
}
__device__ __forceinline__ uint64_t lane_search(const uint64_t *__restrict__ arr, uint64_t lo, uint64_t hi,
                                                uint64_t key) {
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (arr[mid] <= key) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ eme_u128 eme_pack(const ew_v4u q) {
  return (eme_u128)((uint64_t)q.x | ((uint64_t)q.y << 32)) | ((eme_u128)((uint64_t)q.z | ((uint64_t)q.w << 32)) << 64);
}
__device__ __forceinline__ ew_v4u eme_unpack(const eme_u128 v) {
  ew_v4u q;
  q.x = (uint32_t)v; q.y = (uint32_t)(v >> 32); q.z = (uint32_t)(v >> 64); q.w = (uint32_t)(v >> 96);
  return q;
}

// A lane's EME_RUN output bytes, produced front to back into its slice of the
// wave's tile in LDS, 16 bytes at a time.  The producers below run over a
// region from its start: the first `skip` bytes fall before the lane's run,
// the next ones fill it.
struct EmeWin {
  eme_u128 w;         // the 16-B unit being filled
  eme_u128 cv;        // the last aligned 16 source bytes loaded ...
  uint64_t ca;        // ... and their offset in d_data (~0: none)
  uint64_t skip;
  uint32_t done, want;
  uint8_t *lds;
  __device__ __forceinline__ bool full() const { return done >= want; }
  __device__ __forceinline__ void advance(uint32_t nb) {
    done += nb;
    if (!(done & 15u) || done == want) {
      *(ew_v4u *)(lds + ((done - 1u) & ~15u)) = eme_unpack(w);
      w = 0;
    }
  }
  __device__ __forceinline__ void put(uint8_t b) {
    if (skip) { --skip; return; }
    if (done < want) {
      w |= (eme_u128)b << (8u * (done & 15u));
      advance(1);
    }
  }
  // tag v(value)
  __device__ __forceinline__ void fld(uint8_t tag, uint64_t v) {
    const uint32_t s = 1 + sov(v);
    if (skip >= s) { skip -= s; return; }
    if (full()) return;
    put(tag);
    while (v >= 0x80) { put((uint8_t)(v | 0x80)); v >>= 7; }
    put((uint8_t)v);
  }
  // the aligned 16 bytes at a: each is loaded once as the run moves forward
  __device__ __forceinline__ eme_u128 block(const uint8_t *__restrict__ data, uint64_t a) {
    if (a != ca) {
      cv = eme_pack(*(const ew_v4u *)(data + a));
      ca = a;
    }
    return cv;
  }
  // data[off, off + nb), 1 <= nb <= 16, little-endian in the low nb bytes
  // (the rest is unspecified).  data is 16-B aligned; the loads are aligned
  // 16 bytes that lie inside [data, data + data_len) -- the array's last,
  // partial 16 bytes are read a byte at a time.
  __device__ __forceinline__ eme_u128 load_run(const uint8_t *__restrict__ data, uint64_t data_len, uint64_t off,
                                               uint32_t nb) {
    const uint64_t a = off & ~15ull;
    const uint32_t sh = (uint32_t)(off & 15u);
    const bool two = sh + nb > 16u;
    if (a + (two ? 32u : 16u) <= data_len) {
      eme_u128 v = block(data, a);
      if (sh) {
        v >>= 8u * sh;
        if (two) v |= block(data, a + 16) << (8u * (16u - sh));
      }
      return v;
    }
    eme_u128 v = 0;
    for (uint32_t i = 0; i < nb; ++i) v |= (eme_u128)data[off + i] << (8u * i);
    return v;
  }
  // data[off, off + len)
  __device__ __forceinline__ void bytes(const uint8_t *__restrict__ data, uint64_t data_len, uint64_t off,
                                        uint64_t len) {
    if (skip >= len) { skip -= len; return; }
    off += skip;
    len -= skip;
    skip = 0;
    while (len && done < want) {
      const uint32_t f = done & 15u;
      const uint32_t nb = (uint32_t)std::min<uint64_t>(len, std::min(16u - f, want - done));
      eme_u128 v = load_run(data, data_len, off, nb);
      if (nb < 16u) v &= ((eme_u128)1 << (8u * nb)) - 1;
      w |= v << (8u * f);
      off += nb;
      len -= nb;
      advance(nb);
    }
  }
};

// The `want` bytes of the output at p, which lies in message m, into lds.
__device__ __forceinline__ void gen_run(const EmeArgs &a, uint64_t p, uint32_t want, uint64_t m, uint8_t *lds) {
  EmeWin W;
  W.w = 0;
  W.cv = 0;
  W.ca = ~0ull;
  W.skip = 0;
  W.done = 0;
  W.want = want;
  W.lds = lds;
  uint64_t r = p - a.moff[m];   // the place inside message m; 0 in the messages after it
  for (; !W.full(); ++m, r = 0) {
    const emsg_out M = a.msgs[m];
    MsgLay L;
    msg_layout(M, a.X, a.NX, L);
    if (r < L.e[0]) {
      W.skip = r;
      W.fld(0x08, M.type); W.fld(0x10, M.to); W.fld(0x18, M.from);
      W.fld(0x20, M.term); W.fld(0x28, M.log_term); W.fld(0x30, M.index);
      r = L.e[0];
    }
    if (!W.full() && r < L.e[1]) {
      const uint64_t j1 = M.ents_first + M.n_ents;
      const uint64_t q = r - L.e[0] + a.X[M.ents_first];
      uint64_t j = lane_search(a.X, M.ents_first, j1, q);
      uint64_t x0 = a.X[j];
      W.skip = q - x0;
      for (; j < j1 && !W.full(); ++j) {
        const ewal_entry e = a.ents[j];
        const uint64_t x1 = a.X[j + 1];
        const uint64_t hdr = x1 - x0 - e.data_len;   // `3a v(|E|)` and E's four fields
        x0 = x1;
        if (W.skip >= hdr) {
          W.skip -= hdr;
        } else {
          W.fld(0x3a, entry_size(e.type, e.term, e.index, e.data_len));
          W.fld(0x08, (uint64_t)(int64_t)e.type); W.fld(0x10, e.term); W.fld(0x18, e.index);
          W.fld(0x22, e.data_len);
        }
        W.bytes(a.data, a.data_len, e.data_off, e.data_len);
      }
      r = L.e[1];
    }
    if (!W.full() && r < L.e[2]) {
      W.skip = r - L.e[1];
      W.fld(0x40, M.commit); W.fld(0x4a, L.S); W.fld(0x0a, M.snap_data_len);
      r = L.e[2];
    }
    if (!W.full() && r < L.e[3]) {
      W.skip = r - L.e[2];
      W.bytes(a.data, a.data_len, M.snap_data_off, M.snap_data_len);
      r = L.e[3];
    }
    if (!W.full() && r < L.e[4]) {
      const uint64_t k1 = M.snap_nodes_off + M.snap_n_nodes;
      const uint64_t q = r - L.e[3] + a.NX[M.snap_nodes_off];
      uint64_t k = lane_search(a.NX, M.snap_nodes_off, k1, q);
      W.skip = q - a.NX[k];
      for (; k < k1 && !W.full(); ++k) W.fld(0x10, a.u64[k]);
      r = L.e[4];
    }
    if (!W.full() && r < L.e[5]) {
      W.skip = r - L.e[4];
      W.fld(0x18, M.snap_index); W.fld(0x20, M.snap_term);
      r = L.e[5];
    }
    if (!W.full() && r < L.e[6]) {
      const uint64_t k1 = M.snap_removed_off + M.snap_n_removed;
      const uint64_t q = r - L.e[5] + a.NX[M.snap_removed_off];
      uint64_t k = lane_search(a.NX, M.snap_removed_off, k1, q);
      W.skip = q - a.NX[k];
      for (; k < k1 && !W.full(); ++k) W.fld(0x28, a.u64[k]);
      r = L.e[6];
    }
    if (!W.full()) {
      W.skip = r - L.e[6];
      W.put(0x50);
      W.put(M.reject ? 1 : 0);
    }
  }
}

// Persistent workgroups, tiles dealt round-robin (EME_WAVES consecutive tiles
// a round, one per wave).  The lanes produce their runs into the wave's tile
// in LDS; the wave then stores the tile to d_out 1 KiB a store.
__global__ __launch_bounds__(64 * EME_WAVES) void k_menc_body(const EmeArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_tile[EME_WAVES][EME_TILE];
  const uint32_t lane = threadIdx.x & 63u;
  uint8_t *st = s_tile[threadIdx.x >> 6];
  const uint64_t ntiles = (a.total + EME_TILE - 1) / EME_TILE;
  for (uint64_t tb = blockIdx.x; tb * EME_WAVES < ntiles; tb += gridDim.x) {
    const uint64_t t = tb * EME_WAVES + (threadIdx.x >> 6);
    const uint64_t t0 = t * EME_TILE, t1 = std::min<uint64_t>(t0 + EME_TILE, a.total);
    if (t < ntiles) {
      // the messages of the tile's first and last byte
      const uint64_t m_lo = wave_search(a.moff, 0, a.n, t0, lane);
      const uint64_t m_hi =
          wave_search(a.moff, m_lo, std::min<uint64_t>(a.n, m_lo + EME_TILE / EME_MIN_MSG + 2), t1 - 1, lane);
      const uint64_t p = t0 + (uint64_t)EME_RUN * lane;
      if (p < t1)
        gen_run(a, p, (uint32_t)std::min<uint64_t>(EME_RUN, t1 - p), lane_search(a.moff, m_lo, m_hi + 1, p),
                st + EME_RUN * lane);
    }
    __syncthreads();
    if (t < ntiles) {
#pragma unroll
      for (uint32_t k = 0; k < EME_RUN / 16u; ++k) {
        const uint32_t o = 16u * (k * 64u + lane);
        const uint64_t q = t0 + o;
        if (q >= t1) break;
        const ew_v4u v = *(const ew_v4u *)(st + o);
        if (q + 16 <= t1) {
          *(ew_v4u *)(a.out + q) = v;
        } else {   // the output's last, partial 16 bytes
          const eme_u128 x = eme_pack(v);
          for (uint32_t i = 0; i < (uint32_t)(t1 - q); ++i) a.out[q + i] = (uint8_t)(x >> (8u * i));
        }
      }
    }
    __syncthreads();
  }
}
