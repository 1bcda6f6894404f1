// aux_kernels.hip -- snapshot CRC batch verify, batched raft quorum commit and
// the batched WAL write pipeline.
//
//   k_snap    snap.loadSnap (snap/snapshotter.go:76-111): snappb.Snapshot
//             Unmarshal (snap/snappb/snap.pb.go:42-120), crc32.Update(0, tab,
//             Data) against the stored Crc, then raftpb.Snapshot Unmarshal
//             (raft/raftpb/raft.pb.go:279-406).  The CRC of each file's Data
//             comes from the same stream prefixes as the WAL path (k_stream
//             with find_cand = 0 over the packed batch).
//   k_commit  raft.maybeCommit (raft/raft.go:248-258, q() :275-277) +
//             raftLog.maybeCommit / term / at / isOutOfBounds
//             (raft/log.go:115-154, 194-217), one lane per raft group.
//   k_wr_*    (*WAL).SaveEntry / SaveState / Cut (wal/wal.go:219-279) over a
//             batch of records: sizes, bodies, one stream pass for every
//             chained CRC, frames (the banner further down).
#include "ewal_device.h"
#include "ewal_internal.h"
#include "ewal_wire.h"

__global__ __launch_bounds__(256) void k_snap(const uint8_t *__restrict__ buf, const uint32_t *__restrict__ pwave,
                       const uint32_t *__restrict__ v, const uint32_t *__restrict__ g_slice,
                       const uint32_t *__restrict__ g_shift, SnapDesc *__restrict__ sd,
                       esnap_snapshot *__restrict__ snaps, uint32_t n) {
  __shared__ uint32_t s_t4[1024];
  __shared__ uint32_t s_svp[1024];   // S_256 (prefix_at's Horner step)
  stage_lds<256>(s_t4, 1024, [&](int i) { return g_slice[i]; });
  stage_lds<256>(s_svp, 1024, [&](int i) { return g_shift[EW_VLOG * 1024 + i]; });
  __syncthreads();
  uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n) return;
  SnapDesc d = sd[f];
  PbField a1, a2, a3, a4, a5;
  pbf_init(a1); pbf_init(a2); pbf_init(a3); pbf_init(a4); pbf_init(a5);
  int unrec;
  int st = pb_walk<PB_VAR32, PB_BYTES, PB_NONE, PB_NONE, PB_NONE>(buf + d.off, (int64_t)d.len, a1, a2, a3, a4, a5,
                                                                  unrec, nullptr, nullptr, 0);
  d.stored = (uint32_t)a1.v;
  d.doff = d.off + (a2.blen > 0 ? (uint64_t)a2.boff : 0);
  d.dlen = a2.blen > 0 ? (uint64_t)a2.blen : 0;
  d.computed = 0;
  if (st == 0) {
    // crc32.Update(0, crcTable, Data) = S_n(~0 ^ P(s)) ^ P(e) ^ ~0
    if (a2.split) {   // Data = the concatenation of its segments (snap.pb.go append)
      const uint32_t lin = bytes_field_lin(buf + d.off, (int64_t)d.len, 2, 0x6u, d.off, buf, pwave, v, s_t4, s_svp, g_shift);
      d.computed = gshift_n(g_shift, d.dlen, 0xffffffffu) ^ lin ^ 0xffffffffu;
    } else if (d.dlen == 0) {
      d.computed = 0;
    } else {
      const uint32_t Ps = prefix_at(d.doff, pwave, v, buf, s_t4, s_svp);
      const uint32_t Pe = prefix_at(d.doff + d.dlen, pwave, v, buf, s_t4, s_svp);
      d.computed = gshift_n(g_shift, d.dlen, 0xffffffffu ^ Ps) ^ Pe ^ 0xffffffffu;
    }
    if (d.computed != d.stored) {
      st = EWAL_ERR_SNAP_CRC;
    } else if (a2.split) {
      d.resid = 2;   // raftpb.Snapshot over the concatenation: gathered, then k_snap_resid
    } else {
      PbField s1, s2, s3, s4, s5;
      pbf_init(s1); pbf_init(s2); pbf_init(s3); pbf_init(s4); pbf_init(s5);
      esnap_snapshot *o = snaps + f;
      int ur = 0;
      int st2 = d.dlen ? pb_walk<PB_BYTES, PB_REP64, PB_VAR64, PB_VAR64, PB_REP64>(
                             buf + d.doff, (int64_t)d.dlen, s1, s2, s3, s4, s5, ur, o->nodes, o->removed, 64)
                       : 0;
      // Snapshot.XXX_unrecognized, Data in several segments, more Nodes or
      // RemovedNodes than esnap_snapshot holds: k_snap_resid lists them
      if (st2 == 0 && (ur || s1.split || s2.split || s5.split)) d.resid = 1;
      st = st2;
      o->index = s3.v;
      o->term = s4.v;
      o->data_off = s1.blen > 0 ? d.doff + (uint64_t)s1.boff : d.doff;
      o->data_len = s1.blen > 0 ? (uint64_t)s1.blen : 0;
      o->n_nodes = (int64_t)s2.v;
      o->n_removed = (int64_t)s5.v;
    }
  }
  d.st = st;
  sd[f] = d;
}

// ---- residual snapshot encodings (rare; include/ewal.h esnap_copy_field)
// k_snap_gather: one block per listed file whose envelope Data came in
// several segments: the concatenation Go's append builds, into scratch.
__global__ __launch_bounds__(256) void k_snap_gather(const uint8_t *__restrict__ buf, const SnapDesc *__restrict__ sd,
                                                     const uint32_t *__restrict__ rlist,
                                                     const uint64_t *__restrict__ goff, uint8_t *__restrict__ scratch,
                                                     uint32_t nr) {
  const uint32_t r = blockIdx.x;
  if (r >= nr) return;
  const SnapDesc d = sd[rlist[r]];
  if (d.resid != 2) return;
  uint8_t *dst = scratch + goff[r];
  uint64_t pos = 0;
  // snappb.Snapshot: Crc (1) varint, Data (2) bytes
  pb_each(buf + d.off, (int64_t)d.len, 2, 0x2u, 0x4u, [&](bool b, uint64_t o, uint64_t n) {
    if (!b) return;
    const uint8_t *src = buf + d.off + o;
    for (uint64_t j = threadIdx.x; j < n; j += blockDim.x) dst[pos + j] = src[j];
    pos += n;
  });
}

// k_snap_resid: one lane per listed file, raftpb.Snapshot Unmarshal over
// the file's Data (or its gathered concatenation): the FILL pass writes the
// status, esnap_snapshot's fields and the file's segments (emsg_segment:
// offsets into d_buf, or into scratch for a gathered file); the count pass
// only counts the segments.
template <bool FILL>
__global__ __launch_bounds__(256) void k_snap_resid(const uint8_t *__restrict__ buf, const uint8_t *__restrict__ scratch,
                                                    SnapDesc *__restrict__ sd, const uint32_t *__restrict__ rlist,
                                                    const uint64_t *__restrict__ goff, uint32_t nr,
                                                    uint64_t *__restrict__ cnt, const uint64_t *__restrict__ first,
                                                    emsg_segment *__restrict__ segs,
                                                    esnap_snapshot *__restrict__ snaps) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nr) return;
  const uint32_t f = rlist[r];
  SnapDesc d = sd[f];
  const bool gathered = d.resid == 2;
  const uint64_t base = gathered ? goff[r] : d.doff;
  const uint8_t *p = (gathered ? scratch : buf) + base;
  const int64_t l = (int64_t)d.dlen;
  uint64_t ns = 0;
  auto emit = [&](int32_t kind, uint64_t off, uint64_t len) {
    if (FILL) {
      emsg_segment g;
      g.kind = kind;
      g.pad = gathered ? 1 : 0;
      g.ent = -1;
      g.off = off;
      g.len = len;
      segs[first[r] + ns] = g;
    }
    ++ns;
  };
  PbField s1, s2, s3, s4, s5;
  pbf_init(s1); pbf_init(s2); pbf_init(s3); pbf_init(s4); pbf_init(s5);
  esnap_snapshot *o = snaps + f;
  int ur = 0;
  const int st = pb_walk<PB_BYTES, PB_REP64, PB_VAR64, PB_VAR64, PB_REP64>(
      p, l, s1, s2, s3, s4, s5, ur, FILL ? o->nodes : nullptr, FILL ? o->removed : nullptr, 64,
      [&](int64_t u0, int64_t u1) { emit(EMSG_SEG_SNAP_UNREC, base + (uint64_t)u0, (uint64_t)(u1 - u0)); });
  pb_each(p, l, 1, 0x3cu, 0x2u, [&](bool b, uint64_t o2, uint64_t n) {
    if (b) emit(EMSG_SEG_SNAP_DATA, base + o2, n);
  });
  if (s2.split) pb_each(p, l, 2, 0x3cu, 0x2u, [&](bool b, uint64_t v, uint64_t) {
    if (!b) emit(EMSG_SEG_SNAP_NODE, v, 0);
  });
  if (s5.split) pb_each(p, l, 5, 0x3cu, 0x2u, [&](bool b, uint64_t v, uint64_t) {
    if (!b) emit(EMSG_SEG_SNAP_REMOVED, v, 0);
  });
  if (!FILL) {
    cnt[r] = ns;
    return;
  }
  o->index = s3.v;
  o->term = s4.v;
  // one contiguous range of the file, else ~0: esnap_copy_field assembles it
  o->data_off = (gathered || s1.split) ? ~0ull : (s1.blen > 0 ? d.doff + (uint64_t)s1.boff : d.doff);
  o->data_len = s1.blen > 0 ? (uint64_t)s1.blen : 0;
  o->n_nodes = (int64_t)s2.v;
  o->n_removed = (int64_t)s5.v;
  d.st = st;
  sd[f] = d;
}

// q-th largest of n <= 16 voters by rank counting (ties handled as Go's sort
// would place them: the value at sorted-descending position q-1).
// q-th largest of the n <= N match indexes of group g (any correct sort of
// raft.go:252's mis gives the same order statistic): rank-select over N
// register slots, so a wave of 5/7-voter groups compares 8 x 8, not 16 x 16.
template <int N>
__device__ __forceinline__ uint64_t quorum_select(const uint64_t *__restrict__ match, uint64_t G, uint64_t g, int n) {
  uint64_t m[N];
#pragma unroll
  for (int v = 0; v < N; ++v) m[v] = v < n ? match[(uint64_t)v * G + g] : 0ull;
  const int q = n / 2 + 1;
  uint64_t mci = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    int gt = 0, ge = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      gt += (j < n && m[j] > m[i]);
      ge += (j < n && m[j] >= m[i]);
    }
    if (i < n && gt < q && q <= ge) mci = m[i];
  }
  return mci;
}

// Any voter count (nvoters is a uint8): rank-select straight from memory
// (more than 16 voters is rare; the register forms above cover 5 / 7).
__device__ __noinline__ uint64_t quorum_select_any(const uint64_t *__restrict__ match, uint64_t G, uint64_t g, int n) {
  const int q = n / 2 + 1;
  for (int i = 0; i < n; ++i) {
    const uint64_t mi = match[(uint64_t)i * G + g];
    int gt = 0, ge = 0;
    for (int j = 0; j < n; ++j) {
      const uint64_t mj = match[(uint64_t)j * G + g];
      gt += mj > mi;
      ge += mj >= mi;
    }
    if (gt < q && q <= ge) return mi;
  }
  return 0;
}

// One lane per raft group, EW_COMMIT_ILP groups per lane (g, g + T, ...): the
// loads that do not depend on the voter count (committed, term, the log
// window bounds) are issued for every group of the lane before the first
// match load, so a wave keeps 4x the independent requests in flight (the
// kernel is a chain nvoters -> match -> select -> term gather -> store).
#ifndef EW_COMMIT_ILP
#define EW_COMMIT_ILP 4
#endif
__global__ __launch_bounds__(256) void k_commit(uint64_t G, const uint64_t *__restrict__ match,
                                                const uint8_t *__restrict__ nvoters, const uint64_t *__restrict__ term,
                                                uint64_t *__restrict__ committed,
                                                const uint64_t *__restrict__ log_offset,
                                                const uint64_t *__restrict__ log_ptr,
                                                const uint64_t *__restrict__ log_terms, uint8_t *__restrict__ changed,
                                                uint8_t *__restrict__ status) {
  const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t g0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int n[EW_COMMIT_ILP];
  uint64_t c[EW_COMMIT_ILP], tm[EW_COMMIT_ILP], off[EW_COMMIT_ILP], p0[EW_COMMIT_ILP], p1[EW_COMMIT_ILP];
#pragma unroll
  for (int k = 0; k < EW_COMMIT_ILP; ++k) {
    const uint64_t g = g0 + (uint64_t)k * T;
    const bool in = g < G;
    n[k] = in ? nvoters[g] : 0;
    c[k] = in ? committed[g] : 0;
    tm[k] = in ? term[g] : 0;
    off[k] = in ? log_offset[g] : 0;
    p0[k] = in ? log_ptr[g] : 0;
    p1[k] = in ? log_ptr[g + 1] : 0;
  }
#pragma unroll
  for (int k = 0; k < EW_COMMIT_ILP; ++k) {
    const uint64_t g = g0 + (uint64_t)k * T;
    if (g >= G) break;
    const int nv = n[k];
    uint8_t chg = 0, st = 0;
    if (nv <= 0) {
      st = EWAL_PANIC_BOUNDS;   // mis[q-1] on an empty slice (raft/raft.go:255)
    } else {
      const uint64_t mci = nv <= 8 ? quorum_select<8>(match, G, g, nv)
                           : nv <= 16 ? quorum_select<16>(match, G, g, nv) : quorum_select_any(match, G, g, nv);
      if (mci > c[k]) {   // raftLog.maybeCommit: term(mci) == Term (raft/log.go:148-154)
        const uint64_t nlog = p1[k] - p0[k];
        const uint64_t last = nlog - 1 + off[k];    // lastIndex(), uint64 wrap
        uint64_t t = 0;
        bool panic = false;
        if (!(mci < off[k] || mci > last)) {        // raftLog.at / isOutOfBounds (raft/log.go:194-217)
          const uint64_t kk = mci - off[k];
          if (kk >= nlog) panic = true; else t = log_terms[p0[k] + kk];
        }
        if (panic) {
          st = EWAL_PANIC_BOUNDS;
        } else if (t == tm[k]) {
          committed[g] = mci;
          chg = 1;
        }
      }
    }
    changed[g] = chg;
    status[g] = st;
  }
}

// The same over one 192-B record per group (ecommit_group: up to 7 voters'
// Match, committed, Term, the log bounds and the terms of the log's last 13
// entries), read with coalesced loads, instead of 7 strided match words and
// a term gather that fetches a whole 128-B line for 8 bytes.  The quorum
// index's term comes from the record's tail window when it is one of the
// last 13 entries (the usual case: the uncommitted tail of a raft log is a
// few appends deep), else from the log_terms gather as in k_commit.
__global__ __launch_bounds__(64) void k_commit_rec(uint64_t G, const ecommit_group *__restrict__ rec,
                                                   const uint64_t *__restrict__ log_ptr,
                                                   const uint64_t *__restrict__ log_terms,
                                                   uint64_t *__restrict__ committed_out,
                                                   uint8_t *__restrict__ changed, uint8_t *__restrict__ status) {
  // one wave per workgroup, persistent over chunks of 64 records (12 KiB):
  // a chunk is read with fully coalesced 16-B loads (a lane reading its own
  // 192-B record directly would touch 64 lines per load instruction) while
  // the previous one is selected from LDS
  typedef uint32_t v4u __attribute__((ext_vector_type(4)));
  __shared__ v4u s_rec[64 * 12];
  const uint32_t lane = threadIdx.x;
  const uint64_t nchunk = (G + 63) / 64;
  auto load = [&](uint64_t ch, v4u (&x)[12]) {
    const uint64_t g0 = ch * 64;
    const uint64_t n12 = (G - g0 < 64 ? G - g0 : 64) * 12;
    const v4u *src = (const v4u *)(rec + g0);
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const uint32_t i = (uint32_t)k * 64 + lane;
      x[k] = (ch < nchunk && i < n12) ? __builtin_nontemporal_load(src + i) : v4u{0, 0, 0, 0};   // read once
    }
  };
  v4u cur[12], nxt[12];
  uint64_t ch = blockIdx.x;
  load(ch, cur);
  for (; ch < nchunk; ch += gridDim.x) {
    load(ch + gridDim.x, nxt);
#pragma unroll
    for (int k = 0; k < 12; ++k) s_rec[k * 64 + lane] = cur[k];
    __syncthreads();
    const uint64_t g = ch * 64 + lane;
    if (g < G) {
      const uint64_t *w = (const uint64_t *)(s_rec + lane * 12);   // the record's 8-byte words
      const uint64_t c = w[7], tm = w[8], off = w[9], w10 = w[10];
      const uint64_t nlog = (uint32_t)w10;
      const int nv = (int)((w10 >> 32) & 0xff);
      uint8_t chg = 0, st = 0;
      uint64_t cn = c;
      if (nv <= 0) {
        st = EWAL_PANIC_BOUNDS;   // mis[q-1] on an empty slice (raft/raft.go:255)
      } else if (nv > 7) {
        st = EWAL_UNSUPPORTED_ENCODING;   // more voters than a record holds: ecommit_batch_device
      } else {
        uint64_t m[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) m[v] = v < 7 ? w[v] : 0ull;
        const int qn = nv / 2 + 1;
        uint64_t mci = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {   // rank-select: the qn-th largest (quorum_select's rule)
          int gt = 0, ge = 0;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            gt += (j < nv && m[j] > m[i]);
            ge += (j < nv && m[j] >= m[i]);
          }
          if (i < nv && gt < qn && qn <= ge) mci = m[i];
        }
        if (mci > c) {   // raftLog.maybeCommit: term(mci) == Term (raft/log.go:148-154)
          const uint64_t last = nlog - 1 + off;   // lastIndex(), uint64 wrap
          uint64_t t = 0;
          bool panic = false;
          if (!(mci < off || mci > last)) {       // raftLog.at / isOutOfBounds (raft/log.go:194-217)
            const uint64_t kk = mci - off;
            if (kk >= nlog) {
              panic = true;
            } else if (nlog - 1 - kk < 13) {
              t = w[11 + (nlog - 1 - kk)];
            } else if (log_ptr && log_terms) {
              t = log_terms[log_ptr[g] + kk];
            } else {
              st = EWAL_UNSUPPORTED_ENCODING;    // the term lies before the tail window and no log was given
            }
          }
          if (panic) {
            st = EWAL_PANIC_BOUNDS;
          } else if (!st && t == tm) {
            cn = mci;
            chg = 1;
          }
        }
      }
      committed_out[g] = cn;
      changed[g] = chg;
      status[g] = st;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 12; ++k) cur[k] = nxt[k];
  }
}

// ===========================================================================
// Batched WAL writes, one pipeline for both entry points: SaveEntry over an
// ewal_entry[] (ewal_encode_entries_device; wal/wal.go:248-263) and Save
// (SaveState + SaveEntry, wal/wal.go:248-279) + Cut (wal/wal.go:219-238: a
// crcType record carrying the running CRC, then the metadata record) over an
// ewal_save_rec[] (ewal_save_device), as ONE chained call.  frame = int64 LE
// len || walpb.Record{Type, Crc, Data} (wal/encoder.go:25-37); every header
// byte comes from ewal_wire.h.  Every record contributes one contiguous chunk
// to the "data-only" stream (Entry / HardState marshal, the Cut's metadata
// bytes; a crcType record adds nothing: Data is nil; frame headers are not in
// it), so ONE stream pass gives every chained CRC:
//   crc after the chunk ending at x = ~(P'(x) ^ (x < 4 ? R0 >> 8x : 0)),
// P' over the stream whose first min(4, E) bytes are XORed with R0 = ~prev
// (a reflected register started at R0 over k < 4 bytes equals one started at
// 0 over the XORed bytes, then XORed with R0 >> 8k).
//
// The kernels are templates over the record layout R and read it through
// wr_view: for R = ewal_entry the kind is a constant, so the HardState and
// Cut branches and pcrc fold away.
// ===========================================================================
using ewal_wire::entry_head;
using ewal_wire::entry_size;
using ewal_wire::frame_head;
using ewal_wire::frame_size;
using ewal_wire::sov;
using ewal_wire::state_marshal;

struct WrRec {
  int32_t kind, etype;
  uint64_t a, b, c, data_off, data_len;
  bool data_nil;
};
// Entry.Marshal always writes 22 v(len): a nil Data encodes as an empty one
__device__ __forceinline__ WrRec wr_view(const ewal_entry &e) {
  return WrRec{EWAL_SAVE_ENTRY, e.type, e.term, e.index, 0, e.data_off, e.data_len, false};
}
__device__ __forceinline__ WrRec wr_view(const ewal_save_rec &r) {
  return WrRec{r.kind, r.etype, r.a, r.b, r.c, r.data_off, r.data_len, r.data_nil != 0};
}

// the first hl <= N bytes of h -> dst, one byte a lane.  h lives in the lane's scratch (the varints index it at
// run time), so the lane reads its byte there: a select over N registers instead keeps N lane masks in SGPRs
// across the record loop and costs the kernel a wave of occupancy.
template <int N>
__device__ __forceinline__ void wave_put(uint8_t *__restrict__ dst, const uint8_t (&h)[N], uint32_t hl) {
  static_assert(N <= 64, "one byte a lane");
  const int lane = threadIdx.x & 63;
  if ((uint32_t)lane < hl) dst[lane] = h[lane];
}

// Wave-cooperative copy of n bytes src -> dst (any alignment): byte stores for
// the unaligned head and tail of dst, dword stores in between (two aligned
// source dwords and v_alignbyte per output dword).  Source reads stay inside
// [src_base, src_base + src_len).
__device__ __forceinline__ void wave_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint64_t n,
                                          const uint8_t *src_base, uint64_t src_len) {
  const int lane = threadIdx.x & 63;
  const uint64_t head = std::min<uint64_t>(n, (4 - ((uintptr_t)dst & 3)) & 3);
  if ((uint64_t)lane < head) dst[lane] = src[lane];
  const uint64_t m = (n - head) >> 2;                     // whole output dwords
  uint32_t *d32 = (uint32_t *)(dst + head);
  const uint8_t *s = src + head;
  const uintptr_t send = (uintptr_t)(src_base + src_len);
  for (uint64_t k = lane; k < m; k += 64) {
    const uint8_t *p = s + 4 * k;
    const uintptr_t a = (uintptr_t)p & ~(uintptr_t)3;
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3);
    uint32_t w;
    if (sh == 0) {
      w = *(const uint32_t *)a;
    } else if (a + 8 <= send) {
      w = __builtin_amdgcn_alignbyte(((const uint32_t *)a)[1], ((const uint32_t *)a)[0], sh);
    } else {
      w = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    }
    d32[k] = w;
  }
  const uint64_t t0 = head + 4 * m;
  if ((uint64_t)lane < n - t0) dst[t0 + lane] = src[t0 + lane];
}

// esz[i] = chunk size of record i (0: no chunk -- an empty HardState writes
// nothing, raft.IsEmptyHardState, wal/wal.go:266-268); errflag: a payload
// outside d_data (entries and non-nil Cut metadata only) or an unknown kind
template <typename R>
__global__ void k_wr_sizes(const R *__restrict__ recs, uint64_t n, uint64_t data_len, uint64_t *__restrict__ esz,
                           uint32_t *__restrict__ errflag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const WrRec r = wr_view(recs[i]);
  uint64_t z = 0;
  const bool hasd = r.kind == EWAL_SAVE_ENTRY || (r.kind == EWAL_SAVE_CUT && !r.data_nil);
  if (hasd && (r.data_len > data_len || r.data_off > data_len - r.data_len)) atomicOr(errflag, 1u);
  if (r.kind == EWAL_SAVE_ENTRY) {
    z = entry_size(r.etype, r.a, r.b, r.data_len);
  } else if (r.kind == EWAL_SAVE_STATE) {
    if (r.a | r.b | r.c) z = 3 + sov(r.a) + sov(r.b) + sov(r.c);
  } else if (r.kind == EWAL_SAVE_CUT) {
    z = r.data_nil ? 0 : r.data_len;
  } else {
    atomicOr(errflag, 1u);
  }
  esz[i] = z;
}

// chunk i at xoff[i] of the data-only stream; one wave per record (grid-stride)
template <typename R>
__global__ __launch_bounds__(256) void k_wr_body(const uint8_t *__restrict__ data, uint64_t data_len,
                                                 const R *__restrict__ recs, uint64_t n,
                                                 const uint64_t *__restrict__ xoff, uint8_t *__restrict__ es) {
  const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t i = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n; i += nw) {
    const WrRec r = wr_view(recs[i]);
    uint8_t h[48];
    uint32_t hl = 0;
    uint64_t dl = 0;
    if (r.kind == EWAL_SAVE_ENTRY) {
      hl = (uint32_t)(entry_head(h, r.etype, r.a, r.b, r.data_len) - h);
      dl = r.data_len;
    } else if (r.kind == EWAL_SAVE_STATE) {
      if (r.a | r.b | r.c) hl = (uint32_t)state_marshal(h, r.a, r.b, r.c);
    } else if (r.kind == EWAL_SAVE_CUT && !r.data_nil) {
      dl = r.data_len;
    }
    uint8_t *o = es + xoff[i];
    wave_put(o, h, hl);
    if (dl) wave_copy(o + hl, data + r.data_off, dl, data, data_len);
  }
}

// XOR the stream's first min(4, E) bytes with r (and back)
__global__ void k_wr_xor4(uint8_t *es, uint64_t E, uint32_t r) {
  if (threadIdx.x < 4 && threadIdx.x < E) es[threadIdx.x] ^= (uint8_t)(r >> (8 * threadIdx.x));
}

__device__ __forceinline__ uint32_t wr_crc_at(uint64_t x, uint32_t R0, uint64_t E, const uint32_t *pwave,
                                              const uint32_t *v, const uint8_t *es, const uint32_t *t4,
                                              const uint32_t *svp) {
  const uint32_t p = (E && x) ? prefix_at(x, pwave, v, es, t4, svp) : 0u;
  return ~(p ^ (x < 4 ? (R0 >> (8 * x)) : 0u));
}

// crc[i] = the running CRC after record i's chunk (its Record.Crc), pcrc[i]
// = before it (a Cut's crcType record); fsz[i] = bytes of record i's frames
template <typename R>
__global__ __launch_bounds__(256) void k_wr_crc(const uint8_t *__restrict__ es, uint64_t E, const R *__restrict__ recs,
                                                const uint64_t *__restrict__ xoff, const uint64_t *__restrict__ esz,
                                                uint64_t n, uint32_t R0, const uint32_t *__restrict__ pwave,
                                                const uint32_t *__restrict__ v, const uint32_t *__restrict__ g_slice,
                                                const uint32_t *__restrict__ g_shift, uint32_t *__restrict__ crc,
                                                uint32_t *__restrict__ pcrc, uint64_t *__restrict__ fsz) {
  __shared__ uint32_t s_t4[1024];
  __shared__ uint32_t s_svp[1024];
  stage_lds<256>(s_t4, 1024, [&](int i) { return g_slice[i]; });
  stage_lds<256>(s_svp, 1024, [&](int i) { return g_shift[EW_VLOG * 1024 + i]; });
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const WrRec r = wr_view(recs[i]);
  const uint64_t L = esz[i];
  const uint32_t c = wr_crc_at(xoff[i] + L, R0, E, pwave, v, es, s_t4, s_svp);
  crc[i] = c;
  uint64_t f = 0;
  if (r.kind == EWAL_SAVE_ENTRY || (r.kind == EWAL_SAVE_STATE && L)) {
    f = frame_size(r.kind == EWAL_SAVE_ENTRY ? 2 : 3, c, L, false);   // entryType, stateType
  } else if (r.kind == EWAL_SAVE_CUT) {
    const uint32_t c0 = wr_crc_at(xoff[i], R0, E, pwave, v, es, s_t4, s_svp);
    pcrc[i] = c0;
    f = frame_size(4, c0, 0, true) + frame_size(1, c, L, r.data_nil);   // crcType (Data nil), metadataType
  }
  fsz[i] = f;
}

// one frame (frame_head, then the L chunk bytes unless nil) at dst; one wave
__device__ __forceinline__ void wr_frame(uint8_t *dst, int32_t t, uint32_t c, bool nil, const uint8_t *chunk, uint64_t L,
                                         const uint8_t *es, uint64_t es_len) {
  uint8_t h[32];
  const uint32_t hl = frame_head(h, t, c, L, nil);
  wave_put(dst, h, hl);
  // no branch around the copy (0 bytes copy nothing): a chunk address loaded for a copy that is then skipped
  // stays in flight, and the record loop's next trip would start by waiting for it and for this trip's stores
  wave_copy(dst + hl, chunk, nil ? 0 : L, es, es_len);
}

// record i's frames at foff[i]; one wave per record (grid-stride)
template <typename R>
__global__ __launch_bounds__(256) void k_wr_frame(const uint8_t *__restrict__ es, uint64_t es_len,
                                                  const R *__restrict__ recs, const uint64_t *__restrict__ xoff,
                                                  const uint64_t *__restrict__ esz, const uint32_t *__restrict__ crc,
                                                  const uint32_t *__restrict__ pcrc, const uint64_t *__restrict__ foff,
                                                  uint64_t n, uint8_t *__restrict__ out) {
  const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t i = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n; i += nw) {
    const WrRec r = wr_view(recs[i]);
    const uint64_t L = esz[i];
    uint8_t *dst = out + foff[i];
    // | and &, not || and &&: L is read on every path, so its load is never left in flight either
    if ((r.kind == EWAL_SAVE_ENTRY) | ((r.kind == EWAL_SAVE_STATE) & (L != 0))) {
      wr_frame(dst, r.kind == EWAL_SAVE_ENTRY ? 2 : 3, crc[i], false, es + xoff[i], L, es, es_len);
    } else if (r.kind == EWAL_SAVE_CUT) {
      const uint32_t c0 = pcrc[i];
      wr_frame(dst, 4, c0, true, es, 0, es, es_len);
      wr_frame(dst + frame_size(4, c0, 0, true), 1, crc[i], r.data_nil, es + xoff[i], L, es, es_len);
    }
  }
}
