// ewal_wire.h -- the protobuf MarshalTo forms of etcd's generated code that
// the writers need (walpb.Record, raftpb.Entry / HardState), shared by the
// engine's host writer (ewal_host.cpp), its device write / Message / snapshot
// kernels (aux_kernels.hip, msg_encode.hip, snap_save.hip) and the
// synthetic-WAL generator (ewal_synth.cpp, bench / test plumbing).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

// The forms below marked EWAL_HD are the one encoder of host and device code:
// the write, Message and snapshot kernels call them as the host writers do.
#ifdef __HIPCC__
#define EWAL_HD __host__ __device__
#else
#define EWAL_HD
#endif

namespace ewal_wire {

// bytes of v's varint: ceil(bits(v | 1) / 7)
EWAL_HD inline uint32_t sov(uint64_t x) { return (70u - (uint32_t)__builtin_clzll(x | 1)) / 7u; }
EWAL_HD inline uint8_t *put_varint(uint8_t *o, uint64_t v) {
  while (v >= 0x80) { *o++ = (uint8_t)(v | 0x80); v >>= 7; }
  *o++ = (uint8_t)v;
  return o;
}
// raftpb.Entry.MarshalTo, raft/raftpb/raft.pb.go:921-943: the head
// 08 v(type) 10 v(term) 18 v(index) 22 v(n) (<= 44 bytes), then the n Data bytes
EWAL_HD inline uint64_t entry_size(int32_t type, uint64_t term, uint64_t index, uint64_t n) {
  return 4 + sov((uint64_t)(int64_t)type) + sov(term) + sov(index) + sov(n) + n;
}
EWAL_HD inline uint8_t *entry_head(uint8_t *o, int32_t type, uint64_t term, uint64_t index, uint64_t n) {
  *o++ = 0x08; o = put_varint(o, (uint64_t)(int64_t)type);
  *o++ = 0x10; o = put_varint(o, term);
  *o++ = 0x18; o = put_varint(o, index);
  *o++ = 0x22; o = put_varint(o, n);
  return o;
}
inline uint8_t *entry_marshal(uint8_t *o, int32_t type, uint64_t term, uint64_t index, const uint8_t *d, uint64_t n) {
  o = entry_head(o, type, term, index, n);
  if (n) std::memcpy(o, d, n);
  return o + n;
}
// raftpb.HardState.MarshalTo, raft.pb.go:1079-1097 (<= 33 bytes)
EWAL_HD inline size_t state_marshal(uint8_t *o, uint64_t term, uint64_t vote, uint64_t commit) {
  uint8_t *s = o;
  *o++ = 0x08; o = put_varint(o, term);
  *o++ = 0x10; o = put_varint(o, vote);
  *o++ = 0x18; o = put_varint(o, commit);
  return (size_t)(o - s);
}
// walpb.Record.MarshalTo, wal/walpb/record.pb.go:175-196, prefixed by the
// int64 LE length (wal/encoder.go:32-35).  frame_head writes everything in
// front of Data -- the length, 08 v(type) 10 v(crc) and, for a non-nil Data of
// n bytes, 1a v(n) -- and returns its length (<= 31 bytes).
EWAL_HD inline size_t frame_size(int64_t type, uint32_t crc, uint64_t n, bool nil) {
  size_t r = 1 + sov((uint64_t)type) + 1 + sov(crc);
  if (!nil) r += 1 + sov(n) + n;
  return 8 + r;
}
EWAL_HD inline uint32_t frame_head(uint8_t *o, int64_t type, uint32_t crc, uint64_t n, bool nil) {
  uint8_t *p = o + 8;
  *p++ = 0x08; p = put_varint(p, (uint64_t)type);
  *p++ = 0x10; p = put_varint(p, crc);
  if (!nil) { *p++ = 0x1a; p = put_varint(p, n); }
  const uint32_t hl = (uint32_t)(p - o);
  const uint64_t L = (uint64_t)(hl - 8) + (nil ? 0 : n);
  for (int k = 0; k < 8; ++k) o[k] = (uint8_t)(L >> (8 * k));
  return hl;
}
inline uint8_t *frame_write(uint8_t *o, int64_t type, uint32_t crc, const uint8_t *d, uint64_t n, bool nil) {
  o += frame_head(o, type, crc, n, nil);
  if (!nil) {
    if (n) std::memcpy(o, d, n);
    o += n;
  }
  return o;
}

// raftpb.Snapshot.MarshalTo, raft/raftpb/raft.pb.go:954-999, around Data: the
// head `0a v(len(Data))` (always written: nil and empty Data encode alike) and
// the trailer {10 v(node)}* 18 v(Index) 20 v(Term) {28 v(removed)}*
// XXX_unrecognized.
inline size_t snap_head_size(uint64_t dlen) { return 1 + sov(dlen); }
inline size_t snap_trailer_size(const uint64_t *nodes, uint64_t n_nodes, uint64_t index, uint64_t term,
                                const uint64_t *removed, uint64_t n_removed, uint64_t unrec_len) {
  size_t r = 1 + sov(index) + 1 + sov(term) + unrec_len;
  for (uint64_t k = 0; k < n_nodes; ++k) r += 1 + sov(nodes[k]);
  for (uint64_t k = 0; k < n_removed; ++k) r += 1 + sov(removed[k]);
  return r;
}
inline uint8_t *snap_trailer_marshal(uint8_t *o, const uint64_t *nodes, uint64_t n_nodes, uint64_t index,
                                     uint64_t term, const uint64_t *removed, uint64_t n_removed,
                                     const uint8_t *unrec, uint64_t unrec_len) {
  for (uint64_t k = 0; k < n_nodes; ++k) { *o++ = 0x10; o = put_varint(o, nodes[k]); }
  *o++ = 0x18; o = put_varint(o, index);
  *o++ = 0x20; o = put_varint(o, term);
  for (uint64_t k = 0; k < n_removed; ++k) { *o++ = 0x28; o = put_varint(o, removed[k]); }
  if (unrec_len) std::memcpy(o, unrec, unrec_len);
  return o + unrec_len;
}
// snappb.Snapshot{Crc, Data}.MarshalTo, snap/snappb/snap.pb.go:158-176: the
// envelope header `08 v(crc) 12 v(len(body))`; its longest form (a 5-byte crc)
inline size_t snap_env_max(uint64_t blen) { return 1 + 5 + 1 + sov(blen); }

}  // namespace ewal_wire
