// Host check of the one wire encoder (etcd_amd/csrc/ewal_wire.h) that the host
// writers and the device write / Message / snapshot kernels share: the closed
// form of sov against the shift loop, and entry_head / frame_head against
// entry_marshal / frame_write and against bytes spelled out here with a loop
// varint.  Exit 0 and "ok" when every case holds.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ewal_wire.h"

using namespace ewal_wire;

static long bad = 0;
#define CHECK(c) do { if (!(c)) { if (!bad++) std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

static uint32_t sov_loop(uint64_t x) { uint32_t n = 0; do { n++; x >>= 7; } while (x); return n; }
static void ref_varint(std::vector<uint8_t> &o, uint64_t v) {
  for (; v >= 0x80; v >>= 7) o.push_back((uint8_t)(v | 0x80));
  o.push_back((uint8_t)v);
}
static void ref_field(std::vector<uint8_t> &o, uint8_t tag, uint64_t v) { o.push_back(tag); ref_varint(o, v); }

int main() {
  // sov and put_varint at the varint width boundaries
  std::vector<uint64_t> vals = {0, 1, ~0ull};
  for (int k = 1; k <= 9; k++)
    for (int d = -1; d <= 1; d++) vals.push_back((1ull << (7 * k)) + (uint64_t)(int64_t)d);
  for (uint64_t v : vals) {
    CHECK(sov(v) == sov_loop(v));
    std::vector<uint8_t> want;
    ref_varint(want, v);
    uint8_t got[12];
    std::memset(got, 0xA5, sizeof got);
    CHECK(put_varint(got, v) == got + want.size() && want.size() == sov(v));
    CHECK(!std::memcmp(got, want.data(), want.size()) && got[want.size()] == 0xA5);
  }
  CHECK(sov((1ull << 63) - 1) == 9 && sov(1ull << 63) == 10 && sov(~0ull) == 10);

  // entry_head + payload == entry_marshal; a negative Type is a 10-byte varint
  const int32_t types[] = {0, 1, -1, INT32_MIN, INT32_MAX};
  const uint64_t lens[] = {0, 1, 127, 128, 16383, 16384};
  std::vector<uint8_t> pay(16384);
  for (size_t i = 0; i < pay.size(); i++) pay[i] = (uint8_t)(i * 131 + 7);
  for (int32_t t : types)
    for (uint64_t term : vals)
      for (uint64_t n : lens) {
        const uint64_t index = ~term;
        std::vector<uint8_t> want;
        ref_field(want, 0x08, (uint64_t)(int64_t)t);
        ref_field(want, 0x10, term);
        ref_field(want, 0x18, index);
        ref_field(want, 0x22, n);
        const size_t hl = want.size();
        want.insert(want.end(), pay.begin(), pay.begin() + n);
        CHECK(entry_size(t, term, index, n) == want.size());
        if (t < 0) CHECK(want[0] == 0x08 && want[11] == 0x10 && sov((uint64_t)(int64_t)t) == 10);
        std::vector<uint8_t> a(want.size() + 1, 0xA5), b(hl + 1, 0xA5);
        CHECK(entry_marshal(a.data(), t, term, index, pay.data(), n) == a.data() + want.size());
        CHECK(entry_head(b.data(), t, term, index, n) == b.data() + hl);
        CHECK(!std::memcmp(a.data(), want.data(), want.size()) && a[want.size()] == 0xA5);
        CHECK(!std::memcmp(b.data(), want.data(), hl) && b[hl] == 0xA5);
      }

  // HardState
  for (uint64_t v : vals) {
    std::vector<uint8_t> want;
    ref_field(want, 0x08, v);
    ref_field(want, 0x10, ~v);
    ref_field(want, 0x18, v >> 1);
    uint8_t got[40];
    CHECK(state_marshal(got, v, ~v, v >> 1) == want.size() && !std::memcmp(got, want.data(), want.size()));
  }

  // frame_head == the prefix of frame_write
  const uint32_t crcs[] = {0, 0x7f, 0x80, 0x3fff, 0x4000, 0xffffffffu};
  for (int64_t t = 1; t <= 4; t++)
    for (uint32_t c : crcs)
      for (int nil = 0; nil <= 1; nil++)
        for (uint64_t n : lens) {
          std::vector<uint8_t> rec;
          ref_field(rec, 0x08, (uint64_t)t);
          ref_field(rec, 0x10, c);
          if (!nil) ref_field(rec, 0x1a, n);
          const uint64_t L = rec.size() + (nil ? 0 : n);
          std::vector<uint8_t> want(8);
          for (int k = 0; k < 8; k++) want[k] = (uint8_t)(L >> (8 * k));
          want.insert(want.end(), rec.begin(), rec.end());
          const size_t hl = want.size();
          if (!nil) want.insert(want.end(), pay.begin(), pay.begin() + n);
          CHECK(frame_size(t, c, n, nil) == want.size());
          std::vector<uint8_t> a(want.size() + 1, 0xA5), b(hl + 1, 0xA5);
          CHECK(frame_write(a.data(), t, c, pay.data(), n, nil) == a.data() + want.size());
          CHECK(frame_head(b.data(), t, c, n, nil) == hl);
          CHECK(!std::memcmp(a.data(), want.data(), want.size()) && a[want.size()] == 0xA5);
          CHECK(!std::memcmp(b.data(), a.data(), hl) && b[hl] == 0xA5);
        }
  if (bad) {
    std::fprintf(stderr, "%ld checks failed\n", bad);
    return 1;
  }
  std::puts("ok");
  return 0;
}
