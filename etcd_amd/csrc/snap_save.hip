// snap_save.hip -- Snapshotter.save (snap/snapshotter.go:46-60) for a batch of
// snapshots whose Data is resident in HBM: one fused copy + CRC pass.
//
//   file = 08 v(crc) 12 v(len b) b
//   b    = 0a v(len Data) Data {10 v(node)}* 18 v(Index) 20 v(Term) {28 v(removed)}* XXX_unrecognized
//   crc  = crc32.Update(0, table, b)
//
// The host lays the files out (esnap_save_packed_device) so that every Data's
// destination is congruent to its source mod 16 and cuts the 16-B aligned
// middle of every Data into tiles of ESS_TILE bytes.
//   k_snap_copy    one wave per tile: each 16 B is loaded once, stored once,
//                  and its CRC contribution comes from the registers of that
//                  load; the tile's raw remainder lin(tile) goes to rem[].
//   k_snap_finish  one workgroup per snapshot: the tile remainders combined in
//                  order with the shift operators, the unaligned head / tail
//                  bytes of Data (< 16 each), the host-built body head and
//                  trailer, then the envelope header right-aligned against
//                  the body.
// No atomics; every output byte has exactly one writer.
#include "ewal_device.h"
#include "ewal_internal.h"
#include "ewal_wire.h"

#define ESS_TILE 32768u        // bytes of Data per tile (one wave); 2^ESS_TILE_LOG
#define ESS_TILE_LOG 15
#define ESS_WAVES 12           // waves per k_snap_copy workgroup (3 per SIMD, as k_stream)
#define ESS_THREADS (ESS_WAVES * 64)
#define ESS_FIN_THREADS 256

// One tile: bytes [k ESS_TILE, (k + 1) ESS_TILE) of the 16-B aligned middle of snapshot `file`'s Data.
struct SaveTile {
  uint32_t file, k;
};
// One snapshot.  Data = d_data[src, src + dlen); the body starts at d_out + body.
struct SaveFile {
  uint64_t src, dlen;
  uint64_t body, blen;
  uint64_t tile0;          // its first tile
  uint32_t ntiles;
  uint32_t hlen;           // body head `0a v(dlen)`
  uint64_t meta;           // head then trailer bytes, in the meta blob
  uint64_t tlen;           // trailer bytes
  uint32_t chead;          // raw(~0, head): the register after the body head
  uint32_t ltrail;         // lin(trailer)
};

__device__ __forceinline__ void ss_load(const uint8_t *p, uint32_t (&D)[19]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const ew_v4u w = __builtin_nontemporal_load((const ew_v4u *)(p + 1024 * r));
    D[4 * r] = w.x; D[4 * r + 1] = w.y; D[4 * r + 2] = w.z; D[4 * r + 3] = w.w;
  }
}
__device__ __forceinline__ void ss_store(uint8_t *p, const uint32_t (&D)[19]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    ew_v4u w;
    w.x = D[4 * r]; w.y = D[4 * r + 1]; w.z = D[4 * r + 2]; w.w = D[4 * r + 3];
    __builtin_nontemporal_store(w, (ew_v4u *)(p + 1024 * r));
  }
}

// Persistent workgroups (one per CU: the conflict-free slicing tables take
// 128 KiB of LDS), tiles dealt round-robin over the waves.  A wave walks its
// tile in 8 KiB pairs of 4 KiB units, the next pair's loads in flight while
// this one is stored and summed: unit loads are k_stream's (load r covers unit
// bytes [1024 r, +1024), lane (g, m) takes chunk g of piece 16 r + m), the
// stores put the same registers at the same offsets, and row_transpose() then
// gives lane l the 64 contiguous bytes of piece l for crc_pieces().  Per lane
// acc = S_4096(acc) ^ lin(piece) over the units (Horner); at the tile's end
// the lanes' values are moved to the tile's end and xored across the wave.
// The tile's last bytes (< 4 KiB, a multiple of 16) take the guarded path:
// lane l owns piece l directly.
__global__ __launch_bounds__(ESS_THREADS, 1) void k_snap_copy(const uint8_t *__restrict__ data, uint8_t *__restrict__ out,
                                                              const SaveTile *__restrict__ tiles, uint32_t ntiles,
                                                              const SaveFile *__restrict__ files,
                                                              const uint32_t *__restrict__ g_slice,
                                                              const uint32_t *__restrict__ g_shift,
                                                              uint32_t *__restrict__ rem) {
  __shared__ __attribute__((aligned(16))) uint8_t s_slice[EW_SLICE_DWORDS * 4];
  __shared__ uint32_t s_sh[7 * 1024];   // byte tables of S_64 .. S_4096 (shift levels 6 .. 12)
  const uint32_t *s_s12 = s_sh + 6 * 1024;
  const int tid = threadIdx.x, lane = tid & 63;
  stage_lds<ESS_THREADS>((uint32_t *)s_slice, EW_SLICE_DWORDS, [&](int i) { return g_slice[slice_src(i)]; });
  stage_lds<ESS_THREADS>(s_sh, 7 * 1024, [&](int i) { return g_shift[6 * 1024 + i]; });
  __syncthreads();
  uint32_t Lt[4];
  lane_regs(lane, Lt);
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t lo = (uint32_t)(64 * (lane & 15) + 16 * (lane >> 4));
  for (uint32_t t = blockIdx.x * ESS_WAVES + wv; t < ntiles; t += gridDim.x * ESS_WAVES) {
    const SaveTile tl = tiles[t];
    const SaveFile &f = files[tl.file];
    const uint64_t fsrc = f.src, fdlen = f.dlen;
    const uint64_t ha = std::min<uint64_t>(fdlen, (16u - (uint32_t)(fsrc & 15u)) & 15u);   // Data's unaligned head
    const uint64_t to = ha + (uint64_t)tl.k * ESS_TILE;
    const uint64_t src = fsrc + to, dst = f.body + f.hlen + to;
    const uint32_t nbytes =
        __builtin_amdgcn_readfirstlane((uint32_t)std::min<uint64_t>(ESS_TILE, ((fdlen - ha) & ~15ull) - (uint64_t)tl.k * ESS_TILE));
    const uint32_t nfull = nbytes >> 12, np = nfull >> 1;
    const uint8_t *sp = data + src + lo;
    uint8_t *dp = out + dst + lo;
    uint32_t acc = 0;
    uint32_t DA[2][19], DB[2][19];
    auto load_pair = [&](uint32_t k, uint32_t (&T)[2][19]) {
      ss_load(sp + (size_t)k * 8192, T[0]);
      ss_load(sp + (size_t)k * 8192 + 4096, T[1]);
    };
    auto run_pair = [&](uint32_t k, uint32_t (&T)[2][19]) {
      ss_store(dp + (size_t)k * 8192, T[0]);
      ss_store(dp + (size_t)k * 8192 + 4096, T[1]);
      row_transpose(T[0]);
      row_transpose(T[1]);
      uint32_t c[2];
      crc_pieces<2>(s_slice, Lt, T, c);
      acc = tab_apply(s_s12, tab_apply(s_s12, acc) ^ c[0]) ^ c[1];
    };
    if (np) load_pair(0, DA);
    for (uint32_t k = 0; k < np; k += 2) {
      if (k + 1 < np) load_pair(k + 1, DB);
      __builtin_amdgcn_sched_barrier(0);
      run_pair(k, DA);
      if (k + 1 >= np) break;
      if (k + 2 < np) load_pair(k + 2, DA);
      __builtin_amdgcn_sched_barrier(0);
      run_pair(k + 1, DB);
    }
    if (nfull & 1) {
      uint32_t D1[1][19];
      ss_load(sp + (size_t)np * 8192, D1[0]);
      ss_store(dp + (size_t)np * 8192, D1[0]);
      row_transpose(D1[0]);
      uint32_t c[1];
      crc_pieces<1>(s_slice, Lt, D1, c);
      acc = tab_apply(s_s12, acc) ^ c[0];
    }
    // the tile's last R bytes: piece l = bytes [64 l, 64 l + 16 nch) of them
    const uint32_t R = nbytes & 4095u;
    uint32_t e = 0;
    if (nfull && R == 0) {   // whole units only: the lanes' moves by 64 (63 - l) bytes from the LDS tables
      e = acc;
#pragma unroll
      for (int m = 0; m < 6; ++m)
        if (((63 - lane) >> m) & 1) e = tab_apply(s_sh + m * 1024, e);
    } else if (nfull) {
      e = gshift_n(g_shift, (uint64_t)R + 64u * (63u - (uint32_t)lane), acc);
    }
    if (64u * (uint32_t)lane < R) {
      const uint32_t left = R - 64u * (uint32_t)lane;
      const int nch = left >= 64u ? 4 : (int)(left >> 4);
      const uint8_t *rs = data + src + ((size_t)nfull << 12) + 64 * lane;
      uint8_t *rd = out + dst + ((size_t)nfull << 12) + 64 * lane;
      uint32_t D[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        ew_v4u w = {0u, 0u, 0u, 0u};
        if (q < nch) {
          w = __builtin_nontemporal_load((const ew_v4u *)(rs + 16 * q));
          __builtin_nontemporal_store(w, (ew_v4u *)(rd + 16 * q));
        }
        D[4 * q] = w.x; D[4 * q + 1] = w.y; D[4 * q + 2] = w.z; D[4 * q + 3] = w.w;
      }
      uint32_t x = D[0];
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < 4 * nch) x = perm_step(s_slice, Lt, x, (k + 1 < 4 * nch) ? D[(k + 1) & 15] : 0u);
      e ^= gshift_n(g_shift, (uint64_t)(left - 16u * (uint32_t)nch), x);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) e ^= __shfl_xor(e, m);
    if (lane == 0) rem[t] = e;
  }
}

// One workgroup per snapshot.  With Data = head (a bytes up to the first 16-B
// boundary) | mid (the tiles) | tail (< 16 bytes), the register runs
//   c = chead -> raw over head -> S_mid(c) ^ lin(mid) -> raw over tail -> S_tlen(c) ^ ltrail
// and crc = ~c (Update(0, ...)'s inversions: chead starts from ~0).
__global__ __launch_bounds__(ESS_FIN_THREADS) void k_snap_finish(const uint8_t *__restrict__ data, uint8_t *__restrict__ out,
                                                                 const SaveFile *__restrict__ files,
                                                                 const uint8_t *__restrict__ meta,
                                                                 const uint32_t *__restrict__ rem,
                                                                 const uint32_t *__restrict__ g_slice,
                                                                 const uint32_t *__restrict__ g_shift,
                                                                 esnap_saved *__restrict__ saved) {
  __shared__ uint32_t s_red[ESS_FIN_THREADS / 64];
  const SaveFile f = files[blockIdx.x];
  const uint32_t tid = threadIdx.x;
  const uint64_t a = std::min<uint64_t>(f.dlen, (16u - (uint32_t)(f.src & 15u)) & 15u);
  const uint64_t mid = (f.dlen - a) & ~15ull, tl = f.dlen - a - mid;
  // lin(mid): thread j folds tiles [j per, (j + 1) per) in order, moves the
  // value to mid's end, and the workgroup xors
  const uint32_t per = (f.ntiles + ESS_FIN_THREADS - 1) / ESS_FIN_THREADS;
  const uint32_t t0 = std::min(tid * per, f.ntiles), t1 = std::min(t0 + per, f.ntiles);
  uint32_t acc = 0;
  for (uint32_t t = t0; t < t1; ++t) {
    const uint64_t left = mid - (uint64_t)t * ESS_TILE;
    acc = (left >= ESS_TILE ? gshift_pow2(g_shift, ESS_TILE_LOG, acc) : gshift_n(g_shift, left, acc)) ^ rem[f.tile0 + t];
  }
  if (t0 < t1) acc = gshift_n(g_shift, mid - std::min<uint64_t>((uint64_t)t1 * ESS_TILE, mid), acc);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) acc ^= __shfl_xor(acc, m);
  if ((tid & 63) == 0) s_red[tid >> 6] = acc;
  // the bytes the copy pass does not write: Data's head and tail, the body
  // head, the trailer
  const uint8_t *sd = data + f.src;
  uint8_t *dd = out + f.body + f.hlen;
  if (tid < a) dd[tid] = sd[tid];
  if (tid < tl) dd[a + mid + tid] = sd[a + mid + tid];
  if (tid < f.hlen) out[f.body + tid] = meta[f.meta + tid];
  for (uint64_t k = tid; k < f.tlen; k += ESS_FIN_THREADS) dd[f.dlen + k] = meta[f.meta + f.hlen + k];
  __syncthreads();
  if (tid != 0) return;
  uint32_t linmid = 0;
#pragma unroll
  for (int w = 0; w < ESS_FIN_THREADS / 64; ++w) linmid ^= s_red[w];
  uint32_t c = f.chead;
  for (uint64_t k = 0; k < a; ++k) c = g_slice[(c ^ sd[k]) & 0xff] ^ (c >> 8);
  c = gshift_n(g_shift, mid, c) ^ linmid;
  for (uint64_t k = 0; k < tl; ++k) c = g_slice[(c ^ sd[a + mid + k]) & 0xff] ^ (c >> 8);
  c = gshift_n(g_shift, f.tlen, c) ^ f.ltrail;
  const uint32_t crc = ~c;
  // snappb.Snapshot's header 08 v(crc) 12 v(blen), ending where the body starts
  const uint64_t hl = 2 + ewal_wire::sov(crc) + ewal_wire::sov(f.blen);
  uint8_t *p = out + f.body - hl;
  *p++ = 0x08; p = ewal_wire::put_varint(p, crc);
  *p++ = 0x12; ewal_wire::put_varint(p, f.blen);
  esnap_saved s;
  s.off = f.body - hl;
  s.len = hl + f.blen;
  s.crc = crc;
  s.pad = 0;
  saved[blockIdx.x] = s;
}
