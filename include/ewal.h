/*
 * ewal.h -- C ABI of the MI355X-native etcd WAL replay-and-verify engine.
 *
 * Drop-in boundary for the reference's (mzsanford/etcd v0.5.0-alpha) hot
 * path.  Each entry point names the Go interface it replaces (file:line,
 * relative to the reference root).  A cgo shim binds these
 * with plain pointers and sizes; no HIP or torch types cross the boundary
 * except opaque handles and device pointers given as `const void *`.
 *
 * Ownership: the caller owns every buffer passed in; the library owns its
 * device workspace and stream inside an ewal_ctx.  Threading: one ctx per
 * host thread; calls are blocking.  Errors: a negative return is an
 * infrastructure failure (HIP); a non-negative return is an EWAL_* status
 * that maps 1:1 onto the reference's sentinel errors and panic classes.
 * There is no CPU fallback: without a usable GPU every compute entry point
 * returns EWAL_E_NODEVICE.
 */
#ifndef EWAL_H
#define EWAL_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (same numbering as oracle/ewal_oracle.h) ------------ */
enum {
  EWAL_OK = 0,
  EWAL_EOF = 1,                    /* io.EOF: clean end (internal only) */
  EWAL_ERR_UNEXPECTED_EOF = 2,     /* io.ErrUnexpectedEOF */
  EWAL_ERR_RECORD_CRC = 3,         /* walpb.ErrCRCMismatch   wal/walpb/record.go:22 */
  EWAL_ERR_WAL_CRC = 4,            /* wal.ErrCRCMismatch     wal/wal.go:48 */
  EWAL_ERR_METADATA_CONFLICT = 5,  /* wal.ErrMetadataConflict wal/wal.go:45 */
  EWAL_ERR_INDEX_NOT_FOUND = 6,    /* wal.ErrIndexNotFound   wal/wal.go:47 */
  EWAL_ERR_WRONG_TYPE = 7,         /* proto.ErrWrongType */
  EWAL_ERR_UNEXPECTED_TYPE = 8,    /* "unexpected block type %d" wal/wal.go:194; detail = type */
  EWAL_ERR_FILE_NOT_FOUND = 9,     /* wal.ErrFileNotFound    wal/wal.go:46 */
  EWAL_ERR_SNAP_CRC = 10,          /* snap.ErrCRCMismatch    snap/snapshotter.go:25 */
  EWAL_ERR_NO_SNAPSHOT = 11,       /* snap.ErrNoSnapshot     snap/snapshotter.go:24 */
  EWAL_PANIC_NEG_LENGTH = 32,      /* make([]byte, l<0)      wal/decoder.go:34 */
  EWAL_PANIC_BOUNDS = 33,          /* runtime bounds panic in Unmarshal/Skip */
  EWAL_PANIC_ENTRY = 34,           /* mustUnmarshalEntry     wal/decoder.go:61-69 */
  EWAL_PANIC_STATE = 35,           /* mustUnmarshalState     wal/decoder.go:71-77 */
  EWAL_PANIC_INDEX_GAP = 36,       /* ents[:e.Index-ri] past len wal/wal.go:173 */
  EWAL_NONTERMINATING = 37,        /* the reference never returns */
  EWAL_PANIC_COMMITTED_CONFLICT = 38, /* panic("conflict with committed entry"), raft/log.go:57 */
  EWAL_PANIC_NIL_PROGRESS = 39,    /* r.prs[m.From] is nil and is dereferenced, raft/raft.go:458,462 */
  EWAL_PANIC_NEED_SNAPSHOT = 40,   /* panic("need non-empty snapshot"), raft/raft.go:559 */
  EWAL_PANIC_FIRST_ENTRY = 41,     /* panic("cannot return the first entry in log"), raft/log.go:131 */
  EWAL_PANIC_LEADER_TO_CANDIDATE = 42, /* panic("invalid transition [leader -> candidate]"), raft/raft.go:320 */
  EWAL_PANIC_NIL_ENTRY = 43,       /* at(lastIndex()) is nil and is dereferenced, raft/log.go:137-138 */
  EWAL_PANIC_DOUBLE_CONF = 44,     /* panic("unexpected double uncommitted config entry"), raft/raft.go:344 */
  EWAL_PANIC_COMPACT_APPLIED = 45, /* panic("raft: compact index (%d) exceeds applied index (%d)"), raft/raft.go:523-525 */
  EWAL_PANIC_COMPACT_BOUNDS = 46,  /* panic("compact %d out of bounds [%d:%d]"), raft/log.go:162-164 */
  EWAL_PANIC_CONF_TYPE = 47,       /* panic("unexpected conf type"), raft/node.go:235 */
  EWAL_UNSUPPORTED_ENCODING = 48,  /* protobuf groups nested deeper than the device
                                      walker's stack; reported, never guessed.  An
                                      unknown group may hold groups 16 deep (17
                                      start-group tags nested) and every call is still
                                      exact; with 18 nested, bytes Go accepts get this
                                      status: ReadAll stops at that frame (fail_record /
                                      fail_offset name it, in a batch for that shard
                                      alone), esnap_verify_packed gives it as the file's
                                      status, emsg_decode_batch_device as the message's */
  EWAL_PANIC_NONE_ID = 49,         /* panic("cannot use none id"), raft/raft.go:136-138 */
  /* infrastructure (negative) */
  EWAL_E_HIP = -1,
  EWAL_E_INVAL = -2,
  EWAL_E_NOMEM = -3,
  EWAL_E_NODEVICE = -4,
  EWAL_E_TIMEOUT = -5,
  EWAL_E_IO = -6
};

/* Record types, wal/wal.go:34-39 */
enum { EWAL_METADATA = 1, EWAL_ENTRY = 2, EWAL_STATE = 3, EWAL_CRC = 4 };

typedef struct ewal_ctx ewal_ctx;

/* Result of (*WAL).ReadAll, wal/wal.go:164-216.  On error the reference
 * returns (nil, HardState{}, nil, err): only status/detail/fail_* and
 * n_records are meaningful then. */
typedef struct ewal_result {
  int32_t status;          /* EWAL_OK or an EWAL_ERR_/EWAL_PANIC_ class */
  int32_t flags;
  int64_t detail;          /* unexpected block type value; gap index */
  int64_t fail_record;     /* ordinal of the frame that failed, -1 if none */
  int64_t fail_offset;     /* byte offset of that frame in the stream, -1 */
  int64_t n_records;       /* frames decoded before the end / failure */
  uint32_t last_crc;       /* decoder.lastCRC() -> seeds the encoder, wal/wal.go:213 (set with
                              ErrIndexNotFound too: a split WAL's next range starts from it) */
  uint32_t n_unrec;        /* ents / HardState carrying XXX_unrecognized: ewal_copy_unrec */
  uint64_t enti;           /* w.enti: Index of the last entry record */
  int64_t metadata_off;    /* metadata []byte as (offset,len) into the stream; -1 == nil */
  int64_t metadata_len;
  int32_t has_state;       /* 0 -> HardState{} */
  int32_t n_slow;          /* diagnostics: frames decoded by the general (non-canonical) walker */
  uint64_t state_term, state_vote, state_commit;
  int64_t n_ents;          /* len(ents); fetch with ewal_copy_entries */
  int64_t n_candidates;    /* diagnostics: frame-start candidates found */
  int64_t n_runs;          /* diagnostics: chain runs in the framing pass */
  double device_ms;        /* device time of the pipeline (HIP events) */
  double stream_ms;        /* device time of the k_stream HBM pass alone */
  double post_ms;          /* device time from the end of the stream pass to the end of the pipeline: the part
                              of device_ms the stream pass does not hide (diagnostics) */
  double frames_ms;        /* device time of the frame pass kernel k_frames, when it ran as one launch after the
                              stream pass (0 in the overlapped pipeline, where post_ms is its exposed part) */
} ewal_result;

/* raftpb.Entry, raft/raftpb/raft.pb.go:100-106.  Data is a zero-copy
 * (offset,len) view of the stream; data_nil mirrors Go's nil slice.
 * data_nil == 2: Data is instead the range [data_off, data_off + data_len) of
 * the split bytes (ewal_copy_split_bytes / ewal_batch_copy_split_bytes) -- the
 * concatenation Go's append builds when the Entry's Data, or the Record.Data
 * holding the Entry, is repeated with several non-empty segments
 * (raft.pb.go:254, wal/walpb/record.pb.go:112; etcd's encoder never writes
 * that, a crafted WAL can). */
typedef struct ewal_entry {
  uint64_t term;
  uint64_t index;
  uint64_t data_off;
  uint64_t data_len;
  int32_t type;
  int32_t data_nil;
} ewal_entry;

/* XXX_unrecognized of a returned Entry / the HardState (raft.pb.go:100-106,
 * 143-148: the unknown fields Unmarshal appended, raft.pb.go:270), bytes at
 * [off, off+len) of the side buffer (ewal_copy_unrec_bytes).  Entries and a
 * HardState not listed have a nil XXX_unrecognized. */
typedef struct ewal_unrec {
  int64_t ent;             /* index into ents, or -1: the HardState */
  uint64_t off, len;
} ewal_unrec;

/* One decoded frame (walpb.Record + chain state), wal/walpb/record.pb.go:30-35 */
typedef struct ewal_record {
  uint64_t offset;         /* frame start (int64 length prefix) */
  uint64_t data_off;
  uint64_t data_len;
  int64_t type;
  uint32_t crc;            /* stored Record.Crc */
  uint32_t chained_crc;    /* decoder crc after this frame (== crc when it verified) */
} ewal_record;

/* ---- context ------------------------------------------------------------ */
int ewal_ctx_create(int device, ewal_ctx **out);
/* Releases every device resource of ctx.  Contract: destroy every ctx before
 * the process exits (a Go caller: before main returns / os.Exit).  The
 * library covers a ctx left alive with EWAL_OPT_OVERLAP: its two CU-masked
 * streams are destroyed by an atexit handler the library registers when it
 * creates them, before the HIP runtime's own teardown (round 6: such a ctx
 * crashed in __cxa_finalize at exit). */
void ewal_ctx_destroy(ewal_ctx *ctx);
/* Run on a caller-owned hipStream_t (NULL = the ctx's own stream).  The
 * ctx's own stream is a blocking stream: it is ordered with the legacy
 * default stream (stream 0, torch's default stream), so inputs written there
 * are complete before the ctx reads them.  A caller-owned non-blocking
 * stream gets no such ordering: the caller orders its own work on it. */
int ewal_ctx_set_stream(ewal_ctx *ctx, void *hip_stream);
/* Pre-size ctx's workspace for a ReadAll over up to wal_bytes and load the
 * device code, so that the first ReadAll (the one-shot restart,
 * etcdserver/server.go:153-156) allocates nothing.  A server calls it while
 * it reads the WAL files from disk: OpenAtIndex's directory listing gives
 * their total size first.  Optional: without it the first call sizes the
 * workspace itself. */
#define EWAL_RESERVE_HOST_STAGING 1u   /* also the HBM staging buffer of ewal_readall_host / ewal_wal_readall */
int ewal_ctx_reserve(ewal_ctx *ctx, uint64_t wal_bytes, uint32_t flags);
/* Path options of ctx (default 0: the fused frame pass first, the general
 * path when it cannot decide a WAL).  EWAL_OPT_GENERAL_PATH: every ReadAll
 * takes the general path (framing by candidate links, per-frame descriptors)
 * -- the same results, slower; for cross-checking the two paths.  No
 * environment variable changes the path. */
#define EWAL_OPT_GENERAL_PATH 1u
/* EWAL_OPT_OVERLAP: a single ReadAll of >= 512 MiB streams its bytes in four
 * chunks on 224 CUs (a CU-masked stream) while each finished chunk's frame
 * pass runs on the other 32 (a second CU-masked stream).  Off by default:
 * measured on MI355X it does not pay (profiles/r05/): the
 * stream pass loses speed faster than the frame pass gains CUs, and masks
 * of more than 32 CUs on the frame side slowed the stream side 2.4x.  A ctx
 * with this option owns two extra streams: destroy it before the process
 * exits (a live one is cleaned up at exit, see ewal_ctx_destroy). */
#define EWAL_OPT_OVERLAP 2u
/* Record-dense WALs (round 5): the stream pass also stores the lin of every
 * 256-B super-piece's first 128-B half, and the frame pass takes every frame
 * start's prefix from the nearest 128-B boundary instead of the nearest 256-B
 * one (half the tail bytes).  By default a ctx turns it on when its previous
 * single ReadAll had >= 4 frames per 4 KiB (average frame <= 1 KiB);
 * EWAL_OPT_VH_ON / EWAL_OPT_VH_OFF force it either way (the same results). */
#define EWAL_OPT_VH_ON 4u
#define EWAL_OPT_VH_OFF 8u
int ewal_ctx_set_options(ewal_ctx *ctx, uint32_t opts);
const char *ewal_status_string(int status);
/* Device time (ms) of the last pipeline call on this ctx (HIP events). */
float ewal_last_device_ms(ewal_ctx *ctx);
/* Device time (ms) of the last call's k_stream HBM pass (HIP events). */
float ewal_last_stream_ms(ewal_ctx *ctx);
int ewal_device_count(void);

/* ---- WAL replay/verify -------------------------------------------------- */
/* (*WAL).ReadAll over the concatenated bytes of OpenAtIndex's files
 * names[nameIndex:] (wal/wal.go:126-134, MultiReadCloser semantics), with
 * w.ri = ri.  d_buf is DEVICE memory, 16-byte aligned, len bytes. */
int ewal_readall_device(ewal_ctx *ctx, const void *d_buf, uint64_t len, uint64_t ri, ewal_result *out);
/* Batched ReadAll over n_shards independent WALs (one raft group's
 * names[nameIndex:] each) laid end to end in ONE device
 * buffer: shard s is the lens[s] bytes after shards 0..s-1; out[s] is exactly
 * ewal_readall_device's result for that shard alone with w.ri = ri[s]
 * (ordinals and offsets relative to the shard; stream_ms is the batch's
 * k_stream, device_ms the batch's pipeline plus any shard replayed alone).
 * One stream pass and one fused frame + check pass cover the batch; a shard
 * that pass cannot decide -- torn or corrupt framing, an index rewind, an
 * encoding the canonical parser declines, unknown fields -- is replayed alone
 * (flags |= EWAL_FLAG_SHARD_FALLBACK) while every other shard keeps the
 * batch's result.  Shards whose returned ents / HardState carry
 * XXX_unrecognized have n_unrec > 0 and a side list per shard
 * (ewal_batch_copy_unrec).  Returns 0 or a negative infrastructure error;
 * per-shard verdicts are in out[].  Replaces, per shard,
 * wal.OpenAtIndex(...).ReadAll() (wal/wal.go:108,164). */
#define EWAL_FLAG_SHARD_FALLBACK 1
/* ewal_result.flags: metadata_off / metadata_len index the split bytes (the
 * metadata record's Data repeated with several non-empty segments), not the
 * stream */
#define EWAL_FLAG_METADATA_SPLIT 2
/* ewal_result.flags (diagnostics): the fused frame pass decided this result
 * (no per-frame descriptors were built); absent: the general path did */
#define EWAL_FLAG_FAST_PATH 4
int ewal_readall_batch_device(ewal_ctx *ctx, const void *d_buf, uint64_t n_shards, const uint64_t *lens,
                              const uint64_t *ri, ewal_result *out);
/* After ewal_readall_batch_device: shard s's ents (Data offsets relative to
 * the shard).  Returns the number copied (<= cap) or a negative error. */
int64_t ewal_batch_copy_entries(ewal_ctx *ctx, uint64_t shard, ewal_entry *out, int64_t cap);
/* After ewal_readall_batch_device: the ctx-owned DEVICE array that
 * ewal_batch_copy_entries reads, and its length in entries (NULL and 0 when
 * the batch returned no entry).  Shard s's ents are the range
 * enode_reqs_from_batch (below) names.  The array is valid until the next
 * pipeline call on the ctx (any ReadAll, batch or single); the step calls,
 * enode_batch_device included, leave it alone.  Read only.  EWAL_E_INVAL when
 * the ctx's last ReadAll was not a batch that returned EWAL_OK (a single
 * ReadAll in between supersedes the batch's ranges). */
int ewal_batch_entries_device(ewal_ctx *ctx, const ewal_entry **d_ents, uint64_t *n_total);
/* After ewal_readall_batch_device: shard s's XXX_unrecognized side list
 * (ewal_unrec, ent = index into that shard's ents or -1 for its HardState)
 * and the bytes it indexes.  Return the number copied (<= cap). */
int64_t ewal_batch_copy_unrec(ewal_ctx *ctx, uint64_t shard, ewal_unrec *out, int64_t cap);
int64_t ewal_batch_copy_unrec_bytes(ewal_ctx *ctx, uint64_t shard, uint8_t *out, int64_t cap);
/* Copy host bytes into ctx-owned device memory (16-B aligned; valid until
 * the next staging call on this ctx). */
int ewal_stage_to_device(ewal_ctx *ctx, const void *h_buf, uint64_t len, void **d_out);
/* Device memory owned by the caller through the library (for callers that
 * have no HIP runtime of their own, e.g. cgo): alloc/free/copy. */
int ewal_device_alloc(ewal_ctx *ctx, uint64_t len, void **d_out);
int ewal_device_free(ewal_ctx *ctx, void *d_buf);
int ewal_upload(ewal_ctx *ctx, void *d_dst, const void *h_src, uint64_t len);
int ewal_download(ewal_ctx *ctx, void *h_dst, const void *d_src, uint64_t len);
/* Same, from host memory: staged to the device first (PCIe-inclusive). */
int ewal_readall_host(ewal_ctx *ctx, const void *h_buf, uint64_t len, uint64_t ri, ewal_result *out);
/* After a successful readall: copy the ents / per-frame descriptors out.
 * Return the number copied (<= cap) or a negative error.  The descriptors
 * are rebuilt on demand from the ctx's stream-pass state and the ReadAll's
 * stream bytes: d_buf must still hold them (the same lifetime rule as the
 * ents' Data views), and any later compute call on the ctx (another ReadAll,
 * a batch, a CRC, snapshot or save call, a staging call that reuses the
 * staging buffer) makes ewal_copy_records return EWAL_E_INVAL. */
int64_t ewal_copy_entries(ewal_ctx *ctx, ewal_entry *out, int64_t cap);
int64_t ewal_copy_records(ewal_ctx *ctx, ewal_record *out, int64_t cap);
/* After a successful readall with n_unrec > 0: the side list (sorted by ent)
 * and its bytes. */
int64_t ewal_copy_unrec(ewal_ctx *ctx, ewal_unrec *out, int64_t cap);
int64_t ewal_copy_unrec_bytes(ewal_ctx *ctx, uint8_t *out, int64_t cap);
/* After a successful readall: the split bytes the data_nil == 2 ents and an
 * EWAL_FLAG_METADATA_SPLIT metadata index (gathered on the device).  Copies
 * min(cap, total) bytes; returns the total (0: none) or a negative error.
 * The batched form: shard s's (a shard with split fields is replayed alone). */
int64_t ewal_copy_split_bytes(ewal_ctx *ctx, uint8_t *out, int64_t cap);
int64_t ewal_batch_copy_split_bytes(ewal_ctx *ctx, uint64_t shard, uint8_t *out, int64_t cap);

/* What one rank's range of ONE WAL split by file contributes to the joined
 * verdict (etcd_amd/shard.py split_verdict applies ReadAll's
 * cross-file rules with it), from the last ReadAll on ctx over that range --
 * all frames of its chain, those after a failure included.  Frames are
 * ordinals in the range, offsets are into the range's stream (d_buf must
 * still hold it, as for ewal_copy_records).  The rules it serves:
 *   crc seam       wal/wal.go:184-192 (every file opens with crcType{running
 *                  CRC}, wal/wal.go:93,232-234)
 *   metadata       wal/wal.go:178-183
 *   ents / enti    wal/wal.go:170-174, 203-206 (the index-gap rule across the
 *                  range boundary, rewinds below the range's w.ri, and the
 *                  global ErrIndexNotFound) */
typedef struct ewal_range_info {
  int64_t n_frames;              /* frames on the chain */
  int64_t first_crc;             /* Crc of frame 0 when it is a crcType record, else -1 */
  int64_t md_first_frame;        /* the first metadataType frame, -1: none */
  int64_t md_first_off, md_first_len;   /* its Data; off -1 == nil */
  int64_t md_value_frame;        /* the first metadataType frame with non-nil Data (the value ReadAll keeps), -1 */
  int64_t md_value_off, md_value_len;
  int64_t first_entry_frame;     /* the first entryType frame, -1: none */
  int64_t last_entry_frame;
  uint64_t first_entry_index;    /* its Entry.Index */
  uint64_t min_entry_index;      /* the least Entry.Index of the range */
  uint64_t last_entry_index;     /* the last entry frame's Index (w.enti after the range) */
  int64_t last_op_frame;         /* the last entry frame with Index >= the ReadAll's ri (the last
                                    append to ents, wal/wal.go:171-173), -1: none */
  uint64_t last_op_index;
  int32_t md_split;              /* bit 0: md_first_off, bit 1: md_value_off index the split bytes
                                    (ewal_copy_split_bytes: a metadata Data in several segments) */
  int32_t first_pre_crc;         /* 1: frame 0 failed inside decoder.decode before its CRC check
                                    (framing, walpb.Record.Unmarshal, wal/decoder.go:30-41) -- that
                                    failure wins over the caller's deferred check; 0: it did not fail
                                    there (an Entry / HardState decode failure comes after the check) */
  /* frame 0 (EWAL_RANGE_DEFER_FIRST: the caller's CRC check) */
  int64_t first_type;            /* Record.Type, -1: no frame */
  uint64_t first_dlen;           /* len(Data) */
  uint32_t first_stored_crc;     /* Record.Crc */
  uint32_t first_u0;             /* crc32.Update(0, Castagnoli, Data) (the stored CRC for a crcType frame) */
  uint64_t end_off;              /* where the frame chain ended (decoder.decode's terminal): n_bytes when
                                    the range ended on a frame boundary */
  uint64_t n_bytes;              /* the range's length */
  /* the range's last stateType frame (ReadAll's `state = mustUnmarshalState`,
     wal/wal.go:176-177): the HardState the whole WAL returns when no later
     range holds one */
  int64_t state_frame;           /* -1: none */
  uint64_t state_term, state_vote, state_commit;
  int32_t state_unrec;           /* 1: that HardState carries XXX_unrecognized */
  int32_t pad2;
} ewal_range_info;
int ewal_copy_range_info(ewal_ctx *ctx, ewal_range_info *out);

/* ONE WAL split across ranks INSIDE a file: rank r takes the
 * bytes [c_r, c_{r+1}) of the stream, where c_r is the first frame-start
 * candidate at or after r * len / ranks (ewal_range_probe; c_0 = 0).  The
 * running CRC before a range's frame 0 is the previous range's, so with
 * EWAL_RANGE_DEFER_FIRST frame 0's CRC check (decoder.decode's Validate,
 * wal/decoder.go:42-46, or the crcType rule, wal/wal.go:184-192) is left to
 * the caller, who makes it with ewal_copy_range_info's first_* operands
 * (first_u0 = crc32.Update(0, Data), combined with the running CRC by
 * ewal_crc32_combine); every other rule is ReadAll's over the range with
 * w.ri = ri.  etcd_amd/shard.py split_verdict joins the ranges. */
#define EWAL_RANGE_DEFER_FIRST 1u
int ewal_readall_range_device(ewal_ctx *ctx, const void *d_buf, uint64_t len, uint64_t ri, uint32_t flags,
                              ewal_result *out);
/* The first frame-start candidate at or after `from` within `window` bytes of
 * a device stream of len bytes (*pos, -1: none), and the Index of the first
 * entry record on the frame chain from it within 64 frames (*first_entry_index,
 * -1: none) -- the range's w.ri candidate. */
int ewal_range_probe(ewal_ctx *ctx, const void *d_buf, uint64_t len, uint64_t from, uint64_t window, int64_t *pos,
                     int64_t *first_entry_index);
/* The same, taking only candidates at positions that are multiples of align
 * (a power of two): with 16 a range of a device-resident WAL starts on an
 * address every kernel can read without a copy (ewal_multi_plan_device). */
int ewal_range_probe_aligned(ewal_ctx *ctx, const void *d_buf, uint64_t len, uint64_t from, uint64_t window,
                             uint32_t align, int64_t *pos, int64_t *first_entry_index);

/* ---- ONE WAL over several ranges: ReadAll's verdict joined (host C++) ------
 * Range k of a WAL split into contiguous ranges (by file, or inside a file)
 * was read by ReadAll on its own (ewal_readall_device / _range_device with
 * w.ri = ri); its row carries that ReadAll's result and ewal_copy_range_info.
 * ewal_split_verdict applies ReadAll's cross-range rules in order, before
 * each range's own first failure (wal/wal.go:164-216):
 *   crc seam        a crcType frame 0 against the running CRC (wal/wal.go:184-192)
 *   deferred frame 0 (a range starting inside a file) Validate with the running
 *                   CRC, crc32.Update(running, Data) = ewal_crc32_combine(running,
 *                   first_u0, first_dlen) (wal/decoder.go:42-46)
 *   metadata        metadata != nil && !DeepEqual (wal/wal.go:178-183)
 *   ents            the range's first entry op against len(ents) carried over
 *                   (the index-gap panic, wal/wal.go:170-173); ErrIndexNotFound
 *                   over all ranges (wal/wal.go:203-206)
 * resplit = k >= 0: the verdict needs ranges k.. read as ONE range (a frame
 * cut short at range k's end, bytes range k left unconsumed, a rewind below a
 * range's w.ri): the caller reads them joined, marks the later rows empty
 * (n_bytes 0) and calls again.  md: the metadata bytes of every range in
 * order -- its first metadata frame's Data (when md_first_frame >= 0 and
 * md_first_off >= 0) then the value kept (md_value_frame >= 0). */
typedef struct ewal_range_row {
  int32_t status;                /* ReadAll's status over the range */
  int32_t deferred;              /* 1: read with EWAL_RANGE_DEFER_FIRST */
  int64_t fail_record;           /* the range's ordinal, -1 */
  int64_t n_records;
  uint64_t ri;                   /* the range's w.ri */
  uint32_t last_crc;             /* ReadAll's running CRC after the range */
  uint32_t pad;
  int64_t detail;                /* ReadAll's detail (block type, gap index) */
  ewal_range_info info;          /* ewal_copy_range_info of that ReadAll */
} ewal_range_row;
typedef struct ewal_split_result {
  int32_t status;
  int32_t resplit;               /* -1: final; k: read ranges k.. joined and call again */
  int64_t fail_record;           /* the global frame ordinal of the failure, -1 */
  int64_t n_records;             /* frames verified */
  int64_t detail;
  uint32_t last_crc;             /* decoder.lastCRC() after the WAL (EWAL_OK) */
  uint32_t pad;
  uint64_t enti;                 /* w.enti: the last entry's Index (EWAL_OK) */
  /* the rest of ReadAll's (metadata, state, ents) on EWAL_OK (wal/wal.go:206-215) */
  int32_t md_range;              /* the range whose metadata Data ReadAll returns, -1: nil */
  int32_t md_split;              /* 1: md_off indexes that range's split bytes, 0: its stream */
  int64_t md_off, md_len;        /* the Data inside that range */
  int64_t md_blob_off;           /* the same bytes inside the md blob given to ewal_split_verdict */
  int32_t state_range;           /* the range whose last HardState ReadAll returns, -1: HardState{} */
  int32_t pad2;
  uint64_t state_term, state_vote, state_commit;
  int64_t n_ents;                /* len(ents): ranges' ents stitched as ewal_split_ents_layout says */
} ewal_split_result;
int ewal_split_verdict(const ewal_range_row *rows, uint64_t n, uint64_t ri_global, const uint8_t *md, uint64_t md_len,
                       ewal_split_result *out);
/* Where each range's ents land in the joined ents of a final EWAL_OK verdict
 * (wal/wal.go:170-173, `ents = append(ents[:e.Index-w.ri], e)` carried across
 * the ranges): range k's ents (its own ReadAll's, with w.ri = rows[k].ri) are
 * joined ents [base[k], base[k] + count[k]), where base[k] = rows[k].ri - ri
 * and count[k] is cut where a later range's base overwrites them; ranges
 * without entry ops get count 0.  Returns len(ents) or a negative error. */
int64_t ewal_split_ents_layout(const ewal_range_row *rows, uint64_t n, uint64_t ri_global, int64_t *base,
                               int64_t *count);
/* ReadAll over ONE WAL (the bytes of names[nameIndex:], h_buf, len) split
 * across n_ctx contexts in one process -- one host thread per context, each
 * on its own device or sharing one: by file when file_off (n_files + 1
 * offsets, file_off[0] = 0, file_off[n_files] = len) and file_index (the
 * index in each file's name) are given, each range a run of whole files
 * with w.ri = max(ri, its first file's index); else inside the stream, range
 * r starting at the first frame-start candidate after r * len / n_ctx
 * (ewal_range_probe) with frame 0's check deferred.  The ranges' verdicts
 * are joined by ewal_split_verdict (re-reading ranges joined when it asks).
 * out->status etc. are exactly (*WAL).ReadAll's over the whole stream with
 * w.ri = ri; *n_resplit (nullable) counts the joined re-reads. */
int ewal_readall_multi(ewal_ctx *const *ctxs, uint32_t n_ctx, const void *h_buf, uint64_t len, const uint64_t *file_off,
                       const uint64_t *file_index, uint32_t n_files, uint64_t ri, ewal_split_result *out,
                       uint32_t *n_resplit);

/* ---- ONE WAL over several contexts: ReadAll's whole result ---------------
 * An ewal_multi drives n_ctx DISTINCT contexts (they may share a device; one
 * ctx is never used from two threads) and keeps, after each call, what
 * (*WAL).ReadAll returns over the whole stream (wal/wal.go:164-216, its
 * caller etcdserver/server.go:153-168): the verdict in ewal_split_result
 * (status, lastCRC, enti, the metadata's range and bytes, the HardState,
 * len(ents)) and, on EWAL_OK, the joined ents, metadata, split bytes and
 * XXX_unrecognized side list through the ewal_multi_copy_* calls -- which
 * read the ranges' ReadAll state left on each ctx: no other call may run on
 * those ctxs in between.  A ctx stays ordered with the legacy default stream
 * (ewal_ctx_set_stream); on a shared device a ctx's blocking stream also
 * waits for the others' null-stream allocations and copies, which is why the
 * host path stages into each ctx's reusable buffer instead of allocating. */
typedef struct ewal_multi ewal_multi;
int ewal_multi_create(ewal_ctx *const *ctxs, uint32_t n_ctx, ewal_multi **out);
void ewal_multi_destroy(ewal_multi *m);
/* From host bytes (each range staged into its ctx's staging buffer), split as
 * ewal_readall_multi says.  out->resplit is always -1 on return. */
int ewal_multi_readall(ewal_multi *m, const void *h_buf, uint64_t len, const uint64_t *file_off,
                       const uint64_t *file_index, uint32_t n_files, uint64_t ri, ewal_split_result *out);
/* Device-resident ranges: range r is the bytes [starts[r], starts[r + 1]) of
 * the stream, already in HBM at d_ranges[r] (16-B aligned) where ctx r reads
 * them, read with w.ri = ris[r] and flags[r] (EWAL_RANGE_DEFER_FIRST for a
 * range starting inside a file; flags NULL: every range but the first).  No
 * allocation, no host copy of the WAL.  A joined re-read the verdict asks for
 * runs on ctx k when ranges k.. form one contiguous device span; otherwise
 * out->resplit = k comes back and the caller reads ranges k.. joined itself. */
int ewal_multi_readall_device(ewal_multi *m, const void *const *d_ranges, const uint64_t *starts, const uint64_t *ris,
                              const uint32_t *flags, uint64_t ri, ewal_split_result *out);
/* Ranges of ONE device-resident stream d_buf[0, len) that every ctx of m can
 * read (the contexts on d_buf's device): starts[0..n_ctx] (range r opens at a
 * 16-B aligned frame-start candidate after r * len / n_ctx, found by
 * ewal_range_probe_aligned on ctx r) and each range's w.ri; then
 * d_ranges[r] = d_buf + starts[r] for ewal_multi_readall_device.  A range
 * whose 64 MiB probe window holds no aligned candidate is left empty
 * (starts[r] == starts[r + 1]: the range before reads on through it). */
int ewal_multi_plan_device(ewal_multi *m, const void *d_buf, uint64_t len, uint64_t ri, uint64_t *starts,
                           uint64_t *ris);
/* After a final EWAL_OK: len(ents) entries joined in order (Data offsets into
 * the whole stream, or into ewal_multi_copy_split_bytes for data_nil == 2),
 * the metadata Data (returns its length; 0 with md_range -1: nil), the
 * ranges' split bytes joined, the XXX_unrecognized side list (ent into the
 * joined ents, -1 the HardState; sorted) and its bytes.  Each returns the
 * total (entries, bytes) and copies min(cap, total). */
int64_t ewal_multi_copy_entries(ewal_multi *m, ewal_entry *out, int64_t cap);
int64_t ewal_multi_copy_metadata(ewal_multi *m, uint8_t *out, int64_t cap);
int64_t ewal_multi_copy_split_bytes(ewal_multi *m, uint8_t *out, int64_t cap);
int64_t ewal_multi_copy_unrec(ewal_multi *m, ewal_unrec *out, int64_t cap);
int64_t ewal_multi_copy_unrec_bytes(ewal_multi *m, uint8_t *out, int64_t cap);
/* The last call's ranges (rows and stream starts; returns n_ctx) and timing:
 * out4 = {wall ms of the call, the slowest range's device ms, host ms in the
 * join, joined re-reads}. */
int ewal_multi_copy_rows(ewal_multi *m, ewal_range_row *out, uint64_t *starts, uint32_t cap);
int ewal_multi_timing(ewal_multi *m, double *out4);

/* ---- directory-level API: wal.OpenAtIndex + ReadAll + writer ----------- */
typedef struct ewal_wal ewal_wal;
/* wal.OpenAtIndex(dirpath, index), wal/wal.go:108-159 (file selection:
 * wal/util.go:20-88): selects and opens names[nameIndex:]; their bytes are
 * read by ewal_wal_readall (pieces read by a few threads while the finished
 * ones are already copied to HBM) or on demand by ewal_wal_bytes. */
int ewal_open_at_index(const char *dirpath, uint64_t index, ewal_wal **out);
/* The file-name helpers OpenAtIndex uses (host-only), wal/util.go:20-88:
 * parseWalName (1 = parsed), searchIndex over sorted names (the index, -1
 * when none), isValidSeq (1 / 0), walName (out: 38 bytes). */
int ewal_parse_wal_name(const char *name, uint64_t *seq, uint64_t *index);
int64_t ewal_search_index(const char *const *names, uint64_t n, uint64_t index);
int ewal_is_valid_seq(const char *const *names, uint64_t n);
void ewal_wal_name(uint64_t seq, uint64_t index, char *out);
int ewal_wal_readall(ewal_wal *w, ewal_ctx *ctx, ewal_result *out);
/* total bytes of the opened files (size ewal_ctx_reserve before ReadAll) */
uint64_t ewal_wal_size(ewal_wal *w);
/* Start reading the opened files into host memory in the background (reader
 * threads, 64 MiB pieces) and return at once: a restarting server calls it
 * right after OpenAtIndex so the reads overlap its GPU context creation;
 * ewal_wal_readall then uploads the pieces already read and waits for the
 * rest.  Optional (ReadAll starts the reads itself). */
int ewal_wal_prefetch(ewal_wal *w);
const uint8_t *ewal_wal_bytes(ewal_wal *w, uint64_t *len);
uint64_t ewal_wal_seq(ewal_wal *w);
void ewal_wal_close(ewal_wal *w);

/* Write path (the on-disk format the hot path reads), wal/wal.go:72-100,
 * 219-292, wal/encoder.go:25-37.  Host C++; CRC via SSE4.2. */
typedef struct ewal_writer ewal_writer;
int ewal_create(const char *dirpath, const uint8_t *metadata, uint64_t mlen, int metadata_nil, ewal_writer **out);
int ewal_writer_save_entry(ewal_writer *w, int32_t type, uint64_t term, uint64_t index, const uint8_t *data, uint64_t n);
int ewal_writer_save_state(ewal_writer *w, uint64_t term, uint64_t vote, uint64_t commit);
int ewal_writer_cut(ewal_writer *w);
int ewal_writer_sync(ewal_writer *w);
void ewal_writer_close(ewal_writer *w);

/* In-memory encoder (encoder.encode over a growing buffer). */
typedef struct ewal_encoder ewal_encoder;
ewal_encoder *ewal_encoder_new(uint32_t prev_crc, uint64_t reserve);
int ewal_encoder_encode(ewal_encoder *e, int64_t type, const uint8_t *data, uint64_t n, int data_nil);
int ewal_encoder_save_entry(ewal_encoder *e, int32_t type, uint64_t term, uint64_t index, const uint8_t *data, uint64_t n);
int ewal_encoder_save_state(ewal_encoder *e, uint64_t term, uint64_t vote, uint64_t commit);
const uint8_t *ewal_encoder_bytes(ewal_encoder *e, uint64_t *len);
uint32_t ewal_encoder_crc(ewal_encoder *e);
void ewal_encoder_free(ewal_encoder *e);

/* ---- batched write path: (*WAL).SaveEntry / encoder.encode on the GPU ---- */
/* encoder.encode(&walpb.Record{Type: entryType, Data: pbutil.MustMarshal(e)})
 * for n entries in order (wal/wal.go:248-263, wal/encoder.go:25-37): the
 * frames, byte-identical to the reference's encoder, and the chained CRC
 * (c_i = crc32.Update(c_{i-1}, Castagnoli, Entry_i bytes), c_{-1} = prev_crc).
 * d_data: the entries' payloads on the device (d_ents[i].data_off/data_len
 * index it, data_len_total bytes); d_ents: n ewal_entry on the device.
 * d_out: device buffer of cap bytes.  *out_len = bytes written, *last_crc =
 * c_{n-1} (prev_crc when n == 0).  EWAL_E_NOMEM when the frames exceed cap,
 * EWAL_E_INVAL when an entry's payload lies outside d_data. */
int ewal_encode_entries_device(ewal_ctx *ctx, const void *d_data, uint64_t data_len_total, const ewal_entry *d_ents,
                               uint64_t n, uint32_t prev_crc, void *d_out, uint64_t cap, uint64_t *out_len,
                               uint32_t *last_crc);

/* Batched WAL writes on the GPU: a sequence of (*WAL).SaveState / SaveEntry /
 * Cut calls (wal/wal.go:219-279) encoded as ONE chained call.  Each record:
 *   EWAL_SAVE_ENTRY  SaveEntry(&Entry{Type: etype, Term: a, Index: b, Data})
 *   EWAL_SAVE_STATE  SaveState(&HardState{Term: a, Vote: b, Commit: c});
 *                    an empty HardState writes nothing (wal/wal.go:266-268)
 *   EWAL_SAVE_CUT    Cut's records: crcType{Crc: running CRC}, then
 *                    metadataType{Data: w.md} (wal/wal.go:232-237); Data is
 *                    the (data_off, data_len) bytes, or nil when data_nil
 * Data lives in d_data; d_recs on the device.  The frames go to d_out (cap
 * bytes): *out_len bytes, *last_crc the running CRC after the last record
 * (prev_crc when nothing was written).  h_rec_off (nullable, host, n
 * entries): the offset of each record's first frame in d_out -- a Cut's is
 * where the next file (walName(seq+1, enti+1)) starts.  Byte-identical to
 * the reference encoder (wal/encoder.go:25-37) over the same calls. */
#define EWAL_SAVE_ENTRY 2
#define EWAL_SAVE_STATE 3
#define EWAL_SAVE_CUT 4
typedef struct ewal_save_rec {
  int32_t kind;
  int32_t etype;
  uint64_t a, b, c;
  uint64_t data_off, data_len;
  int32_t data_nil;
  int32_t pad;
} ewal_save_rec;
int ewal_save_device(ewal_ctx *ctx, const void *d_data, uint64_t data_len_total, const ewal_save_rec *d_recs,
                     uint64_t n, uint32_t prev_crc, void *d_out, uint64_t cap, uint64_t *out_len, uint32_t *last_crc,
                     uint64_t *h_rec_off);

/* ---- CRC primitives (pkg/crc, pkg/crc/crc.go:23-41) ---------------------- */
/* crc32.Update(crc, MakeTable(poly), p) on a DEVICE buffer.  d_buf must be
 * 16-byte aligned (EWAL_E_INVAL otherwise, when n > 0). */
int ewal_crc32_update_device(ewal_ctx *ctx, uint32_t crc, uint32_t poly, const void *d_buf, uint64_t n,
                             uint32_t *out);
/* crc32.Update on host memory (SSE4.2 for Castagnoli) -- for small writes. */
uint32_t ewal_crc32_update_host(uint32_t crc, uint32_t poly, const uint8_t *p, uint64_t n);
/* Update(c1, A || B) from c1=Update(0,A)... : returns Update(crc_a, B) given
 * crc_b = Update(0, B) and len_b, without touching the bytes. */
uint32_t ewal_crc32_combine(uint32_t poly, uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* ---- snapshots: snap.loadSnap / Snapshotter.Load, snap/snapshotter.go:62-111 */
/* Batch-verify snapshot FILES (snappb.Snapshot envelopes) resident in one
 * device buffer at offs[i], lens[i].  status[i] = EWAL_OK / EWAL_ERR_SNAP_CRC /
 * unmarshal class; crc outputs are the stored and recomputed CRCs.  A file
 * whose snappb.Snapshot or raftpb.Snapshot holds unknown groups nested deeper
 * than the device walker's stack gets EWAL_UNSUPPORTED_ENCODING (Go loads it);
 * its status alone is meaningful then.  d_buf
 * must be 16-byte aligned (EWAL_E_INVAL otherwise); offs[i] may be any byte. */
int esnap_verify_packed(ewal_ctx *ctx, const void *d_buf, uint64_t buf_len, const uint64_t *offs,
                        const uint64_t *lens, uint32_t n, uint32_t poly, int32_t *status,
                        uint32_t *stored_crc, uint32_t *computed_crc);
/* Snapshotter.Load(): newest-first over dir's *.snap, first success wins,
 * tried failures renamed *.broken.  On success *out_name (malloc'd, caller
 * frees with free()) names the snapshot file loaded; snapshot fields out.
 * Only the errors Go's loadSnap returns rename a file .broken; a Go panic
 * class (or EWAL_UNSUPPORTED_ENCODING: protobuf groups nested deeper than
 * the device walker's stack) stops Load with *out_name naming that file,
 * not renamed. */
typedef struct esnap_snapshot {
  uint64_t index, term;
  uint64_t data_off, data_len;   /* raftpb.Snapshot.Data within the file */
  int64_t n_nodes, n_removed;
  uint64_t nodes[64], removed[64];
} esnap_snapshot;
/* After esnap_verify_packed: the decoded raftpb.Snapshot of file i (only
 * meaningful when status[i] == EWAL_OK).  data_off == ~0: Data is not one
 * range of the file (several segments); n_nodes / n_removed > 64: only the
 * first 64 are held -- esnap_copy_field returns the full values. */
int esnap_copy_snapshot(ewal_ctx *ctx, uint32_t i, esnap_snapshot *out);
/* The full value of one raftpb.Snapshot field of file i of the last
 * esnap_verify_packed (d_buf still alive) or esnap_load_dir (i = 0): the
 * bytes of Data (the concatenation Go's append builds over repeated fields,
 * raft.pb.go:279-406) or of Snapshot.XXX_unrecognized, or the uint64 values
 * of Nodes / RemovedNodes.  Copies min(cap, full) bytes / values to out;
 * returns the full count or a negative error. */
enum { ESNAP_FIELD_DATA = 0, ESNAP_FIELD_UNREC = 1, ESNAP_FIELD_NODES = 2, ESNAP_FIELD_REMOVED = 3 };
int64_t esnap_copy_field(ewal_ctx *ctx, uint32_t i, int32_t field, void *out, int64_t cap);
int esnap_load_dir(ewal_ctx *ctx, const char *dirpath, uint32_t poly, esnap_snapshot *out, char **out_name);
/* Snapshotter.snapNames (snap/snapshotter.go:115-131): the *.snap names,
 * newest first, NUL-separated into out (cap bytes; *len = bytes needed).
 * Returns the count (0: ErrNoSnapshot) or a negative error. */
int64_t esnap_names(const char *dirpath, char *out, uint64_t cap, uint64_t *len);

/* ---- snapshots: Snapshotter.save / SaveSnap, snap/snapshotter.go:39-60 ---- */
/* One raftpb.Snapshot to save (a HOST array, one per snapshot).  Data is the
 * device range d_data[data_off, data_off + data_len) at any byte offset;
 * Nodes / RemovedNodes are ranges of the host array h_u64 (in uint64 units),
 * XXX_unrecognized a range of the host bytes h_unrec (unrec_len 0: nil). */
typedef struct esnap_save_rec {
  uint64_t index, term;
  uint64_t data_off, data_len;
  uint64_t nodes_off, n_nodes;
  uint64_t removed_off, n_removed;
  uint64_t unrec_off, unrec_len;
} esnap_save_rec;
/* Where file i landed in d_out, and the CRC stored in it. */
typedef struct esnap_saved {
  uint64_t off, len;
  uint32_t crc, pad;
} esnap_saved;
/* A capacity of d_out that esnap_save_packed_device never exceeds for these
 * records (the files' bytes plus at most 19 bytes of layout slack per file);
 * from the host arrays alone.  ~0 when the sum does not fit 64 bits. */
uint64_t esnap_save_bound(const esnap_save_rec *recs, uint32_t n, const uint64_t *h_u64);
/* Snapshotter.save's bytes (snap/snapshotter.go:46-60) for n snapshots in ONE
 * call on the ctx's stream:
 *   b    = raftpb.Snapshot.Marshal()       raft/raftpb/raft.pb.go:954-999
 *   crc  = crc32.Update(0, MakeTable(poly), b)
 *   file = snappb.Snapshot{Crc, Data: b}.Marshal()   snap/snappb/snap.pb.go:158-176
 * File i is d_out[out[i].off, out[i].off + out[i].len), byte-identical to the
 * reference's; out[i].crc is its stored CRC.  The offsets are OUTPUTS: the
 * library places every file so that its Data lands at an address congruent
 * to its source mod 16 (the copy is then aligned 16-byte loads and stores).
 * Files are in order of i, do not overlap, lie inside [0, cap), may have
 * small gaps between them, and no byte of d_out outside the files is written
 * -- the output feeds esnap_verify_packed directly.  One fused pass: every
 * byte of Data is loaded from HBM once and stored once, its CRC contribution
 * taken from the registers of that load (etcd_amd/csrc/snap_save.hip).
 * d_data and d_out are DEVICE buffers, 16-byte aligned, that do not overlap.
 * Decided on the host before any kernel is launched (d_out untouched):
 *   EWAL_E_INVAL  a Data range outside d_data, a range that wraps, d_out
 *                 overlapping d_data, a base pointer not 16-byte aligned
 *   EWAL_E_NOMEM  the layout needs more than cap (cap >= esnap_save_bound()
 *                 is always enough)
 * n == 0: EWAL_OK, nothing written. */
int esnap_save_packed_device(ewal_ctx *ctx, const void *d_data, uint64_t data_len_total, const esnap_save_rec *recs,
                             uint32_t n, const uint64_t *h_u64, const uint8_t *h_unrec, uint32_t poly, void *d_out,
                             uint64_t cap, esnap_saved *out);
/* The file name save uses, "%016x-%016x.snap" % (term, index)
 * (snap/snapshotter.go:47): 38 characters; out: 39 bytes with the NUL. */
void esnap_snap_name(uint64_t term, uint64_t index, char *out);
/* Snapshotter.SaveSnap (snap/snapshotter.go:39-44) for one snapshot: nothing
 * is written when raft.IsEmptySnap holds (index == 0, raft/node.go:79-81):
 * EWAL_OK with *out_name = NULL.  Otherwise the file is built on the GPU,
 * downloaded, and written to dirpath/<esnap_snap_name> with mode 0666,
 * truncating an existing file (ioutil.WriteFile); *out_name (malloc'd, the
 * caller frees it with free()) is its name.  I/O failures: EWAL_E_IO. */
int esnap_save_dir(ewal_ctx *ctx, const char *dirpath, const void *d_data, uint64_t data_len_total,
                   const esnap_save_rec *rec, const uint64_t *h_u64, const uint8_t *h_unrec, uint32_t poly,
                   char **out_name);
/* For bindings: bytes of Data per tile of the fused pass, sizeof(esnap_save_rec),
 * sizeof(esnap_saved). */
uint32_t esnap_save_tile_bytes(void);
uint32_t esnap_save_rec_size(void);
uint32_t esnap_saved_size(void);

/* ---- raft quorum commit: raft.maybeCommit, raft/raft.go:248-258 ---------- */
/* Batched over G independent raft groups (SoA).  match[v*G + g] for voter
 * v < nvoters[g] (1..255); log terms for group g are log_terms[log_ptr[g] ..
 * log_ptr[g+1]) at raft indices log_offset[g] + k.  committed[] is updated in
 * place; changed[g] = maybeCommit's return; status[g] = 0, or
 * EWAL_PANIC_BOUNDS where Go panics (no voters: mis[q-1] on an empty slice;
 * raftLog.at past the log).  All pointers are DEVICE pointers. */
int ecommit_batch_device(ewal_ctx *ctx, uint64_t G, const uint64_t *match, const uint8_t *nvoters,
                         const uint64_t *term, uint64_t *committed, const uint64_t *log_offset,
                         const uint64_t *log_ptr, const uint64_t *log_terms, uint8_t *changed,
                         uint8_t *status, double *device_ms);
/* The same maybeCommit over one 192-B record per group (the kernel reads
 * each group's state with coalesced loads instead of seven strided match
 * words plus a term gather that costs a whole line).  tail_term[k] is the
 * term of raftLog.ents[nlog-1-k] for k < min(13, nlog); when the quorum index lies
 * further back its term is read from log_terms[log_ptr[g] + (index -
 * log_offset)] (both may be NULL when the caller knows it never does: such a
 * group then gets status EWAL_UNSUPPORTED_ENCODING, as does a group with more
 * than 7 voters -- ecommit_batch_device takes those).  Outputs are SoA:
 * committed_out[g] (the new raftLog.committed), changed[g], status[g] as in
 * ecommit_batch_device.  All pointers are DEVICE pointers. */
typedef struct ecommit_group {
  uint64_t match[7];       /* Progress.Match of voters 0 .. nvoters-1 (raft/raft.go:252) */
  uint64_t committed;      /* raftLog.committed */
  uint64_t term;           /* raft.Term */
  uint64_t log_offset;     /* raftLog.offset: the index of ents[0] */
  uint32_t nlog;           /* len(raftLog.ents) */
  uint8_t nvoters;         /* 1..7 */
  uint8_t pad[3];
  uint64_t tail_term[13];  /* term of ents[nlog-1-k] */
} ecommit_group;
int ecommit_batch_rec_device(ewal_ctx *ctx, uint64_t G, const ecommit_group *groups, const uint64_t *log_ptr,
                             const uint64_t *log_terms, uint64_t *committed_out, uint8_t *changed,
                             uint8_t *status, double *device_ms);

/* ---- follower append: raft.handleAppendEntries, raft/raft.go:410-416 -------
 * Batched over n msgApp for n different raft groups: raftLog.maybeAppend with
 * matchTerm, findConflict, append, at, isOutOfBounds and lastIndex
 * (raft/log.go:49-84, 115-117, 141-146, 194-217), then the msgAppResp that
 * send (raft/raft.go:190-199) queues.  The log of group g is the window
 * d_terms[terms_off, terms_off + nlog) of entry terms -- the same windows
 * ecommit_batch_device reads -- with room for terms_cap entries; the entries
 * of message i are ewal_entry views d_ents[ents_first, + n_ents) as ReadAll
 * and emsg_decode_batch_device return them.  All arithmetic is Go's uint64
 * and wraps. */
/* follower state of one raft group; a DEVICE array of G, updated in place */
typedef struct elog_group {        /* 64 bytes */
  uint64_t id;          /* raft.id   -> From of the response (raft.go:190-199) */
  uint64_t term;        /* raft.Term -> Term of the response                   */
  uint64_t committed;   /* raftLog.committed                    (updated) */
  uint64_t unstable;    /* raftLog.unstable                     (updated) */
  uint64_t log_offset;  /* raftLog.offset: the index of ents[0]           */
  uint64_t nlog;        /* len(raftLog.ents)                    (updated) */
  uint64_t terms_off;   /* ents[k].Term == d_terms[terms_off + k], k < nlog */
  uint64_t terms_cap;   /* room at terms_off, in entries                  */
} elog_group;
/* one msgApp; a DEVICE array of n */
typedef struct elog_app {          /* 64 bytes */
  uint64_t group;                  /* which elog_group handles it */
  uint64_t from, index, log_term, commit;   /* m.From, m.Index, m.LogTerm, m.Commit */
  uint64_t ents_first, n_ents;     /* m.Entries = d_ents[ents_first, +n_ents) (ewal_entry) */
  uint64_t pad;
} elog_app;
/* what happened to message i; a DEVICE array of n */
typedef struct elog_app_result {   /* 48 bytes */
  int32_t status;       /* EWAL_OK, EWAL_PANIC_BOUNDS, EWAL_PANIC_COMMITTED_CONFLICT */
  int32_t accepted;     /* maybeAppend's return (0: the response rejects) */
  uint64_t conflict;    /* findConflict's ci; 0: none */
  uint64_t app_first, n_app;   /* the entries appended: d_ents[app_first, +n_app), a suffix
                                  of the message's range; n_app == 0: nothing appended */
  uint64_t last_index;  /* raftLog.lastIndex() afterwards */
  uint64_t committed;   /* raftLog.committed afterwards */
} elog_app_result;
/* Per message i (handleAppendEntries exactly), with lastIndex = nlog - 1 +
 * log_offset, lastnewi = index + n_ents, from = index + 1:
 *   matchTerm(index, log_term): raftLog.at(index) is nil when index <
 *     log_offset or index > lastIndex -> the response rejects.  When at passes
 *     isOutOfBounds but index - log_offset >= nlog Go indexes past ents (only
 *     possible when nlog - 1 + log_offset wrapped): EWAL_PANIC_BOUNDS.
 *   findConflict compares terms only, by position from + k (an entry's own
 *     index field is not looked at); ci = the first position whose log term
 *     differs or that lies past lastIndex, 0: none -- also when it is 0
 *     because from + k wrapped.
 *   0 < ci <= committed: EWAL_PANIC_COMMITTED_CONFLICT.
 *   accepted with ci > 0: d_terms[terms_off + (ci - log_offset) + j] =
 *     d_ents[app_first + j].term for j < n_app, nlog = ci - log_offset + n_app,
 *     unstable = min(unstable, ci).
 *   every accepted message: committed = max(committed, min(commit, lastnewi)).
 * A panicking message leaves its group and d_terms unchanged; d_res[i] carries
 * the status, the unchanged last_index and committed, and 0 elsewhere;
 * d_resp[i] is 144 zero bytes (Go sends nothing).
 * No word of d_terms outside [terms_off + ci - log_offset, + n_app) is
 * written.  Only committed, unstable and nlog of a group that received an
 * accepted message may change; groups that received no message are not
 * touched.
 * d_resp[i] (nullable array) is the msgAppResp after send: type = 4, to =
 * from, from = group.id, term = group.term, index = lastIndex() after the
 * append -- or m.Index with reject = 1 --, every other field 0: with the
 * h_out of a size query d_resp feeds emsg_encode_batch_device unchanged.
 * Each group handles at most ONE message per call (a second one is a
 * sequential dependency: the next call).  The term windows of the groups the
 * messages name must not overlap each other: the caller's contract, not
 * checked.
 * Checked on the device before anything is modified (then d_groups, d_terms,
 * d_res, d_resp are untouched and the counters are 0):
 *   EWAL_E_INVAL  group >= G; two messages naming the same group; an entry
 *                 range outside n_ents_total, or one that wraps; terms_off +
 *                 terms_cap outside n_terms, or wrapping; nlog > terms_cap
 *                 (INVAL wins over NOMEM when both occur in one call)
 *   EWAL_E_NOMEM  a message's group has nlog + n_ents > terms_cap (exact
 *                 enough: an append leaves at most index + 1 - log_offset +
 *                 n_ents <= nlog + n_ents entries, whatever ci is)
 * and on the host: EWAL_E_INVAL for a NULL ctx, for d_groups, d_apps, d_res
 * NULL (or d_terms / d_ents NULL with a non-zero count) while n > 0, for
 * d_groups, d_apps, d_res, d_resp not 16-byte aligned or d_terms not 8-byte
 * aligned, and for n or G >= 2^31 - 1.  n == 0: EWAL_OK, counters 0.
 * *n_accepted = messages accepted, *n_appended = entries appended (both
 * nullable).  A compute call on the ctx's stream (ewal_ctx_set_stream) like
 * the others; a repeated call of the same or a smaller shape allocates
 * nothing. */
struct emsg_out;
int elog_append_batch_device(ewal_ctx *ctx, elog_group *d_groups, uint64_t G,
                             uint64_t *d_terms, uint64_t n_terms,
                             const elog_app *d_apps, uint64_t n,
                             const ewal_entry *d_ents, uint64_t n_ents_total,
                             elog_app_result *d_res,
                             struct emsg_out *d_resp /* nullable, n; emsg_out is declared below */,
                             uint64_t *n_accepted, uint64_t *n_appended);
/* For bindings / tests: sizeof(elog_group), sizeof(elog_app),
 * sizeof(elog_app_result), and the longest message (in entries) the
 * lane-per-message kernel takes -- longer ones go to the wave-per-message
 * kernel. */
uint32_t elog_group_size(void);
uint32_t elog_app_size(void);
uint32_t elog_app_result_size(void);
uint32_t elog_lane_max_entries(void);

/* ---- leader msgAppResp step: stepLeader's msgAppResp case, raft/raft.go:456-466
 * Batched over n msgAppResp for the leaders of G raft groups: the term switch
 * of Step (raft.go:393-405), progress.update / maybeDecrTo (:71-90),
 * raft.maybeCommit (:248-258 with raft/log.go:148-154) and sendAppend /
 * bcastAppend (:202-236 with needSnapshot :556-564, send :190-199 and
 * raftLog.term / entries / at / slice, log.go:119-134, 194-217).  What the
 * follower append leaves as msgAppResp comes in; progress, commit and the next
 * fan-out's msgApp / msgSnap, as emsg_out records that
 * emsg_encode_batch_device takes directly, come out.  The log of group g is
 * the ewal_entry range d_ents[ents_first, + nlog): only its terms are read (an
 * entry's own index field is not looked at) and d_ents is never written.  All
 * arithmetic is Go's uint64 and wraps. */
/* leader state of one raft group; a DEVICE array of G, updated in place */
typedef struct elead_group {       /* 256 bytes */
  uint64_t id, term;               /* raft.id, raft.Term */
  uint64_t committed;              /* raftLog.committed              (updated) */
  uint64_t log_offset, nlog;       /* raftLog.offset, len(raftLog.ents) */
  uint64_t ents_first;             /* raftLog.ents[k] is d_ents[ents_first + k] (ewal_entry) */
  uint64_t n_peers;                /* len(r.prs), the leader itself included: 0..7 */
  uint64_t peer_id[7];             /* the keys of r.prs */
  uint64_t match[7], next[7];      /* Progress.match / .next         (updated) */
  uint64_t reserved[4];            /* 0 */
} elead_group;
/* raftLog.snapshot of group g; read only when a msgSnap is sent.  The fields
 * mean what the snap_* fields of emsg_out mean. */
typedef struct elead_snap {        /* 64 bytes */
  uint64_t index, term, data_off, data_len, nodes_off, n_nodes, removed_off, n_removed;
} elead_snap;
/* one msgAppResp; a DEVICE array of n */
typedef struct elead_resp {        /* 48 bytes */
  uint64_t group;                  /* which elead_group steps it */
  uint64_t from, term, index;      /* m.From, m.Term, m.Index */
  int32_t reject, pad;             /* m.Reject */
  uint64_t pad2;
} elead_resp;
/* what response i did */
enum {
  ELEAD_NOT_STEPPED = 0,  /* after a step-down or a panic in its group's run: the caller's to step */
  ELEAD_IGNORED = 1,      /* 0 < m.Term < r.Term */
  ELEAD_STEP_DOWN = 2,    /* m.Term > r.Term: becomeFollower is the caller's */
  ELEAD_STALE = 3,        /* a reject that maybeDecrTo refuses */
  ELEAD_PROBE = 4,        /* a reject: next decremented, one sendAppend(from) */
  ELEAD_UPDATED = 5,      /* update(index), maybeCommit false */
  ELEAD_COMMITTED = 6,    /* update(index), maybeCommit true, bcastAppend */
  ELEAD_PANICKED = 7      /* Go panics (status says where), or the group is unsupported */
};
typedef struct elead_result {      /* 48 bytes; a DEVICE array of n */
  int32_t status;                  /* EWAL_OK, an EWAL_PANIC_ class, EWAL_UNSUPPORTED_ENCODING */
  int32_t action;                  /* ELEAD_* */
  uint64_t msg_first, n_msgs;      /* its messages: d_msgs[msg_first, + n_msgs) */
  uint64_t committed;              /* raftLog.committed after this response */
  uint64_t match, next;            /* prs[from] after this response (0, 0 when there is none) */
} elead_result;
/* Order.  Responses that name the same group must be adjacent in d_resps; they
 * are stepped in array order, each one seeing the state the previous one left
 * (a leader of F followers gets up to F responses a round -- the follower
 * call takes one message per group, this one a run per group).  A run may be
 * of any length and lie anywhere in the array.
 * Per response (Step, then stepLeader's msgAppResp case):
 *   m.Term == 0 or == group.term: stepped (below).
 *   m.Term < group.term: ELEAD_IGNORED, nothing else happens.
 *   m.Term > group.term: ELEAD_STEP_DOWN.  The record is not touched and there
 *     are no messages: the caller runs becomeFollower (and reset) on the host.
 *     Every later response of that group in this call is ELEAD_NOT_STEPPED,
 *     has no effect, and is the caller's to step afterwards.
 *   removed[m.From] and msgDenied (raft.go:376-387) are the caller's routing
 *     and are not restated: such messages must not be handed to this call
 *     (econf_gate_batch_device, below, filters d_resps by removed[from]).
 *   reject != 0: maybeDecrTo(index) is false when match != 0 or next - 1 !=
 *     index: ELEAD_STALE, no message.  Otherwise next = next - 1, or 1 when
 *     that is 0: ELEAD_PROBE and one sendAppend(from).
 *   reject == 0: update(index): match = index, next = index + 1.  Then
 *     maybeCommit: mci = the q-th largest of the n_peers match values, q =
 *     n_peers / 2 + 1; when mci > committed and raftLog.term(mci) ==
 *     group.term, committed = mci: ELEAD_COMMITTED and bcastAppend, one
 *     sendAppend per peer slot whose peer_id != id, in slot order (Go's map
 *     order is unspecified; slot order is this library's).  Else ELEAD_UPDATED.
 * sendAppend(to) writes one emsg_out: to, from = id, term = group.term, index
 * = next - 1 of that peer, and
 *   index < log_offset (needSnapshot): type = 7 (msgSnap), the eight snap_*
 *     fields copied from d_snaps[g], every other field 0;
 *   otherwise type = 3 (msgApp), log_term = raftLog.term(next - 1) (0 when out
 *     of bounds), commit = committed, Entries = raftLog.entries(next) =
 *     slice(next, lastIndex + 1) as ents_first = group.ents_first + (next -
 *     log_offset) and n_ents; a nil slice is ents_first = n_ents = 0; all
 *     snapshot fields 0.
 * Where Go panics the response gets a status:
 *   EWAL_PANIC_NIL_PROGRESS   from is not among the first n_peers peer_id
 *   EWAL_PANIC_NEED_SNAPSHOT  needSnapshot with d_snaps[g].term == 0, or
 *                             d_snaps == NULL
 *   EWAL_PANIC_FIRST_ENTRY    entries(i) with i == log_offset
 *   EWAL_PANIC_BOUNDS         at / slice index past ents (only when nlog - 1 +
 *                             log_offset wrapped)
 * and a group with n_peers > 7 gives EWAL_UNSUPPORTED_ENCODING in the same
 * way: reported, never guessed.  Such a response -- wherever it panics, the
 * k-th message of a broadcast included -- has action ELEAD_PANICKED, emits no
 * message, leaves the record exactly as it was before that response, reports
 * the unchanged committed and prs[from], and puts the rest of its group's run
 * at ELEAD_NOT_STEPPED.  Responses stepped before it keep their effect.
 * d_res[i].match / next are prs[from] after the response for every action (0,
 * 0 when from is not a key, or the group is unsupported); msg_first is the
 * number of messages of the responses before i, also when n_msgs == 0.
 * Output placement.  The messages are dense and deterministic, ordered by
 * response, then by peer slot; *n_msgs is their number, *n_committed the
 * number of ELEAD_COMMITTED responses (both nullable).  No emsg_out at or
 * past *n_msgs is written; no word of a group that no response names is
 * written; only committed, match[] and next[] of a named group may change.
 * d_msgs == NULL is a size query: *n_msgs, *n_committed and d_res (msg_first
 * and n_msgs included) are filled and no group is modified.
 * Checked on the device before anything is modified (then d_groups, d_res and
 * d_msgs are untouched and the counters are 0):
 *   EWAL_E_INVAL  group >= G; a group's responses not adjacent; ents_first +
 *                 nlog outside n_ents_total, or wrapping; two equal peer_id
 *                 within the first min(n_peers, 7) slots of a named group;
 *                 reserved != 0 in a named group
 *   EWAL_E_NOMEM  the number of messages is greater than msgs_cap (INVAL wins
 *                 when both occur in one call)
 * and on the host: EWAL_E_INVAL for a NULL ctx, for d_groups, d_resps, d_res
 * NULL (or d_ents NULL with a non-zero count) while n > 0, for d_groups,
 * d_snaps, d_resps, d_res, d_msgs not 16-byte aligned or d_ents not 8-byte
 * aligned, and for n or G >= 2^31 - 1.  n == 0: EWAL_OK, counters 0.
 * A compute call on the ctx's stream (ewal_ctx_set_stream) like the others;
 * ewal_last_device_ms covers it; a repeated call of the same or a smaller
 * shape allocates nothing. */
int elead_step_batch_device(ewal_ctx *ctx, elead_group *d_groups, uint64_t G,
                            const elead_snap *d_snaps /* G, nullable */,
                            const ewal_entry *d_ents, uint64_t n_ents_total,
                            const elead_resp *d_resps, uint64_t n,
                            elead_result *d_res,
                            struct emsg_out *d_msgs /* NULL: size query */, uint64_t msgs_cap,
                            uint64_t *n_msgs, uint64_t *n_committed);
/* For bindings / tests: the sizes of the four records. */
uint32_t elead_group_size(void);
uint32_t elead_snap_size(void);
uint32_t elead_resp_size(void);
uint32_t elead_result_size(void);

/* ---- leader msgProp / msgBeat step: stepLeader's msgProp and msgBeat cases,
 * raft/raft.go:441-455.  Batched over n local messages for the leaders of G
 * raft groups -- the step that starts a replication round: appendEntry
 * (:279-285) with raftLog.append (raft/log.go:71-75), progress.update
 * (:71-74) and maybeCommit (:248-258), then bcastAppend (:229-236); and
 * bcastHeartbeat / sendHeartbeat (:219-226, :238-246).  Client proposals and
 * heartbeat ticks (etick_batch_device's d_beats, below, as they lie) come in; the grown log (d_ents is WRITTEN here, and only
 * here), progress, commit and the fan-out's emsg_out records come out.  The
 * groups are elead_step_batch_device's elead_group records, unchanged, so the
 * same array feeds both calls; what a proposal needs beyond them lives in a
 * side array.  All arithmetic is Go's uint64 and wraps. */
typedef struct elead_prop_state {   /* 32 bytes; a DEVICE array of G, updated in place */
  uint64_t ents_cap;      /* room at elead_group.ents_first, in entries (>= nlog) */
  uint64_t unstable;      /* raftLog.unstable                        (updated) */
  uint64_t pending_conf;  /* raft.pendingConf, 0 or 1                (updated) */
  uint64_t reserved;      /* 0 */
} elead_prop_state;
typedef struct elead_local {        /* 48 bytes; one local message; a DEVICE array of n */
  uint64_t group;                   /* which elead_group steps it */
  uint64_t kind;                    /* 1 = msgBeat, 2 = msgProp (raft.go:17-27) */
  int32_t etype, data_nil;          /* msgProp: Entries[0].Type, and whether Data is nil */
  uint64_t data_off, data_len;      /* Entries[0].Data = d_data[data_off, + data_len) */
  uint64_t pad;
} elead_local;
enum { ELEAD_L_NOT_STEPPED = 0,     /* after a panic in its group's run: the caller's to step */
       ELEAD_L_BEAT = 1,            /* msgBeat: bcastHeartbeat */
       ELEAD_L_APPENDED = 2,        /* msgProp: appendEntry, bcastAppend */
       ELEAD_L_DROPPED = 3,         /* msgProp: a ConfChange while pendingConf */
       ELEAD_L_PANICKED = 4 };      /* Go panics (status says where), or the group is unsupported */
typedef struct elead_local_result { /* 48 bytes; a DEVICE array of n */
  int32_t status, action;           /* EWAL_OK, an EWAL_PANIC_ class, EWAL_UNSUPPORTED_ENCODING; ELEAD_L_* */
  uint64_t msg_first, n_msgs;       /* its messages: d_msgs[msg_first, + n_msgs) */
  uint64_t index;                   /* the Index given to the entry (0 unless APPENDED) */
  uint64_t ent_pos;                 /* where it was written in d_ents   (0 unless APPENDED) */
  uint64_t committed;               /* raftLog.committed after this record */
} elead_local_result;
/* Order, output placement, the size query (d_msgs == NULL), the stream, the
 * timing and the allocation rule are elead_step_batch_device's, with "record"
 * for "response": a group's records are adjacent and stepped in array order,
 * runs have any length and lie anywhere, the messages are dense and ordered by
 * record, then by peer slot, msg_first counts the messages of the records
 * before i also when n_msgs == 0, and no emsg_out at or past *n_msgs is
 * written.  *n_appended = the ELEAD_L_APPENDED records (nullable, as *n_msgs).
 * Proposals carry Term == 0 (send, raft.go:190-199), so Step's term switch is
 * "local message"; removed[] / msgDenied routing stays the caller's
 * (econf_gate_batch_device with ECONF_FROM_SELF, below).
 * Per record:
 *   kind 1 (msgBeat): one emsg_out per peer slot whose peer_id != id, in slot
 *     order: type = 3 (sendHeartbeat's empty msgApp), to, from = id, term =
 *     group.term, every other field 0.  ELEAD_L_BEAT; nothing else changes.
 *   kind 2 (msgProp), e = Entries[0]:
 *     etype == 1 (EntryConfChange) while pending_conf != 0: ELEAD_L_DROPPED,
 *       nothing else happens.  Otherwise a ConfChange sets pending_conf = 1.
 *     appendEntry: e.Term = group.term, e.Index = lastIndex() + 1 (lastIndex =
 *       nlog - 1 + log_offset).  raftLog.append(lastIndex(), e) is ents =
 *       append(slice(log_offset, lastIndex() + 1), e): where that slice is nil
 *       -- an empty log, or nlog - 1 + log_offset or lastIndex() + 1 wrapping
 *       -- THE LOG BECOMES THE ONE NEW ENTRY (nlog = 1), as in Go; otherwise
 *       nlog grows by one.  unstable = min(unstable, e.Index).  Then
 *       prs[id].update(lastIndex()) and maybeCommit, as in
 *       elead_step_batch_device, its result ignored.
 *     bcastAppend, always: one sendAppend per peer slot whose peer_id != id,
 *       in slot order, bit for bit the records elead_step_batch_device
 *       documents (msgSnap from d_snaps, log_term, commit, and the ents_first /
 *       n_ents range, which now ends with the new entry).  ELEAD_L_APPENDED.
 *     The entry is stored at d_ents[ents_first + k], k its position in the new
 *       log: {term, index, data_off, data_len, type = etype, data_nil};
 *       d_res[i].index and .ent_pos (= ents_first + k) name it.
 * Written: of a named group committed, nlog, match[] and next[] (of prs[id]
 * only); of its state record unstable and pending_conf; the appended d_ents
 * slots; d_res; d_msgs below *n_msgs.  Nothing of a group that no record
 * names, and no entry of the log as the call found it, except slot 0 in the
 * nil-slice case above.
 * Where Go panics the record gets a status:
 *   EWAL_PANIC_NIL_PROGRESS   a proposal for a group whose id is not among
 *                             the first n_peers peer_id (prs[r.id] is nil)
 *   EWAL_PANIC_NEED_SNAPSHOT, EWAL_PANIC_FIRST_ENTRY, EWAL_PANIC_BOUNDS
 *                             in the broadcast or in maybeCommit's term(), as
 *                             in elead_step_batch_device
 * and the first record (of either kind) of a group with n_peers > 7 gets
 * EWAL_UNSUPPORTED_ENCODING in the same way.  Such a record -- wherever it
 * panics, the k-th message of the broadcast included -- has action
 * ELEAD_L_PANICKED, emits nothing, leaves the group record, the state record
 * and d_ents exactly as they were before that record, reports the unchanged
 * committed, and puts the rest of its group's run at ELEAD_L_NOT_STEPPED.
 * Records stepped before it keep their effect.  A msgBeat cannot panic.
 * Checked on the device before anything is modified (then d_groups, d_state,
 * d_ents, d_res and d_msgs are untouched and the counters are 0):
 *   EWAL_E_INVAL  group >= G; a group's records not adjacent; kind not 1 or 2;
 *                 data_nil not 0 or 1 (either kind); a proposal's Data range
 *                 outside data_len_total, or wrapping; and of a named group:
 *                 ents_first + ents_cap outside n_ents_total, or wrapping;
 *                 nlog > ents_cap; two equal peer_id within the first
 *                 min(n_peers, 7) slots; reserved != 0 in the group or the
 *                 state record; pending_conf > 1
 *   EWAL_E_NOMEM  a named group has nlog + (the kind-2 records of its run) >
 *                 ents_cap (dropped proposals count: the room is decided
 *                 before any is stepped); or the messages exceed msgs_cap
 *                 (INVAL wins when both occur in one call)
 * and on the host as in elead_step_batch_device, d_state sharing d_groups'
 * rules.  n == 0: EWAL_OK, counters 0.
 * The entry windows [ents_first, + ents_cap) of the named groups must not
 * overlap each other: the caller's contract, not checked.  The free slots of
 * a window are never read here, but emsg_encode_batch_device checks every
 * entry of the d_ents it is given: keep them zero when d_ents goes there. */
int elead_local_batch_device(ewal_ctx *ctx, elead_group *d_groups, elead_prop_state *d_state, uint64_t G,
                             const elead_snap *d_snaps /* G, nullable */,
                             ewal_entry *d_ents, uint64_t n_ents_total, uint64_t data_len_total,
                             const elead_local *d_locals, uint64_t n, elead_local_result *d_res,
                             struct emsg_out *d_msgs /* NULL: size query */, uint64_t msgs_cap,
                             uint64_t *n_msgs, uint64_t *n_appended);
/* For bindings / tests: the sizes of the three records. */
uint32_t elead_prop_state_size(void);
uint32_t elead_local_size(void);
uint32_t elead_local_result_size(void);

/* ---- election step: raft.Step for msgHup, msgVote and msgVoteResp,
 * raft/raft.go:372-408.  Batched over n election messages for G raft groups --
 * the round that gives a restarted host its leaders: the msgVote case of
 * stepFollower / stepCandidate / stepLeader (:467-468, :482-483, :511-518),
 * stepCandidate's msgVoteResp case (:484-492), campaign (:358-370), poll
 * (:177-187), reset (:260-273), becomeFollower / becomeCandidate / becomeLeader
 * (:309-349) and raftLog.isUpToDate (raft/log.go:136-139).  A group is its
 * elead_group plus its elead_prop_state, both unchanged (the same arrays feed
 * the three leader-side calls; elead_group.reserved stays 0), plus the side
 * record below.  becomeLeader's empty entry is appended to d_ents and the
 * winner's bcastAppend comes out as emsg_out records, as
 * elead_local_batch_device would write them; msgVote and msgVoteResp come out
 * as emsg_out records too.  All arithmetic is Go's uint64 and wraps; None is 0. */
typedef struct evote_state {        /* 64 bytes; a DEVICE array of G, updated in place */
  uint64_t state;                   /* raft.state: 0 follower, 1 candidate, 2 leader (Go's StateType) */
  uint64_t vote;                    /* HardState.Vote */
  uint64_t lead;                    /* raft.lead */
  uint64_t elapsed;                 /* raft.elapsed: Go's int as its bits; etick_batch_device counts it */
  uint64_t voted;                   /* bit s: r.votes has the key peer_id[s] */
  uint64_t granted;                 /* bit s: that value is true (a subset of voted) */
  uint64_t reserved[2];             /* 0 */
} evote_state;
typedef struct evote_msg {          /* 64 bytes; one message; a DEVICE array of n */
  uint64_t group;                   /* which group steps it */
  uint64_t kind;                    /* 0 = msgHup, 5 = msgVote, 6 = msgVoteResp (raft.go:17-34) */
  uint64_t from, term, index, log_term;   /* m.From, m.Term, m.Index, m.LogTerm */
  int32_t reject, pad;              /* m.Reject; 0 */
  uint64_t pad2;                    /* 0 */
} evote_msg;
enum { EVOTE_NOT_STEPPED = 0,       /* after a panic in its group's run: the caller's to step */
       EVOTE_IGNORED = 1,           /* 0 < m.Term < r.Term */
       EVOTE_GRANTED = 2,           /* msgVote: the vote was granted */
       EVOTE_REJECTED = 3,          /* msgVote: a rejecting msgVoteResp was sent */
       EVOTE_CAMPAIGNED = 4,        /* msgHup: became candidate, msgVote sent */
       EVOTE_WON = 5,               /* became leader */
       EVOTE_LOST = 6,              /* the rejecting quorum: becomeFollower(r.Term, None) */
       EVOTE_POLLED = 7,            /* msgVoteResp counted, no decision */
       EVOTE_NO_CASE = 8,           /* msgVoteResp at a follower or leader: the step function has no case */
       EVOTE_PANICKED = 9 };        /* Go panics (status says where), or the record is unsupported */
typedef struct evote_result {       /* 48 bytes; a DEVICE array of n */
  int32_t status, action;           /* EWAL_OK, an EWAL_PANIC_ class, EWAL_UNSUPPORTED_ENCODING; EVOTE_* */
  uint64_t msg_first, n_msgs;       /* its messages: d_msgs[msg_first, + n_msgs) */
  uint64_t term, vote;              /* raft.Term and Vote after this record */
  int32_t state;                    /* raft.state after this record */
  int32_t flags;                    /* bit 0: Step's term switch ran becomeFollower before the case */
} evote_result;
/* Order, output placement, the size query (d_msgs == NULL), the stream, the
 * timing and the allocation rule are elead_step_batch_device's, with "record"
 * for "response": a group's records are adjacent and stepped in array order,
 * each one seeing the state the previous one left (two candidates' msgVote in
 * one run is the normal case), runs have any length and lie anywhere, the
 * messages are dense and ordered by record, then by peer slot, msg_first counts
 * the messages of the records before i also when n_msgs == 0, and no emsg_out
 * at or past *n_msgs is written.  *n_won = the EVOTE_WON records (nullable, as
 * *n_msgs).  removed[] / msgDenied routing (raft.go:376-387) and the deferred
 * r.Commit copy stay the caller's (the routing is econf_gate_batch_device's and
 * econf_batch_device's kind 3, below).
 * Per record, in Go's order:
 *   kind 0 (msgHup) runs campaign() first (below); tickElection's come from
 *     etick_batch_device's d_hups (below) as they lie.  A msgHup is a local
 *     message: raft builds it with Term 0 (raft.go:296) and node.Step drops one
 *     that arrives over the network (node.go:281-284), so the record's from,
 *     term, index and log_term are not read and the term switch below is the
 *     m.Term == 0 case whatever they hold.
 *   The term switch: m.Term == 0 is a local message; m.Term > r.Term runs
 *     becomeFollower(m.Term, lead) with lead = None for a msgVote and m.From
 *     for a msgVoteResp (Go's quirk, kept) and sets flags bit 0; m.Term <
 *     r.Term is EVOTE_IGNORED and nothing else happens.
 *   Then the case of the state the group is in NOW.
 * reset(term) writes Term = term, lead = vote = elapsed = 0, voted = granted =
 *   0, for every peer slot match = 0 and next = lastIndex() + 1 (lastIndex =
 *   nlog - 1 + log_offset), match = lastIndex() for the slot whose peer_id ==
 *   id (if any), and pending_conf = 0.  becomeFollower then sets lead and
 *   state = 0.
 * msgVote at a follower: Go's short circuit is kept -- isUpToDate is evaluated
 *   only when vote == 0 or vote == from.  It dereferences at(lastIndex()):
 *   where that is nil (an empty log at a non-zero offset, or nlog - 1 +
 *   log_offset wrapped) the status is EWAL_PANIC_NIL_ENTRY; an empty log at
 *   offset 0 passes isOutOfBounds and indexes past ents: EWAL_PANIC_BOUNDS.
 *   Granted when log_term > the last entry's term, or equal with index >=
 *   lastIndex(): elapsed = 0, vote = from, one emsg_out {type 6, to = from,
 *   from = id, term = r.Term}, EVOTE_GRANTED.  Otherwise the same message with
 *   reject = 1, EVOTE_REJECTED.  A candidate or a leader (at an equal term, or
 *   for a local message) always rejects.
 * msgHup: at a leader EWAL_PANIC_LEADER_TO_CANDIDATE (checked first).  A group
 *   whose id is not among its first n_peers peer_id gets
 *   EWAL_UNSUPPORTED_ENCODING: it is not promotable (tickElection never sends
 *   the message) and its self vote has no slot -- reported, never guessed.
 *   Otherwise becomeCandidate: reset(Term + 1), vote = id, state = 1; then
 *   poll(id, true).  With q() = n_peers / 2 + 1 == 1 becomeLeader runs (there is
 *   nobody to broadcast to): EVOTE_WON.  Otherwise EVOTE_CAMPAIGNED and one
 *   emsg_out {type 5, to, from = id, term, index = lastIndex(), log_term =
 *   term(lastIndex())} per peer slot whose peer_id != id, in slot order
 *   (term() on an empty log at offset 0: EWAL_PANIC_BOUNDS).
 * msgVoteResp at a candidate: poll(from, !reject) -- only the first answer of
 *   a from counts; gr = popcount(granted), len(votes) = popcount(voted).  A from
 *   that is not among the peer slots gets EWAL_UNSUPPORTED_ENCODING (Go would
 *   count it; the mask cannot).  q() == gr is tested first: becomeLeader, then
 *   bcastAppend, EVOTE_WON.  Else q() == len(votes) - gr:
 *   becomeFollower(Term, None), EVOTE_LOST.  Else EVOTE_POLLED.  At a follower
 *   or a leader: EVOTE_NO_CASE (possibly after the term switch).
 * becomeLeader: reset(Term), lead = id, state = 2.  Then the scan of
 *   entries(committed + 1): committed + 1 == log_offset is
 *   EWAL_PANIC_FIRST_ENTRY; a nil slice is no scan; one entry of d_ents with
 *   type == 1 (EntryConfChange) sets pending_conf = 1, a second one is
 *   EWAL_PANIC_DOUBLE_CONF.  Then appendEntry(Entry{}) exactly as
 *   elead_local_batch_device documents a msgProp: the entry is stored as
 *   {term, index, 0, 0, type 0, data_nil 1}, the nil-slice case "the log
 *   becomes the one new entry" included, with unstable = min(unstable, index),
 *   prs[id].update and maybeCommit (EWAL_PANIC_NIL_PROGRESS when a candidate's
 *   id is not among its peers).  The winner's bcastAppend is bit for bit
 *   elead_step_batch_device's sendAppend records, msgSnap included, with its
 *   panics.
 * A panicking or unsupported record -- wherever it panics, after a reset or in
 * the k-th message of a broadcast -- has action EVOTE_PANICKED, emits nothing,
 * leaves all three records and d_ents exactly as they were before that record,
 * reports the unchanged term, vote and state with flags 0, and puts the rest
 * of its group's run at EVOTE_NOT_STEPPED.  Records stepped before it keep
 * their effect.  The first record of a group with n_peers > 7 gets
 * EWAL_UNSUPPORTED_ENCODING in the same way.
 * Written: of a named group term, committed, nlog, match[] and next[]; of its
 * elead_prop_state unstable and pending_conf; of its evote_state everything
 * but reserved; becomeLeader's d_ents slots; d_res; d_msgs below *n_msgs.  Only
 * the words that changed are stored.  Nothing of a group that no record names.
 * Checked on the device before anything is modified (then the three group
 * arrays, d_ents, d_res and d_msgs are untouched and the counters are 0):
 *   EWAL_E_INVAL  group >= G; a group's records not adjacent; kind not 0, 5 or
 *                 6; reject not 0 or 1; pad or pad2 not 0; and of a named
 *                 group: evote_state.state > 2; voted or granted with bits at
 *                 or above min(n_peers, 7); granted & ~voted != 0; a reserved
 *                 word not 0 in any of its three records; and the group and
 *                 window checks of elead_local_batch_device
 *   EWAL_E_NOMEM  a named group has nlog + (the kind-0 and kind-6 records of
 *                 its run) > ents_cap (the room is decided before any record
 *                 is stepped); or the messages exceed msgs_cap (INVAL wins
 *                 when both occur in one call)
 * and on the host as in elead_local_batch_device, d_pstate and d_vstate
 * sharing d_groups' rules.  n == 0: EWAL_OK, counters 0.  The entry windows of
 * the named groups must not overlap each other: the caller's contract. */
int evote_step_batch_device(ewal_ctx *ctx, elead_group *d_groups, elead_prop_state *d_pstate,
                            evote_state *d_vstate, uint64_t G, const elead_snap *d_snaps /* G, nullable */,
                            ewal_entry *d_ents, uint64_t n_ents_total,
                            const evote_msg *d_in, uint64_t n, evote_result *d_res,
                            struct emsg_out *d_msgs /* NULL: size query */, uint64_t msgs_cap,
                            uint64_t *n_msgs, uint64_t *n_won);
/* For bindings / tests: the sizes of the three records. */
uint32_t evote_state_size(void);
uint32_t evote_msg_size(void);
uint32_t evote_result_size(void);

/* ---- Ready: newReady (raft/node.go:332-348), node.run's accept branch
 * (:239-255) and Storage.Save's record order (wal/wal.go:281-288, called
 * before any message is sent, etcdserver/server.go:256-259).  Batched over n
 * selected groups of G -- the joint between the step calls above and the write
 * side: what the steps left in elead_group, elead_prop_state and evote_state
 * comes in; per group a Ready (the HardState, the unstable entries and the
 * newly committed entries as views of d_ents, the SoftState, whether a
 * snapshot appeared) and the ewal_save_rec records that ewal_save_device takes
 * directly come out, and the group is advanced as the accept branch does.  The
 * three step records are unchanged (the same arrays feed every call); what
 * node.run keeps in locals and raftLog.applied live in the side record below.
 * All arithmetic is Go's uint64 and wraps; lastIndex = nlog - 1 + log_offset. */
typedef struct eready_state {       /* 64 bytes; a DEVICE array of G, updated in place */
  uint64_t hs_term, hs_vote, hs_commit;  /* prevHardSt (node.go:196, 243-245) */
  uint64_t lead, state;             /* prevSoftSt.Lead / .RaftState (node.go:195, 240-242) */
  uint64_t snapi;                   /* prevSnapi (node.go:197, 246-248) */
  uint64_t applied;                 /* raftLog.applied (log.go:17, 109-113) */
  uint64_t soft_dirty;              /* 0 or 1, see below */
} eready_state;
#define EREADY_SOFT 1
#define EREADY_HARD 2
#define EREADY_SNAP 4
#define EREADY_UPDATES 8
typedef struct eready_result {      /* 96 bytes; a DEVICE array of n */
  int32_t status;                   /* EWAL_OK, EWAL_PANIC_BOUNDS, EWAL_UNSUPPORTED_ENCODING */
  int32_t flags;                    /* EREADY_SOFT=1, EREADY_HARD=2, EREADY_SNAP=4, EREADY_UPDATES=8 */
  uint64_t term, vote, commit;      /* rd.HardState: all 0 when there is no update */
  uint64_t ents_first, n_ents;      /* rd.Entries as a view of d_ents; nil is 0, 0 */
  uint64_t committed_first, n_committed;   /* rd.CommittedEntries, likewise */
  uint64_t save_first, n_save;      /* this group's records in d_save */
  uint64_t lead;                    /* rd.SoftState (valid when EREADY_SOFT, else 0) */
  int32_t state, pad;
} eready_result;
/* Selection i is group d_sel[i], or group i when d_sel == NULL (then n == G).
 * Per selected group, in Go's order:
 *   rd.Entries = unstableEnts() = slice(unstable, lastIndex + 1) (raft/log.go:
 *     86-94, 202-210): nil when lo >= hi (lastIndex + 1 wrapping to 0 included)
 *     or isOutOfBounds holds for either end; otherwise the view ents_first +
 *     (unstable - log_offset), n_ents = lastIndex + 1 - unstable.
 *   rd.CommittedEntries = nextEnts() (log.go:102-107): nil unless committed >
 *     applied, then slice(applied + 1, committed + 1) with the same nil rules.
 *   A slice that passes both isOutOfBounds tests but indexes past ents (only a
 *     wrapped nlog - 1 + log_offset gets there) is EWAL_PANIC_BOUNDS.
 *   rd.HardState: r.HardState is {group.term, vstate.vote, group.committed} --
 *     every Step ends with r.Commit = raftLog.committed (raft/raft.go:374), the
 *     copy the step calls leave to the caller: it lands here.  StartNode's
 *     window before the first Step (node.go:141-142 set committed without it)
 *     is the caller's: it seeds hs_* from the HardState it restored, not from
 *     the log.  rd.HardState is that triple when it differs from hs_*, else
 *     zero; EREADY_HARD iff it is not the empty state.  Go's quirk is kept: a
 *     differing but all-zero HardState looks like "no update" and is never
 *     accepted (node.go:243).
 *   rd.SoftState (EREADY_SOFT): vstate.lead != lead, vstate.state != state, or
 *     soft_dirty == 1.  SoftState.Nodes and ShouldStop change only through
 *     addNode / removeNode / msgDenied, the caller's on the host: after any of
 *     them it sets soft_dirty (econf_batch_device, below, is all three on the
 *     device and sets it itself).  Go compares Nodes with reflect.DeepEqual over a
 *     slice built in map order, so with two or more peers Go's own answer is
 *     not deterministic; that is NOT reproduced -- the library's order is slot
 *     order, as everywhere else.
 *   rd.Snapshot: raftLog.snapshot.Index is d_snaps[g].index (0 when d_snaps ==
 *     NULL); EREADY_SNAP iff it differs from snapi and is not 0.  The snapshot
 *     is d_snaps[g]; saving it is esnap_save_*'s job and the caller's.  On the
 *     device d_snaps[g] is written by a follower's restore and by
 *     ecompact_batch_device (below): after a compaction the next call here
 *     reports EREADY_SNAP on its own.
 *   EREADY_UPDATES = containsUpdates() without its Messages term (node.go:
 *     83-86): the messages are the step calls' emsg_out output, the caller
 *     knows their count, and accepting a group that has only messages changes
 *     nothing.
 * Storage.Save(rd.HardState, rd.Entries) as ewal_save_rec records, per group:
 *   one EWAL_SAVE_STATE {a = term, b = vote, c = commit} iff EREADY_HARD
 *   (SaveState skips the empty state), then one EWAL_SAVE_ENTRY per entry of
 *   rd.Entries in order {etype = type, a = term, b = index, c = 0, data_off,
 *   data_len and data_nil copied, pad 0}.  The dummy entry at position 0 is
 *   saved when unstable == 0, as Go does.  The records are dense, ordered by
 *   selection position, then as above; save_first counts the records of the
 *   selections before it also when n_save == 0; nothing at or past *n_save is
 *   written.  One ewal_save_device call is one CRC chain: the groups'
 *   [save_first, + n_save) ranges are how a caller with one WAL per group cuts
 *   d_save.  An unstable entry with data_nil == 2 has its bytes outside d_data:
 *   the group gets EWAL_UNSUPPORTED_ENCODING -- reported, never guessed.
 * Accept (only when d_save != NULL, only groups with status EWAL_OK):
 *   EREADY_SOFT: lead / state overwritten, soft_dirty = 0; EREADY_HARD: hs_*
 *   overwritten; EREADY_SNAP: snapi = index; resetNextEnts: applied =
 *   committed when committed > applied (also when the slice came out nil --
 *   Go's quirk); resetUnstable: elead_prop_state.unstable = lastIndex + 1.
 *   Only the words that changed are stored.
 * Written: d_rstate and elead_prop_state.unstable of accepted groups, d_res,
 * d_save below *n_save.  elead_group, evote_state, d_snaps and d_ents are
 * never written; groups not selected are not touched.  A panicking or
 * unsupported group has flags 0, every other result field but status and
 * save_first 0, no save records, and is left exactly as it was.
 * d_save == NULL is the peek and the size query: d_res, *n_save and *n_ready
 * are filled and nothing else is modified.  *n_ready = the groups with
 * EREADY_UPDATES (both counters nullable).
 * Not covered: entries that elog_append_batch_device appended into its own
 * d_terms windows (that call keeps terms only; a follower stepped by
 * efollow_step_batch_device, below, has its entries in d_ents and is covered),
 * and one chained save per group's own WAL (see save_first above).
 * Checked on the device before anything is modified (then every array is
 * untouched and the counters are 0):
 *   EWAL_E_INVAL  a selected group >= G; a group selected twice; state > 2 in
 *                 the evote_state or the eready_state; soft_dirty > 1;
 *                 elead_group.reserved, elead_prop_state.reserved or
 *                 evote_state.reserved not 0; ents_first + nlog outside
 *                 n_ents_total or wrapping
 *   EWAL_E_NOMEM  the save records exceed save_cap (INVAL wins when both occur)
 * and on the host: NULL arguments, d_groups / d_pstate / d_vstate / d_rstate /
 * d_snaps / d_res / d_save not 16-byte aligned, d_ents or d_sel not 8-byte
 * aligned, n or G >= 2^31 - 1, d_sel == NULL with n != G: EWAL_E_INVAL.  n ==
 * 0: EWAL_OK, counters 0.  A compute call on the ctx's stream;
 * ewal_last_device_ms covers it; a repeated call of the same or a smaller
 * shape allocates nothing. */
int eready_batch_device(ewal_ctx *ctx, const elead_group *d_groups, elead_prop_state *d_pstate,
                        const evote_state *d_vstate, eready_state *d_rstate, uint64_t G,
                        const elead_snap *d_snaps /* G, nullable */,
                        const ewal_entry *d_ents, uint64_t n_ents_total,
                        const uint64_t *d_sel /* n group numbers; NULL: n == G, group i */, uint64_t n,
                        eready_result *d_res,
                        ewal_save_rec *d_save /* NULL: peek */, uint64_t save_cap,
                        uint64_t *n_save, uint64_t *n_ready);
/* For bindings / tests: the sizes of the two records. */
uint32_t eready_state_size(void);
uint32_t eready_result_size(void);

/* ---- follower step: raft.Step for msgApp and msgSnap, raft/raft.go:372-408.
 * Batched over n messages for G raft groups -- the other N - 1 replicas' half
 * of a replication round, on the records the calls above share: Step's term
 * switch (:393-405), the msgApp and msgSnap cases of stepFollower (:504-510)
 * and stepCandidate (:476-481; stepLeader has none), handleAppendEntries
 * (:410-416), handleSnapshot (:418-424), raft.restore (:535-554) and, from
 * raft/log.go, maybeAppend, findConflict, append, matchTerm, at, slice,
 * isOutOfBounds, lastIndex and restore.  A group is its elead_group, its
 * elead_prop_state, its evote_state and (for a restore) its eready_state and
 * d_snaps[g]; its log is the window d_ents[ents_first, + ents_cap).  What the
 * leader-side calls emit as msgApp / msgSnap comes in; the grown or restored
 * log -- whole 40-byte entries, so eready_batch_device and ewal_save_device
 * take a follower as they take a leader -- and one msgAppResp per stepped
 * message, as emsg_out records that elead_step_batch_device's caller unpacks
 * or emsg_encode_batch_device marshals, come out.  All arithmetic is Go's
 * uint64 and wraps; lastIndex = nlog - 1 + log_offset. */
typedef struct efollow_msg {        /* 96 bytes; one message; a DEVICE array of n */
  uint64_t group;                   /* which group steps it */
  uint64_t kind;                    /* 3 = msgApp, 7 = msgSnap (raft.go:17-34) */
  uint64_t from, term, index, log_term, commit;   /* m.From, m.Term, m.Index, m.LogTerm, m.Commit */
  uint64_t ents_first, n_ents;      /* m.Entries = d_src[ents_first, + n_ents) (ewal_entry) */
  uint64_t data_delta;              /* added, wrapping, to data_off of every copied entry whose data_nil == 0:
                                       it rebases an ingress buffer into d_data */
  uint64_t snap;                    /* kind 7: m.Snapshot is d_in_snaps[snap] */
  uint64_t pad;                     /* 0 */
} efollow_msg;
enum { EFOLLOW_NOT_STEPPED = 0,     /* after a panic in its group's run: the caller's to step */
       EFOLLOW_IGNORED = 1,         /* 0 < m.Term < r.Term */
       EFOLLOW_NO_CASE = 2,         /* a leader (at an equal term, or for a local message): no case, no message */
       EFOLLOW_APPENDED = 3,        /* maybeAppend returned true, also with n_app == 0 */
       EFOLLOW_REJECTED = 4,        /* matchTerm failed: the response rejects */
       EFOLLOW_RESTORED = 5,        /* msgSnap: raft.restore returned true */
       EFOLLOW_SNAP_STALE = 6,      /* msgSnap: s.Index <= committed, restore returned false */
       EFOLLOW_DEFERRED = 7,        /* the run rule below: the caller's to step in the next call */
       EFOLLOW_PANICKED = 8 };      /* Go panics (status says where), or the record is unsupported */
typedef struct efollow_result {     /* 96 bytes; a DEVICE array of n */
  int32_t status, action;           /* EWAL_OK, an EWAL_PANIC_ class, EWAL_UNSUPPORTED_ENCODING; EFOLLOW_* */
  uint64_t msg_first, n_msgs;       /* its response: d_msgs[msg_first, + n_msgs), n_msgs 0 or 1 */
  uint64_t conflict;                /* findConflict's ci; 0: none */
  uint64_t app_first, n_app;        /* the entries appended: d_src[app_first, + n_app), a suffix of the
                                       message's range; 0, 0: nothing appended */
  uint64_t dst_first;               /* where they went: d_ents[dst_first, + n_app); 0 when n_app == 0 */
  uint64_t last_index, committed, term;   /* lastIndex(), raftLog.committed, raft.Term after this record */
  int32_t state;                    /* raft.state after this record */
  int32_t flags;                    /* bit 0: Step's term switch ran becomeFollower; bit 1: a candidate conceded */
  uint64_t pad;
} efollow_result;
/* Order, output placement, the size query (d_msgs == NULL), the stream, the
 * timing and the allocation rule are evote_step_batch_device's: a group's
 * records are adjacent and stepped in array order, each one seeing what the
 * previous one left, the responses are dense and ordered by record, msg_first
 * counts the responses of the records before i also when n_msgs == 0, and no
 * emsg_out at or past *n_msgs is written.  removed[] / msgDenied routing and
 * the deferred r.Commit copy stay the caller's (the routing is
 * econf_gate_batch_device's, below).
 * The run rule.  After a record of a run has appended entries (n_app > 0) or
 * restored, a later record of that run that carries entries (n_ents > 0) or is
 * a msgSnap is EFOLLOW_DEFERRED with status EWAL_OK, and so is the rest of the
 * run: no effect, no message, the caller's to step in the next call.  Records
 * without entries (heartbeats, commit-only msgApp) are stepped and see the
 * grown or restored log.
 * Per record, in Go's order:
 *   The term switch: m.Term == 0 is a local message; m.Term > r.Term runs
 *     becomeFollower(m.Term, m.From) -- reset as evote_step_batch_device
 *     documents it -- and sets flags bit 0; m.Term < r.Term is EFOLLOW_IGNORED.
 *   Then the case of the state the group is in NOW.
 *     follower, msgApp: elapsed = 0, lead = from, handleAppendEntries.
 *     follower, msgSnap: elapsed = 0, handleSnapshot; lead is NOT set (Go's
 *       quirk, kept).
 *     candidate, msgApp: becomeFollower(r.Term, from), flags bit 1, then
 *       handleAppendEntries.
 *     candidate, msgSnap: becomeFollower(m.Term, from), flags bit 1, then
 *       handleSnapshot; with m.Term == 0 this sets Term to 0 (Go's quirk, kept).
 *     leader: EFOLLOW_NO_CASE.
 *   handleAppendEntries: maybeAppend exactly as elog_append_batch_device
 *     documents it (matchTerm, findConflict by position,
 *     EWAL_PANIC_COMMITTED_CONFLICT, EWAL_PANIC_BOUNDS, committed =
 *     max(committed, min(commit, index + n_ents))), on the terms of d_ents.
 *     With ci > 0 the whole entries d_src[app_first + j] are copied to
 *     d_ents[ents_first + (ci - log_offset) + j], j < n_app, data_off rebased
 *     by data_delta where data_nil == 0 (an entry with data_nil == 2 is copied
 *     untouched: Ready reports it); nlog = ci - log_offset + n_app;
 *     elead_prop_state.unstable = min(unstable, ci).  One emsg_out {type 4, to
 *     = from, from = id, term = r.Term, index = lastIndex()}: EFOLLOW_APPENDED
 *     -- or index = m.Index with reject = 1: EFOLLOW_REJECTED.
 *   handleSnapshot, s = d_in_snaps[snap]: s.index <= committed is
 *     EFOLLOW_SNAP_STALE, the response carries index = committed.  Otherwise
 *     EFOLLOW_RESTORED: d_ents[ents_first] = {term: s.term, index 0, data 0/0,
 *     type 0, data_nil 1}, nlog = 1, log_offset = committed = s.index,
 *     unstable = s.index + 1, eready_state.applied = s.index, d_snaps[g] = s;
 *     prs is rebuilt from s.Nodes = d_u64[nodes_off, + n_nodes): the distinct
 *     ids take the slots in first-occurrence order, the slot whose id equals id
 *     gets (match, next) = (s.index, s.index + 1), the others (0, s.index + 1),
 *     the slots past them are zeroed; eready_state.soft_dirty = 1 iff n_peers
 *     or one of the first n_peers peer_id changed; pending_conf and the votes
 *     are untouched; the response carries index = lastIndex() = s.index.
 *     r.removed from RemovedNodes stays the caller's, as removed[] does
 *     everywhere: EFOLLOW_RESTORED tells it (econf_batch_device's kind 4,
 *     below, is that half on the device).
 *     The leader's d_snaps[g] that a msgSnap carries has a device-side writer
 *     too: ecompact_batch_device (below).
 * EWAL_UNSUPPORTED_ENCODING, reported, never guessed: the first record of a
 * group with n_peers > 7; a restore with n_nodes > 64 or more than 7 distinct
 * ids; a restore while evote_state.voted != 0 (unreachable in Go: every way of
 * becoming a follower resets the votes).
 * A panicking or unsupported record has action EFOLLOW_PANICKED, emits
 * nothing, leaves all four records, d_snaps and d_ents exactly as they were
 * before that record, reports the unchanged last_index, committed, term and
 * state with flags 0, and puts the rest of its run at EFOLLOW_NOT_STEPPED.
 * Records stepped before it keep their effect.
 * Written: of a named group term, committed, log_offset, nlog, n_peers,
 * peer_id[], match[] and next[]; of its elead_prop_state unstable and
 * pending_conf; of its evote_state everything but reserved; of its
 * eready_state applied and soft_dirty; d_snaps[g]; the appended or restored
 * d_ents slots; d_res; d_msgs below *n_msgs.  Only the words that changed are
 * stored.  Nothing of a group that no record names.  d_msgs == NULL fills
 * d_res and the counters and modifies nothing else.  *n_appended = the entries
 * appended, *n_restored = the EFOLLOW_RESTORED records (all three nullable).
 * d_src may be d_ents itself (in process a leader's msgApp names its own
 * window).  The source ranges must not overlap the named groups' windows, and
 * the windows must not overlap each other: the caller's contract.  So is this:
 * d_in_snaps must not be d_snaps, nor share a row with it -- a restore stores
 * d_snaps[g] while other records of the call read their Snapshot.  In process
 * the leader's snapshot is copied out of its emsg_out record into an array of
 * its own (etcd_amd/raftfollow.py::msgs_from_out does that).
 * Checked on the device before anything is modified (then every array is
 * untouched and the counters are 0):
 *   EWAL_E_INVAL  the group, adjacency, window and reserved-word checks of
 *                 evote_step_batch_device; kind not 3 or 7; pad != 0; a source
 *                 range outside n_src_total, or wrapping; a kind-7 record with
 *                 snap >= n_in_snaps, with a Nodes range outside n_u64, or
 *                 with d_rstate or d_snaps NULL
 *   EWAL_E_NOMEM  a kind-3 record with nlog + n_ents > ents_cap (nlog as the
 *                 call found it -- exact enough: the run rule lets one record
 *                 of a run grow the log); a kind-7 record with ents_cap == 0;
 *                 or the messages exceed msgs_cap (INVAL wins when both occur)
 * and on the host as in evote_step_batch_device, d_rstate, d_snaps and
 * d_in_snaps sharing d_groups' rules, d_src and d_u64 d_ents'.  n == 0:
 * EWAL_OK, counters 0. */
int efollow_step_batch_device(ewal_ctx *ctx, elead_group *d_groups, elead_prop_state *d_pstate,
                              evote_state *d_vstate, eready_state *d_rstate /* nullable */, uint64_t G,
                              elead_snap *d_snaps /* G, nullable, WRITTEN by a restore */,
                              ewal_entry *d_ents, uint64_t n_ents_total,
                              const ewal_entry *d_src, uint64_t n_src_total,
                              const elead_snap *d_in_snaps, uint64_t n_in_snaps,
                              const uint64_t *d_u64, uint64_t n_u64,
                              const efollow_msg *d_in, uint64_t n, efollow_result *d_res,
                              struct emsg_out *d_msgs /* NULL: size query */, uint64_t msgs_cap,
                              uint64_t *n_msgs, uint64_t *n_appended, uint64_t *n_restored);
/* For bindings / tests: the sizes of the two records. */
uint32_t efollow_msg_size(void);
uint32_t efollow_result_size(void);

/* ---- log compaction: node.Compact (raft/node.go:226-227, 325-330), that is
 * raft.compact (raft/raft.go:522-531) with raftLog.term (raft/log.go:119-124),
 * raftLog.snap (:171-179) and raftLog.compact (:156-169) under
 * isOutOfAppliedBounds (:219-224); the policy that says when it is due is
 * raftLog.shouldCompact (:181-183), its caller EtcdServer.snapshot
 * (etcdserver/server.go:313-316, 562-571).  Batched over n requests, at most
 * one per group, for G raft groups on the records the calls above share -- the
 * step that gives a window's room back and that produces the d_snaps[g] a
 * leader ships as msgSnap.  A group is its elead_group, its elead_prop_state
 * and (read only) its eready_state; its log is the window d_ents[ents_first,
 * + ents_cap).  All arithmetic is Go's uint64 and wraps; lastIndex = nlog - 1 +
 * log_offset. */
#define ECOMPACT_AT_APPLIED 1u      /* ecompact_req.flags bit 0 */
#define ECOMPACT_PEEK 1u            /* ecompact_batch_device's flags bit 0 */
typedef struct ecompact_req {       /* 96 bytes; one request; a DEVICE array of n */
  uint64_t group;                   /* which group compacts */
  uint64_t flags;                   /* bit 0: ECOMPACT_AT_APPLIED; every other bit 0 */
  uint64_t index;                   /* node.Compact's index; 0 with ECOMPACT_AT_APPLIED */
  uint64_t threshold;               /* ECOMPACT_AT_APPLIED: raftLog.compactThreshold; otherwise not looked at */
  uint64_t data_off, data_len;      /* Snapshot.Data = d_data[data_off, + data_len) */
  uint64_t nodes_off, n_nodes;      /* Snapshot.Nodes = d_u64[nodes_off, + n_nodes) */
  uint64_t removed_off, n_removed;  /* Snapshot.RemovedNodes = d_u64[removed_off, + n_removed); the four mean
                                       what elead_snap's fields mean */
  uint64_t pad[2];                  /* 0 */
} ecompact_req;
enum { ECOMPACT_NOT_STEPPED = 0,    /* never reported by this call: a zeroed result row */
       ECOMPACT_NOT_DUE = 1,        /* ECOMPACT_AT_APPLIED: shouldCompact is false */
       ECOMPACT_COMPACTED = 2,      /* raft.compact returned */
       ECOMPACT_PANICKED = 3 };     /* Go panics (status says where), or the request is unsupported */
typedef struct ecompact_result {    /* 64 bytes; a DEVICE array of n */
  int32_t status, action;           /* EWAL_OK, an EWAL_PANIC_ class, EWAL_UNSUPPORTED_ENCODING; ECOMPACT_* */
  uint64_t index, term;             /* the snapshot's Index and Term */
  uint64_t n_left;                  /* raftLog.compact's return value: len(ents) afterwards */
  uint64_t shift;                   /* the entries dropped: index - the old log_offset */
  uint64_t src_first, dst_first;    /* the survivors lay at d_ents[src_first, + n_left) and lie at
                                       d_ents[dst_first, + n_left) now: ents_first + shift, ents_first */
  uint64_t unstable;                /* raftLog.unstable after the request */
} ecompact_result;
/* Per request, in Go's order:
 *   The index.  With ECOMPACT_AT_APPLIED the request restates shouldCompact
 *     with the caller's threshold: when (applied - log_offset) > threshold is
 *     false (the subtraction wraps, as Go's does) the action is
 *     ECOMPACT_NOT_DUE with status EWAL_OK, every other result field is 0 and
 *     nothing changes; otherwise the index is eready_state.applied, where
 *     EtcdServer.snapshot compacts.  Without the flag the index is req.index.
 *   raft.compact: index > applied is EWAL_PANIC_COMPACT_APPLIED.
 *   term = raftLog.term(index): d_ents[ents_first + (index - log_offset)].term,
 *     or 0 when isOutOfBounds holds; EWAL_PANIC_BOUNDS where at() indexes past
 *     ents (an empty log at offset 0).
 *   raftLog.compact: index < log_offset is EWAL_PANIC_COMPACT_BOUNDS (after the
 *     check above that is all isOutOfAppliedBounds has left).  ents =
 *     slice(index, lastIndex + 1): where Go's slice is nil -- index > lastIndex,
 *     which needs applied > lastIndex and which no sequence of this library's
 *     calls produces, or lastIndex + 1 wrapping to 0 -- Go is left with a
 *     zero-length log; that is EWAL_UNSUPPORTED_ENCODING, reported, never
 *     guessed.  Otherwise, with shift = index - log_offset: n_left = nlog -
 *     shift, elead_prop_state.unstable = max(index + 1, unstable), log_offset =
 *     index, nlog = n_left, and THE SURVIVORS ARE MOVED TO THE WINDOW'S BASE:
 *     d_ents[ents_first + j] = the old d_ents[ents_first + shift + j], j <
 *     n_left, whole 40-byte entries, bit for bit.  ents_first and ents_cap do
 *     not change.  Go reslices; a fixed window has to slide, or the room never
 *     comes back: every observable of the log (offset, len, each entry,
 *     unstable) is Go's.  shift == 0 is legal and moves nothing: only the
 *     snapshot is replaced.  The slots past n_left keep what they held.
 *   raftLog.snap: d_snaps[g] = {index, term, data_off, data_len, nodes_off,
 *     n_nodes, removed_off, n_removed}; r.removedNodes() comes from the request,
 *     as removed[] is the caller's everywhere (the econf_state's ids, below,
 *     copied into d_u64).  ECOMPACT_COMPACTED.
 * Go assigns the snapshot before raftLog.compact can panic; here a panicking
 * group is left exactly as it was, d_snaps[g] included, as in every other call
 * -- the process in Go is dead at that point.  A panicking or unsupported
 * request has action ECOMPACT_PANICKED, every other result field but status 0,
 * and nothing of its group is modified.
 * Written: of a compacted group log_offset and nlog, of its elead_prop_state
 * unstable (only the words that changed), d_snaps[g], the moved d_ents slots;
 * d_res.  eready_state and evote_state are never written: the next
 * eready_batch_device reports EREADY_SNAP on its own, because d_snaps[g].index
 * != snapi.  Groups that no request names are untouched.  With ECOMPACT_PEEK in
 * flags d_res and the counters are filled and nothing else is modified; a peek
 * with ECOMPACT_AT_APPLIED finds the due groups, so that the host has
 * Snapshot.Data made for exactly those and the second call carries their data
 * ranges.  *n_compacted = the ECOMPACT_COMPACTED requests, *n_moved = the
 * entries moved (both nullable).
 * The windows [ents_first, + ents_cap) of the named groups must not overlap
 * each other: the caller's contract, not checked.  So is this: views of a
 * compacted group's window taken before the call go stale -- emsg_out
 * .ents_first, eready_result's views, efollow_msg ranges with d_src == d_ents.
 * The caller marshals or saves first.
 * Checked on the device before anything is modified (then every array is
 * untouched and the counters are 0):
 *   EWAL_E_INVAL  group >= G; a group named twice; a flags bit other than bit
 *                 0; pad != 0; ECOMPACT_AT_APPLIED with index != 0; a Data
 *                 range outside data_len_total, a Nodes or RemovedNodes range
 *                 outside n_u64, or any of them wrapping; and the group, window
 *                 and reserved-word checks of elead_local_batch_device
 * and on the host: NULL arguments (d_ents only when n_ents_total != 0), the
 * record arrays not 16-byte aligned, d_ents not 8-byte aligned, a bit of flags
 * other than ECOMPACT_PEEK, n or G >= 2^31 - 1: EWAL_E_INVAL.  EWAL_E_NOMEM
 * only when the ctx's own staging cannot grow.  n == 0: EWAL_OK, counters 0.  A
 * compute call on the ctx's stream; ewal_last_device_ms covers it; a repeated
 * call of the same or a smaller shape allocates nothing. */
int ecompact_batch_device(ewal_ctx *ctx, elead_group *d_groups, elead_prop_state *d_pstate,
                          const eready_state *d_rstate, uint64_t G,
                          elead_snap *d_snaps /* G, WRITTEN */,
                          ewal_entry *d_ents, uint64_t n_ents_total, uint64_t data_len_total, uint64_t n_u64,
                          const ecompact_req *d_reqs, uint64_t n, ecompact_result *d_res,
                          uint32_t flags /* ECOMPACT_PEEK = 1 */,
                          uint64_t *n_compacted, uint64_t *n_moved /* entries moved; both nullable */);
/* For bindings / tests: the sizes of the two records. */
uint32_t ecompact_req_size(void);
uint32_t ecompact_result_size(void);

/* ---- Tick: node.Tick() (raft/node.go:237-238, 262-269), that is r.tick():
 * tickElection at a follower or a candidate, tickHeartbeat at a leader
 * (raft/raft.go:287-307, set in becomeFollower / becomeCandidate / becomeLeader,
 * :309-349), with promotable (:590-595) and isElectionTimeout (:608-617).
 * Batched over n selected groups of G -- the timer that starts every other
 * step: it keeps evote_state.elapsed, which the step calls only ever reset, and
 * it alone produces the msgHup that evote_step_batch_device and the msgBeat that
 * elead_local_batch_device consume (etcdserver/server.go:255 fires it for every
 * group on every interval).  A group is its elead_group (read only: id, term,
 * n_peers, peer_id[]) and its evote_state.  All elapsed arithmetic is Go's int:
 * int64 that wraps, compared signed; evote_state.elapsed holds the
 * two's-complement bits. */
enum { ETICK_IDLE = 1,              /* elapsed incremented, no timeout test passed, no draw */
       ETICK_HELD = 2,              /* tickElection: d >= 0, a draw was consumed, no timeout */
       ETICK_HUP = 3,               /* tickElection fired: elapsed = 0, one msgHup */
       ETICK_BEAT = 4,              /* tickHeartbeat fired: elapsed = 0, one msgBeat */
       ETICK_NOT_PROMOTABLE = 5,    /* tickElection at a node not among its own peers: elapsed = 0 */
       ETICK_PANICKED = 6 };        /* the group is unsupported (n_peers > 7) */
typedef struct etick_result {       /* 32 bytes; a DEVICE array of n */
  int32_t status, action;           /* EWAL_OK or EWAL_UNSUPPORTED_ENCODING; ETICK_* */
  uint64_t elapsed;                 /* raft.elapsed after this tick */
  uint64_t out_pos;                 /* HUP: its index in d_hups; BEAT: in d_beats; else 0 */
  uint64_t draw;                    /* the rand.Int() value consumed (HELD, HUP), else 0 */
} etick_result;
/* Selection i is group d_sel[i], or group i when d_sel == NULL (then n == G),
 * as in eready_batch_device.  election and heartbeat are raft.electionTimeout
 * and raft.heartbeatTimeout (the server's are 10 and 1, etcdserver/server.go).
 * Per selected group, in Go's order:
 *   state == 2 (leader), tickHeartbeat: e = elapsed + 1; e > heartbeat: elapsed
 *     = 0 and one elead_local {group, kind = 1 (msgBeat), every other field 0},
 *     ETICK_BEAT; otherwise elapsed = e, ETICK_IDLE.
 *   state 0 or 1, tickElection: promotable() is "id is among the first n_peers
 *     peer_id".  Not promotable: elapsed = 0 WITHOUT the increment,
 *     ETICK_NOT_PROMOTABLE.  Promotable: e = elapsed + 1, d = e - election.
 *     d < 0: elapsed = e, ETICK_IDLE, and NO draw is consumed.  d >= 0: with r
 *     the draw, d > r % election: elapsed = 0 and one evote_msg {group, kind = 0
 *     (msgHup), from = id, every other field 0}, ETICK_HUP; otherwise elapsed =
 *     e, ETICK_HELD.
 *   A group with n_peers > 7: EWAL_UNSUPPORTED_ENCODING, ETICK_PANICKED, left as
 *     it was (d_res[i].elapsed is the unchanged word) -- reported, never guessed.
 * The draw.  Go takes rand.Int() from the process-wide source that every
 * node's goroutine shares: which value a group receives is unspecified in the
 * reference.  As with map order elsewhere, the library fixes a rule.  With
 * d_draws given, selection i's draw is d_draws[i] (a shim that replays Go's own
 * stream fills it).  With d_draws == NULL it is etick_draw(seed, id,
 * group.term, e), e the incremented elapsed:
 *   x = seed ^ id * 0x9E3779B97F4A7C15 ^ term * 0xBF58476D1CE4E5B9
 *            ^ elapsed * 0x94D049BB133111EB
 *   x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27;
 *   x *= 0x94D049BB133111EB; x ^= x >> 31; return x >> 1
 * mod 2^64; 63 bits, as rand.Int()'s.  etick_draw(1, 2, 3, 4) ==
 * 0x5a86a12931d3dfc7.
 * Output placement.  d_hups and d_beats are dense and ordered by selection
 * position; *n_hups and *n_beats are their lengths (both nullable); nothing at
 * or past them is written.  d_hups goes to evote_step_batch_device as it lies
 * (a group appears once, so its adjacency rule holds), d_beats to
 * elead_local_batch_device.  The removed[r.id] gate in front of the resulting
 * Step (raft.go:376-387) stays the caller's (econf_gate_batch_device with
 * ECONF_FROM_SELF over d_hups and d_beats, below), as do the wall clock that says
 * when to call and, if Go's stream is wanted, filling d_draws.
 * Written: evote_state.elapsed of selected groups, only where it changed;
 * d_res; the two outputs.  elead_group is read only (its match[] and next[]
 * are not even read); no other word of any record is touched.
 * d_hups == NULL with d_beats == NULL is the peek: d_res and the counters are
 * filled and nothing else is modified; the draw is a pure function, so the
 * peek and the call agree.
 * Checked on the device before anything is modified (then every array is
 * untouched and the counters are 0):
 *   EWAL_E_INVAL  a selected group >= G; a group selected twice;
 *                 evote_state.state > 2; elead_group.reserved or
 *                 evote_state.reserved not 0; two equal peer_id within the
 *                 first min(n_peers, 7) slots; a d_draws[i] >= 2^63
 *   EWAL_E_NOMEM  the msgHup exceed hups_cap or the msgBeat beats_cap (INVAL
 *                 wins when both occur)
 * and on the host: EWAL_E_INVAL for a NULL ctx; for d_groups, d_vstate or d_res
 * NULL while n > 0; for exactly one of d_hups and d_beats NULL; for d_sel ==
 * NULL with n != G; for d_groups, d_vstate, d_res, d_hups, d_beats not 16-byte
 * aligned or d_sel, d_draws not 8-byte aligned; for n or G >= 2^31 - 1; for
 * election outside [1, 2^31 - 1] (Go divides by zero at 0; a negative divisor
 * is not restated) and heartbeat outside [0, 2^31 - 1].  n == 0: EWAL_OK,
 * counters 0.  A compute call on the ctx's stream; ewal_last_device_ms covers
 * it; a repeated call of the same or a smaller shape allocates nothing. */
int etick_batch_device(ewal_ctx *ctx, const elead_group *d_groups, evote_state *d_vstate, uint64_t G,
                       const uint64_t *d_sel /* n group numbers; NULL: n == G, group i */, uint64_t n,
                       int64_t election, int64_t heartbeat,
                       const uint64_t *d_draws /* n, nullable */, uint64_t seed,
                       etick_result *d_res,
                       evote_msg *d_hups /* NULL with d_beats NULL: peek */, uint64_t hups_cap,
                       elead_local *d_beats, uint64_t beats_cap,
                       uint64_t *n_hups, uint64_t *n_beats);
/* Host only: the draw rule above (etcd_amd/csrc/tick_step.h). */
uint64_t etick_draw(uint64_t seed, uint64_t id, uint64_t term, uint64_t elapsed);
/* For bindings / tests: sizeof(etick_result). */
uint32_t etick_result_size(void);

/* ---- Membership: node.ApplyConfChange (raft/node.go:228-236, 318-323) with
 * raft.addNode / removeNode (raft/raft.go:426-435) and setProgress /
 * delProgress (:582-588); the removed[] / msgDenied lines at the head of
 * raft.Step (:376-387); the removed half of raft.restore (:549-552); and the
 * server loop's EntryConfChange arm (etcdserver/server.go:265-286) with
 * ConfChange.Unmarshal (raft/raftpb/raft.pb.go:705-813).  Three calls on the
 * records the step calls share, plus one side record: the key set of
 * r.removed, in insertion order.  StartNode and RestartNode build
 * newRaft(id, nil, ...): a node gets its peers only by applying the committed
 * ConfChange entries of its log, so these calls are what lets a restarted host
 * reach its first election without per-group host work.  All arithmetic is
 * Go's uint64 and wraps. */
typedef struct econf_state {        /* 128 bytes; a DEVICE array of G, updated in place */
  uint64_t n_removed;               /* len(r.removed): 0..14 */
  uint64_t removed[14];             /* its keys in insertion order; the slots past n_removed are not read */
  uint64_t reserved;                /* 0 */
} econf_state;
typedef struct econf_req {          /* 32 bytes; one request; a DEVICE array of n */
  uint64_t group;                   /* which group steps it */
  uint64_t kind;                    /* 1 addNode, 2 removeNode (ConfChange.Type + 1), 3 msgDenied, 4 reload */
  uint64_t node;                    /* cc.NodeID; kind 3: m.From; kind 4: 0 */
  uint64_t pad;                     /* 0 */
} econf_req;
enum { ECONF_NOT_STEPPED = 0,       /* after a panic in its group's run: the caller's to step */
       ECONF_ADDED = 1,             /* kind 1 */
       ECONF_REMOVED = 2,           /* kind 2 */
       ECONF_DENIED_BACK = 3,       /* kind 3 from a removed node: a msgDenied goes back (none to oneself) */
       ECONF_STOPPED = 4,           /* kind 3 from a live node: removed[id] = true */
       ECONF_RELOADED = 5,          /* kind 4 */
       ECONF_PANICKED = 6 };        /* Go panics (status says where), or the request is unsupported */
typedef struct econf_result {       /* 48 bytes; a DEVICE array of n */
  int32_t status, action;           /* EWAL_OK, EWAL_PANIC_CONF_TYPE, EWAL_UNSUPPORTED_ENCODING; ECONF_* */
  uint64_t msg_first, n_msgs;       /* its messages: d_msgs[msg_first, + n_msgs) */
  uint64_t n_peers, n_removed;      /* len(r.prs) and len(r.removed) after this request */
  uint64_t pad;                     /* 0 */
} econf_result;
/* econf_batch_device.  Order, output placement, the size query (d_msgs ==
 * NULL), the stream, the timing and the allocation rule are
 * elead_local_batch_device's, with "request" for "record": a group's requests
 * are adjacent and stepped in array order, each one seeing the state the
 * previous one left, runs have any length and lie anywhere, the messages are
 * dense and ordered by request, msg_first counts the messages of the requests
 * before i also when n_msgs == 0, and no emsg_out at or past *n_msgs is
 * written.  *n_changed = the ADDED, REMOVED, STOPPED and RELOADED requests
 * (nullable, as *n_msgs).  A group is its elead_group,
 * its elead_prop_state, its evote_state, its eready_state and its econf_state.
 * Per request, lastIndex = nlog - 1 + log_offset:
 *   kind 1, addNode(node): setProgress(node, 0, lastIndex + 1); pending_conf =
 *     0.  An id among the first n_peers peer_id keeps its slot and its (match,
 *     next) are overwritten -- the leader's own id included: Go's quirk is
 *     kept.  A new id takes slot n_peers, and n_peers grows by one; at n_peers
 *     == 7 that is EWAL_UNSUPPORTED_ENCODING.  removed[] is NOT cleared for a
 *     re-added id, as in Go.  ECONF_ADDED.
 *   kind 2, removeNode(node): delProgress(node); pending_conf = 0;
 *     removed[node] = true.  The slots after the deleted one move down by one
 *     with their match and next, the freed slot is zeroed, and the bits of
 *     evote_state.voted / granted move with their slots.  An id that is not a
 *     key still enters removed[]; an id already there is not stored twice; a
 *     15th id is EWAL_UNSUPPORTED_ENCODING.  Go keeps r.votes[node] after the
 *     delete and the masks cannot: at a CANDIDATE (state 1) whose deleted slot
 *     has its voted bit set the request is EWAL_UNSUPPORTED_ENCODING; in the
 *     other two states the votes are not read before the next reset, and the
 *     bit is dropped.  ECONF_REMOVED.
 *   kind 3, Step(Message{Type: msgDenied, From: node}), raft.go:376-387 only:
 *     removed[node]: no state change, and unless node == id one emsg_out {type
 *     = 8 (msgDenied), to = node, from = id, term = group.term, every other
 *     field 0}; ECONF_DENIED_BACK.  Otherwise removed[id] = true (a 15th id:
 *     EWAL_UNSUPPORTED_ENCODING); ECONF_STOPPED.
 *   kind 4, the removed half of raft.restore, which
 *     efollow_step_batch_device leaves to the caller: removed[] becomes the
 *     RemovedNodes range d_u64[removed_off, + n_removed) of d_snaps[group],
 *     duplicates dropped in first-occurrence order; the slots past the new
 *     n_removed are zeroed.  More than 14 distinct ids:
 *     EWAL_UNSUPPORTED_ENCODING.  ECONF_RELOADED.
 *   any other kind: EWAL_PANIC_CONF_TYPE, panic("unexpected conf type").
 *   The first request of a group with n_peers > 7 gets
 *     EWAL_UNSUPPORTED_ENCODING, as everywhere else.
 * eready_state.soft_dirty is set to 1 when n_peers or one of the first n_peers
 * peer_id changed (SoftState.Nodes) and when removed[id] changed (ShouldStop,
 * raft.go:158-162): the next eready_batch_device reports EREADY_SOFT.
 * A panicking or unsupported request has action ECONF_PANICKED, emits nothing,
 * leaves every record of its group exactly as it was before that request, and
 * puts the rest of its group's run at ECONF_NOT_STEPPED; the requests stepped
 * before it keep their effect.  Results of PANICKED and NOT_STEPPED requests
 * report the unchanged n_peers and n_removed.
 * Written, only where a word changed: of a named group n_peers, peer_id[],
 * match[], next[]; pending_conf; voted, granted; soft_dirty; the econf_state;
 * d_res; d_msgs below *n_msgs.  Nothing of a group that no request names.
 * Checked on the device before anything is modified (then every array is
 * untouched and the counters are 0):
 *   EWAL_E_INVAL  group >= G; a group's requests not adjacent; a request's pad
 *                 not 0; a kind-4 request with d_snaps == NULL or its
 *                 RemovedNodes range outside n_u64, or wrapping; and of a named
 *                 group: reserved != 0 in any of its five records; n_removed >
 *                 14; two equal peer_id within the first min(n_peers, 7) slots;
 *                 pending_conf > 1; soft_dirty > 1; evote_state.state > 2;
 *                 voted or granted bits at or past n_peers, or granted outside
 *                 voted
 *   EWAL_E_NOMEM  the messages exceed msgs_cap (INVAL wins when both occur)
 * and on the host: EWAL_E_INVAL for a NULL ctx; for d_groups, d_pstate,
 * d_vstate, d_rstate, d_cstate, d_reqs or d_res NULL while n > 0; for d_u64 ==
 * NULL with n_u64 > 0; for any record array not 16-byte aligned or d_u64 not
 * 8-byte aligned; for n or G >= 2^31 - 1.  n == 0: EWAL_OK, counters 0.  A
 * compute call on the ctx's stream; ewal_last_device_ms covers it; a repeated
 * call of the same or a smaller shape allocates nothing. */
int econf_batch_device(ewal_ctx *ctx, elead_group *d_groups, elead_prop_state *d_pstate, evote_state *d_vstate,
                       eready_state *d_rstate, econf_state *d_cstate, uint64_t G,
                       const elead_snap *d_snaps /* G, nullable */, const uint64_t *d_u64, uint64_t n_u64,
                       const econf_req *d_reqs, uint64_t n, econf_result *d_res,
                       struct emsg_out *d_msgs /* NULL: size query */, uint64_t msgs_cap,
                       uint64_t *n_msgs, uint64_t *n_changed);

/* econf_scan_committed_device: the ConfChange half of the server loop over
 * rd.CommittedEntries (etcdserver/server.go:265-286).  d_ready is the
 * eready_result[n] of an eready_batch_device call; selection i's committed
 * entries are d_ents[committed_first, + n_committed).  One lane per committed
 * entry over all selections.  Per entry, in order:
 *   type 0 (EntryNormal) is the application's and is skipped.
 *   type 1 (EntryConfChange): ConfChange.Unmarshal over d_data[data_off, +
 *     data_len).  Empty or nil Data decodes as ConfChange{}: addNode(0), as in
 *     Go.  Fields 1-3 (ID, Type, NodeID) are varints with a wire-type check,
 *     OR-ed as the generated code does (a repeated field ORs; Type keeps 32
 *     bits); field 4 (Context) is bytes, of which only the bounds matter here;
 *     unknown fields go through proto.Skip with the depth limit and the error
 *     classes emsg_decode_batch_device has.  It emits one econf_req {group,
 *     kind = uint32(Type) + 1, node = NodeID, 0} and, at the same position of
 *     d_applied, what s.w.Trigger(cc.ID, nil) and raftIndex / raftTerm need.
 *   A type-1 entry whose Unmarshal fails has the status
 *     emsg_decode_batch_device gives that error (EWAL_ERR_UNEXPECTED_EOF,
 *     EWAL_ERR_WRONG_TYPE, EWAL_PANIC_BOUNDS, EWAL_NONTERMINATING,
 *     EWAL_UNSUPPORTED_ENCODING); an entry with data_nil == 2 (its Data is not
 *     in d_data) has EWAL_UNSUPPORTED_ENCODING; an entry type other than 0 or 1
 *     has EWAL_ERR_UNEXPECTED_TYPE with detail = the type.  The server panics
 *     at each (server.go:275-282).  The selection's row names the FIRST such
 *     entry; it and the later entries of that selection emit nothing, the
 *     earlier ones keep theirs.
 * The requests are dense, ordered by selection and then by entry.  Each group
 * is selected once, so the array goes to econf_batch_device as it lies.
 * d_reqs == NULL with d_applied == NULL is the size query: d_scan and the
 * counters are filled.  Nothing but the three outputs is ever written.
 * *n_reqs = the requests, *n_entries = the committed entries looked at (both
 * nullable).
 * Checked on the device before anything is written:
 *   EWAL_E_INVAL  a selected group >= G; a committed range outside
 *                 n_ents_total, or wrapping; the committed entries of all
 *                 selections together >= 2^31 - 1 (ranges that coincide); a
 *                 scanned type-1 entry's data_nil
 *                 not 0, 1 or 2, or its Data range outside data_len_total, or
 *                 wrapping
 *   EWAL_E_NOMEM  the requests exceed reqs_cap (INVAL wins when both occur)
 * and on the host: NULL ctx; d_ready or d_scan NULL while n > 0; d_ents NULL
 * with n_ents_total > 0; d_data NULL with data_len_total > 0; exactly one of
 * d_reqs and d_applied NULL; d_ready, d_scan, d_reqs, d_applied not 16-byte
 * aligned, d_ents or d_sel not 8-byte aligned; n, G or n_ents_total >= 2^31 -
 * 1; d_sel == NULL with n != G: EWAL_E_INVAL.  n == 0: EWAL_OK.  Stream,
 * timing and allocation as above. */
typedef struct econf_applied {      /* 32 bytes; a DEVICE array parallel to d_reqs */
  uint64_t id;                      /* cc.ID */
  uint64_t index, term;             /* e.Index, e.Term */
  uint64_t ent_pos;                 /* the entry's position in d_ents */
} econf_applied;
typedef struct econf_scan_result {  /* 48 bytes; a DEVICE array of n */
  int32_t status;                   /* EWAL_OK, or the first failing entry's class */
  int32_t detail;                   /* EWAL_ERR_UNEXPECTED_TYPE: the entry's type; else 0 */
  uint64_t req_first, n_reqs;       /* this selection's requests: d_reqs[req_first, + n_reqs) */
  uint64_t bad_pos;                 /* the failing entry's position in d_ents (0 when status == EWAL_OK) */
  uint64_t n_scanned;               /* the entries before the failing one; n_committed when none fails */
  uint64_t pad;                     /* 0 */
} econf_scan_result;
int econf_scan_committed_device(ewal_ctx *ctx, const struct eready_result *d_ready,
                                const uint64_t *d_sel /* as given to eready_batch_device */, uint64_t n, uint64_t G,
                                const ewal_entry *d_ents, uint64_t n_ents_total,
                                const void *d_data, uint64_t data_len_total,
                                econf_scan_result *d_scan,
                                econf_req *d_reqs /* NULL with d_applied NULL: size query */,
                                econf_applied *d_applied, uint64_t reqs_cap,
                                uint64_t *n_reqs, uint64_t *n_entries);

/* econf_gate_batch_device: r.removed[m.From] in front of every step call
 * (raft.go:376-382), a stable filter over any of the step calls' input arrays.
 * d_recs is n records of rec_bytes each, rec_bytes in {48, 64, 96}: elead_resp
 * and elead_local, evote_msg, efollow_msg.  Word 0 of a record is its group;
 * m.From is its 8-byte word from_word -- 1 for elead_resp, 2 for evote_msg and
 * efollow_msg -- or, with ECONF_FROM_SELF, the group's id: elead_local, whose
 * From is the node's own (node.go:222), and etick_batch_device's msgHup.
 * Per record:
 *   removed[from], from != id: one emsg_out {type = 8 (msgDenied), to = from,
 *     from = id, term = group.term, every other field 0}; ECONF_G_DENIED.
 *   removed[from], from == id: no message; ECONF_G_DROPPED.
 *   otherwise the record is copied whole to d_pass; ECONF_G_PASS.
 * d_pass and d_msgs are dense and keep the order of d_recs, so runs stay
 * adjacent and d_pass goes to its step call as it lies.  d_res[i].pass_pos /
 * .msg_pos is where record i's copy / message went (0 when it has none).
 * d_pass == NULL with d_msgs == NULL is the size query.  The groups and the
 * econf_state are read only; *n_pass and *n_msgs are nullable.
 * Checked on the device before anything is written:
 *   EWAL_E_INVAL  a record's group >= G; of a named group n_removed > 14 or
 *                 econf_state.reserved != 0
 *   EWAL_E_NOMEM  the copies exceed pass_cap or the messages msgs_cap (INVAL
 *                 wins when both occur)
 * and on the host: NULL ctx; d_groups, d_cstate, d_recs or d_res NULL while n
 * > 0; exactly one of d_pass and d_msgs NULL; rec_bytes not 48, 64 or 96;
 * from_word neither ECONF_FROM_SELF nor in [1, rec_bytes / 8); an array not
 * 16-byte aligned; d_pass overlapping d_recs; n or G >= 2^31 - 1:
 * EWAL_E_INVAL.  n == 0: EWAL_OK.  Stream, timing and allocation as above. */
#define ECONF_FROM_SELF 0xffffffffu
enum { ECONF_G_PASS = 1, ECONF_G_DENIED = 2, ECONF_G_DROPPED = 3 };
typedef struct econf_gate_result {  /* 32 bytes; a DEVICE array of n */
  int32_t status, action;           /* EWAL_OK; ECONF_G_* */
  uint64_t pass_pos, msg_pos;
  uint64_t pad;                     /* 0 */
} econf_gate_result;
int econf_gate_batch_device(ewal_ctx *ctx, const elead_group *d_groups, const econf_state *d_cstate, uint64_t G,
                            const void *d_recs, uint64_t n, uint32_t rec_bytes, uint32_t from_word,
                            econf_gate_result *d_res,
                            void *d_pass /* NULL with d_msgs NULL: size query */, uint64_t pass_cap,
                            struct emsg_out *d_msgs, uint64_t msgs_cap,
                            uint64_t *n_pass, uint64_t *n_msgs);
/* For bindings / tests: the sizes of the records above. */
uint32_t econf_state_size(void);
uint32_t econf_req_size(void);
uint32_t econf_result_size(void);
uint32_t econf_applied_size(void);
uint32_t econf_scan_result_size(void);
uint32_t econf_gate_result_size(void);

/* ---- StartNode / RestartNode: raft.StartNode and raft.RestartNode
 * (raft/node.go:125-161) with newRaft(id, nil, ...) (raft/raft.go:135-154),
 * newLog (raft/log.go:26-34), raft.restore (raft.go:535-554, log.go:185-192),
 * loadState / loadEnts (raft.go:597-606, log.go:40-43), StartNode's
 * ConfChange.Marshal entries (raft/raftpb/raft.pb.go:1108-1130) and the locals
 * node.run starts with (node.go:194-197).  Batched over n requests, at most one
 * per group, for G raft groups: the call that BUILDS the records every call
 * above runs on -- a group's elead_group, elead_prop_state, evote_state,
 * eready_state and econf_state, d_snaps[g] and the window of d_ents -- from a
 * batch replay's result (kind 1) or from a list of peers (kind 2).  With
 * ewal_batch_entries_device and enode_reqs_from_batch a replay's entries reach
 * their groups' windows without leaving the device.  All arithmetic is Go's
 * uint64 and wraps; lastIndex = nlog - 1 + log_offset. */
typedef struct enode_req {          /* 128 bytes; one node to build; a DEVICE array of n */
  uint64_t group;                   /* which row of the five record arrays (and d_snaps) it builds */
  uint64_t kind;                    /* 0 none (e.g. a shard whose ReadAll failed), 1 RestartNode, 2 StartNode */
  uint64_t id;                      /* raft id */
  uint64_t ents_first, ents_cap;    /* the window given to the group in d_ents */
  uint64_t src_first, n_src;        /* kind 1: ents = d_src[src_first, + n_src) (ReadAll's ents);
                                       kind 2: peers = d_peers[src_first, + n_src) */
  uint64_t data_delta;              /* kind 1: added to data_off where data_nil == 0 (the shard's base in the WAL buffer) */
  uint64_t hs_term, hs_vote, hs_commit;  /* kind 1: st (zeros when ReadAll had no state record) */
  uint64_t snap;                    /* kind 1: row of d_in_snaps, or UINT64_MAX: snapshot == nil */
  uint64_t pad[4];                  /* 0 */
} enode_req;
/* raft.Peer; Context = d_ctx[ctx_off, + ctx_len) */
typedef struct enode_peer { uint64_t id, ctx_off, ctx_len, pad; } enode_peer;   /* 32 bytes */
enum { ENODE_NONE = 0,              /* kind 0: nothing built */
       ENODE_RESTARTED = 1,         /* kind 1, no snapshot or restore returned false */
       ENODE_RESTARTED_SNAP = 2,    /* kind 1, restore returned true */
       ENODE_STARTED = 3,           /* kind 2 */
       ENODE_PANICKED = 4 };        /* Go panics (status says where), or the request is unsupported */
typedef struct enode_result {       /* 48 bytes; a DEVICE array of n */
  int32_t status, action;           /* EWAL_OK, EWAL_PANIC_NONE_ID, EWAL_UNSUPPORTED_ENCODING; ENODE_* */
  uint64_t nlog, committed, log_offset, n_peers;  /* as built; 0 for NONE and PANICKED */
  uint64_t data_first;              /* kind 2: its ConfChange bytes start at d_data[data_first]; else 0 */
} enode_result;
/* Per request, in Go's order:
 *   both kinds: id == 0 is EWAL_PANIC_NONE_ID.  newRaft, then
 *     becomeFollower(0, None): term, vote, lead, state and elapsed 0; votes
 *     (voted, granted), prs (n_peers and the three peer arrays) and removed
 *     empty; pending_conf 0; the log is the dummy entry alone with log_offset,
 *     committed, applied and unstable 0 and the snapshot empty.
 *   kind 1, RestartNode(id, _, _, snapshot, st, ents):
 *     snap != UINT64_MAX: restore(s), s = d_in_snaps[snap].  s.index <= 0
 *       returns false and nothing of s is taken, not even its Nodes (Go's
 *       quirk, kept).  Otherwise log_offset = committed = applied = s.index,
 *       d_snaps[g] = s, prs is rebuilt from s.Nodes = d_u64[nodes_off, +
 *       n_nodes) by the slot rule efollow_step_batch_device documents (the
 *       distinct ids take the slots in first-occurrence order; the slot whose
 *       id equals id gets (match, next) = (s.index, s.index + 1), the others
 *       (0, s.index + 1)), and removed[] from s.RemovedNodes = d_u64[
 *       removed_off, + n_removed) by econf_batch_device's kind-4 rule
 *       (duplicates dropped in first-occurrence order).  ENODE_RESTARTED_SNAP.
 *     loadState: term = hs_term, vote = hs_vote, committed = hs_commit,
 *       unconditionally: there is no clamp, and a zero HardState sets committed
 *       back to 0 after a restore, as Go does.
 *     loadEnts: the log IS the n_src entries (the entry a restore left is
 *       replaced with the rest): d_ents[ents_first + j] = d_src[src_first + j],
 *       data_off rebased by data_delta where data_nil == 0 (an entry with
 *       data_nil == 2 is copied untouched, and so is one with data_nil == 1,
 *       whose data_off a replay leaves undefined); nlog = n_src; unstable = log_offset
 *       + n_src.  With n_src == 0 nlog is 0 and lastIndex wraps, as everywhere
 *       else.  The entries' own index fields are not examined.
 *     node.run's locals, the eready_state: hs_* = st, lead 0, state 0, snapi =
 *       d_snaps[g].index, applied = s.index or 0, soft_dirty 0.
 *   kind 2, StartNode(id, peers, _, _): slot 0 of the window is the dummy
 *     entry {0, 0, 0, 0, type 0, data_nil 1}; slot 1 + i is {term 1, index i +
 *     1, type 1 (EntryConfChange), data_nil 0} whose Data is ConfChange{ID 0,
 *     Type 0 (AddNode), NodeID peers[i].id, Context}.Marshal(): 08 00 10 00 18
 *     v(id) 22 v(len) ctx, every field written.  The bytes of all requests are
 *     dense in d_data in request order, then peer order: request i's start at
 *     d_data[data_first], and an entry's data_off = data_base + its position
 *     in d_data (data_base: where d_data lies in the buffer the entries' Data
 *     offsets mean).  nlog = 1 + n_src, committed = n_src, unstable = 0,
 *     n_peers = 0: the peers arrive when the committed entries are applied
 *     (econf_scan_committed_device, econf_batch_device).  eready_state.hs_* =
 *     {0, 0, n_src}: StartNode sets raftLog.committed without a Step
 *     (node.go:141-142), so Go's first Ready carries no HardState; this is the
 *     seeding eready_batch_device's comment leaves to the caller, done here.
 *     Everything else is 0.  ENODE_STARTED.
 *   kind 0: ENODE_NONE, nothing is read or written but d_res.
 * EWAL_UNSUPPORTED_ENCODING, reported, never guessed, for a restore that runs
 * (s.index > 0) with n_nodes > 64, more than 7 distinct Nodes or more than 14
 * distinct RemovedNodes.
 * Written: EVERY word of the five records of a built group, reserved words as
 * 0 -- the "changed words only" rule of the step calls does not apply, the
 * records' previous content is undefined and not read; d_snaps[g] (all zero
 * without a restore); the window's first nlog slots; d_data below *n_data;
 * d_res.  Slots past nlog, groups no request names and the groups of kind-0
 * requests are untouched.  A panicking or unsupported request has action
 * ENODE_PANICKED, every result field but status and action 0, and leaves its
 * group and its window exactly as they were.
 * d_data == NULL is the size query: d_res, *n_data (the ConfChange bytes),
 * *n_copied (the entries copied) and *n_built (the RESTARTED, RESTARTED_SNAP
 * and STARTED requests) are filled and nothing else is modified (all three
 * counters nullable).  A call without a kind-2 request still needs a non-NULL
 * d_data to build; data_cap may be 0 then.
 * The source ranges must not overlap the named groups' windows, and the
 * windows must not overlap each other; d_in_snaps must not be d_snaps, nor
 * share a row with it: the caller's contract, as in efollow_step_batch_device.
 * Checked on the device before anything is modified (then every array is
 * untouched and the counters are 0):
 *   EWAL_E_INVAL  group >= G; a group named by two requests (kind 0 included);
 *                 kind > 2; pad != 0; and for kinds 1 and 2: a window outside
 *                 n_ents_total, or wrapping; a source range outside n_src_total
 *                 (kind 1) or n_peers_total (kind 2), or wrapping; snap neither
 *                 UINT64_MAX nor < n_in_snaps; a Nodes or RemovedNodes range of
 *                 that snapshot outside n_u64 (whatever s.index is); a peer's
 *                 Context range outside ctx_len; enode_peer.pad != 0
 *   EWAL_E_NOMEM  n_src > ents_cap (kind 1); 1 + n_src > ents_cap (kind 2); the
 *                 ConfChange bytes exceed data_cap (INVAL wins when both occur)
 * and at the decision point, with the same guarantee: EWAL_E_INVAL when the
 * entries to copy, or the peers to marshal, number 2^31 x 256 or more over the
 * whole call (the copy and marshal passes' lanes are 32-bit workgroup
 * ordinals).  The three totals (entries, peers, bytes) are uint64 sums over
 * the requests; requests may name overlapping source or peer ranges, so the
 * array lengths do not bound them, and a sum that wraps is not detected: keep
 * the call's totals below 2^64.
 * and on the host: EWAL_E_INVAL for a NULL ctx; for any of the six group
 * arrays, d_reqs or d_res NULL while n > 0; for d_ents, d_src, d_in_snaps,
 * d_u64, d_peers or d_ctx NULL with a length > 0; for a record array (d_peers
 * and d_in_snaps included) not 16-byte aligned or d_ents, d_src, d_u64 not
 * 8-byte aligned; for n or G >= 2^31 - 1.  n == 0: EWAL_OK, counters 0.  A
 * compute call on the ctx's stream; ewal_last_device_ms covers it; a repeated
 * call of the same or a smaller shape allocates nothing. */
int enode_batch_device(ewal_ctx *ctx, elead_group *d_groups, elead_prop_state *d_pstate, evote_state *d_vstate,
                       eready_state *d_rstate, econf_state *d_cstate, elead_snap *d_snaps, uint64_t G,
                       ewal_entry *d_ents, uint64_t n_ents_total,
                       const ewal_entry *d_src, uint64_t n_src_total,
                       const elead_snap *d_in_snaps, uint64_t n_in_snaps, const uint64_t *d_u64, uint64_t n_u64,
                       const enode_peer *d_peers, uint64_t n_peers_total, const uint8_t *d_ctx, uint64_t ctx_len,
                       uint8_t *d_data /* NULL: size query */, uint64_t data_base, uint64_t data_cap,
                       const enode_req *d_reqs, uint64_t n, enode_result *d_res,
                       uint64_t *n_data, uint64_t *n_copied, uint64_t *n_built);
/* Host only: the requests of a batch replay.  res[n_shards] is what
 * ewal_readall_batch_device just returned on ctx, shard_off[s] the place of
 * shard s in the buffer the entries' Data offsets shall mean.  Request s gets
 * group = s; kind = 1 when res[s].status == EWAL_OK and res[s].n_unrec == 0,
 * else 0; src_first and n_src = shard s's range of the array
 * ewal_batch_entries_device returns; data_delta = shard_off[s]; hs_* =
 * res[s]'s HardState (zeros without a state record); pad = 0.  id, ents_first,
 * ents_cap and snap are not touched: the caller fills them, before or after.
 * EWAL_E_INVAL: a NULL argument, n_shards is not the last batch's, or the
 * ctx's last ReadAll was not a batch that returned EWAL_OK. */
int enode_reqs_from_batch(ewal_ctx *ctx, const ewal_result *res, uint64_t n_shards, const uint64_t *shard_off,
                          enode_req *h_reqs);
/* For bindings / tests: the sizes of the three records. */
uint32_t enode_req_size(void);
uint32_t enode_peer_size(void);
uint32_t enode_result_size(void);

/* ---- raft ingress: raftpb.Message.Unmarshal, raft/raftpb/raft.pb.go:407-617
 * (called per POST /raft in etcdserver/etcdhttp/http.go:119-146), batched
 * over n messages resident in one device buffer at offs[i], lens[i] (host
 * arrays).  status = EWAL_OK / EWAL_ERR_UNEXPECTED_EOF / EWAL_ERR_WRONG_TYPE /
 * EWAL_PANIC_BOUNDS / EWAL_NONTERMINATING as Unmarshal returns or panics
 * (EWAL_UNSUPPORTED_ENCODING only for protobuf groups nested deeper than the
 * device walker's stack).  The fields hold what Go leaves in the struct
 * (partial on error).  Entries go to a ctx-owned array: message i's are
 * [ents_first, ents_first + n_ents), fetched with emsg_copy_entries (Data
 * offsets are offsets into d_buf; data_nil == 2: Data is the concatenation
 * of that entry's EMSG_SEG_ENTRY_DATA segments).  The byte values Go builds
 * by append and the Snapshot's repeated fields are message i's segments
 * [segs_first, segs_first + n_segs) (emsg_copy_segments), in order:
 *   EMSG_SEG_UNREC         Message.XXX_unrecognized  (raft.pb.go:612-616)
 *   EMSG_SEG_ENTRY_UNREC   Entries[ent].XXX_unrecognized
 *   EMSG_SEG_ENTRY_DATA    Entries[ent].Data, repeated non-empty segments
 *   EMSG_SEG_SNAP_UNREC    Snapshot.XXX_unrecognized
 *   EMSG_SEG_SNAP_DATA     Snapshot.Data's segments (used when
 *                          snap_data_off == -2: a split field)
 *   EMSG_SEG_SNAP_NODE     one Snapshot.Nodes value (in off)
 *   EMSG_SEG_SNAP_REMOVED  one Snapshot.RemovedNodes value (in off)
 * a byte value is the concatenation of its kind's [off, off + len) ranges of
 * d_buf (none: nil). */
typedef struct emsg_message {
  int32_t status;
  int32_t reject;
  uint64_t type, to, from, term, log_term, index, commit;
  uint64_t ents_first, n_ents;
  uint64_t snap_index, snap_term;
  int64_t snap_data_off, snap_data_len;   /* Snapshot.Data in d_buf; off -1 == nil, -2: split (segments) */
  uint64_t snap_n_nodes, snap_n_removed;
  int64_t unrec_len;                       /* len(XXX_unrecognized) */
  uint64_t segs_first, n_segs;
} emsg_message;
enum {
  EMSG_SEG_UNREC = 0,
  EMSG_SEG_ENTRY_UNREC = 1,
  EMSG_SEG_ENTRY_DATA = 2,
  EMSG_SEG_SNAP_UNREC = 3,
  EMSG_SEG_SNAP_DATA = 4,
  EMSG_SEG_SNAP_NODE = 5,
  EMSG_SEG_SNAP_REMOVED = 6
};
typedef struct emsg_segment {
  int32_t kind;            /* EMSG_SEG_* */
  int32_t pad;
  int64_t ent;             /* the entry, counted within its message (EMSG_SEG_ENTRY_*), else -1 */
  uint64_t off, len;       /* a range of d_buf, or (value, 0) */
} emsg_segment;
int emsg_decode_batch_device(ewal_ctx *ctx, const void *d_buf, uint64_t buf_len, const uint64_t *offs,
                             const uint64_t *lens, uint32_t n, emsg_message *out, uint64_t *n_entries);
int64_t emsg_copy_entries(ewal_ctx *ctx, uint64_t first, ewal_entry *out, int64_t cap);
int64_t emsg_copy_segments(ewal_ctx *ctx, uint64_t first, emsg_segment *out, int64_t cap);

/* ---- raft egress: raftpb.Message.Marshal, raft/raftpb/raft.pb.go:849-872,
 * 1000-1068 (called per outgoing message by send,
 * etcdserver/cluster_store.go:118-144), batched over n messages whose payload
 * is resident in HBM.  One emsg_out per message (a DEVICE array): */
typedef struct emsg_out {
  uint64_t type, to, from, term, log_term, index, commit;  /* uint64(m.Type) etc., as MarshalTo casts them */
  uint64_t ents_first, n_ents;       /* Entries = d_ents[ents_first, ents_first + n_ents) */
  uint64_t snap_index, snap_term;
  uint64_t snap_data_off, snap_data_len;     /* Snapshot.Data, a range of d_data */
  uint64_t snap_nodes_off, snap_n_nodes;     /* Snapshot.Nodes, a range of d_u64 (uint64 units) */
  uint64_t snap_removed_off, snap_n_removed; /* Snapshot.RemovedNodes, likewise */
  int32_t reject, pad;
} emsg_out;                                   /* 144 bytes */
typedef struct emsg_encoded { uint64_t off, len; } emsg_encoded;
/* Message i becomes d_out[h_out[i].off, + h_out[i].len), byte-identical to
 * (*Message).Marshal() with its nested Entry.MarshalTo (raft.pb.go:921-943:
 * field 4 always written, Type sign-extended as uint64(int32)) and
 * Snapshot.MarshalTo (:954-999: field 9 always written with a real body, so
 * Message{} is 24 bytes).  An entry's Data is d_data[data_off, + data_len)
 * (ewal_entry, as ReadAll, the write path and emsg_decode_batch_device return
 * them).  The messages are packed back to back in order of i, off[0] == 0;
 * *out_len is their sum and no byte of d_out at or past it is written, so
 * d_out with h_out's offs and lens feeds emsg_decode_batch_device directly.
 * The entry ranges (and the Data, Nodes, RemovedNodes ranges) of different
 * messages may coincide or overlap: a leader's fan-out shares one range
 * among its followers' messages.
 * d_out == NULL is a size query: h_out (nullable) and *out_len are filled,
 * nothing is written.  n == 0: EWAL_OK, *out_len = 0.
 * Errors, all decided before any byte of d_out is written:
 *   EWAL_E_INVAL  an entry range outside n_ents_total; a Data, Nodes or
 *                 RemovedNodes range outside its array, or one that wraps
 *                 (every entry of d_ents and every message is checked); an
 *                 entry with data_nil == 2 (its Data is not in d_data);
 *                 d_data or d_out not 16-byte aligned; d_out overlapping
 *                 d_data; n, n_ents_total or n_u64 >= 2^31 - 1; entry or
 *                 node sizes whose sum does not fit 64 bits
 *   EWAL_E_NOMEM  the total is greater than cap
 * A compute call on the ctx (it invalidates ewal_copy_records like the
 * others) that runs on the ctx's stream (ewal_ctx_set_stream); a repeated
 * call of the same or a smaller shape allocates nothing.
 * XXX_unrecognized of Message, Entry and Snapshot is not encoded: etcd's own
 * encoder never produces it and ewal_entry has no place for it. */
int emsg_encode_batch_device(ewal_ctx *ctx, const void *d_data, uint64_t data_len_total,
                             const emsg_out *d_msgs, uint64_t n,
                             const ewal_entry *d_ents, uint64_t n_ents_total,
                             const uint64_t *d_u64, uint64_t n_u64,
                             void *d_out, uint64_t cap,
                             emsg_encoded *h_out /* host, n, nullable */, uint64_t *out_len);
/* Host only: the exact sum of Message.Size() over host copies of the same
 * arrays; ~0 when it does not fit 64 bits or a range lies outside its array. */
uint64_t emsg_encode_size(const emsg_out *h_msgs, uint64_t n, const ewal_entry *h_ents, uint64_t n_ents_total,
                          const uint64_t *h_u64, uint64_t n_u64);
/* For bindings / tests: the bytes of d_out one wave of the body kernel owns,
 * sizeof(emsg_out), sizeof(emsg_encoded). */
uint32_t emsg_encode_tile_bytes(void);
uint32_t emsg_out_size(void);
uint32_t emsg_encoded_size(void);

#ifdef __cplusplus
}
#endif
#endif
