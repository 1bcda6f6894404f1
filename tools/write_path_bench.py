#!/usr/bin/env python3
"""Wall-time benchmark of the batched WAL write path: ewal_encode_entries_device
and ewal_save_device over the same entries.

Input: --entries (64 Ki) entries of --bytes (1 KiB) Data each, Term 5, Index
1.., resident on the device; the same batch as ewal_entry[] for the one call
and as EWAL_SAVE_ENTRY records for the other.

Lines (median of --steps calls after --warmup, the two interleaved per step):
  encode  wall time of the synchronous ewal_encode_entries_device call
  save    wall time of the synchronous ewal_save_device call (with h_rec_off)
Both calls end in a stream synchronise, so the host clock covers the device
work and the two decision points in between.  GB/s figures are output bytes
over the median.  The first step's frames, CRC and offsets are checked against
the oracle's writer.  Prints one JSON line; --out writes it to a file too.
One process, one library (EWAL_LIB_PATH selects another build of it for an
A/B run: alternate fresh processes, as tools/ab_run.py does).  Needs the GPU.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=64 << 10)
    ap.add_argument("--bytes", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from etcd_amd import _lib as L
    from etcd_amd import wal as W
    from oracle import oracle as O   # checker only

    n, prev = a.entries, 0x9E3779B1
    data = np.random.default_rng(6).integers(0, 256, size=n * a.bytes, dtype=np.uint8)
    ents, recs = (L.EntryDesc * n)(), (L.SaveRec * n)()
    for i in range(n):
        e, r = ents[i], recs[i]
        e.term, e.index, e.data_off, e.data_len = 5, i + 1, i * a.bytes, a.bytes
        r.kind, r.a, r.b, r.data_off, r.data_len = L.SAVE_ENTRY, 5, i + 1, i * a.bytes, a.bytes
    cap = len(data) + 80 * n + 64
    ctx = W.Context(0)
    d_data, d_ents, d_recs, d_out = (ctx.alloc(len(data) + 64), ctx.alloc(C.sizeof(ents)), ctx.alloc(C.sizeof(recs)),
                                     ctx.alloc(cap))
    d_data.upload_ptr(data.ctypes.data, len(data))
    d_ents.upload(bytes(ents))
    d_recs.upload(bytes(recs))
    out_len, crc, offs = C.c_uint64(), C.c_uint32(), (C.c_uint64 * n)()

    def call(which):
        args = (ctx.handle, d_data.ptr, len(data), d_ents.ptr if which == "encode" else d_recs.ptr, n, prev, d_out.ptr,
                cap, C.byref(out_len), C.byref(crc))
        t = time.perf_counter()
        rc = L.lib.ewal_encode_entries_device(*args) if which == "encode" else L.lib.ewal_save_device(*args, offs)
        ms = (time.perf_counter() - t) * 1e3
        L.check(rc)
        return ms

    want = None
    lines = {"encode": [], "save": []}
    for k in range(a.warmup + a.steps):
        for which in ("encode", "save"):
            ms = call(which)
            if k == 0:
                if want is None:
                    w = O.WalEncoder(prev)
                    woffs = []
                    for i in range(n):
                        woffs.append(len(w.getvalue()) if i < 64 else None)
                        w.save_entry(0, 5, i + 1, data[i * a.bytes:(i + 1) * a.bytes].tobytes())
                    want = (w.getvalue(), w.crc, woffs[:64])
                assert (out_len.value, crc.value) == (len(want[0]), want[1]), which
                assert d_out.download(out_len.value) == want[0], which
                if which == "save":
                    assert list(offs[:64]) == want[2]
            if k >= a.warmup:
                lines[which].append(ms)

    def summ(v):
        med = statistics.median(v)
        return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "gbps_out": round(len(want[0]) / med / 1e6, 1)}

    result = {"tool": "tools/write_path_bench.py", "lib": os.path.basename(L.LIB_PATH),
              "input": "%d entries of %d B Data" % (n, a.bytes), "data_bytes": int(len(data)),
              "out_bytes": len(want[0]), "steps": a.steps, "warmup": a.warmup,
              "what": "wall time of the synchronous call", "lines": {k: summ(v) for k, v in lines.items()}}
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    for b in (d_data, d_ents, d_recs, d_out):
        b.free()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
