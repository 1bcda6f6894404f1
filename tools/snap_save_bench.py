#!/usr/bin/env python3
"""Device-time benchmark of the batched Snapshotter.save (esnap_save_packed_device).

Input: the configs[3] resident set of bench.py's `snap` workload -- sizes
log-uniform 1-256 MiB (random.Random(4)), drawn until --size-gib (16 GiB: 348
snapshots) -- as raw Data on the device, every Data at a 16-byte aligned
offset (ewal_crc32_update_device, the comparison's CRC, needs that).

Lines (median of --steps steps after --warmup, the three interleaved per step):
  fused     esnap_save_packed_device: HIP events around its two kernels
  d2d       hipMemcpyDtoDAsync of every Data range (the same sum of bytes), HIP
            events on the null stream: the floor of a 1-read-1-write pass
  two_pass  what the parent commit offers: ewal_crc32_update_device over the
            same bytes in ONE call (its k_stream pass's device time,
            ewal_last_stream_ms -- the scan kernels after it are left out, in
            the comparison's favour) plus that same d2d copy
GB/s figures are 2 x sum(data_len) over the time (one read + one write of
every Data byte), for all three lines.  Prints one JSON line; --out writes it
to a file too.  One process; needs the GPU.

--shape single / small time the two extreme shapes instead -- one 256 MiB
snapshot, and 10,000 snapshots log-uniform 4-64 KiB -- to show the tile grid
fills the device in both.
"""
import argparse
import ctypes as C
import json
import math
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from etcd_amd import _lib as L  # noqa: E402
from etcd_amd import snap as S  # noqa: E402
from etcd_amd import wal as W  # noqa: E402


def hip_check(rc):
    if rc != 0:
        raise RuntimeError("HIP error %d" % rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-gib", type=float, default=16.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", choices=["set", "single", "small"], default="set")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hip = C.CDLL("libamdhip64.so.7")
    rng = random.Random(4)
    budget = int(a.size_gib * (1 << 30))
    pool = np.random.default_rng(4).integers(0, 256, size=(256 << 20) + 4096, dtype=np.uint8)
    ctx = W.Context(0)
    snaps, total = [], 0
    lo, hi = ((4 << 10), (64 << 10)) if a.shape == "small" else ((1 << 20), (256 << 20))
    while (len(snaps) < 10000) if a.shape == "small" else (total < budget and not (a.shape == "single" and snaps)):
        n = (256 << 20) if a.shape == "single" else int(math.exp(rng.uniform(math.log(lo), math.log(hi))))
        snaps.append(dict(data_off=total, data_len=n, index=len(snaps) + 1, term=1, nodes=[1, 2, 3],
                          pool_off=rng.randrange(0, len(pool) - n)))
        total += (n + 15) // 16 * 16
    dbuf = ctx.alloc(total + 16)
    t0 = time.time()
    for s in snaps:
        dbuf.upload_ptr(pool.ctypes.data + s["pool_off"], s["data_len"], s["data_off"])
    gen_s = time.time() - t0
    nbytes = sum(s["data_len"] for s in snaps)
    cap = S.save_bound(snaps)
    dout = ctx.alloc(cap)

    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        hip_check(hip.hipEventCreate(C.byref(e)))

    def fused():
        res = S.save_packed(ctx, dbuf, total, snaps, dout, cap)
        return float(L.lib.ewal_last_device_ms(ctx.handle)), res

    def d2d():
        hip_check(hip.hipEventRecord(ev[0], None))
        for s in snaps:
            hip_check(hip.hipMemcpyDtoDAsync(C.c_void_p(dout.ptr.value + s["data_off"]),
                                             C.c_void_p(dbuf.ptr.value + s["data_off"]), C.c_size_t(s["data_len"]), None))
        hip_check(hip.hipEventRecord(ev[1], None))
        hip_check(hip.hipEventSynchronize(ev[1]))
        ms = C.c_float()
        hip_check(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
        return ms.value

    def crc():
        out = C.c_uint32()
        t = time.perf_counter()
        L.check(L.lib.ewal_crc32_update_device(ctx.handle, 0, L.CASTAGNOLI, dbuf.ptr, total, C.byref(out)))
        wall = (time.perf_counter() - t) * 1e3
        return float(L.lib.ewal_last_stream_ms(ctx.handle)), wall

    lines = {"fused": [], "d2d": [], "two_pass": [], "crc_stream": [], "crc_call_wall": [], "fused_call_wall": []}
    first = None
    for k in range(a.warmup + a.steps):
        t = time.perf_counter()
        f, res = fused()
        fw = (time.perf_counter() - t) * 1e3
        if first is None:
            first = res
            # the files verify on the read side (loadSnap's CRC check)
            st, sc, cc = S.verify_packed(dout, cap, [r[0] for r in res], [r[1] for r in res])
            assert st == [L.OK] * len(snaps) and sc == cc == [r[2] for r in res]
        assert res == first
        d = d2d()
        c, cw = crc()
        if k >= a.warmup:
            lines["fused"].append(f)
            lines["d2d"].append(d)
            lines["crc_stream"].append(c)
            lines["two_pass"].append(c + d)
            lines["crc_call_wall"].append(cw)
            lines["fused_call_wall"].append(fw)

    def summ(v):
        q = statistics.quantiles(v, n=4)
        med = statistics.median(v)
        return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "iqr_ms": round(q[2] - q[0], 4), "gbps_2x_data": round(2 * nbytes / med / 1e6, 1)}

    out = {k: summ(v) for k, v in lines.items()}
    spread = max(out["fused"]["max_ms"] - out["fused"]["min_ms"], out["two_pass"]["max_ms"] - out["two_pass"]["min_ms"])
    gain = out["two_pass"]["median_ms"] - out["fused"]["median_ms"]
    result = {
        "tool": "tools/snap_save_bench.py",
        "shape": a.shape,
        "input": "%s: %d snapshots, %.3f GiB of Data, sizes %s (random.Random(4)), 16-byte aligned on the device" %
                 ({"set": "configs[3] resident set", "single": "one snapshot", "small": "many small snapshots"}[a.shape],
                  len(snaps), nbytes / (1 << 30),
                  "256 MiB" if a.shape == "single" else "log-uniform %d KiB-%d KiB" % (lo >> 10, hi >> 10)),
        "data_bytes": nbytes, "snapshots": len(snaps), "steps": a.steps, "warmup": a.warmup,
        "tile_bytes": S.SAVE_TILE, "upload_s": round(gen_s, 2),
        "lines": out,
        "fused_over_d2d": round(out["fused"]["median_ms"] / out["d2d"]["median_ms"], 3),
        "two_pass_over_fused": round(out["two_pass"]["median_ms"] / out["fused"]["median_ms"], 3),
        "spread_ms_max_minus_min": round(spread, 4),
        "fused_beats_two_pass_by_more_than_spread": bool(gain > spread),
    }
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    ctx.close()
    return 0 if result["fused_beats_two_pass_by_more_than_spread"] else 1


if __name__ == "__main__":
    sys.exit(main())
