#!/usr/bin/env python3
"""Device-time benchmark of the batched log compaction (ecompact_batch_device).

Shapes (--shape; one process per shape, --shape all starts one child per shape
in turn):
  scan       1 Mi groups, ECOMPACT_AT_APPLIED, none due: the price of the policy pass
  tail       1 Mi groups with 64-entry windows, drop 48, keep 16 (disjoint)
  overlap    the same, drop 16, keep 48 (overlapping: staged)
  snapcount  1 024 groups, drop 10 000, keep 1 000 (etcd's default snapCount)
  worst      one group, 1 Mi entries kept, shift 1

Every group's log fills its window of d_ents, everything committed and applied.
Every step restores d_groups, d_pstate, d_snaps and d_ents from pristine device
copies first (outside the timed window): the call updates them in place.

Lines (--warmup 3 then --steps 20):
  step   the call's device time: HIP events from before its first memset to
         after its last kernel (ewal_last_device_ms; the host's decision point
         between the counting and the apply pass is inside)
  peek   the same call with ECOMPACT_PEEK (results alone)
  wall   the real call's host wall time
Yardsticks, existing code and not the code under test, in the same process:
  memcpy  hipMemcpyDtoDAsync of the moved entries' byte count, HIP events around
          it (twice that count -- two copies -- where the class is staged: it
          moves every byte twice)
  ready   eready_batch_device's peek over the same G
The first step's results, group records, snapshots and a sample of the moved
entries are checked against what the shape must give.  Prints one JSON line;
--out writes it to a file too.  Needs the GPU.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK_GBPS = 8000.0
SHAPES = ["scan", "tail", "overlap", "snapcount", "worst"]
TERM = 5
NOT_DUE, COMPACTED = 1, 2
# shape: (groups, entries a window, entries dropped, description)
SPEC = {"scan": (1 << 20, 2, 0, "1 Mi groups, AT_APPLIED, none due"),
        "tail": (1 << 20, 64, 48, "1 Mi groups x 64 entries, drop 48, keep 16 (disjoint)"),
        "overlap": (1 << 20, 64, 16, "1 Mi groups x 64 entries, drop 16, keep 48 (staged)"),
        "snapcount": (1 << 10, 11000, 10000, "1 024 groups, drop 10 000, keep 1 000"),
        "worst": (1, (1 << 20) + 1, 1, "one group, 1 Mi entries kept, shift 1")}


def build(shape, G):
    """(groups (G, 32), pstate (G, 4), vstate (G, 8), rstate (G, 8), snaps (G, 8), ents, reqs (G, 12)) as uint64 arrays."""
    _, per, drop, _ = SPEC[shape]
    k = np.arange(G, dtype=np.uint64)
    first = k * np.uint64(per)
    off = np.uint64(1000) + k
    last = off + np.uint64(per - 1)
    g = np.zeros((G, 32), dtype=np.uint64)
    g[:, 0], g[:, 1], g[:, 2], g[:, 3], g[:, 4], g[:, 5], g[:, 6] = 1, TERM, last, off, per, first, 3
    g[:, 7:10] = np.arange(1, 4, dtype=np.uint64)
    g[:, 14:17] = last[:, None]
    g[:, 21:24] = (last + np.uint64(1))[:, None]
    ps = np.zeros((G, 4), dtype=np.uint64)
    ps[:, 0], ps[:, 1] = per, last + np.uint64(1)
    vs = np.zeros((G, 8), dtype=np.uint64)
    vs[:, 0], vs[:, 2] = 2, 1                              # a leader, led by itself
    rs = np.zeros((G, 8), dtype=np.uint64)
    rs[:, 0], rs[:, 2], rs[:, 3], rs[:, 4], rs[:, 6] = TERM, last, 1, 2, last
    sn = np.zeros((G, 8), dtype=np.uint64)
    n = G * per
    ents = np.zeros((n, 5), dtype=np.uint64)
    ents[:, 0] = TERM
    ents[:, 1] = np.arange(n, dtype=np.uint64) % np.uint64(per) + np.repeat(off, per)
    ents[:, 2] = np.arange(n, dtype=np.uint64) * np.uint64(16)
    ents[:, 3] = 16
    q = np.zeros((G, 12), dtype=np.uint64)
    q[:, 0] = k
    if shape == "scan":
        q[:, 1], q[:, 3] = 1, 10000
    else:
        q[:, 2] = off + np.uint64(drop)
        q[:, 4], q[:, 5], q[:, 7] = k % np.uint64(64), 64, 3
    return g, ps, vs, rs, sn, ents, q


def run_shape(a):
    from etcd_amd import _lib as L
    from etcd_amd import wal as W

    def hip_check(rc):
        if rc != 0:
            raise RuntimeError("HIP error %d" % rc)

    hip = C.CDLL("libamdhip64.so.7")
    G0, per, drop, desc = SPEC[a.shape]
    G = a.groups or G0
    g, ps, vs, rs, sn, ents, q = build(a.shape, G)
    keep = per - drop if a.shape != "scan" else 0
    moved = G * keep if drop else 0
    staged = 0 < drop < keep
    ctx = W.Context(0)

    def up(arr):
        d = ctx.alloc(arr.nbytes + 64)
        if arr.nbytes:
            arr = np.ascontiguousarray(arr)
            d.upload_ptr(arr.ctypes.data, arr.nbytes)
        return d

    host = (g, ps, sn, ents)
    pristine = [up(x) for x in host]
    live = [ctx.alloc(x.nbytes + 64) for x in host]      # filled by restore()
    d_vs, d_rs, d_in = up(vs), up(rs), up(q)
    d_res, d_rres = ctx.alloc(G * 64 + 64), ctx.alloc(G * 96 + 64)
    nc, nm = C.c_uint64(0), C.c_uint64(0)

    def restore():
        for d, p, arr in zip(live, pristine, host):
            hip_check(hip.hipMemcpyDtoD(d.ptr, p.ptr, C.c_size_t(arr.nbytes)))
        hip_check(hip.hipDeviceSynchronize())

    def call(flags=0):
        t = time.perf_counter()
        L.check(L.lib.ecompact_batch_device(ctx.handle, live[0].ptr, live[1].ptr, d_rs.ptr, G, live[2].ptr, live[3].ptr,
                                            len(ents), 1 << 20, 64, d_in.ptr, G, d_res.ptr, flags, C.byref(nc),
                                            C.byref(nm)))
        return float(L.lib.ewal_last_device_ms(ctx.handle)), (time.perf_counter() - t) * 1e3

    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        hip_check(hip.hipEventCreate(C.byref(e)))
    d_scr = ctx.alloc(max(moved, 1) * 40 + 64) if moved else None

    def memcpy_ms():
        """hipMemcpyDtoDAsync of the moved bytes out of the pristine entries (twice for the staged class)."""
        hip_check(hip.hipEventRecord(ev[0], None))
        for _ in range(2 if staged else 1):
            hip_check(hip.hipMemcpyDtoDAsync(d_scr.ptr, pristine[3].ptr, C.c_size_t(moved * 40), None))
        hip_check(hip.hipEventRecord(ev[1], None))
        hip_check(hip.hipEventSynchronize(ev[1]))
        ms = C.c_float(0)
        hip_check(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
        return float(ms.value)

    def ready_ms():
        ns, nr = C.c_uint64(0), C.c_uint64(0)
        L.check(L.lib.eready_batch_device(ctx.handle, live[0].ptr, live[1].ptr, d_vs.ptr, d_rs.ptr, G, live[2].ptr,
                                          live[3].ptr, len(ents), None, G, d_rres.ptr, None, 0, C.byref(ns),
                                          C.byref(nr)))
        return float(L.lib.ewal_last_device_ms(ctx.handle))

    lines = {"step": [], "peek": [], "wall": [], "ready": []}
    if moved:
        lines["memcpy"] = []
    done = 0 if a.shape == "scan" else G
    for k in range(a.warmup + a.steps):
        restore()
        r = ready_ms()
        m = memcpy_ms() if moved else None
        p, _ = call(flags=1)
        assert (nc.value, nm.value) == (done, moved)
        e, w = call()
        assert (nc.value, nm.value) == (done, moved)
        if k == 0:
            res = np.frombuffer(d_res.download(G * 64), dtype=np.uint64).reshape(G, 8)
            g1 = np.frombuffer(live[0].download(g.nbytes), dtype=np.uint64).reshape(G, 32)
            if a.shape == "scan":
                assert (res[:, 0] == np.uint64(NOT_DUE << 32)).all() and not res[:, 1:].any() and (g1 == g).all()
            else:
                idx = g[:, 3] + np.uint64(drop)
                assert (res[:, 0] == np.uint64(COMPACTED << 32)).all() and (res[:, 1] == idx).all()
                assert (res[:, 2] == TERM).all() and (res[:, 3] == keep).all() and (res[:, 4] == drop).all()
                assert (g1[:, 3] == idx).all() and (g1[:, 4] == keep).all()
                s1 = np.frombuffer(live[2].download(sn.nbytes), dtype=np.uint64).reshape(G, 8)
                assert (s1[:, 0] == idx).all() and (s1[:, 1] == TERM).all() and (s1[:, 2:] == q[:, 4:10]).all()
                for gi in sorted({0, G // 2, G - 1}):      # a sample of windows: the tail lies at the base now
                    win = np.frombuffer(live[3].download(per * 40, gi * per * 40), dtype=np.uint64).reshape(per, 5)
                    assert (win[:keep] == ents[gi * per + drop:(gi + 1) * per]).all()
                    assert (win[max(keep, drop):] == ents[gi * per + max(keep, drop):(gi + 1) * per]).all()
            parts = {"request_read": 2 * 96 * G, "group_read": 2 * (256 + 32 + 8) * G, "result": 64 * G,
                     "scratch": 2 * 48 * G, "snapshot": 64 * done, "group_write": 24 * done,
                     "entry_move": (160 if staged else 80) * moved}
            how = ("per request 96 B of request and 296 B of its group's records, read by both passes, 64 B of result, "
                   "48 B of descriptor written and read; per compacted group 64 B of snapshot and the three words that "
                   "changed; per moved entry 40 B read and 40 B written, twice where the class is staged")
        if k >= a.warmup:
            lines["step"].append(e)
            lines["peek"].append(p)
            lines["wall"].append(w)
            lines["ready"].append(r)
            if moved:
                lines["memcpy"].append(m)
    nbytes = sum(parts.values())

    def summ(v):
        med = statistics.median(v)
        return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    med, pk, rd = (statistics.median(lines[x]) for x in ("step", "peek", "ready"))
    gbps = nbytes / med / 1e6
    result = {"tool": "tools/compact_bench.py", "shape": a.shape, "input": desc, "requests": G, "compacted": done,
              "entries_moved": moved, "move_class": "none" if not moved else "staged" if staged else "disjoint",
              "steps": a.steps, "warmup": a.warmup, "lines": {k: summ(v) for k, v in lines.items()},
              "ms_per_call": round(med, 4), "ns_per_request": round(med * 1e6 / G, 4),
              "ns_per_entry": round(med * 1e6 / moved, 4) if moved else None, "algorithmic_bytes": nbytes,
              "bytes": how, "bytes_parts": parts, "gbps_algorithmic": round(gbps, 1), "hbm_peak_gbps": HBM_PEAK_GBPS,
              "hbm_frac": round(gbps / HBM_PEAK_GBPS, 4), "peek_over_ready_peek": round(pk / rd, 3),
              "step_over_ready_peek": round(med / rd, 3)}
    if moved:
        mc = statistics.median(lines["memcpy"])
        result.update(memcpy_bytes=moved * 40 * (2 if staged else 1), memcpy_copies=2 if staged else 1,
                      step_over_memcpy=round(med / mc, 3), step_minus_peek_over_memcpy=round((med - pk) / mc, 3))
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    ctx.close()
    return 0


def run_all(a):
    outdir = a.out or os.path.join(ROOT, "profiles", "compact")
    for s in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", s, "--steps", str(a.steps), "--warmup",
               str(a.warmup), "--out", os.path.join(outdir, "shape_%s.json" % s)]
        if a.groups:
            cmd += ["--groups", str(a.groups)]
        subprocess.check_call(cmd, timeout=a.child_timeout)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=SHAPES + ["all"], default="all")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=0, help="groups per shape (default: the shape's own)")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=None, help="a JSON file (one shape) or a directory (--shape all)")
    a = ap.parse_args()
    return run_all(a) if a.shape == "all" else run_shape(a)


if __name__ == "__main__":
    sys.exit(main())
