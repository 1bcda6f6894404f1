#!/usr/bin/env python3
"""Device-time benchmark of the batched follower step (efollow_step_batch_device).

Shapes (--shape; one process per shape, --shape all starts one child per shape
in turn):
  app1     1 Mi follower groups, one msgApp with one new entry each
  beat     1 Mi follower groups, one heartbeat (an empty msgApp with a commit) each
  burst    16 Ki follower groups, one msgApp with 64 new entries each
  restore  64 Ki follower groups, one msgSnap each (three Nodes)
  catchup  one follower that gets ONE msgApp of 1 Mi entries, next to 100 000
           groups that get a heartbeat

Every group has a two-entry log at offset 1000 + g in its own window of d_ents;
the messages' entries lie in a source array of their own.  Every step restores
the four group arrays, d_snaps and d_ents from pristine device copies first
(outside the timed window): the call updates them in place.

Lines (--warmup 3 then --steps 20):
  step   the call's device time: HIP events from before its first memset to
         after its last kernel (ewal_last_device_ms; the host's decision point
         between the counting and the apply pass is inside)
  size   the same call with d_msgs == NULL (results alone)
  wall   the real call's host wall time
  elog   in app1's process only: elog_append_batch_device (existing code) on the
         equivalent elog_group / d_terms state and the same messages, timed the
         same way: the yardstick.  It writes 8 B of term per entry where this
         call writes 40 B, and carries no term switch, lead, elapsed or progress.
The first step's results are checked against what the shape must give.  Prints
one JSON line; --out writes it to a file too.  Needs the GPU.
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
SHAPES = ["app1", "beat", "burst", "restore", "catchup"]
TERM = 5
APPENDED, RESTORED = 3, 5
# shape: (groups, entries a message, description)
SPEC = {"app1": (1 << 20, 1, "1 Mi groups, one msgApp with one entry each"),
        "beat": (1 << 20, 0, "1 Mi heartbeats"),
        "burst": (1 << 14, 64, "16 Ki groups x 64 entries"),
        "restore": (1 << 16, 0, "64 Ki restores"),
        "catchup": (100001, 1 << 20, "one 1 Mi-entry catch-up plus 100 k heartbeats")}


def build(shape, G):
    """(groups (G, 32), pstate (G, 4), vstate (G, 8), rstate (G, 8), snaps (G, 8), ents, src, in_snaps, u64,
    msgs (G, 12), entries per message (G,)) as uint64 arrays."""
    _, per, _ = SPEC[shape]
    k = np.arange(G, dtype=np.uint64)
    ne = np.full(G, per, dtype=np.uint64)
    if shape == "catchup":
        ne[:] = 0
        ne[G // 2] = per
    cap = ne + np.uint64(2)
    first = np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.uint64)
    off = np.uint64(1000) + k
    g = np.zeros((G, 32), dtype=np.uint64)
    g[:, 0], g[:, 1], g[:, 2], g[:, 3], g[:, 4], g[:, 5], g[:, 6] = 2, TERM, off, off, 2, first, 3
    g[:, 7:10] = np.arange(1, 4, dtype=np.uint64)
    g[:, 21:24] = (off + np.uint64(2))[:, None]
    ps = np.zeros((G, 4), dtype=np.uint64)
    ps[:, 0], ps[:, 1] = cap, off + np.uint64(2)
    vs = np.zeros((G, 8), dtype=np.uint64)
    vs[:, 1], vs[:, 2], vs[:, 3] = 1, 1, 3                 # voted for 1, led by 1, three ticks since
    rs = np.zeros((G, 8), dtype=np.uint64)
    rs[:, 0], rs[:, 1], rs[:, 2], rs[:, 6] = TERM, 1, off, off
    sn = np.zeros((G, 8), dtype=np.uint64)
    ents = np.zeros((int(cap.sum()), 5), dtype=np.uint64)
    for j in range(2):
        ents[first + np.uint64(j), 0] = TERM
        ents[first + np.uint64(j), 1] = off + np.uint64(j)
        ents[first + np.uint64(j), 4] = 1 << 32
    nsrc = int(ne.sum())
    sfirst = np.concatenate([[0], np.cumsum(ne)[:-1]]).astype(np.uint64)
    src = np.zeros((nsrc, 5), dtype=np.uint64)
    if nsrc:
        owner = np.repeat(k, ne.astype(np.int64))
        within = np.arange(nsrc, dtype=np.uint64) - sfirst[owner.astype(np.int64)]
        src[:, 0] = TERM
        src[:, 1] = off[owner.astype(np.int64)] + np.uint64(2) + within
        src[:, 2] = np.arange(nsrc, dtype=np.uint64) * np.uint64(16)
        src[:, 3] = 16
    m = np.zeros((G, 12), dtype=np.uint64)
    m[:, 0], m[:, 2], m[:, 3] = k, 1, TERM
    if shape == "restore":
        m[:, 1], m[:, 10] = 7, k
        ins = np.zeros((G, 8), dtype=np.uint64)
        ins[:, 0], ins[:, 1], ins[:, 4], ins[:, 5] = off + np.uint64(50), TERM, np.uint64(3) * k, 3
        u64 = np.tile(np.arange(1, 4, dtype=np.uint64), G)
    else:
        m[:, 1], m[:, 4], m[:, 5], m[:, 6] = 3, off + np.uint64(1), TERM, off + np.uint64(1) + ne
        m[:, 7], m[:, 8], m[:, 9] = np.where(ne > 0, sfirst, 0), ne, 1 << 20
        ins, u64 = np.zeros((0, 8), dtype=np.uint64), np.zeros(0, dtype=np.uint64)
    return g, ps, vs, rs, sn, ents, src, ins, u64, m, ne


def run_shape(a):
    from etcd_amd import _lib as L
    from etcd_amd import wal as W

    def hip_check(rc):
        if rc != 0:
            raise RuntimeError("HIP error %d" % rc)

    hip = C.CDLL("libamdhip64.so.7")
    G0, _, desc = SPEC[a.shape]
    G = a.groups or G0
    g, ps, vs, rs, sn, ents, src, ins, u64, m, ne = build(a.shape, G)
    total_app = int(ne.sum())
    ctx = W.Context(0)

    def up(arr):
        d = ctx.alloc(arr.nbytes + 64)
        if arr.nbytes:
            arr = np.ascontiguousarray(arr)
            d.upload_ptr(arr.ctypes.data, arr.nbytes)
        return d

    host = (g, ps, vs, rs, sn, ents)
    live = [up(x) for x in host]
    pristine = [up(x) for x in host]
    d_src, d_ins, d_u64, d_in = up(src), up(ins), up(u64), up(m)
    d_res, d_msgs = ctx.alloc(G * 96 + 64), ctx.alloc(G * 144 + 64)
    nm, na, nr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def restore(lv, pr, hs):
        for d, p, arr in zip(lv, pr, hs):
            hip_check(hip.hipMemcpyDtoD(d.ptr, p.ptr, C.c_size_t(arr.nbytes)))
        hip_check(hip.hipDeviceSynchronize())

    def call(out=True):
        t = time.perf_counter()
        L.check(L.lib.efollow_step_batch_device(ctx.handle, live[0].ptr, live[1].ptr, live[2].ptr, live[3].ptr, G,
                                                live[4].ptr, live[5].ptr, len(ents), d_src.ptr, len(src), d_ins.ptr,
                                                len(ins), d_u64.ptr, len(u64), d_in.ptr, G, d_res.ptr,
                                                d_msgs.ptr if out else None, G, C.byref(nm), C.byref(na),
                                                C.byref(nr)))
        return float(L.lib.ewal_last_device_ms(ctx.handle)), (time.perf_counter() - t) * 1e3

    lines = {"step": [], "size": [], "wall": []}
    restoring = a.shape == "restore"
    for k in range(a.warmup + a.steps):
        restore(live, pristine, host)
        s, _ = call(out=False)
        assert (nm.value, na.value, nr.value) == (G, total_app, G if restoring else 0)
        e, w = call()
        if k == 0:
            res = np.frombuffer(d_res.download(G * 96), dtype=np.uint64).reshape(G, 12)
            off = g[:, 3]
            assert (res[:, 0] == np.uint64((RESTORED if restoring else APPENDED) << 32)).all()
            assert (res[:, 1] == np.arange(G, dtype=np.uint64)).all() and (res[:, 2] == 1).all()
            assert (res[:, 5] == ne).all()
            g1 = np.frombuffer(live[0].download(g.nbytes), dtype=np.uint64).reshape(G, 32)
            out = np.frombuffer(d_msgs.download(G * 144), dtype=np.uint64).reshape(G, 18)
            assert (out[:, 0] == 4).all() and (out[:, 1] == 1).all() and (out[:, 2] == 2).all()
            if restoring:
                assert (g1[:, 3] == off + np.uint64(50)).all() and (g1[:, 4] == 1).all()
                assert (out[:, 5] == off + np.uint64(50)).all()
                s1 = np.frombuffer(live[4].download(sn.nbytes), dtype=np.uint64).reshape(G, 8)
                assert (s1 == ins).all()
            else:
                assert (g1[:, 4] == ne + np.uint64(2)).all() and (g1[:, 2] == off + np.uint64(1) + ne).all()
                assert (out[:, 5] == off + np.uint64(1) + ne).all()
                e1 = np.frombuffer(live[5].download(ents.nbytes), dtype=np.uint64).reshape(-1, 5)
                if total_app:
                    dst = (np.repeat(g[:, 5] + np.uint64(2), ne.astype(np.int64)) +
                           (np.arange(total_app, dtype=np.uint64) -
                            np.repeat(m[:, 7], ne.astype(np.int64)))).astype(np.int64)
                    want = src.copy()
                    want[:, 2] += np.uint64(1 << 20)
                    assert (e1[dst] == want).all()
            parts = {"msg_read": 96 * G, "group_read": (256 + 32 + 64 + 64) * G, "result": 96 * G, "response": 144 * G,
                     "scratch": 2 * (8 + 48) * G, "entry_copy": 80 * total_app,
                     "snapshot": ((64 + 24) + 64 + 40) * G if restoring else 0,
                     # the changed words: elapsed, and committed / nlog or the restore's
                     "group_write": (8 + (16 if total_app or not restoring else 0) + (14 * 8 if restoring else 0)) * G}
            how = ("per record 96 B of message, 416 B of its group's four records (read by both passes: counted once), "
                   "96 B of result, 144 B of response, 56 B of scratch written and read, the words that changed; per "
                   "copied entry 40 B read and 40 B written; per restore the snapshot, its Nodes, d_snaps[g] and the "
                   "log's one entry")
        if k >= a.warmup:
            lines["step"].append(e)
            lines["size"].append(s)
            lines["wall"].append(w)
    nbytes = sum(parts.values())

    extra = {}
    if a.shape == "app1":
        # existing code on the equivalent state: elog_group rows, terms-only windows of three
        for d in live + pristine + [d_res, d_msgs]:
            d.free()
        lg = np.zeros((G, 8), dtype=np.uint64)
        lg[:, 0], lg[:, 1], lg[:, 2], lg[:, 3], lg[:, 4], lg[:, 5] = 2, TERM, g[:, 3], g[:, 3] + np.uint64(2), g[:, 3], 2
        lg[:, 6], lg[:, 7] = np.arange(G, dtype=np.uint64) * np.uint64(3), 3
        terms = np.zeros((G, 3), dtype=np.uint64)
        terms[:, :2] = TERM
        apps = np.zeros((G, 8), dtype=np.uint64)
        apps[:, 0], apps[:, 1], apps[:, 2], apps[:, 3], apps[:, 4] = m[:, 0], 1, m[:, 4], TERM, m[:, 6]
        apps[:, 5], apps[:, 6] = m[:, 7], m[:, 8]
        lhost = (lg, terms)
        llive, lprist = [up(x) for x in lhost], [up(x) for x in lhost]
        d_apps, d_lres, d_resp = up(apps), ctx.alloc(G * 48 + 64), ctx.alloc(G * 144 + 64)
        lines["elog"] = []
        for k in range(a.warmup + a.steps):
            restore(llive, lprist, lhost)
            L.check(L.lib.elog_append_batch_device(ctx.handle, llive[0].ptr, G, llive[1].ptr, 3 * G, d_apps.ptr, G,
                                                   d_src.ptr, len(src), d_lres.ptr, d_resp.ptr, C.byref(nm),
                                                   C.byref(na)))
            assert (nm.value, na.value) == (G, G)
            if k >= a.warmup:
                lines["elog"].append(float(L.lib.ewal_last_device_ms(ctx.handle)))
        lmed, med = statistics.median(lines["elog"]), statistics.median(lines["step"])
        extra = {"elog_ns_per_message": round(lmed * 1e6 / G, 4), "step_over_elog_per_message": round(med / lmed, 3),
                 "step_over_elog_per_appended_byte": round((med / 40) / (lmed / 8), 3)}

    def summ(v):
        med = statistics.median(v)
        return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    med = statistics.median(lines["step"])
    gbps = nbytes / med / 1e6
    result = {"tool": "tools/follow_bench.py", "shape": a.shape, "input": desc, "records": G, "entries": total_app,
              "steps": a.steps, "warmup": a.warmup, "lines": {k: summ(v) for k, v in lines.items()},
              "ms_per_call": round(med, 4), "ns_per_record": round(med * 1e6 / G, 4),
              "ns_per_entry": round(med * 1e6 / total_app, 4) if total_app else None, "algorithmic_bytes": nbytes,
              "bytes": how, "bytes_parts": parts, "gbps_algorithmic": round(gbps, 1), "hbm_peak_gbps": HBM_PEAK_GBPS,
              "hbm_frac": round(gbps / HBM_PEAK_GBPS, 4)}
    result.update(extra)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    ctx.close()
    return 0


def run_all(a):
    outdir = a.out or os.path.join(ROOT, "profiles", "follow")
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
