#!/usr/bin/env python3
"""Device-time benchmark of the three membership calls (econf_batch_device,
econf_scan_committed_device, econf_gate_batch_device).

Shapes, each over 1 Mi groups (--groups) in one process:
  add     one addNode of a new id per group of 3 peers
  remove  one removeNode of the middle peer per group of 3 peers
  scan    the bootstrap scan: 3 committed ConfChangeAddNode entries per group
          (3 Mi entries, 3 Mi requests)
  gate    one evote_msg (a msgVote) per group; every fourth group has removed
          its sender
Yardsticks, in the same process at the same G:
  tick    etick_batch_device on followers at elapsed 0 (tick_bench.py's quiet):
          the project's one-lane-per-group call over the same records
  memcpy  per shape a device-to-device copy of half the bytes the shape must
          read and write, so that the copy moves as many bytes as the shape

Every step restores the records a shape writes from pristine device copies
first, outside the timed window.  Lines (--warmup 3 then --steps 20): the
call's device time (ewal_last_device_ms: from before its first memset to after
its last kernel, the host's decision points inside) and the size query's.  The
first step's outputs are checked.  Writes profiles/conf/shape_<name>.json and
prints one JSON line per shape.  Needs the GPU.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK_GBPS = 8000.0
SHAPES = ["add", "remove", "scan", "gate"]
ELECTION, HEARTBEAT = 10, 1


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conf"))
    a = ap.parse_args()
    from etcd_amd import _lib as L
    from etcd_amd import wal as W

    hip = C.CDLL("libamdhip64.so.7")

    def hip_check(rc):
        if rc != 0:
            raise RuntimeError("HIP error %d" % rc)

    G = a.groups
    ctx = W.Context(0)
    k = np.arange(G, dtype=np.uint64)

    def up(arr):
        arr = np.ascontiguousarray(arr)
        d = ctx.alloc(arr.nbytes + 64)
        if arr.nbytes:
            d.upload_ptr(arr.ctypes.data, arr.nbytes)
        return d

    def down(d, like):
        return np.frombuffer(d.download(like.nbytes), dtype=like.dtype).reshape(like.shape)

    groups = np.zeros((G, 32), np.uint64)
    groups[:, 0], groups[:, 1], groups[:, 4], groups[:, 6] = 1, 5, 1, 3
    groups[:, 7:10] = [1, 2, 3]
    groups[:, 21:24] = 1
    pstate = np.zeros((G, 4), np.uint64)
    pstate[:, 0], pstate[:, 1], pstate[:, 2] = 8, 1, 1
    vstate, rstate, cstate = np.zeros((G, 8), np.uint64), np.zeros((G, 8), np.uint64), np.zeros((G, 16), np.uint64)
    host = dict(groups=groups, pstate=pstate, vstate=vstate, rstate=rstate, cstate=cstate)
    live = {n: up(v) for n, v in host.items()}
    pristine = {n: up(v) for n, v in host.items()}
    n1, n2 = C.c_uint64(0), C.c_uint64(0)

    def restore(names):
        for n in names:
            hip_check(hip.hipMemcpyDtoD(live[n].ptr, pristine[n].ptr, C.c_size_t(host[n].nbytes)))
        hip_check(hip.hipDeviceSynchronize())

    def ms():
        return float(L.lib.ewal_last_device_ms(ctx.handle))

    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip_check(hip.hipEventCreate(C.byref(ev0)))
    hip_check(hip.hipEventCreate(C.byref(ev1)))
    scratch = [ctx.alloc(640 * G + 64), ctx.alloc(640 * G + 64)]

    def memcpy_ms(nbytes):
        """A device-to-device copy of nbytes / 2 bytes: it reads and writes nbytes in all."""
        t = C.c_float(0)
        half = C.c_size_t(nbytes // 2)
        hip_check(hip.hipDeviceSynchronize())
        hip_check(hip.hipEventRecord(ev0, None))
        hip_check(hip.hipMemcpyDtoDAsync(scratch[0].ptr, scratch[1].ptr, half, None))
        hip_check(hip.hipEventRecord(ev1, None))
        hip_check(hip.hipEventSynchronize(ev1))
        hip_check(hip.hipEventElapsedTime(C.byref(t), ev0, ev1))
        return float(t.value)

    def summ(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    def timed(step, query, prepare, check, nbytes):
        lines = {"step": [], "query": [], "memcpy": []}
        for i in range(a.warmup + a.steps):
            prepare()
            q = query()
            s = step()
            if i == 0:
                check()
            m = memcpy_ms(nbytes)
            if i >= a.warmup:
                lines["step"].append(s)
                lines["query"].append(q)
                lines["memcpy"].append(m)
        return lines

    # ---- the yardstick: the tick over the same groups --------------------------------------------
    d_tres = ctx.alloc(G * 32 + 64)
    tick = []
    for i in range(a.warmup + a.steps):
        restore(["vstate"])
        L.check(L.lib.etick_batch_device(ctx.handle, live["groups"].ptr, live["vstate"].ptr, G, None, G, ELECTION,
                                         HEARTBEAT, None, 7, d_tres.ptr, None, 0, None, 0, C.byref(n1), C.byref(n2)))
        d_h, d_b = ctx.alloc(64), ctx.alloc(64)
        L.check(L.lib.etick_batch_device(ctx.handle, live["groups"].ptr, live["vstate"].ptr, G, None, G, ELECTION,
                                         HEARTBEAT, None, 7, d_tres.ptr, d_h.ptr, 0, d_b.ptr, 0, C.byref(n1),
                                         C.byref(n2)))
        d_h.free()
        d_b.free()
        assert (n1.value, n2.value) == (0, 0)
        if i >= a.warmup:
            tick.append(ms())
    d_tres.free()
    tick_med = statistics.median(tick)
    results = {}

    # ---- add / remove ------------------------------------------------------------------------------
    for shape, kind, node in (("add", 1, 900), ("remove", 2, 2)):
        reqs = np.zeros((G, 4), np.uint64)
        reqs[:, 0], reqs[:, 1], reqs[:, 2] = k, kind, node
        d_reqs, d_res, d_msgs = up(reqs), ctx.alloc(G * 48 + 64), ctx.alloc(144 + 64)

        def call(emit):
            L.check(L.lib.econf_batch_device(ctx.handle, live["groups"].ptr, live["pstate"].ptr, live["vstate"].ptr,
                                             live["rstate"].ptr, live["cstate"].ptr, G, None, None, 0, d_reqs.ptr, G,
                                             d_res.ptr, d_msgs.ptr if emit else None, 0, C.byref(n1), C.byref(n2)))
            assert (n1.value, n2.value) == (0, G)
            return ms()

        def check():
            g1 = down(live["groups"], groups)
            res = down(d_res, np.zeros((G, 6), np.uint64))
            assert (res[:, 0] == np.uint64(kind << 32)).all() and not down(live["pstate"], pstate)[:, 2].any()
            assert down(live["rstate"], rstate)[:, 7].all()
            if shape == "add":
                assert (g1[:, 6] == 4).all() and (g1[:, 10] == 900).all() and (g1[:, 24] == 1).all()
            else:
                assert (g1[:, 6] == 2).all() and (g1[:, 8] == 3).all() and (g1[:, 9] == 0).all()
                assert (down(live["cstate"], cstate)[:, :2] == [1, 2]).all()
        changed = 8 * ((4 if shape == "add" else 7) + 2 + (0 if shape == "add" else 2))
        parts = {"records_read": (256 + 32 + 64 + 16 + 128) * G, "requests_read": 2 * 32 * G, "scratch": 2 * 8 * G,
                 "result": 48 * G, "changed_words": changed * G}
        nbytes = sum(parts.values())
        lines = timed(lambda: call(True), lambda: call(False), lambda: restore(list(host)), check, nbytes)
        results[shape] = (lines, parts, G)
        for d in (d_reqs, d_res, d_msgs):
            d.free()

    # ---- scan ----------------------------------------------------------------------------------------
    body = [b"\x08" + varint(1000 + j) + b"\x10\x00\x18" + varint(j + 1) + b"\x22\x00" for j in range(3)]
    blen = [len(b) for b in body]
    per = sum(blen)
    data = np.frombuffer(b"".join(body) * G, dtype=np.uint8)
    ents = np.zeros((3 * G, 5), np.uint64)
    for j in range(3):
        ents[j::3, 0], ents[j::3, 1] = 5, j + 1
        ents[j::3, 2], ents[j::3, 3], ents[j::3, 4] = k * np.uint64(per) + np.uint64(sum(blen[:j])), blen[j], 1
    ready = np.zeros((G, 12), np.uint64)
    ready[:, 6], ready[:, 7] = 3 * k, 3
    d_ready, d_ents, d_data = up(ready), up(ents), up(data)
    d_scan, d_sreq, d_app = ctx.alloc(G * 48 + 64), ctx.alloc(3 * G * 32 + 64), ctx.alloc(3 * G * 32 + 64)

    def scan(emit):
        L.check(L.lib.econf_scan_committed_device(ctx.handle, d_ready.ptr, None, G, G, d_ents.ptr, 3 * G, d_data.ptr,
                                                  len(data), d_scan.ptr, d_sreq.ptr if emit else None,
                                                  d_app.ptr if emit else None, 3 * G, C.byref(n1), C.byref(n2)))
        assert (n1.value, n2.value) == (3 * G, 3 * G)
        return ms()

    def check_scan():
        rq = down(d_sreq, np.zeros((3 * G, 4), np.uint64))
        ap_ = down(d_app, np.zeros((3 * G, 4), np.uint64))
        assert (rq[:, 0] == np.repeat(k, 3)).all() and (rq[:, 1] == 1).all() and (rq[:, 2] == np.tile([1, 2, 3], G)).all()
        assert (ap_[:, 0] == np.tile([1000, 1001, 1002], G)).all() and (ap_[:, 3] == np.arange(3 * G)).all()
        sc = down(d_scan, np.zeros((G, 6), np.uint64))
        assert not sc[:, 0].any() and (sc[:, 2] == 3).all() and (sc[:, 1] == 3 * k).all()
    parts = {"ready_read": 2 * 16 * G, "entries_read": 40 * 3 * G + 16 * 3 * G, "data_read": len(data),
             "scratch": (2 * 48 + 2 * 8) * 3 * G + (8 + 4) * 2 * G, "requests": 64 * 3 * G, "rows": 48 * G}
    results["scan"] = (timed(lambda: scan(True), lambda: scan(False), lambda: None, check_scan, sum(parts.values())),
                       parts, 3 * G)
    for d in (d_ready, d_ents, d_data, d_scan, d_sreq, d_app):
        d.free()

    # ---- gate ----------------------------------------------------------------------------------------
    cst = cstate.copy()
    cst[::4, 0], cst[::4, 1] = 1, 2
    msgs = np.zeros((G, 8), np.uint64)
    msgs[:, 0], msgs[:, 1], msgs[:, 2], msgs[:, 3] = k, 5, 2, 6
    n_deny = len(range(0, G, 4))
    d_cst, d_in, d_gres = up(cst), up(msgs), ctx.alloc(G * 32 + 64)
    d_pass, d_gm = ctx.alloc((G - n_deny) * 64 + 64), ctx.alloc(n_deny * 144 + 64)

    def gate(emit):
        L.check(L.lib.econf_gate_batch_device(ctx.handle, live["groups"].ptr, d_cst.ptr, G, d_in.ptr, G, 64, 2, d_gres.ptr,
                                              d_pass.ptr if emit else None, G - n_deny, d_gm.ptr if emit else None, n_deny,
                                              C.byref(n1), C.byref(n2)))
        assert (n1.value, n2.value) == (G - n_deny, n_deny)
        return ms()

    def check_gate():
        p = down(d_pass, np.zeros((G - n_deny, 8), np.uint64))
        assert np.array_equal(p, msgs[k % 4 != 0])
        m = down(d_gm, np.zeros((n_deny, 18), np.uint64))
        assert (m[:, 0] == 8).all() and (m[:, 1] == 2).all() and (m[:, 2] == 1).all() and (m[:, 3] == 5).all()
    parts = {"records_read": 16 * G + 64 * G, "cstate_read": 128 * G, "scratch": 2 * 32 * G, "result": 32 * G,
             "copies": 2 * 64 * (G - n_deny), "messages": 144 * n_deny}
    results["gate"] = (timed(lambda: gate(True), lambda: gate(False), lambda: restore(["groups"]), check_gate,
                             sum(parts.values())), parts, G)

    os.makedirs(a.out, exist_ok=True)
    for shape in SHAPES:
        lines, parts, lanes = results[shape]
        med, cp = statistics.median(lines["step"]), statistics.median(lines["memcpy"])
        nbytes = sum(parts.values())
        r = {"tool": "tools/conf_bench.py", "shape": shape, "groups": G, "lanes": lanes, "steps": a.steps,
             "warmup": a.warmup, "lines": {n: summ(v) for n, v in lines.items()}, "tick_quiet": summ(tick),
             "ms_per_call": round(med, 4), "ns_per_group": round(med * 1e6 / G, 4), "algorithmic_bytes": nbytes,
             "bytes_parts": parts, "gbps_algorithmic": round(nbytes / med / 1e6, 1), "hbm_peak_gbps": HBM_PEAK_GBPS,
             "step_over_tick": round(med / tick_med, 3), "step_over_memcpy": round(med / cp, 3)}
        print(json.dumps(r))
        with open(os.path.join(a.out, "shape_%s.json" % shape), "w") as f:
            f.write(json.dumps(r, indent=1) + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
