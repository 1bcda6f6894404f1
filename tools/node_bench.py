#!/usr/bin/env python3
"""Device-time benchmark of the batched StartNode / RestartNode (enode_batch_device).

Shapes (--shape; one process per shape, --shape all starts one child per shape
in turn), each 1 Mi groups, one request per group in group order:
  restart       RestartNode without a snapshot, 16 entries a group: the copy of
                16 Mi entries out of one source array into the groups' windows
  restart_snap  RestartNode with a snapshot (three Nodes, one RemovedNode) and
                4 entries a group
  start         StartNode with three peers (no Context): 3 Mi ConfChange entries
                marshalled into d_data

The call writes every record it names, so nothing is restored between steps:
a repeated call reads nothing of what the previous one left.

Lines (--warmup 3 then --steps 20):
  step   the call's device time: HIP events from before its first memset to
         after its last kernel (ewal_last_device_ms; the host's decision point
         between the counting and the apply pass is inside)
  size   the same call with d_data == NULL (results alone)
  wall   the real call's host wall time
The first step's results are checked against what the shape must give.  Prints
one JSON line; --out writes it to a file too.  Needs the GPU.  The comparable
kernel is tools/follow_bench.py's copy: run `follow_bench.py --shape burst
--groups 262144` (16 Mi entries) in the same session.
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
SHAPES = ["restart", "restart_snap", "start"]
# shape: (entries or peers a group, description)
SPEC = {"restart": (16, "1 Mi groups x 16 entries, no snapshot"),
        "restart_snap": (4, "1 Mi groups x 4 entries, a snapshot of three Nodes and one RemovedNode each"),
        "start": (3, "1 Mi groups x 3 peers")}
NO_SNAP = (1 << 64) - 1
RESTARTED, RESTARTED_SNAP, STARTED = 1, 2, 3
CC_BYTES = 8                      # 08 00 10 00 18 id 22 00 for an id below 128


def build(shape, G):
    """(reqs (G, 16), src (n, 5), in_snaps (m, 8), u64, peers (p, 4), the window a group gets) as uint64 arrays."""
    per, _ = SPEC[shape]
    k = np.arange(G, dtype=np.uint64)
    cap = per + 2
    reqs = np.zeros((G, 16), np.uint64)
    reqs[:, 0], reqs[:, 2], reqs[:, 3], reqs[:, 4], reqs[:, 6] = k, k % np.uint64(3) + np.uint64(1), k * np.uint64(cap), cap, per
    reqs[:, 11] = np.uint64(NO_SNAP)
    src = np.zeros((0, 5), np.uint64)
    in_snaps = np.zeros((0, 8), np.uint64)
    u64 = np.zeros(0, np.uint64)
    peers = np.zeros((0, 4), np.uint64)
    if shape == "start":
        reqs[:, 1] = 2
        reqs[:, 5] = 0                               # every group names the same three peers
        peers = np.array([[1, 0, 0, 0], [2, 0, 0, 0], [3, 0, 0, 0]], dtype=np.uint64)
        return reqs, src, in_snaps, u64, peers, cap
    reqs[:, 1] = 1
    reqs[:, 5] = k * np.uint64(per)
    reqs[:, 7] = k * np.uint64(4096)                 # the shard's base in the WAL buffer
    j = np.arange(G * per, dtype=np.uint64)
    base = 100 if shape == "restart_snap" else 0
    src = np.zeros((G * per, 5), np.uint64)
    src[:, 0], src[:, 1], src[:, 2], src[:, 3] = 1, j % np.uint64(per) + np.uint64(base), (j % np.uint64(per)) * np.uint64(64), 48
    reqs[:, 8], reqs[:, 9], reqs[:, 10] = 1, 0, base + per - 1
    if shape == "restart_snap":
        reqs[:, 11] = k
        in_snaps = np.zeros((G, 8), np.uint64)
        in_snaps[:, 0], in_snaps[:, 1], in_snaps[:, 4], in_snaps[:, 5], in_snaps[:, 6], in_snaps[:, 7] = 100, 1, 0, 3, 3, 1
        u64 = np.array([1, 2, 3, 9], dtype=np.uint64)
    return reqs, src, in_snaps, u64, peers, cap


def run_shape(a):
    from etcd_amd import _lib as L
    from etcd_amd import wal as W

    G = a.groups or (1 << 20)
    per, desc = SPEC[a.shape]
    reqs, src, in_snaps, u64, peers, cap = build(a.shape, G)
    n_ents = G * cap
    n_data = 3 * CC_BYTES * G if a.shape == "start" else 0
    ctx = W.Context(0)

    def up(arr):
        d = ctx.alloc(arr.nbytes + 64)
        if arr.nbytes:
            d.upload_ptr(arr.ctypes.data, arr.nbytes)
        return d

    recs = [ctx.alloc(G * b + 64) for b in (256, 32, 64, 64, 128, 64)]
    d_ents = ctx.alloc(n_ents * 40 + 64)
    d_src, d_in, d_u64, d_peers, d_reqs = up(src), up(in_snaps), up(u64), up(peers), up(reqs)
    d_res, d_data = ctx.alloc(G * 48 + 64), ctx.alloc(n_data + 64)
    nd, nc, nb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def call(emit=True):
        t = time.perf_counter()
        L.check(L.lib.enode_batch_device(ctx.handle, *[r.ptr for r in recs], G, d_ents.ptr, n_ents, d_src.ptr, len(src),
                                         d_in.ptr, len(in_snaps), d_u64.ptr, len(u64), d_peers.ptr, len(peers), None, 0,
                                         d_data.ptr if emit else None, 0, n_data, d_reqs.ptr, G, d_res.ptr,
                                         C.byref(nd), C.byref(nc), C.byref(nb)))
        return float(L.lib.ewal_last_device_ms(ctx.handle)), (time.perf_counter() - t) * 1e3

    want_copied = G * per if a.shape != "start" else 0
    lines = {"step": [], "size": [], "wall": []}
    for k in range(a.warmup + a.steps):
        s, _ = call(emit=False)
        assert (nd.value, nc.value, nb.value) == (n_data, want_copied, G)
        e, w = call()
        assert (nd.value, nc.value, nb.value) == (n_data, want_copied, G)
        if k == 0:
            res = np.frombuffer(d_res.download(G * 48), dtype=np.uint64).reshape(G, 6)
            action = {"restart": RESTARTED, "restart_snap": RESTARTED_SNAP, "start": STARTED}[a.shape]
            assert (res[:, 0] == np.uint64(action << 32)).all()
            g = np.frombuffer(recs[0].download(G * 256), dtype=np.uint64).reshape(G, 32)
            assert (g[:, 0] == reqs[:, 2]).all() and (g[:, 5] == reqs[:, 3]).all()
            ents = np.frombuffer(d_ents.download(n_ents * 40), dtype=np.uint64).reshape(G, cap, 5)
            if a.shape == "start":
                assert (g[:, 4] == 4).all() and (g[:, 2] == 3).all() and (g[:, 6] == 0).all()
                assert (ents[:, 1:4, 1] == np.arange(1, 4, dtype=np.uint64)[None, :]).all() and (ents[:, 1:4, 3] == CC_BYTES).all()
                assert (ents[:, 1, 2] == np.arange(G, dtype=np.uint64) * np.uint64(3 * CC_BYTES)).all()
                body = np.frombuffer(d_data.download(n_data), dtype=np.uint8).reshape(G, 3, CC_BYTES)
                assert (body[:, :, 5] == np.array([1, 2, 3], dtype=np.uint8)[None, :]).all() and (body[:, :, 0] == 8).all()
            else:
                assert (g[:, 4] == per).all() and (g[:, 2] == reqs[:, 10]).all() and (g[:, 1] == 1).all()
                assert (ents[:, :per, 1] == src.reshape(G, per, 5)[:, :, 1]).all()
                assert (ents[:, :per, 2] == src.reshape(G, per, 5)[:, :, 2] + reqs[:, 7][:, None]).all()
                if a.shape == "restart_snap":
                    assert (g[:, 3] == 100).all() and (g[:, 6] == 3).all() and (g[:, 7:10] == np.array([1, 2, 3], dtype=np.uint64)).all()
                    c = np.frombuffer(recs[4].download(G * 128), dtype=np.uint64).reshape(G, 16)
                    assert (c[:, 0] == 1).all() and (c[:, 1] == 9).all()
            del res, g, ents
        if k >= a.warmup:
            lines["step"].append(e)
            lines["size"].append(s)
            lines["wall"].append(w)
    parts = {"req_read": 2 * 128 * G, "scratch": 2 * 48 * G, "result": 48 * G, "records": (256 + 32 + 64 + 64 + 128 + 64) * G,
             "entry_copy": 80 * want_copied,
             "snapshot": (2 * 64 + 64 + 2 * 32) * G if a.shape == "restart_snap" else 0,
             "start_entries": ((1 + per) * 40 + 2 * per * 32 + per * CC_BYTES + per * (128 + 48 + 40)) * G if a.shape == "start" else 0}
    how = ("per request 128 B read by both passes, a 48-B scratch record written and read, 48 B of result and the 608 B "
           "of the five records and d_snaps[g] written; per copied entry 40 B read and 40 B written (its request and "
           "scratch record come from cache); per snapshot its row read twice and written once and its Nodes / "
           "RemovedNodes read twice; per StartNode peer its 32-B enode_peer read by both passes, a 40-B entry row and "
           "its bytes written, and the marshal lane's request, scratch record and entry row")
    nbytes = sum(parts.values())

    def summ(v):
        med = statistics.median(v)
        return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    med = statistics.median(lines["step"])
    gbps = nbytes / med / 1e6
    result = {"tool": "tools/node_bench.py", "shape": a.shape, "input": desc, "groups": G, "entries_copied": want_copied,
              "conf_change_bytes": n_data, "steps": a.steps, "warmup": a.warmup,
              "lines": {k: summ(v) for k, v in lines.items()}, "ms_per_call": round(med, 4),
              "groups_per_s": round(G / med * 1e3), "ns_per_group": round(med * 1e6 / G, 4),
              "ns_per_entry": round(med * 1e6 / want_copied, 4) if want_copied else None,
              "algorithmic_bytes": nbytes, "bytes": how, "bytes_parts": parts, "gbps_algorithmic": round(gbps, 1),
              "entry_copy_gbps": round(80 * want_copied / med / 1e6, 1) if want_copied else None,
              "hbm_peak_gbps": HBM_PEAK_GBPS, "hbm_frac": round(gbps / HBM_PEAK_GBPS, 4)}
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    ctx.close()
    return 0


def run_all(a):
    outdir = a.out or os.path.join(ROOT, "profiles", "node")
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
    ap.add_argument("--groups", type=int, default=0, help="groups per shape (default: 1 Mi)")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=None, help="a JSON file (one shape) or a directory (--shape all)")
    a = ap.parse_args()
    return run_all(a) if a.shape == "all" else run_shape(a)


if __name__ == "__main__":
    sys.exit(main())
