#!/usr/bin/env python3
"""Device-time benchmark of the batched leader msgAppResp step (elead_step_batch_device).

Shapes (--shape; one process per shape, --shape all starts one child per shape
in turn):
  a   1 Mi groups of 3 peers, 2 accepting responses each; the first commits
      (and broadcasts 2 messages), the second only updates
  b   1 Mi groups of 5 peers, 4 accepting responses each; the second commits
      (4 messages)
  c   1 Mi groups of 3 peers, one reject each that probes (1 message)
  d   64 Ki groups of 7 peers, 6 accepting responses each; the third commits
      (6 messages)

Every step restores d_groups from a pristine device copy first (outside the
timed window): the call updates it in place, and a second call on the updated
state would be a different shape.

Lines (--warmup 3 then --steps 20):
  step    the call's device time: HIP events from before its first memset to
          after its last kernel (ewal_last_device_ms; the host's decision
          point between the counting pass and the applying pass is inside)
  wall    the call's host wall time
  commit  ecommit_batch_rec_device (existing code) on the same number of
          groups with the same peers and logs: the yardstick for the cost per
          group of the commit rule alone
GB/s is the algorithmic bytes over the median device time, also as a share of
the HBM roofline bench.py uses; the bytes are counted as `bytes` says.  The
first step's results are checked against what the shape must give.  Prints
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

HBM_PEAK_GBPS = 8000.0   # as bench.py: the MI355X HBM3E spec
SHAPES = ["a", "b", "c", "d"]
U8 = "<u8"
GROUP = np.dtype([("id", U8), ("term", U8), ("committed", U8), ("log_offset", U8), ("nlog", U8), ("ents_first", U8),
                  ("n_peers", U8), ("peer_id", U8, 7), ("match", U8, 7), ("next", U8, 7), ("reserved", U8, 4)])
RESP = np.dtype([("group", U8), ("from_", U8), ("term", U8), ("index", U8), ("reject", "<i4"), ("pad", "<i4"),
                 ("pad2", U8)])
ENT = np.dtype([("term", U8), ("index", U8), ("data_off", U8), ("data_len", U8), ("type", "<i4"), ("data_nil", "<i4")])
RES = np.dtype([("status", "<i4"), ("action", "<i4"), ("msg_first", U8), ("n_msgs", U8), ("committed", U8),
                ("match", U8), ("next", U8)])
MSG = np.dtype([(k, U8) for k in ("type", "to", "from_", "term", "log_term", "index", "commit", "ents_first", "n_ents",
                                  "snap_index", "snap_term", "snap_data_off", "snap_data_len", "snap_nodes_off",
                                  "snap_n_nodes", "snap_removed_off", "snap_n_removed", "reject")])
PROBE, UPDATED, COMMITTED = 4, 5, 6
NLOG = 4
SPEC = {"a": (1 << 20, 3, 2, "1 Mi groups of 3 peers: 2 accepting responses each, the first commits"),
        "b": (1 << 20, 5, 4, "1 Mi groups of 5 peers: 4 accepting responses each, the second commits"),
        "c": (1 << 20, 3, 1, "1 Mi groups of 3 peers: one reject each, all probes"),
        "d": (1 << 16, 7, 6, "64 Ki groups of 7 peers: 6 accepting responses each, the third commits")}


def build(shape, G):
    """The groups (a 4-entry log at offset 1000 + g whose last three terms are
    the leader's; peer 1 leads, the others have matched nothing), their
    entries, the responses, and per response the action and messages wanted."""
    _, P, per, _ = SPEC[shape]
    k = np.arange(G, dtype=np.uint64)
    g = np.zeros(G, GROUP)
    off = 1000 + k
    last = off + NLOG - 1
    g["id"], g["term"], g["committed"], g["log_offset"], g["nlog"], g["ents_first"], g["n_peers"] = \
        1, 5, off + 1, off, NLOG, NLOG * k, P
    g["peer_id"][:, :P] = np.arange(1, P + 1, dtype=np.uint64)
    g["match"][:, 0], g["next"][:, 0] = last, last + 1
    g["next"][:, 1:P] = last[:, None]
    ents = np.zeros(NLOG * G, ENT)
    ents["term"] = np.tile(np.array([4, 5, 5, 5], dtype=np.uint64), G)
    ents["index"] = (off[:, None] + np.arange(NLOG, dtype=np.uint64)[None, :]).reshape(-1)
    ents["data_nil"] = 1
    r = np.zeros(G * per, RESP)
    r["group"] = np.repeat(k, per)
    r["from_"] = np.tile(np.arange(2, 2 + per, dtype=np.uint64), G)
    r["term"] = 5
    if shape == "c":
        r["index"], r["reject"] = np.repeat(last - 1, per), 1
        action = np.full(G * per, PROBE)
        n_msgs = np.ones(G * per, dtype=np.uint64)
    else:
        r["index"] = np.repeat(last, per)
        commit_at = P // 2 - 1                      # the response that completes the quorum
        action = np.tile(np.array([COMMITTED if j == commit_at else UPDATED for j in range(per)]), G)
        n_msgs = np.where(action == COMMITTED, P - 1, 0).astype(np.uint64)
    return g, ents, r, action, n_msgs


def commit_records(groups, ents, P):
    """ecommit_group records of the same groups after their responses' updates."""
    from etcd_amd import raftcommit as RC
    G = len(groups)
    match = np.ascontiguousarray(groups["match"][:, :P].T).copy()
    match[1:] = (groups["log_offset"] + NLOG - 1)[None, :]
    ptr = np.arange(G + 1, dtype=np.uint64) * NLOG
    return RC.pack_groups(match, np.full(G, P, np.uint8), groups["committed"], groups["term"], groups["log_offset"],
                          ptr, ents["term"])


def run_shape(a):
    from etcd_amd import _lib as L
    from etcd_amd import wal as W

    def hip_check(rc):
        if rc != 0:
            raise RuntimeError("HIP error %d" % rc)

    hip = C.CDLL("libamdhip64.so.7")
    G0, P, per, desc = SPEC[a.shape]
    G = a.groups or G0
    groups, ents, resps, want_action, want_msgs = build(a.shape, G)
    n, total = len(resps), int(want_msgs.sum())
    ctx = W.Context(0)

    def up(arr):
        d = ctx.alloc(arr.nbytes + 64)
        if arr.nbytes:
            d.upload_ptr(arr.ctypes.data, arr.nbytes)
        return d

    d_groups, d_ents, d_resps, g0 = up(groups), up(ents), up(resps), up(groups)
    d_res, d_msgs = ctx.alloc(n * 48 + 64), ctx.alloc(total * 144 + 64)
    nm, nc = C.c_uint64(0), C.c_uint64(0)

    def restore():
        hip_check(hip.hipMemcpyDtoD(d_groups.ptr, g0.ptr, C.c_size_t(groups.nbytes)))
        hip_check(hip.hipDeviceSynchronize())

    def call():
        t = time.perf_counter()
        L.check(L.lib.elead_step_batch_device(ctx.handle, d_groups.ptr, G, None, d_ents.ptr, len(ents), d_resps.ptr, n,
                                              d_res.ptr, d_msgs.ptr, total, C.byref(nm), C.byref(nc)))
        return float(L.lib.ewal_last_device_ms(ctx.handle)), (time.perf_counter() - t) * 1e3

    lines = {"step": [], "wall": [], "commit": []}
    for k in range(a.warmup + a.steps):
        restore()
        e, w = call()
        if k == 0:
            res = np.frombuffer(d_res.download(n * 48), dtype=RES)
            assert not res["status"].any() and (res["action"] == want_action).all()
            assert (res["n_msgs"] == want_msgs).all() and nm.value == total
            assert (res["msg_first"] == np.cumsum(want_msgs) - want_msgs).all()
            assert nc.value == int((want_action == COMMITTED).sum())
            g1 = np.frombuffer(d_groups.download(groups.nbytes), dtype=GROUP)
            last = groups["log_offset"] + NLOG - 1
            if a.shape == "c":
                assert (g1["next"][:, 1] == last - 1).all() and (g1["committed"] == groups["committed"]).all()
            else:
                assert (g1["committed"] == last).all() and (g1["match"][:, 1:1 + per] == last[:, None]).all()
            m = np.frombuffer(d_msgs.download(144 * min(total, 4096)), dtype=MSG)
            assert (m["type"] == 3).all() and (m["from_"] == 1).all() and (m["term"] == 5).all()
            assert (m["index"] + m["n_ents"] == m["commit"] + (2 if a.shape == "c" else 0)).all()   # up to the log's end
            # the algorithmic bytes of this call
            upd = int((want_action != PROBE).sum())
            parts = {"group_read": 256 * G, "group_write": 8 * int(nc.value) + 16 * upd + 8 * (n - upd),
                     "response_read": 48 * n, "result": 48 * n, "message": 144 * total,
                     "term_gather": 8 * (total + int(nc.value))}
            how = ("per group 256 B read; 8 B of it written per commit, 16 B per update (match, next), 8 B per probe "
                   "(next); per response 48 B read and 48 B of result; per message 144 B and its log_term's 8 B; 8 B "
                   "for the term of each quorum index that commits")
        if k >= a.warmup:
            lines["step"].append(e)
            lines["wall"].append(w)
    nbytes = sum(parts.values())

    # the yardstick: the commit rule alone, on one 192-B record per group
    rec = commit_records(groups, ents, P)
    d_rec, d_out, d_ch, d_st = up(rec), ctx.alloc(8 * G + 64), ctx.alloc(G + 64), ctx.alloc(G + 64)
    ms = C.c_double(0)
    for k in range(a.warmup + a.steps):
        L.check(L.lib.ecommit_batch_rec_device(ctx.handle, G, d_rec.ptr, None, None, d_out.ptr, d_ch.ptr, d_st.ptr,
                                               C.byref(ms)))
        if k == 0:
            assert not any(d_st.download(G)) and all(d_ch.download(G))
        if k >= a.warmup:
            lines["commit"].append(ms.value)

    def summ(v):
        med = statistics.median(v)
        return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    med, cmed = statistics.median(lines["step"]), statistics.median(lines["commit"])
    gbps = nbytes / med / 1e6
    result = {"tool": "tools/lead_step_bench.py", "shape": a.shape, "input": desc, "groups": G, "peers": P,
              "responses": n, "messages": total, "committed": nc.value, "steps": a.steps, "warmup": a.warmup,
              "lines": {k: summ(v) for k, v in lines.items()},
              "ms_per_call": round(med, 4), "responses_per_s": round(n / med * 1e3),
              "ns_per_group": round(med * 1e6 / G, 3), "commit_only_ns_per_group": round(cmed * 1e6 / G, 3),
              "step_over_commit_only": round(med / cmed, 2),
              "algorithmic_bytes": nbytes, "bytes": how, "bytes_parts": parts,
              "gbps_algorithmic": round(gbps, 1), "hbm_peak_gbps": HBM_PEAK_GBPS,
              "hbm_frac": round(gbps / HBM_PEAK_GBPS, 4)}
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    ctx.close()
    return 0


def run_all(a):
    outdir = a.out or os.path.join(ROOT, "profiles", "lead_step")
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
