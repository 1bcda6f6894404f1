#!/usr/bin/env python3
"""Device-time benchmark of the batched leader msgProp / msgBeat step (elead_local_batch_device).

Shapes (--shape; one process per shape, --shape all starts one child per shape
in turn):
  p1    1 Mi groups of 3 peers, one proposal each (2 Mi messages)
  p4    256 Ki groups of 3 peers, runs of 4 proposals: the same number of
        records and of messages as p1
  p7    64 Ki groups of 7 peers, runs of 6 proposals (6 messages a record)
  beat  1 Mi groups of 3 peers, one msgBeat each

Every group has a 4-entry log at offset 1000 + g whose last three terms are
the leader's; peer 1 leads and the others have matched nothing, with next at
the last index (lead_step_bench.py's groups).  Every step restores d_groups,
d_state and d_ents from pristine device copies first (outside the timed
window): the call updates all three in place.

Lines (--warmup 3 then --steps 20):
  step    the call's device time: HIP events from before its first memset to
          after its last kernel (ewal_last_device_ms; the host's decision
          point between the counting and the applying pass is inside)
  wall    the call's host wall time
  resp_a  in p1's process only: elead_step_batch_device (existing code) on
          lead_step_bench.py's shape a -- the same 1 Mi groups, the same 2 Mi
          messages -- timed the same way
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import lead_step_bench as LSB  # noqa: E402

HBM_PEAK_GBPS = LSB.HBM_PEAK_GBPS
SHAPES = ["p1", "p4", "p7", "beat"]
U8 = "<u8"
STATE = np.dtype([("ents_cap", U8), ("unstable", U8), ("pending_conf", U8), ("reserved", U8)])
LOCAL = np.dtype([("group", U8), ("kind", U8), ("etype", "<i4"), ("data_nil", "<i4"), ("data_off", U8),
                  ("data_len", U8), ("pad", U8)])
RES = np.dtype([("status", "<i4"), ("action", "<i4"), ("msg_first", U8), ("n_msgs", U8), ("index", U8),
                ("ent_pos", U8), ("committed", U8)])
BEAT, APPENDED = 1, 2
NLOG = LSB.NLOG
DATA_LEN = 1 << 20
SPEC = {"p1": (1 << 20, 3, 1, 2, "1 Mi groups of 3 peers: one proposal each"),
        "p4": (1 << 18, 3, 4, 2, "256 Ki groups of 3 peers: runs of 4 proposals"),
        "p7": (1 << 16, 7, 6, 2, "64 Ki groups of 7 peers: runs of 6 proposals"),
        "beat": (1 << 20, 3, 1, 1, "1 Mi groups of 3 peers: one msgBeat each")}


def build(shape, G):
    """The groups (windows of NLOG + run entries), their state records, the
    entry array (free slots zero) and the local messages."""
    _, P, per, kind, _ = SPEC[shape]
    k = np.arange(G, dtype=np.uint64)
    cap = NLOG + per
    g = np.zeros(G, LSB.GROUP)
    off = 1000 + k
    last = off + NLOG - 1
    g["id"], g["term"], g["committed"], g["log_offset"], g["nlog"], g["ents_first"], g["n_peers"] = \
        1, 5, off + 1, off, NLOG, cap * k, P
    g["peer_id"][:, :P] = np.arange(1, P + 1, dtype=np.uint64)
    g["match"][:, 0], g["next"][:, 0] = last, last + 1
    g["next"][:, 1:P] = last[:, None]
    st = np.zeros(G, STATE)
    st["ents_cap"], st["unstable"] = cap, last + 1
    ents = np.zeros((G, cap), LSB.ENT)
    ents["term"][:, :NLOG] = np.array([4, 5, 5, 5], dtype=np.uint64)[None, :]
    ents["index"][:, :NLOG] = off[:, None] + np.arange(NLOG, dtype=np.uint64)[None, :]
    ents["data_nil"][:, :NLOG] = 1
    n = G * per
    loc = np.zeros(n, LOCAL)
    loc["group"] = np.repeat(k, per)
    loc["kind"] = kind
    if kind == 2:
        loc["data_off"] = (np.arange(n, dtype=np.uint64) * 16) % (DATA_LEN - 64)
        loc["data_len"] = 16
    return g, st, ents.reshape(-1), loc


def run_shape(a):
    from etcd_amd import _lib as L
    from etcd_amd import wal as W

    def hip_check(rc):
        if rc != 0:
            raise RuntimeError("HIP error %d" % rc)

    hip = C.CDLL("libamdhip64.so.7")
    G0, P, per, kind, desc = SPEC[a.shape]
    G = a.groups or G0
    groups, state, ents, locs = build(a.shape, G)
    n, total = len(locs), len(locs) * (P - 1)
    cap = NLOG + per
    ctx = W.Context(0)

    def up(arr):
        d = ctx.alloc(arr.nbytes + 64)
        if arr.nbytes:
            d.upload_ptr(arr.ctypes.data, arr.nbytes)
        return d

    live = [up(groups), up(state), up(ents)]
    pristine = [up(groups), up(state), up(ents)]
    d_locs = up(locs)
    d_res, d_msgs = ctx.alloc(n * 48 + 64), ctx.alloc(total * 144 + 64)
    nm, na = C.c_uint64(0), C.c_uint64(0)

    def restore():
        for d, p, arr in zip(live, pristine, (groups, state, ents)):
            hip_check(hip.hipMemcpyDtoD(d.ptr, p.ptr, C.c_size_t(arr.nbytes)))
        hip_check(hip.hipDeviceSynchronize())

    def call():
        t = time.perf_counter()
        L.check(L.lib.elead_local_batch_device(ctx.handle, live[0].ptr, live[1].ptr, G, None, live[2].ptr, len(ents),
                                               DATA_LEN, d_locs.ptr, n, d_res.ptr, d_msgs.ptr, total, C.byref(nm),
                                               C.byref(na)))
        return float(L.lib.ewal_last_device_ms(ctx.handle)), (time.perf_counter() - t) * 1e3

    lines = {"step": [], "wall": []}
    for k in range(a.warmup + a.steps):
        restore()
        e, w = call()
        if k == 0:
            res = np.frombuffer(d_res.download(n * 48), dtype=RES)
            j = np.tile(np.arange(per, dtype=np.uint64), G)
            last = np.repeat(groups["log_offset"] + NLOG - 1, per)
            assert not res["status"].any() and (res["action"] == (APPENDED if kind == 2 else BEAT)).all()
            assert (res["n_msgs"] == P - 1).all() and nm.value == total
            assert (res["msg_first"] == np.arange(n, dtype=np.uint64) * (P - 1)).all()
            assert (res["committed"] == np.repeat(groups["committed"], per)).all()
            g1 = np.frombuffer(live[0].download(groups.nbytes), dtype=LSB.GROUP)
            m = np.frombuffer(d_msgs.download(144 * min(total, 4096)), dtype=LSB.MSG)
            assert (m["type"] == 3).all() and (m["from_"] == 1).all() and (m["term"] == 5).all()
            if kind == 2:
                assert na.value == n and (res["index"] == last + 1 + j).all()
                assert (res["ent_pos"] == np.repeat(groups["ents_first"], per) + NLOG + j).all()
                assert (g1["nlog"] == cap).all() and (g1["match"][:, 0] == groups["match"][:, 0] + per).all()
                e1 = np.frombuffer(live[2].download(ents.nbytes), dtype=LSB.ENT).reshape(G, cap)
                assert (e1["term"][:, NLOG:] == 5).all() and (e1["data_len"][:, NLOG:] == 16).all()
                assert (e1["index"][:, NLOG:] == (last + 1 + j).reshape(G, per)).all()
                # every message runs from the follower's next (the old last index) to the new entry
                rec = np.arange(len(m)) // (P - 1)
                assert (m["index"] + 1 == last[rec]).all() and (m["n_ents"] == 2 + j[rec]).all()
                assert (m["log_term"] == 5).all()
            else:
                assert na.value == 0 and (g1 == groups).all() and not m["index"].any() and not m["n_ents"].any()
            acc = n if kind == 2 else 0
            parts = {"group_read": (256 + 32) * G, "group_write": 24 * G if acc else 0, "local_read": 48 * n,
                     "result": 48 * n, "entry": 40 * acc, "message": 144 * total,
                     "term_gather": 8 * total if acc else 0}
            how = ("per group 256 B + 32 B read once (the lanes of a run read the same lines) and 24 B written "
                   "(nlog, match, next) where a proposal was accepted; per record 48 B read and 48 B of result; per "
                   "accepted proposal a 40-B entry; per message 144 B and, for a proposal's, its log_term's 8 B")
        if k >= a.warmup:
            lines["step"].append(e)
            lines["wall"].append(w)
    nbytes = sum(parts.values())

    extra = {}
    if a.shape == "p1":
        # existing code, the same groups and the same number of messages: lead_step_bench.py's shape a
        ag, aents, aresps, _, amsgs = LSB.build("a", G)
        an, atotal = len(aresps), int(amsgs.sum())
        for d in live + pristine + [d_locs, d_res, d_msgs]:
            d.free()
        d_g, d_g0, d_e, d_r = up(ag), up(ag), up(aents), up(aresps)
        d_ares, d_amsgs = ctx.alloc(an * 48 + 64), ctx.alloc(atotal * 144 + 64)
        lines["resp_a"] = []
        for k in range(a.warmup + a.steps):
            hip_check(hip.hipMemcpyDtoD(d_g.ptr, d_g0.ptr, C.c_size_t(ag.nbytes)))
            hip_check(hip.hipDeviceSynchronize())
            L.check(L.lib.elead_step_batch_device(ctx.handle, d_g.ptr, G, None, d_e.ptr, len(aents), d_r.ptr, an,
                                                  d_ares.ptr, d_amsgs.ptr, atotal, C.byref(nm), C.byref(na)))
            assert nm.value == atotal
            if k >= a.warmup:
                lines["resp_a"].append(float(L.lib.ewal_last_device_ms(ctx.handle)))
        amed = statistics.median(lines["resp_a"])
        extra = {"resp_a_responses": an, "resp_a_messages": atotal,
                 "resp_a_ns_per_message": round(amed * 1e6 / atotal, 4),
                 "ns_per_message_over_resp_a": round((statistics.median(lines["step"]) / total) / (amed / atotal), 3)}

    def summ(v):
        med = statistics.median(v)
        return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    med = statistics.median(lines["step"])
    gbps = nbytes / med / 1e6
    result = {"tool": "tools/lead_prop_bench.py", "shape": a.shape, "input": desc, "groups": G, "peers": P,
              "records": n, "run_length": per, "messages": total, "appended": n if kind == 2 else 0,
              "steps": a.steps, "warmup": a.warmup, "lines": {k: summ(v) for k, v in lines.items()},
              "ms_per_call": round(med, 4), "records_per_s": round(n / med * 1e3),
              "ns_per_record": round(med * 1e6 / n, 4), "ns_per_message": round(med * 1e6 / total, 4),
              "algorithmic_bytes": nbytes, "bytes": how, "bytes_parts": parts,
              "gbps_algorithmic": round(gbps, 1), "hbm_peak_gbps": HBM_PEAK_GBPS,
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
    outdir = a.out or os.path.join(ROOT, "profiles", "lead_prop")
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
