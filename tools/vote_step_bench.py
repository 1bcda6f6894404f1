#!/usr/bin/env python3
"""Device-time benchmark of the batched election step (evote_step_batch_device).

Shapes (--shape; one process per shape, --shape all starts one child per shape
in turn), 1 Mi groups each unless --groups says otherwise:
  hup    3 peers, followers: one msgHup each (CAMPAIGNED, 2 msgVote a record)
  vote   3 peers, followers that have not voted: one msgVote each from a
         candidate whose log is as long (GRANTED, 1 msgVoteResp a record)
  win    3 peers, candidates holding their own vote: the granting msgVoteResp
         that makes the quorum (WON: becomeLeader's entry, 2 msgApp a record)
  win7   7 peers, candidates holding three votes: the fourth (WON, 6 msgApp)

Every group has lead_step_bench.py's 4-entry log at offset 1000 + g and a
window with room for one more entry.  Every step restores d_groups, d_pstate,
d_vstate and d_ents from pristine device copies first (outside the timed
window): the call updates all four in place.

Lines (--warmup 3 then --steps 20):
  step    the call's device time: HIP events from before its first memset to
          after its last kernel (ewal_last_device_ms; the host's decision
          point between the counting and the applying pass is inside)
  wall    the call's host wall time
  resp_a  in win's process only: elead_step_batch_device (existing code) on
          lead_step_bench.py's shape a -- the same 1 Mi groups, 2 Mi responses,
          2 Mi messages -- timed the same way
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import lead_step_bench as LSB  # noqa: E402

HBM_PEAK_GBPS = LSB.HBM_PEAK_GBPS
SHAPES = ["hup", "vote", "win", "win7"]
U8 = "<u8"
PSTATE = np.dtype([("ents_cap", U8), ("unstable", U8), ("pending_conf", U8), ("reserved", U8)])
VSTATE = np.dtype([("state", U8), ("vote", U8), ("lead", U8), ("elapsed", U8), ("voted", U8), ("granted", U8),
                   ("reserved", U8, 2)])
MSG_IN = np.dtype([("group", U8), ("kind", U8), ("from_", U8), ("term", U8), ("index", U8), ("log_term", U8),
                   ("reject", "<i4"), ("pad", "<i4"), ("pad2", U8)])
RES = np.dtype([("status", "<i4"), ("action", "<i4"), ("msg_first", U8), ("n_msgs", U8), ("term", U8), ("vote", U8),
                ("state", "<i4"), ("flags", "<i4")])
GRANTED, CAMPAIGNED, WON = 2, 4, 5
NLOG = LSB.NLOG
TERM = 5
# shape: (groups, peers, kind, wanted action, messages a record, description)
SPEC = {"hup": (1 << 20, 3, 0, CAMPAIGNED, 2, "1 Mi followers of 3 peers: one msgHup each"),
        "vote": (1 << 20, 3, 5, GRANTED, 1, "1 Mi followers of 3 peers: one msgVote each, granted"),
        "win": (1 << 20, 3, 6, WON, 2, "1 Mi candidates of 3 peers: the winning msgVoteResp each"),
        "win7": (1 << 20, 7, 6, WON, 6, "1 Mi candidates of 7 peers: the winning msgVoteResp each")}


def build(shape, G):
    _, P, kind, _, _, _ = SPEC[shape]
    k = np.arange(G, dtype=np.uint64)
    cap = NLOG + 1
    g = np.zeros(G, LSB.GROUP)
    off = 1000 + k
    last = off + NLOG - 1
    g["id"], g["term"], g["committed"], g["log_offset"], g["nlog"], g["ents_first"], g["n_peers"] = \
        1, TERM, off + 1, off, NLOG, cap * k, P
    g["peer_id"][:, :P] = np.arange(1, P + 1, dtype=np.uint64)
    g["match"][:, 0] = last
    g["next"][:, :P] = (last + 1)[:, None]
    ps = np.zeros(G, PSTATE)
    ps["ents_cap"], ps["unstable"] = cap, last + 1
    vs = np.zeros(G, VSTATE)
    if kind == 6:
        vs["state"], vs["vote"] = 1, 1
        vs["voted"] = vs["granted"] = (1 << (P // 2)) - 1          # one vote short of the quorum
    ents = np.zeros((G, cap), LSB.ENT)
    ents["term"][:, :NLOG] = np.array([4, 5, 5, 5], dtype=np.uint64)[None, :]
    ents["index"][:, :NLOG] = off[:, None] + np.arange(NLOG, dtype=np.uint64)[None, :]
    ents["data_nil"][:, :NLOG] = 1
    m = np.zeros(G, MSG_IN)
    m["group"], m["kind"] = k, kind
    if kind == 0:
        m["from_"] = 1
    elif kind == 5:
        m["from_"], m["term"], m["index"], m["log_term"] = 2, TERM + 1, last, 5
    else:
        m["from_"], m["term"] = P // 2 + 1, TERM
    return g, ps, vs, ents.reshape(-1), m


def run_shape(a):
    from etcd_amd import _lib as L
    from etcd_amd import wal as W

    def hip_check(rc):
        if rc != 0:
            raise RuntimeError("HIP error %d" % rc)

    hip = C.CDLL("libamdhip64.so.7")
    G0, P, kind, action, per_msgs, desc = SPEC[a.shape]
    G = a.groups or G0
    groups, pstate, vstate, ents, msgs_in = build(a.shape, G)
    n, total = G, G * per_msgs
    ctx = W.Context(0)

    def up(arr):
        d = ctx.alloc(arr.nbytes + 64)
        if arr.nbytes:
            d.upload_ptr(arr.ctypes.data, arr.nbytes)
        return d

    host = (groups, pstate, vstate, ents)
    live = [up(x) for x in host]
    pristine = [up(x) for x in host]
    d_in = up(msgs_in)
    d_res, d_msgs = ctx.alloc(n * 48 + 64), ctx.alloc(total * 144 + 64)
    nm, nw = C.c_uint64(0), C.c_uint64(0)

    def restore():
        for d, p, arr in zip(live, pristine, host):
            hip_check(hip.hipMemcpyDtoD(d.ptr, p.ptr, C.c_size_t(arr.nbytes)))
        hip_check(hip.hipDeviceSynchronize())

    def call():
        t = time.perf_counter()
        L.check(L.lib.evote_step_batch_device(ctx.handle, live[0].ptr, live[1].ptr, live[2].ptr, G, None, live[3].ptr,
                                              len(ents), d_in.ptr, n, d_res.ptr, d_msgs.ptr, total, C.byref(nm),
                                              C.byref(nw)))
        return float(L.lib.ewal_last_device_ms(ctx.handle)), (time.perf_counter() - t) * 1e3

    lines = {"step": [], "wall": []}
    for k in range(a.warmup + a.steps):
        restore()
        e, w = call()
        if k == 0:
            res = np.frombuffer(d_res.download(n * 48), dtype=RES)
            last = groups["log_offset"] + NLOG - 1
            assert not res["status"].any() and (res["action"] == action).all() and nm.value == total
            assert (res["n_msgs"] == per_msgs).all()
            assert (res["msg_first"] == np.arange(n, dtype=np.uint64) * per_msgs).all()
            g1 = np.frombuffer(live[0].download(groups.nbytes), dtype=LSB.GROUP)
            v1 = np.frombuffer(live[2].download(vstate.nbytes), dtype=VSTATE)
            m = np.frombuffer(d_msgs.download(144 * min(total, 4096)), dtype=LSB.MSG)
            rec = np.arange(len(m)) // per_msgs
            assert (m["from_"] == 1).all() and (m["term"] == g1["term"][rec]).all()
            if kind == 0:
                assert nw.value == 0 and (g1["term"] == TERM + 1).all() and (v1["state"] == 1).all()
                assert (m["type"] == 5).all() and (m["index"] == last[rec]).all() and (m["log_term"] == 5).all()
            elif kind == 5:
                assert nw.value == 0 and (g1["term"] == TERM + 1).all() and (v1["vote"] == 2).all()
                assert (res["flags"] == 1).all() and (m["type"] == 6).all() and not m["reject"].any()
            else:
                assert nw.value == n and (v1["state"] == 2).all() and (v1["lead"] == 1).all()
                assert (g1["nlog"] == NLOG + 1).all() and (g1["match"][:, 0] == last + 1).all()
                e1 = np.frombuffer(live[3].download(ents.nbytes), dtype=LSB.ENT).reshape(G, NLOG + 1)
                assert (e1["term"][:, NLOG] == TERM).all() and (e1["index"][:, NLOG] == last + 1).all()
                assert (m["type"] == 3).all() and (m["index"] == last[rec]).all() and (m["n_ents"] == 1).all()
                assert (m["log_term"] == 5).all()
            won = n if kind == 6 else 0
            parts = {"group_read": (256 + 32 + 64) * G, "message_in": 64 * n, "result": 48 * n,
                     # the changed words: term, state, vote / term, vote / nlog, prs[id], state, vote, lead, the masks
                     "group_write": {0: 24, 5: 16, 6: 64}[kind] * G,
                     "entry": 40 * won, "message": 144 * total, "term_read": 8 * (G if kind != 6 else total + G)}
            how = ("per group 256 B + 32 B + 64 B read twice (the counting and the applying pass; counted once) and "
                   "the words that changed written; per record 64 B read and 48 B of result; per win a 40-B entry; per "
                   "message 144 B; the 8-B terms the step reads from d_ents")
        if k >= a.warmup:
            lines["step"].append(e)
            lines["wall"].append(w)
    nbytes = sum(parts.values())

    extra = {}
    if a.shape == "win":
        # existing code, the same groups and the same number of messages: lead_step_bench.py's shape a
        ag, aents, aresps, _, amsgs = LSB.build("a", G)
        an, atotal = len(aresps), int(amsgs.sum())
        for d in live + pristine + [d_in, d_res, d_msgs]:
            d.free()
        d_g, d_g0, d_e, d_r = up(ag), up(ag), up(aents), up(aresps)
        d_ares, d_amsgs = ctx.alloc(an * 48 + 64), ctx.alloc(atotal * 144 + 64)
        lines["resp_a"] = []
        for k in range(a.warmup + a.steps):
            hip_check(hip.hipMemcpyDtoD(d_g.ptr, d_g0.ptr, C.c_size_t(ag.nbytes)))
            hip_check(hip.hipDeviceSynchronize())
            L.check(L.lib.elead_step_batch_device(ctx.handle, d_g.ptr, G, None, d_e.ptr, len(aents), d_r.ptr, an,
                                                  d_ares.ptr, d_amsgs.ptr, atotal, C.byref(nm), C.byref(nw)))
            assert nm.value == atotal
            if k >= a.warmup:
                lines["resp_a"].append(float(L.lib.ewal_last_device_ms(ctx.handle)))
        amed = statistics.median(lines["resp_a"])
        smed = statistics.median(lines["step"])
        extra = {"resp_a_responses": an, "resp_a_messages": atotal,
                 "resp_a_ns_per_record": round(amed * 1e6 / an, 4),
                 "resp_a_ns_per_message": round(amed * 1e6 / atotal, 4),
                 "ns_per_record_over_resp_a": round((smed / n) / (amed / an), 3),
                 "ns_per_message_over_resp_a": round((smed / total) / (amed / atotal), 3)}

    def summ(v):
        med = statistics.median(v)
        return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    med = statistics.median(lines["step"])
    gbps = nbytes / med / 1e6
    result = {"tool": "tools/vote_step_bench.py", "shape": a.shape, "input": desc, "groups": G, "peers": P,
              "records": n, "messages": total, "won": n if kind == 6 else 0, "steps": a.steps, "warmup": a.warmup,
              "lines": {k: summ(v) for k, v in lines.items()}, "ms_per_call": round(med, 4),
              "records_per_s": round(n / med * 1e3), "ns_per_record": round(med * 1e6 / n, 4),
              "ns_per_message": round(med * 1e6 / total, 4), "algorithmic_bytes": nbytes, "bytes": how,
              "bytes_parts": parts, "gbps_algorithmic": round(gbps, 1), "hbm_peak_gbps": HBM_PEAK_GBPS,
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
    outdir = a.out or os.path.join(ROOT, "profiles", "vote_step")
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
