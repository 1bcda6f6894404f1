#!/usr/bin/env python3
"""Device-time benchmark of the batched Tick (etick_batch_device).

Shapes (--shape; one process per shape, --shape all starts one child per shape
in turn), each 1 Mi groups of 3 peers at election 10, heartbeat 1 (the
server's constants), d_sel NULL and d_draws NULL:
  quiet  followers at elapsed 0: every one IDLE, no output
  beat   leaders at elapsed 1: every one fires a msgBeat
  storm  followers at elapsed 19: every one fires a msgHup (d >= election: no
         lane runs the modulo)
  mixed  one third leaders alternating elapsed 0 and 1, the followers spread
         over elapsed 9..18 (most of them draw and run the modulo)

Every step restores d_vstate from a pristine device copy first (outside the
timed window): the call updates elapsed in place.

Lines (--warmup 3 then --steps 20):
  step   the call's device time: HIP events from before its first memset to
         after its last kernel (ewal_last_device_ms; the host's decision point
         between the counting and the apply pass is inside)
  peek   the same call with d_hups == d_beats == NULL (results alone)
  wall   the emitting call's host wall time
  idle   in quiet's process only: eready_batch_device's peek (existing code) on
         ready_bench.py's shape idle -- as many groups, more bytes a group --
         timed the same way: the yardstick
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
import ready_bench as RB  # noqa: E402
import vote_step_bench as VSB  # noqa: E402

HBM_PEAK_GBPS = LSB.HBM_PEAK_GBPS
SHAPES = ["quiet", "beat", "storm", "mixed"]
U8 = "<u8"
RES = np.dtype([("status", "<i4"), ("action", "<i4"), ("elapsed", U8), ("out_pos", U8), ("draw", U8)])
HUPS = VSB.MSG_IN
BEATS = np.dtype([("group", U8), ("kind", U8), ("etype", "<i4"), ("data_nil", "<i4"), ("data_off", U8), ("data_len", U8),
                  ("pad", U8)])
IDLE, HELD, HUP, BEAT = 1, 2, 3, 4
ELECTION, HEARTBEAT, SEED, TERM = 10, 1, 0x7E57, 5
DESC = {"quiet": "1 Mi followers at elapsed 0", "beat": "1 Mi leaders at elapsed 1",
        "storm": "1 Mi followers at elapsed 19",
        "mixed": "1 Mi groups: a third leaders at elapsed 0 / 1, the followers at elapsed 9..18"}


def draw(seed, ids, term, elapsed):
    """etick_draw over uint64 arrays (numpy's uint64 arithmetic wraps)."""
    with np.errstate(over="ignore"):
        x = np.uint64(seed) ^ ids * np.uint64(0x9E3779B97F4A7C15) ^ np.uint64(term) * np.uint64(0xBF58476D1CE4E5B9) \
            ^ elapsed * np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x >> np.uint64(1)


def build(shape, G):
    """(groups, vstate, the wanted action, elapsed and draw of every group)."""
    k = np.arange(G, dtype=np.uint64)
    g = np.zeros(G, LSB.GROUP)
    g["id"], g["term"], g["nlog"], g["n_peers"] = k + 1, TERM, 1, 3
    g["peer_id"][:, :3] = (k + 1)[:, None] + np.arange(3, dtype=np.uint64)[None, :]
    vs = np.zeros(G, VSB.VSTATE)
    if shape == "quiet":
        vs["elapsed"] = 0
    elif shape == "beat":
        vs["state"], vs["elapsed"] = 2, 1
    elif shape == "storm":
        vs["elapsed"] = 19
    else:
        lead = k % 3 == 0
        vs["state"] = np.where(lead, 2, 0)
        vs["elapsed"] = np.where(lead, (k // 3) % 2, 9 + k % 10)
    lead = vs["state"] == 2
    e = vs["elapsed"] + np.uint64(1)
    d = e.astype(np.int64) - ELECTION
    dr = np.where(~lead & (d >= 0), draw(SEED, g["id"], TERM, e), 0).astype(np.uint64)
    hup = ~lead & (d >= 0) & (d > (dr % np.uint64(ELECTION)).astype(np.int64))
    beat = lead & (e > HEARTBEAT)
    action = np.where(beat, BEAT, np.where(hup, HUP, np.where(~lead & (d >= 0), HELD, IDLE))).astype(np.int32)
    elapsed = np.where(beat | hup, 0, e).astype(np.uint64)
    return g, vs, action, elapsed, dr


def run_shape(a):
    from etcd_amd import _lib as L
    from etcd_amd import wal as W

    def hip_check(rc):
        if rc != 0:
            raise RuntimeError("HIP error %d" % rc)

    hip = C.CDLL("libamdhip64.so.7")
    G = a.groups or (1 << 20)
    groups, vstate, w_action, w_elapsed, w_draw = build(a.shape, G)
    n_hups, n_beats = int((w_action == HUP).sum()), int((w_action == BEAT).sum())
    ctx = W.Context(0)

    def up(arr):
        d = ctx.alloc(arr.nbytes + 64)
        if arr.nbytes:
            d.upload_ptr(arr.ctypes.data, arr.nbytes)
        return d

    d_groups, live, pristine = up(groups), up(vstate), up(vstate)
    d_res, d_hups, d_beats = ctx.alloc(G * 32 + 64), ctx.alloc(n_hups * 64 + 64), ctx.alloc(n_beats * 48 + 64)
    nh, nb = C.c_uint64(0), C.c_uint64(0)

    def restore():
        hip_check(hip.hipMemcpyDtoD(live.ptr, pristine.ptr, C.c_size_t(vstate.nbytes)))
        hip_check(hip.hipDeviceSynchronize())

    def call(emit=True):
        t = time.perf_counter()
        L.check(L.lib.etick_batch_device(ctx.handle, d_groups.ptr, live.ptr, G, None, G, ELECTION, HEARTBEAT, None, SEED,
                                         d_res.ptr, d_hups.ptr if emit else None, n_hups, d_beats.ptr if emit else None,
                                         n_beats, C.byref(nh), C.byref(nb)))
        return float(L.lib.ewal_last_device_ms(ctx.handle)), (time.perf_counter() - t) * 1e3

    lines = {"step": [], "peek": [], "wall": []}
    for k in range(a.warmup + a.steps):
        restore()
        p, _ = call(emit=False)
        assert (nh.value, nb.value) == (n_hups, n_beats)
        e, w = call()
        if k == 0:
            res = np.frombuffer(d_res.download(G * 32), dtype=RES)
            assert not res["status"].any() and (nh.value, nb.value) == (n_hups, n_beats)
            assert (res["action"] == w_action).all() and (res["elapsed"] == w_elapsed).all()
            assert (res["draw"] == w_draw).all()
            fired = (w_action == HUP) | (w_action == BEAT)
            pos = np.where(w_action == HUP, np.cumsum(w_action == HUP) - 1, np.cumsum(w_action == BEAT) - 1)
            assert (res["out_pos"] == np.where(fired, pos, 0).astype(np.uint64)).all()
            v1 = np.frombuffer(live.download(vstate.nbytes), dtype=VSB.VSTATE)
            assert (v1["elapsed"] == w_elapsed).all() and (v1["state"] == vstate["state"]).all()
            if a.shape == "quiet":
                assert n_hups == n_beats == 0 and (w_action == IDLE).all()
            if a.shape == "beat":
                assert n_beats == G
            if a.shape == "storm":
                assert n_hups == G
            if a.shape == "mixed":
                assert min((w_action == x).sum() for x in (IDLE, HELD, HUP, BEAT)) > G // 20
            if n_hups:
                h = np.frombuffer(d_hups.download(64 * n_hups), dtype=HUPS)
                who = np.nonzero(w_action == HUP)[0].astype(np.uint64)
                assert (h["group"] == who).all() and (h["from_"] == groups["id"][who]).all() and not h["kind"].any()
                assert not (h["term"].any() or h["index"].any() or h["log_term"].any() or h["reject"].any())
            if n_beats:
                b = np.frombuffer(d_beats.download(48 * n_beats), dtype=BEATS)
                who = np.nonzero(w_action == BEAT)[0].astype(np.uint64)
                assert (b["group"] == who).all() and (b["kind"] == 1).all() and not b["data_len"].any()
            changed = int((w_elapsed != vstate["elapsed"]).sum())
            parts = {"group_read": (112 + 32 + 64) * G, "scratch": 2 * 32 * G, "result": 32 * G, "elapsed": 8 * changed,
                     "hups": 64 * n_hups, "beats": 48 * n_beats}
            how = ("per group the first 112 B of its elead_group, its 32 B of reserved words and its 64-B evote_state "
                   "read once, a 32-B scratch record written and read, 32 B of result, the elapsed word where it "
                   "changed; 64 B a msgHup, 48 B a msgBeat")
        if k >= a.warmup:
            lines["step"].append(e)
            lines["peek"].append(p)
            lines["wall"].append(w)
    nbytes = sum(parts.values())

    extra = {}
    if a.shape == "quiet":
        # existing code, as many groups: ready_bench.py's shape idle, peeked
        for d in (d_groups, live, pristine, d_res, d_hups, d_beats):
            d.free()
        rg, rps, rvs, rrs, rents = RB.build("idle", G)
        bufs = [up(x) for x in (rg, rps, rvs, rrs, rents)]
        d_rres = ctx.alloc(G * 96 + 64)
        lines["idle"] = []
        for k in range(a.warmup + a.steps):
            L.check(L.lib.eready_batch_device(ctx.handle, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, G, None,
                                              bufs[4].ptr, len(rents), None, G, d_rres.ptr, None, 0, C.byref(nh),
                                              C.byref(nb)))
            assert (nh.value, nb.value) == (0, 0)
            if k >= a.warmup:
                lines["idle"].append(float(L.lib.ewal_last_device_ms(ctx.handle)))
        imed = statistics.median(lines["idle"])
        extra = {"idle_peek_ns_per_group": round(imed * 1e6 / G, 4),
                 "step_over_idle_peek": round(statistics.median(lines["step"]) / imed, 3),
                 "peek_over_idle_peek": round(statistics.median(lines["peek"]) / imed, 3)}

    def summ(v):
        med = statistics.median(v)
        return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    med = statistics.median(lines["step"])
    gbps = nbytes / med / 1e6
    result = {"tool": "tools/tick_bench.py", "shape": a.shape, "input": DESC[a.shape], "groups": G, "hups": n_hups,
              "beats": n_beats, "steps": a.steps, "warmup": a.warmup, "lines": {k: summ(v) for k, v in lines.items()},
              "ms_per_call": round(med, 4), "groups_per_s": round(G / med * 1e3),
              "ns_per_group": round(med * 1e6 / G, 4), "algorithmic_bytes": nbytes, "bytes": how, "bytes_parts": parts,
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
    outdir = a.out or os.path.join(ROOT, "profiles", "tick")
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
