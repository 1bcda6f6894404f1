#!/usr/bin/env python3
"""Device-time benchmark of the batched Ready (eready_batch_device).

Shapes (--shape; one process per shape, --shape all starts one child per shape
in turn):
  idle   1 Mi groups with nothing to report: all stable, all applied, the
         HardState and the SoftState as accepted (no save record)
  prop   1 Mi leaders after one proposal round: one unstable entry and a commit
         advance each (EREADY_HARD: 2 save records a group)
  burst  16 Ki restarted followers with 64 unstable entries each (64 save
         records a group, 1 Mi in all)

Every group has a log at offset 1000 + g in its own window of d_ents, d_sel is
NULL (every group in order) and d_snaps is NULL.  Every step restores d_pstate
and d_rstate from pristine device copies first (outside the timed window): the
call updates both in place.

Lines (--warmup 3 then --steps 20):
  step   the call's device time: HIP events from before its first memset to
         after its last kernel (ewal_last_device_ms; the host's decision point
         between the counting and the emit pass is inside)
  peek   the same call with d_save == NULL (results alone)
  wall   the emitting call's host wall time
  hup    in prop's process only: evote_step_batch_device (existing code) on
         vote_step_bench.py's shape hup -- 1 Mi groups, one record each --
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
import vote_step_bench as VSB  # noqa: E402

HBM_PEAK_GBPS = LSB.HBM_PEAK_GBPS
SHAPES = ["idle", "prop", "burst"]
U8 = "<u8"
RSTATE = np.dtype([("hs_term", U8), ("hs_vote", U8), ("hs_commit", U8), ("lead", U8), ("state", U8), ("snapi", U8),
                   ("applied", U8), ("soft_dirty", U8)])
RES = np.dtype([("status", "<i4"), ("flags", "<i4"), ("term", U8), ("vote", U8), ("commit", U8), ("ents_first", U8),
                ("n_ents", U8), ("committed_first", U8), ("n_committed", U8), ("save_first", U8), ("n_save", U8),
                ("lead", U8), ("state", "<i4"), ("pad", "<i4")])
SAVE = np.dtype([("kind", "<i4"), ("etype", "<i4"), ("a", U8), ("b", U8), ("c", U8), ("data_off", U8), ("data_len", U8),
                 ("data_nil", "<i4"), ("pad", "<i4")])
HARD, UPDATES = 2, 8
TERM = 5
# shape: (groups, entries a log, unstable entries, commit advance, save records a group, description)
SPEC = {"idle": (1 << 20, 4, 0, 0, 0, "1 Mi groups with nothing to report"),
        "prop": (1 << 20, 5, 1, 1, 2, "1 Mi leaders: one unstable entry and a commit advance each"),
        "burst": (1 << 14, 65, 64, 0, 64, "16 Ki followers: 64 unstable entries each")}


def build(shape, G):
    _, nlog, nun, adv, _, _ = SPEC[shape]
    k = np.arange(G, dtype=np.uint64)
    g = np.zeros(G, LSB.GROUP)
    off = 1000 + k
    last = off + np.uint64(nlog - 1)
    g["id"], g["term"], g["committed"], g["log_offset"], g["nlog"], g["ents_first"], g["n_peers"] = \
        1, TERM, last if adv else off + 1, off, nlog, np.uint64(nlog) * k, 3
    g["peer_id"][:, :3] = np.arange(1, 4, dtype=np.uint64)
    ps = np.zeros(G, VSB.PSTATE)
    ps["ents_cap"], ps["unstable"] = nlog, last + 1 - np.uint64(nun)
    vs = np.zeros(G, VSB.VSTATE)
    vs["state"], vs["vote"], vs["lead"] = 2, 1, 1
    rs = np.zeros(G, RSTATE)
    rs["hs_term"], rs["hs_vote"], rs["hs_commit"] = TERM, 1, g["committed"] - np.uint64(adv)
    rs["lead"], rs["state"], rs["applied"] = 1, 2, g["committed"] - np.uint64(adv)
    ents = np.zeros((G, nlog), LSB.ENT)
    ents["term"][:] = TERM
    ents["index"][:] = off[:, None] + np.arange(nlog, dtype=np.uint64)[None, :]
    ents["data_off"][:] = (np.uint64(nlog) * k)[:, None] * 16 + np.arange(nlog, dtype=np.uint64)[None, :] * 16
    ents["data_len"][:] = 16
    return g, ps, vs, rs, ents.reshape(-1)


def run_shape(a):
    from etcd_amd import _lib as L
    from etcd_amd import wal as W

    def hip_check(rc):
        if rc != 0:
            raise RuntimeError("HIP error %d" % rc)

    hip = C.CDLL("libamdhip64.so.7")
    G0, nlog, nun, adv, per_save, desc = SPEC[a.shape]
    G = a.groups or G0
    groups, pstate, vstate, rstate, ents = build(a.shape, G)
    total = G * per_save
    ctx = W.Context(0)

    def up(arr):
        d = ctx.alloc(arr.nbytes + 64)
        if arr.nbytes:
            d.upload_ptr(arr.ctypes.data, arr.nbytes)
        return d

    d_groups, d_vstate, d_ents = up(groups), up(vstate), up(ents)
    host = (pstate, rstate)
    live = [up(x) for x in host]
    pristine = [up(x) for x in host]
    d_res, d_save = ctx.alloc(G * 96 + 64), ctx.alloc(total * 56 + 64)
    ns, nr = C.c_uint64(0), C.c_uint64(0)

    def restore():
        for d, p, arr in zip(live, pristine, host):
            hip_check(hip.hipMemcpyDtoD(d.ptr, p.ptr, C.c_size_t(arr.nbytes)))
        hip_check(hip.hipDeviceSynchronize())

    def call(save=True):
        t = time.perf_counter()
        L.check(L.lib.eready_batch_device(ctx.handle, d_groups.ptr, live[0].ptr, d_vstate.ptr, live[1].ptr, G, None,
                                          d_ents.ptr, len(ents), None, G, d_res.ptr, d_save.ptr if save else None,
                                          total, C.byref(ns), C.byref(nr)))
        return float(L.lib.ewal_last_device_ms(ctx.handle)), (time.perf_counter() - t) * 1e3

    lines = {"step": [], "peek": [], "wall": []}
    for k in range(a.warmup + a.steps):
        restore()
        p, _ = call(save=False)
        assert ns.value == total
        e, w = call()
        if k == 0:
            res = np.frombuffer(d_res.download(G * 96), dtype=RES)
            assert not res["status"].any() and ns.value == total and nr.value == (G if per_save else 0)
            assert (res["flags"] == ((HARD | UPDATES) if adv else UPDATES if nun else 0)).all()
            assert (res["n_ents"] == nun).all() and (res["n_committed"] == adv).all()
            assert (res["n_save"] == per_save).all()
            assert (res["save_first"] == np.arange(G, dtype=np.uint64) * np.uint64(per_save)).all()
            last = groups["log_offset"] + np.uint64(nlog - 1)
            p1 = np.frombuffer(live[0].download(pstate.nbytes), dtype=VSB.PSTATE)
            r1 = np.frombuffer(live[1].download(rstate.nbytes), dtype=RSTATE)
            assert (p1["unstable"] == last + 1).all() and (r1["applied"] == groups["committed"]).all()
            assert (r1["hs_commit"] == groups["committed"]).all()
            if total:
                sv = np.frombuffer(d_save.download(56 * total), dtype=SAVE).reshape(G, per_save)
                first = 0
                if adv:
                    assert (sv["kind"][:, 0] == 3).all() and (sv["a"][:, 0] == TERM).all() and (sv["b"][:, 0] == 1).all()
                    assert (sv["c"][:, 0] == groups["committed"]).all()
                    first = 1
                e0 = ents.reshape(G, nlog)[:, nlog - nun:]
                assert (sv["kind"][:, first:] == 2).all() and (sv["b"][:, first:] == e0["index"]).all()
                assert (sv["a"][:, first:] == TERM).all() and (sv["data_off"][:, first:] == e0["data_off"]).all()
                assert (sv["data_len"][:, first:] == 16).all() and not sv["c"][:, first:].any() and not sv["pad"].any()
            # a second call straight after: nothing
            call()
            assert (ns.value, nr.value) == (0, 0)
            parts = {"group_read": (48 + 32 + 32 + 48 + 64) * G, "result": 96 * G, "scratch": 2 * 32 * G,
                     "entry_flag": 4 * nun * G, "entry_read": 40 * nun * G, "save": 56 * total,
                     # the changed words: unstable; applied and hs_commit
                     "group_write": (8 * (1 if nun else 0) + 16 * adv) * G}
            how = ("per group 224 B of its four records read in the counting pass (and 192 B again in the emit pass: "
                   "counted once), 96 B of result, a 32-B scratch record written and read, the words that changed; per "
                   "unstable entry its data_nil word in the counting pass and its 40 B in the emit pass; per save "
                   "record 56 B")
        if k >= a.warmup:
            lines["step"].append(e)
            lines["peek"].append(p)
            lines["wall"].append(w)
    nbytes = sum(parts.values())

    extra = {}
    if a.shape == "prop":
        # existing code, as many groups: vote_step_bench.py's shape hup
        for d in live + pristine + [d_groups, d_vstate, d_ents, d_res, d_save]:
            d.free()
        hg, hps, hvs, hents, hin = VSB.build("hup", G)
        hhost = (hg, hps, hvs, hents)
        hlive, hprist = [up(x) for x in hhost], [up(x) for x in hhost]
        d_in, d_hres, d_msgs = up(hin), ctx.alloc(G * 48 + 64), ctx.alloc(2 * G * 144 + 64)
        lines["hup"] = []
        for k in range(a.warmup + a.steps):
            for d, p, arr in zip(hlive, hprist, hhost):
                hip_check(hip.hipMemcpyDtoD(d.ptr, p.ptr, C.c_size_t(arr.nbytes)))
            hip_check(hip.hipDeviceSynchronize())
            L.check(L.lib.evote_step_batch_device(ctx.handle, hlive[0].ptr, hlive[1].ptr, hlive[2].ptr, G, None,
                                                  hlive[3].ptr, len(hents), d_in.ptr, G, d_hres.ptr, d_msgs.ptr, 2 * G,
                                                  C.byref(ns), C.byref(nr)))
            assert ns.value == 2 * G
            if k >= a.warmup:
                lines["hup"].append(float(L.lib.ewal_last_device_ms(ctx.handle)))
        hmed = statistics.median(lines["hup"])
        extra = {"hup_ns_per_group": round(hmed * 1e6 / G, 4),
                 "step_over_hup": round(statistics.median(lines["step"]) / hmed, 3)}

    def summ(v):
        med = statistics.median(v)
        return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    med = statistics.median(lines["step"])
    gbps = nbytes / med / 1e6
    result = {"tool": "tools/ready_bench.py", "shape": a.shape, "input": desc, "groups": G, "save_records": total,
              "steps": a.steps, "warmup": a.warmup, "lines": {k: summ(v) for k, v in lines.items()},
              "ms_per_call": round(med, 4), "groups_per_s": round(G / med * 1e3),
              "ns_per_group": round(med * 1e6 / G, 4),
              "ns_per_save_record": round(med * 1e6 / total, 4) if total else None, "algorithmic_bytes": nbytes,
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
    outdir = a.out or os.path.join(ROOT, "profiles", "ready")
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
