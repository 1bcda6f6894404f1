#!/usr/bin/env python3
"""Device-time benchmark of the batched follower append (elog_append_batch_device).

Shapes (--shape; one process per shape, --shape all starts one child per shape
in turn and then states the balance check):
  a   1 Mi groups, each gets a one-entry append that matches at its log's tail
  b   1 Mi groups, each gets a heartbeat with 0 entries, index = log_term = 0
  c   1024 groups, each gets a catch-up message of 4096 entries whose terms
      differ from the follower's log from a random position on
  d   the messages of a and c in one call (1 Mi + 1024 groups)

Every step restores d_groups and d_terms from pristine device copies first
(outside the timed window): the call updates them in place, and a second call
on the updated state would be a different shape.

Lines (--warmup 3 then --steps 20):
  append  the call's device time: HIP events from before its first memset to
          after its last kernel (ewal_last_device_ms; the host's decision
          point between the check pass and the deciding kernels is inside)
  wall    the call's host wall time
GB/s figures are the algorithmic bytes over the median device time; the bytes
are counted from the first step's results as `bytes` says.  The first step's
results are checked against what the shape must give.  Prints one JSON line;
--out writes it to a file too.  Needs the GPU.

Balance (what must hold): time(d) <= time(a) + time(c) + the runs' max-min
spread -- otherwise the long messages are not routed away from the lanes.
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

SHAPES = ["a", "b", "c", "d"]
GROUP = np.dtype([(k, "<u8") for k in ("id", "term", "committed", "unstable", "log_offset", "nlog", "terms_off",
                                       "terms_cap")])
APP = np.dtype([(k, "<u8") for k in ("group", "from_", "index", "log_term", "commit", "ents_first", "n_ents", "pad")])
ENT = np.dtype([("term", "<u8"), ("index", "<u8"), ("data_off", "<u8"), ("data_len", "<u8"), ("type", "<i4"),
                ("data_nil", "<i4")])
RES = np.dtype([("status", "<i4"), ("accepted", "<i4"), ("conflict", "<u8"), ("app_first", "<u8"), ("n_app", "<u8"),
                ("last_index", "<u8"), ("committed", "<u8")])
LONG = 4096


def short_part(G, heartbeat):
    """G groups with a 4-entry log at offset 0 (or 1000 + g) in a window of 8."""
    g = np.zeros(G, GROUP)
    k = np.arange(G, dtype=np.uint64)
    g["id"], g["term"], g["nlog"], g["terms_cap"], g["terms_off"] = k + 1, 5, 4, 8, 8 * k
    g["log_offset"] = 0 if heartbeat else 1000 + k
    g["committed"], g["unstable"] = g["log_offset"] + 1, g["log_offset"] + 4
    terms = np.zeros(8 * G, np.uint64)
    for j, t in enumerate((0, 4, 5, 5)):
        terms[j::8] = t
    a = np.zeros(G, APP)
    a["group"], a["from_"] = k, 77
    if heartbeat:
        ents = np.zeros(0, ENT)
        a["commit"] = 3
        want = dict(n_app=0, last=g["log_offset"] + 3, committed=np.maximum(g["committed"], 0))
    else:
        ents = np.zeros(G, ENT)
        ents["term"], ents["index"], ents["data_nil"] = 5, g["log_offset"] + 4, 1
        a["index"], a["log_term"], a["commit"], a["ents_first"], a["n_ents"] = g["log_offset"] + 3, 5, g["log_offset"] + 4, k, 1
        want = dict(n_app=1, last=g["log_offset"] + 4, committed=g["log_offset"] + 4)
    return g, terms, a, ents, want


def long_part(G, rng):
    """G groups with a log of 1 + LONG entries; the message matches ents[0] and
    carries LONG entries that differ from position p (random) on."""
    g = np.zeros(G, GROUP)
    k = np.arange(G, dtype=np.uint64)
    nlog, cap = 1 + LONG, 2 * LONG + 8
    g["id"], g["term"], g["nlog"], g["terms_cap"], g["terms_off"] = k + 1, 7, nlog, cap, cap * k
    g["log_offset"] = 50000 + k
    g["committed"], g["unstable"] = g["log_offset"], g["log_offset"] + nlog
    terms = np.zeros(cap * G, np.uint64)
    t2 = terms.reshape(G, cap)
    t2[:, :nlog] = 6
    p = rng.integers(0, LONG, size=G)
    ents = np.zeros(G * LONG, ENT)
    et = ents["term"].reshape(G, LONG)
    et[:] = 6
    et[np.arange(LONG)[None, :] >= p[:, None]] = 7
    ents["index"] = (g["log_offset"][:, None] + 1 + np.arange(LONG, dtype=np.uint64)[None, :]).reshape(-1)
    ents["data_nil"] = 1
    a = np.zeros(G, APP)
    a["group"], a["from_"], a["index"], a["log_term"] = k, 78, g["log_offset"], 6
    a["commit"], a["ents_first"], a["n_ents"] = g["log_offset"] + 10, LONG * k, LONG
    want = dict(n_app=(LONG - p).astype(np.uint64), last=g["log_offset"] + LONG,
                committed=g["log_offset"] + 10, conflict=g["log_offset"] + 1 + p.astype(np.uint64))
    return g, terms, a, ents, want


def build(shape, rng, n_short=1 << 20, n_long=1024):
    if shape in ("a", "b"):
        g, terms, a, ents, want = short_part(n_short, shape == "b")
        desc = {"a": "1 Mi groups: a one-entry append matching at the log's tail",
                "b": "1 Mi groups: a heartbeat with 0 entries, index = log_term = 0"}[shape]
        return g, terms, a, ents, [want], desc
    lg, lterms, la, lents, lwant = long_part(n_long, rng)
    if shape == "c":
        return lg, lterms, la, lents, [lwant], "1024 groups: 4096 entries each, conflict at a random position"
    g, terms, a, ents, want = short_part(n_short, False)
    # the long groups after the short ones; the long messages in the middle of the short ones
    lg["terms_off"] += len(terms)
    la["group"] += len(g)
    la["ents_first"] += len(ents)
    half = len(a) // 2
    apps = np.concatenate([a[:half], la, a[half:]])
    order = [dict((k, v[:half] if isinstance(v, np.ndarray) else v) for k, v in want.items()), lwant,
             dict((k, v[half:] if isinstance(v, np.ndarray) else v) for k, v in want.items())]
    return (np.concatenate([g, lg]), np.concatenate([terms, lterms]), apps, np.concatenate([ents, lents]), order,
            "the messages of a and c in one call")


def run_shape(a):
    from etcd_amd import _lib as L
    from etcd_amd import raftlog as R
    from etcd_amd import wal as W

    def hip_check(rc):
        if rc != 0:
            raise RuntimeError("HIP error %d" % rc)

    hip = C.CDLL("libamdhip64.so.7")
    groups, terms, apps, ents, wants, desc = build(a.shape, np.random.default_rng(9), a.short_groups, a.long_groups)
    G, n = len(groups), len(apps)
    ctx = W.Context(0)

    def up(arr):
        d = ctx.alloc(arr.nbytes + 64)
        if arr.nbytes:
            d.upload_ptr(arr.ctypes.data, arr.nbytes)
        return d

    d_groups, d_terms, d_apps, d_ents = up(groups), up(terms), up(apps), up(ents)
    g0, t0 = up(groups), up(terms)   # pristine copies
    d_res, d_resp = ctx.alloc(n * 48 + 64), ctx.alloc(n * 144 + 64)
    acc, app = C.c_uint64(0), C.c_uint64(0)

    def restore():
        hip_check(hip.hipMemcpyDtoD(d_groups.ptr, g0.ptr, C.c_size_t(groups.nbytes)))
        hip_check(hip.hipMemcpyDtoD(d_terms.ptr, t0.ptr, C.c_size_t(terms.nbytes)))
        hip_check(hip.hipDeviceSynchronize())

    def call():
        t = time.perf_counter()
        L.check(L.lib.elog_append_batch_device(ctx.handle, d_groups.ptr, G, d_terms.ptr, len(terms), d_apps.ptr, n,
                                               d_ents.ptr, len(ents), d_res.ptr, d_resp.ptr, C.byref(acc),
                                               C.byref(app)))
        return float(L.lib.ewal_last_device_ms(ctx.handle)), (time.perf_counter() - t) * 1e3

    lines = {"append": [], "wall": []}
    nbytes, how = 0, ""
    for k in range(a.warmup + a.steps):
        restore()
        e, w = call()
        if k == 0:
            res = np.frombuffer(d_res.download(n * 48), dtype=RES)
            assert not res["status"].any() and res["accepted"].all() and acc.value == n
            pos = 0
            for want in wants:
                m = len(want["last"])
                r = res[pos:pos + m]
                assert (r["n_app"] == want["n_app"]).all() and (r["last_index"] == want["last"]).all()
                assert (r["committed"] == want["committed"]).all()
                if "conflict" in want:
                    assert (r["conflict"] == want["conflict"]).all()
                pos += m
            assert pos == n and app.value == int(res["n_app"].sum())
            # a sample of the responses and of the updated windows
            resp = R.responses_from(d_resp.download(144 * min(n, 4)), min(n, 4))
            assert all(x["type"] == 4 and not x["reject"] for x in resp)
            assert resp[0]["index"] == int(res["last_index"][0]) and resp[0]["to"] == int(apps["from_"][0])
            g1 = np.frombuffer(d_groups.download(groups.nbytes), dtype=GROUP)
            gi = apps["group"].astype(np.int64)
            assert (g1["nlog"][gi] - 1 + g1["log_offset"][gi] == res["last_index"]).all()
            assert (g1["committed"][gi] == res["committed"]).all()
            # the algorithmic bytes of this call
            ne = apps["n_ents"].astype(np.int64)
            frm = apps["index"] + 1
            after = (groups["nlog"][gi] - 1 + groups["log_offset"][gi] - apps["index"]).astype(np.int64)
            compared = np.where(res["conflict"] == 0, np.minimum(ne, after),
                                np.minimum((res["conflict"] - frm).astype(np.int64) + 1, after))
            # every entry's term is needed once: compared, appended, or both
            used = np.where(res["conflict"] == 0, np.minimum(ne, after), ne)
            parts = {"app_and_group_read": 128 * n, "group_write": 24 * int(res["accepted"].sum()),
                     "entry_terms_read": 8 * int(used.sum()), "term_gather": 8 * int(n + compared.sum()),
                     "terms_written": 8 * int(res["n_app"].sum()), "result": 48 * n, "response": 144 * n}
            nbytes = sum(parts.values())
            how = ("per message 64 B app + 64 B group read, 48 B result, 144 B response; per accepted message 24 B "
                   "of group written; 8 B per entry term read (the compared ones, and all of a message that appends), "
                   "8 B per log term gathered (the matchTerm word and every compared position), 8 B per term written")
            bytes_parts = parts
        if k >= a.warmup:
            lines["append"].append(e)
            lines["wall"].append(w)

    def summ(v):
        med = statistics.median(v)
        return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    med = statistics.median(lines["append"])
    result = {"tool": "tools/log_append_bench.py", "shape": a.shape, "input": desc, "messages": n, "groups": G,
              "entries": len(ents), "term_words": len(terms), "accepted": acc.value, "appended": app.value,
              "lane_max_entries": R.LANE_MAX, "steps": a.steps, "warmup": a.warmup,
              "lines": {k: summ(v) for k, v in lines.items()},
              "ms_per_call": round(med, 4), "messages_per_s": round(n / med * 1e3),
              "algorithmic_bytes": nbytes, "bytes": how, "bytes_parts": bytes_parts,
              "gbps_algorithmic": round(nbytes / med / 1e6, 1)}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    ctx.close()
    return 0


def run_all(a):
    outdir = a.out or os.path.join(ROOT, "profiles", "log_append")
    res = {}
    for s in SHAPES:
        path = os.path.join(outdir, "shape_%s.json" % s)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--shape", s, "--steps", str(a.steps),
                               "--warmup", str(a.warmup), "--short-groups", str(a.short_groups), "--long-groups",
                               str(a.long_groups), "--out", path], timeout=a.child_timeout)
        res[s] = json.load(open(path))["lines"]["append"]
    spread = max(r["max_ms"] - r["min_ms"] for r in (res["d"], res["a"], res["c"]))
    bal = {"tool": "tools/log_append_bench.py", "check": "time(d) <= time(a) + time(c) + max-min spread",
           "d_ms": res["d"]["median_ms"], "a_ms": res["a"]["median_ms"], "c_ms": res["c"]["median_ms"],
           "spread_ms": round(spread, 4),
           "holds": bool(res["d"]["median_ms"] <= res["a"]["median_ms"] + res["c"]["median_ms"] + spread)}
    print(json.dumps(bal))
    with open(os.path.join(outdir, "balance.json"), "w") as f:
        f.write(json.dumps(bal, indent=1) + "\n")
    return 0 if bal["holds"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=SHAPES + ["all"], default="all")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--short-groups", type=int, default=1 << 20, help="groups of shapes a, b and d's short part")
    ap.add_argument("--long-groups", type=int, default=1024, help="groups of shape c and d's long part")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=None, help="a JSON file (one shape) or a directory (--shape all)")
    a = ap.parse_args()
    return run_all(a) if a.shape == "all" else run_shape(a)


if __name__ == "__main__":
    sys.exit(main())
