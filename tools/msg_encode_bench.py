#!/usr/bin/env python3
"""Device-time benchmark of the batched raftpb.Message encode (emsg_encode_batch_device).

Shapes (--shape; one process per shape, --shape all starts one child per shape
in turn and then states the balance check):
  a   the ingress bench's own mix mirrored (bench.py run_msg): 256 Ki messages
      tiled over 1024 distinct ones -- MsgApp with 1-8 entries of 64 B-1 KiB,
      heartbeats and votes with none
  b   1 Mi heartbeats
  c   fan-out: 64 Ki groups x 4 followers, the four messages of a group share
      one range of 16 x 1 KiB entries
  d   skew: one MsgSnap with 256 MiB of Snapshot.Data plus 100 k heartbeats
  d1  that MsgSnap alone          d2  those heartbeats alone

Lines (--warmup 3 then --steps 20, interleaved per step):
  encode  the call's device time: HIP events from its first kernel to its
          last (ewal_last_device_ms; the host's decision point between the
          size pass and the body pass is inside, and so is the copy of the
          n {off, len} pairs to h_out), the call's wall time, and the device
          time of the same call with h_out == NULL
  d2d     hipMemcpyDtoDAsync of the same number of bytes in the same process
          (HIP events on the null stream): the floor of one read + one write
  cpu     the oracle's or_message_marshal, CPU, single thread, called through
          ctypes: the largest message, plus at most --cpu-sample of the others
          scaled to the rest of the batch
GB/s figures are output bytes over the median time.  The first step's output
is checked against the oracle on a sample of the messages.  Prints one JSON
line; --out writes it to a file too.  Needs the GPU.

Balance (what must hold): time(d) <= time(d1) + time(d2) + the runs' max-min
spread -- otherwise the work split over the waves is wrong.
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

MSG = np.dtype([(k, "<u8") for k in ("type", "to", "from_", "term", "log_term", "index", "commit", "ents_first",
                                      "n_ents", "snap_index", "snap_term", "snap_data_off", "snap_data_len",
                                      "snap_nodes_off", "snap_n_nodes", "snap_removed_off", "snap_n_removed")] +
               [("reject", "<i4"), ("pad", "<i4")])
ENT = np.dtype([("term", "<u8"), ("index", "<u8"), ("data_off", "<u8"), ("data_len", "<u8"), ("type", "<i4"),
                ("data_nil", "<i4")])
SHAPES = ["a", "b", "c", "d", "d1", "d2"]


def heartbeats(n, first=0):
    m = np.zeros(n, MSG)
    k = np.arange(first, first + n, dtype=np.uint64)
    m["type"], m["to"], m["from_"], m["term"], m["commit"] = 8, k % 5 + 2, 1, 5, k
    return m


def build(shape, rng):
    """(data bytes as uint8 array, msgs, ents, u64, description)"""
    ents = np.zeros(0, ENT)
    u64 = np.zeros(0, np.uint64)
    if shape == "a":
        ne = rng.choice([0, 0, 1, 2, 4, 8], size=1024)
        first = np.concatenate([[0], np.cumsum(ne)])
        ents = np.zeros(int(first[-1]), ENT)
        ents["data_len"] = rng.integers(64, 1025, size=len(ents))
        ents["data_off"] = np.concatenate([[0], np.cumsum(ents["data_len"])[:-1]])
        ents["term"], ents["index"] = 5, 1000 + np.arange(len(ents))
        data = rng.integers(0, 256, size=int(ents["data_len"].sum()), dtype=np.uint8)
        d = np.zeros(1024, MSG)
        d["type"] = np.where(ne > 0, 3, rng.choice([1, 5, 8], size=1024))
        d["to"], d["from_"], d["term"], d["log_term"] = 2, 1, 5, 5
        d["index"], d["commit"] = 1000 + 8 * np.arange(1024), 999 + np.arange(1024)
        d["ents_first"], d["n_ents"] = first[:-1], ne
        msgs = np.tile(d, 256)
        desc = "256 Ki messages over 1024 distinct: MsgApp with 1-8 entries of 64 B-1 KiB, heartbeats and votes"
    elif shape == "b":
        data, msgs, desc = np.zeros(0, np.uint8), heartbeats(1 << 20), "1 Mi heartbeats"
    elif shape == "c":
        groups = 64 << 10
        pool = rng.integers(0, 256, size=64 << 20, dtype=np.uint8)
        data = np.tile(pool, groups * 16 * 1024 // len(pool))
        ents = np.zeros(groups * 16, ENT)
        ents["data_len"], ents["data_off"] = 1024, 1024 * np.arange(groups * 16, dtype=np.uint64)
        ents["term"], ents["index"] = 7, 1 + np.arange(groups * 16)
        msgs = np.zeros(groups * 4, MSG)
        g = np.arange(groups * 4, dtype=np.uint64) // 4
        msgs["type"], msgs["to"], msgs["from_"], msgs["term"], msgs["log_term"] = 3, np.arange(groups * 4) % 4 + 2, 1, 7, 7
        msgs["index"], msgs["commit"], msgs["ents_first"], msgs["n_ents"] = 16 * g, 16 * g, 16 * g, 16
        desc = "fan-out: 64 Ki groups x 4 followers sharing one range of 16 x 1 KiB entries per group"
    else:
        snap = np.zeros(0 if shape == "d2" else 1, MSG)
        data = np.zeros(0, np.uint8)
        if len(snap):
            data = np.tile(rng.integers(0, 256, size=16 << 20, dtype=np.uint8), 16)
            snap["type"], snap["to"], snap["from_"], snap["term"] = 7, 2, 1, 5
            snap["snap_index"], snap["snap_term"], snap["snap_data_len"], snap["snap_n_nodes"] = 1 << 20, 5, len(data), 3
            u64 = np.array([1, 2, 3], np.uint64)
        hb = heartbeats(0 if shape == "d1" else 100000)
        # the MsgSnap in the middle of the heartbeats
        msgs = np.concatenate([hb[:len(hb) // 2], snap, hb[len(hb) // 2:]])
        desc = {"d": "skew: one MsgSnap with 256 MiB of Data plus 100 k heartbeats",
                "d1": "one MsgSnap with 256 MiB of Data (it fits the Infinity Cache, so its d2d is not an HBM figure)",
                "d2": "100 k heartbeats"}[shape]
    return data, msgs, ents, u64, desc


def oracle_marshal(O, data, m, ents, u64):
    es = [O.entry_marshal(int(e["type"]), int(e["term"]), int(e["index"]),
                          data[int(e["data_off"]):int(e["data_off"]) + int(e["data_len"])].tobytes())
          for e in ents[int(m["ents_first"]):int(m["ents_first"]) + int(m["n_ents"])]]
    sn = O.snapshot_marshal(data[int(m["snap_data_off"]):int(m["snap_data_off"]) + int(m["snap_data_len"])].tobytes(),
                            [int(x) for x in u64[int(m["snap_nodes_off"]):int(m["snap_nodes_off"]) + int(m["snap_n_nodes"])]],
                            int(m["snap_index"]), int(m["snap_term"]),
                            [int(x) for x in u64[int(m["snap_removed_off"]):int(m["snap_removed_off"]) + int(m["snap_n_removed"])]])
    return O.message_marshal(int(m["type"]), int(m["to"]), int(m["from_"]), int(m["term"]), int(m["log_term"]),
                             int(m["index"]), es, int(m["commit"]), sn, bool(m["reject"]))


def run_shape(a):
    from etcd_amd import _lib as L
    from etcd_amd import raftmsg as M
    from etcd_amd import wal as W
    from oracle import oracle as O   # checker and CPU line only

    def hip_check(rc):
        if rc != 0:
            raise RuntimeError("HIP error %d" % rc)

    hip = C.CDLL("libamdhip64.so.7")
    data, msgs, ents, u64, desc = build(a.shape, np.random.default_rng(9))
    n = len(msgs)
    ctx = W.Context(0)

    def up(arr):
        d = ctx.alloc(arr.nbytes + 64)
        if arr.nbytes:
            d.upload_ptr(arr.ctypes.data, arr.nbytes)
        return d

    d_data, d_msgs, d_ents, d_u64 = up(data), up(msgs), up(ents), up(u64)
    args = (ctx, d_data, len(data), d_msgs, n, d_ents, len(ents), d_u64, len(u64))
    offs, lens, total = M.encode_messages_device(*args, None, 0)
    assert total == L.lib.emsg_encode_size(msgs.ctypes.data_as(C.POINTER(L.OutMsg)), n,
                                           ents.ctypes.data_as(C.POINTER(L.EntryDesc)), len(ents),
                                           u64.ctypes.data_as(C.POINTER(C.c_uint64)), len(u64))
    d_out, d_src = ctx.alloc(total + 64), ctx.alloc(total + 64)
    enc = (L.Encoded * n)()
    tot = C.c_uint64(0)
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        hip_check(hip.hipEventCreate(C.byref(e)))

    def encode(h_out=enc):
        t = time.perf_counter()
        L.check(L.lib.emsg_encode_batch_device(ctx.handle, d_data.ptr, len(data), d_msgs.ptr, n, d_ents.ptr, len(ents),
                                               d_u64.ptr, len(u64), d_out.ptr, total, h_out, C.byref(tot)))
        return float(L.lib.ewal_last_device_ms(ctx.handle)), (time.perf_counter() - t) * 1e3

    def d2d():
        hip_check(hip.hipEventRecord(ev[0], None))
        hip_check(hip.hipMemcpyDtoDAsync(d_out.ptr, d_src.ptr, C.c_size_t(total), None))
        hip_check(hip.hipEventRecord(ev[1], None))
        hip_check(hip.hipEventSynchronize(ev[1]))
        ms = C.c_float()
        hip_check(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
        return ms.value

    lines = {"encode": [], "encode_call_wall": [], "encode_no_h_out": [], "d2d": []}
    for k in range(a.warmup + a.steps):
        d = d2d()     # first: the encode's bytes are the ones left in d_out for the check below
        e, w = encode()
        if k == 0:
            # a sample of the messages against the oracle: the first 64, the last, the largest
            assert tot.value == total and [x.off for x in enc[:4]] == offs[:4]
            for i in sorted(set(range(min(64, n))) | {n - 1, int(np.argmax(np.array(lens)))}):
                got = d_out.download(lens[i], offs[i])
                assert got == oracle_marshal(O, data, msgs[i], ents, u64), i
        e0, _ = encode(None)
        if k >= a.warmup:
            lines["encode_no_h_out"].append(e0)
            lines["encode"].append(e)
            lines["encode_call_wall"].append(w)
            lines["d2d"].append(d)

    # CPU, single thread: the largest message on its own, a sample of the others scaled to the rest
    big = int(np.argmax(np.array(lens)))
    idx = sorted(set(np.linspace(0, n - 1, min(n, a.cpu_sample)).astype(int).tolist()) - {big})
    t = time.perf_counter()
    oracle_marshal(O, data, msgs[big], ents, u64)
    big_ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    for i in idx:
        oracle_marshal(O, data, msgs[i], ents, u64)
    cpu_ms = big_ms + (time.perf_counter() - t) * 1e3 * (n - 1) / max(len(idx), 1)

    def summ(v):
        med = statistics.median(v)
        return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "gbps_out": round(total / med / 1e6, 1)}

    result = {"tool": "tools/msg_encode_bench.py", "shape": a.shape, "input": desc, "messages": n,
              "entries": len(ents), "data_bytes": int(len(data)), "out_bytes": total, "steps": a.steps,
              "warmup": a.warmup, "tile_bytes": M.ENCODE_TILE,
              "lines": {k: summ(v) for k, v in lines.items()},
              "cpu_single_thread": {"what": "oracle or_message_marshal through ctypes, one thread, the largest message and "
                                            "%d of the other %d timed and scaled" % (len(idx), n - 1),
                                    "ms": round(cpu_ms, 2), "gbps_out": round(total / cpu_ms / 1e6, 3)}}
    result["encode_over_d2d"] = round(result["lines"]["encode"]["median_ms"] / result["lines"]["d2d"]["median_ms"], 3)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    ctx.close()
    return 0


def run_all(a):
    outdir = a.out or os.path.join(ROOT, "profiles", "msg_encode")
    res = {}
    for s in SHAPES:
        path = os.path.join(outdir, "shape_%s.json" % s)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--shape", s, "--steps", str(a.steps),
                               "--warmup", str(a.warmup), "--cpu-sample", str(a.cpu_sample), "--out", path],
                              timeout=a.child_timeout)
        res[s] = json.load(open(path))["lines"]["encode"]
    spread = max(r["max_ms"] - r["min_ms"] for r in (res["d"], res["d1"], res["d2"]))
    bal = {"tool": "tools/msg_encode_bench.py", "check": "time(d) <= time(d1) + time(d2) + max-min spread",
           "d_ms": res["d"]["median_ms"], "d1_ms": res["d1"]["median_ms"], "d2_ms": res["d2"]["median_ms"],
           "spread_ms": round(spread, 4),
           "holds": bool(res["d"]["median_ms"] <= res["d1"]["median_ms"] + res["d2"]["median_ms"] + spread)}
    print(json.dumps(bal))
    with open(os.path.join(outdir, "balance.json"), "w") as f:
        f.write(json.dumps(bal, indent=1) + "\n")
    return 0 if bal["holds"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=SHAPES + ["all"], default="all")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-sample", type=int, default=4096)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=None, help="a JSON file (one shape) or a directory (--shape all)")
    a = ap.parse_args()
    return run_all(a) if a.shape == "all" else run_shape(a)


if __name__ == "__main__":
    sys.exit(main())
