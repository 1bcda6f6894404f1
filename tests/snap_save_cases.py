"""Shared inputs of the Snapshotter.save tests (test_gpu_snap_save.py on the
GPU, test_snap_save_host.py without one): snapshots as dicts, the device blob
their Data lives in, and the bytes the reference writes for each (oracle)."""
import json
import os

import numpy as np

from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALIGNS = (0, 1, 3, 4, 8, 15)


def lattice_lengths(T):
    return (0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 16383, 16384, T - 1, T, T + 1, 2 * T + 5)


def pack(datas_aligns, seed_fields=0):
    """[(data bytes, data_off mod 16)] -> (blob, snaps): every Data placed at
    the next offset with that residue; fields vary with the position."""
    blob = bytearray()
    snaps = []
    for k, (data, al) in enumerate(datas_aligns):
        off = (len(blob) + 15) // 16 * 16 + al
        blob += bytes(off - len(blob))
        blob += data
        snaps.append(dict(data_off=off, data_len=len(data), index=1 + k + seed_fields, term=1 + (k % 5),
                          nodes=[1, 2, 3][:k % 4], removed=[7][:k % 2]))
    return bytes(blob), snaps


def lattice(T):
    """The length x alignment lattice: one snapshot per (len, data_off mod 16)."""
    rng = np.random.default_rng(20141021)
    return pack([(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), al) for n in lattice_lengths(T) for al in ALIGNS])


def body(s, blob):
    data = blob[s["data_off"]:s["data_off"] + s["data_len"]]
    return O.snapshot_marshal(data, list(s.get("nodes", ())), s.get("index", 0), s.get("term", 0),
                              list(s.get("removed", ()))) + bytes(s.get("unrec") or b"")


def expected(s, blob, poly=O.CASTAGNOLI):
    """Snapshotter.save's file bytes and stored CRC (snap/snapshotter.go:46-60)."""
    b = body(s, blob)
    crc = O.crc32_update(0, b, poly)
    return O.snappb_marshal(crc, b), crc


def reference_snap():
    """testSnap of snap/snapshotter_test.go:15-20."""
    k = json.load(open(os.path.join(GOLDEN, "reference_kats.json")))["snapshot"]["test_snap"]
    return dict(data=k["data"].encode(), nodes=k["nodes"], index=k["index"], term=k["term"])
