"""bench.py --dump-outputs: a plain run on a small configs[1]-shaped WAL
writes the last timed step's result and frame table as float64 .npy files,
the same as a second ReadAll of the same seeded input gives (and the CPU
oracle's verdict), and its line carries ms_per_step for --steps timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from etcd_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--size-gib", "0.03125", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_dump_outputs_of_a_plain_run(ctx, tmp_path):
    import bench
    line = _bench(tmp_path / "a")
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and "configs" not in line and line["cpu_baseline"] is None
    n = line["config"]["frames_per_gpu"]
    k = int(0.73 * n)
    res = np.load(tmp_path / "a" / "result.npy")
    rec = np.load(tmp_path / "a" / "records.npy")
    assert res.dtype == np.float64 and res.shape == (len(bench.RESULT_FIELDS),)
    assert rec.dtype == np.float64 and rec.shape == (n, len(bench.RECORD_FIELDS))
    r = dict(zip(bench.RESULT_FIELDS, res))
    assert (r["status"], r["fail_record"], r["last_crc"], r["n_ents"]) == (L.ERR_RECORD_CRC, k, 0, 0)
    off, data_off, data_len = rec[:, 0], rec[:, 1], rec[:, 2]
    end = np.append(off[1:], line["config"]["wal_bytes_per_gpu"])
    d = data_len > 0    # (a nil Data has no offset)
    assert off[0] == 0 and (np.diff(off) > 8).all() and d.sum() > n - 8
    assert (data_off[d] >= off[d] + 8).all() and (data_off[d] + data_len[d] <= end[d]).all()
    assert r["fail_offset"] == off[k]
    # the same seeded input built here and read through the fixture's ctx gives the same files,
    # and the CPU oracle the same verdict
    import ctypes as C
    from etcd_amd import wal as W
    from oracle import oracle as O
    buf, n2 = W.synth_wal(int(0.03125 * (1 << 30)), 64, 65536, seed=2)
    assert n2 == n and len(buf) == line["config"]["wal_bytes_per_gpu"]
    buf[int(data_off[k] + data_len[k] // 2)] ^= 0x5A
    o = O.readall(bytes(buf), 1)
    assert (o["status"], o["fail_record"]) == (O.ERR_RECORD_CRC, k)
    dbuf = ctx.alloc(len(buf) + 64)
    try:
        dbuf.upload(bytes(buf))
        rs = L.Result()
        assert L.lib.ewal_readall_device(ctx.handle, dbuf.ptr, len(buf), 1, C.byref(rs)) == L.ERR_RECORD_CRC
        bench.dump_outputs(str(tmp_path / "b"), ctx, rs, n)
    finally:
        dbuf.free()
    for name in ("result.npy", "records.npy"):
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name
