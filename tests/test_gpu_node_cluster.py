"""node_cluster_cases' scenario on the device: every existing call by the real
entry points against raft_model, the membership calls and enode_batch_device
bit for bit against their restatements, the WALs written by ewal_save_device,
replayed by ewal_readall_batch_device and handed to the restart through
enode_reqs_from_batch and ewal_batch_entries_device -- the entries never come
to the host for the call, and the WAL buffer itself is d_data afterwards."""
import ctypes

import numpy as np
import pytest

from etcd_amd import _lib as L
from etcd_amd import raftnode as RN

import cluster_cases as C
import node_cases as N
import node_cluster_cases as NC
import test_gpu_conf_cluster as TC
import tick_cluster_cases as T

pytestmark = pytest.mark.gpu


class DeviceHost:
    def __init__(self, ctx):
        self.ctx = ctx

    def node_call(self, c):
        got, _ = N.check_call(self.ctx, c)
        return got

    def wals(self, cl):
        """ewal_save_device per group: one chained call a WAL, the same bytes as the oracle's encoder."""
        ctx, out = self.ctx, []
        data = bytes(cl.data) + b"\0" * (8 - len(cl.data) % 8)
        d_data = RN._up(ctx, np.frombuffer(data, dtype=np.uint8))
        try:
            for g in cl.real:
                rows = NC.save_rows_of(cl, g)
                recs = np.concatenate([C._rows([[4, 0, 0, 0, 0, 0, 1]], 7), C._rows([list(r) for r in rows], 7)])
                cap = 128 * len(recs) + sum(int(r[5]) for r in rows) + 4096
                bufs = [RN._up(ctx, recs), ctx.alloc(cap)]
                try:
                    n, crc = ctypes.c_uint64(), ctypes.c_uint32()
                    L.check(L.lib.ewal_save_device(ctx.handle, d_data.ptr, len(cl.data), bufs[0].ptr, len(recs), 0,
                                                   bufs[1].ptr, cap, ctypes.byref(n), ctypes.byref(crc), None))
                    out.append(bufs[1].download(n.value))
                finally:
                    RN._free(bufs)
                assert out[-1] == NC.wal_of(cl, g), g
        finally:
            d_data.free()
        return out

    def restart(self, cl, wals):
        ctx, n = self.ctx, len(cl.real)
        blob = b"".join(wals)
        lens = [len(w) for w in wals]
        offs = np.cumsum([0] + lens[:-1]).tolist()
        d_blob = ctx.alloc(len(blob) + 64)
        bufs = []
        try:
            d_blob.upload(blob)
            res = RN.readall_batch_raw(d_blob, lens, [0] * n)
            assert all(res[s].status == L.OK and res[s].n_unrec == 0 for s in range(n))
            ptr, total = RN.entries_device(ctx)
            # the caller's fields first, then the replay's
            rows = np.zeros((n, N.REQ_WORDS), np.uint64)
            for s, g in enumerate(cl.real):
                rows[s, 2:5] = [cl.node_of(g), g * cl.cap, cl.cap]
                rows[s, 11] = N.NO_SNAP
            RN.reqs_from_batch(ctx, res, offs, rows)
            assert [int(v) for v in rows[:, 0]] == list(range(n))
            rows[:, 0] = np.array(cl.real, dtype=np.uint64)          # shard s is group real[s] here
            raw = (ctypes.c_char * (total * 40))()
            L.check(L.lib.ewal_download(ctx.handle, raw, ctypes.c_void_p(ptr), total * 40))
            src = np.frombuffer(raw.raw, dtype=np.uint64).reshape(total, 5).copy()   # for the comparison only
            c, back = NC.restart_call(cl, wals, src_first=[int(v) for v in rows[:, 5]], src=src)
            # every field of every request is what the oracle's replay gives, and so is every replayed entry
            assert np.array_equal(rows, c["reqs"]), np.argwhere(rows != c["reqs"])[:4].tolist()
            for s in range(n):
                first, cnt = int(rows[s, 5]), int(rows[s, 6])
                want = np.array(back[s][1], dtype=np.uint64).reshape(-1, 5)
                seen = src[first:first + cnt].copy()
                seen[seen[:, 4] >> np.uint64(32) == 1, 2] = 0        # a nil Data has no place: the word is not defined
                assert np.array_equal(seen, want), (s, seen.tolist(), want.tolist())
            assert N.validate(c) == N.OK
            want = N.expected(c)
            names = N.ARRAY_KEYS
            bufs = [RN._up(ctx, np.ascontiguousarray(c[k])) for k in names]
            bufs += [RN._up(ctx, rows), ctx.alloc(n * 48 + 64)]
            empty = ctx.alloc(64)
            bufs.append(empty)

            def call(d_data):
                return RN.node_batch_device(ctx, bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], bufs[5], cl.G, bufs[6],
                                            c["n_ents_total"], ptr, total, empty, 0, empty, 0, empty, 0, empty, 0,
                                            bufs[7], n, bufs[8], d_data, 0, 0)

            def fetch(counters):
                got = {k: np.frombuffer(b.download(c[k].nbytes), dtype=np.uint64).reshape(c[k].shape).copy()
                       for k, b in zip(names, bufs)}
                got["res_rows"] = np.frombuffer(bufs[8].download(n * 48), dtype=np.uint64).reshape(n, 6).copy()
                got.update(zip(("n_data", "n_copied", "n_built"), counters), data=b"")
                return got
            N.assert_parity(c, fetch(call(None)), want, emit=False)      # the size query modifies nothing
            got = fetch(call(d_blob))                                    # d_data is the WAL buffer: nothing to write
            N.assert_parity(c, got, want)
            assert d_blob.download(len(blob)) == blob
            # the array is the ctx's until the next ReadAll: still the same bytes after the call
            L.check(L.lib.ewal_download(ctx.handle, raw, ctypes.c_void_p(ptr), total * 40))
            assert raw.raw == src.tobytes()
        finally:
            RN._free(bufs)
            d_blob.free()
        return got, back


def test_start_crash_restart(ctx):
    cl = NC.NodeCluster(TC.DeviceChecks(ctx), T.DeviceBackend(ctx), C.DeviceWire(ctx))
    NC.play(cl, DeviceHost(ctx))
