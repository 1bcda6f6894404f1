"""Batched Snapshotter.save on the GPU (esnap_save_packed_device, esnap_save_dir;
snap/snapshotter.go:39-60) against the oracle: every file is
snappb_marshal(crc32_update(0, body), body) with body = raftpb.Snapshot.Marshal()
byte for byte, the files are ordered, disjoint and inside cap, and no byte of
the output buffer outside them is written (it is pre-filled with a pattern in
every test)."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from etcd_amd import _lib as L
from etcd_amd import snap as S

import snap_save_cases as K

pytestmark = pytest.mark.gpu

PAT = 0xA5
T = S.SAVE_TILE


class Run:
    """One save_packed call over blob / snaps into a pattern-filled buffer."""

    def __init__(self, ctx, blob, snaps, poly=L.CASTAGNOLI, cap=None):
        self.ctx, self.blob, self.snaps, self.poly = ctx, blob, snaps, poly
        self.cap = S.save_bound(snaps) if cap is None else cap
        self.d = ctx.alloc(max(len(blob), 16))
        if blob:
            self.d.upload(blob)
        self.dout = ctx.alloc(max(self.cap, 16))
        self.dout.upload(bytes([PAT]) * max(self.cap, 16))
        self.res = None

    def save(self):
        self.res = S.save_packed(self.ctx, self.d, len(self.blob), self.snaps, self.dout, self.cap, self.poly)
        return self.res

    def out(self):
        return np.frombuffer(self.dout.download(max(self.cap, 16)), dtype=np.uint8)

    def untouched(self):
        return bool((self.out() == PAT).all())

    def check(self):
        """files == oracle, ordered, disjoint, inside cap; the rest still the pattern"""
        out = self.out()
        covered = np.zeros(len(out), dtype=bool)
        end = 0
        for i, (s, (off, ln, crc)) in enumerate(zip(self.snaps, self.res)):
            want, wcrc = K.expected(s, self.blob, self.poly)
            assert off >= end and off + ln <= self.cap, (i, off, ln, end, self.cap)
            assert ln == len(want) and crc == wcrc, (i, s["data_len"], s["data_off"] % 16, ln, len(want), crc, wcrc)
            assert out[off:off + ln].tobytes() == want, (i, s["data_len"], s["data_off"] % 16)
            covered[off:off + ln] = True
            end = off + ln
        assert (out[~covered] == PAT).all(), "bytes outside the files were written"

    def free(self):
        self.d.free()
        self.dout.free()


@pytest.fixture(scope="module")
def lat(ctx):
    blob, snaps = K.lattice(T)
    r = Run(ctx, blob, snaps)
    r.save()
    yield r
    r.free()


def test_reference_kat(ctx):
    k = K.reference_snap()
    blob, snaps = K.pack([(k["data"], 0)])
    snaps[0].update(nodes=k["nodes"], index=k["index"], term=k["term"], removed=[])
    r = Run(ctx, blob, snaps)
    (off, ln, crc), = r.save()
    r.check()
    body = O.snapshot_marshal(b"some snapshot", [1, 2, 3], 1, 1, [])
    assert r.out()[off:off + ln].tobytes() == O.snappb_marshal(O.crc32_update(0, body), body)
    assert S.snap_name(k["term"], k["index"]) == "0000000000000001-0000000000000001.snap"
    r.free()


def test_length_alignment_lattice(lat):
    assert len(lat.snaps) == 16 * 6
    assert sorted({s["data_off"] % 16 for s in lat.snaps}) == list(K.ALIGNS)
    lat.check()


def test_crc_varint_widths(ctx):
    cases = json.load(open(os.path.join(K.GOLDEN, "snap_save_crc_widths.json")))["cases"]
    assert sorted(c["width"] for c in cases)[-5:] == [1, 2, 3, 4, 5]
    datas = [(bytes.fromhex(c["data_hex"]), 3) for c in cases]
    blob, snaps = K.pack(datas)
    for s, c in zip(snaps, cases):
        s.update(index=c["index"], term=c["term"], nodes=[], removed=[])
        _, crc = K.expected(s, blob)
        width = len(S._varint(crc))
        assert crc == c["crc"] and width == (c["width"] or 1) and (c["width"] != 0 or crc == 0), (c, crc)
    r = Run(ctx, blob, snaps)
    r.save()
    r.check()
    r.free()


def test_varint_magnitudes_and_counts(ctx):
    V = [0, 127, 128, 1 << 32, 1 << 63, (1 << 64) - 1]
    big = [1, 1 << 32, (1 << 64) - 1]
    datas, fields = [], []
    k = 0
    for cn in (0, 1, 70):
        for cr in (0, 1, 70):
            for j in range(3):
                datas.append((bytes([k & 255]) * (k % 40), (5 * k) % 16))
                fields.append(dict(nodes=[V[(k + q) % 6] for q in range(cn)], removed=[V[(2 * k + q) % 6] for q in range(cr)],
                                   index=big[j], term=big[(j + k) % 3], unrec=b"\x38\x01" if k % 2 else b""))
                k += 1
    blob, snaps = K.pack(datas)
    for s, f in zip(snaps, fields):
        s.update(f)
    r = Run(ctx, blob, snaps)
    r.save()
    r.check()
    r.free()


def test_several_tiles_per_snapshot(ctx):
    rng = np.random.default_rng(5)
    blob = bytes(5) + rng.integers(0, 256, (8 << 20) + 1, dtype=np.uint8).tobytes()
    blob += bytes(-len(blob) % 16)
    o2 = len(blob)
    blob += rng.integers(0, 256, 3 * T + 7, dtype=np.uint8).tobytes()
    snaps = [dict(data_off=5, data_len=(8 << 20) + 1, index=9, term=2, nodes=[1]),
             dict(data_off=o2, data_len=3 * T + 7, index=10, term=2)]
    r = Run(ctx, blob, snaps)
    r.save()
    r.check()
    r.free()


def test_round_trip_through_verify(ctx):
    rng = np.random.default_rng(6)
    datas = [(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), al)
             for n, al in ((0, 0), (13, 1), (4096, 15), (T + 1, 4), (100, 8))]
    blob, snaps = K.pack(datas)
    snaps[1].update(unrec=b"\x38\x01")
    snaps[3].update(nodes=list(range(70)), removed=[1 << 63])
    r = Run(ctx, blob, snaps)
    res = r.save()
    offs, lens = [x[0] for x in res], [x[1] for x in res]
    st, sc, cc = S.verify_packed(r.dout, r.cap, offs, lens)
    assert st == [L.OK] * len(snaps)
    assert sc == cc == [x[2] for x in res]
    for i, s in enumerate(snaps):
        got = S.snapshot(ctx, i)
        data = blob[s["data_off"]:s["data_off"] + s["data_len"]]
        assert (got["data"] or b"") == data, i
        assert got["nodes"] == list(s["nodes"]) and got["removed"] == list(s["removed"]), i
        assert (got["index"], got["term"]) == (s["index"], s["term"]), i
        assert (got["unrec"] or b"") == (s.get("unrec") or b""), i
    # one flipped byte inside file 2's Data: only that file fails
    body = K.body(snaps[2], blob)
    pos = offs[2] + lens[2] - len(body) + 2 + 1 + 100   # 0a v(4096) is 3 bytes
    b = r.dout.download(1, pos)
    r.dout.upload(bytes([b[0] ^ 0x40]), pos)
    st, _, _ = S.verify_packed(r.dout, r.cap, offs, lens)
    assert st == [L.OK, L.OK, L.ERR_SNAP_CRC, L.OK, L.OK]
    r.free()


def test_koopman(ctx):
    rng = np.random.default_rng(8)
    blob, snaps = K.pack([(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), al)
                          for n, al in ((13, 0), (5000, 3), (T + 17, 9))])
    r = Run(ctx, blob, snaps, poly=L.KOOPMAN)
    res = r.save()
    r.check()
    assert [x[2] for x in res] != [K.expected(s, blob)[1] for s in snaps]
    r.free()


def test_errors(ctx):
    blob = bytes(range(64))
    one = [dict(data_off=3, data_len=20, index=1, term=1)]

    def status(snaps, cap=None, data_len=len(blob)):
        r = Run(ctx, blob, snaps, cap=cap)
        with pytest.raises(L.EwalError) as e:
            S.save_packed(ctx, r.d, data_len, snaps, r.dout, r.cap)
        assert r.untouched()
        r.free()
        return e.value.status

    assert status(one, cap=0) == L.E_NOMEM
    assert status([dict(data_off=60, data_len=5, index=1, term=1)], cap=256) == L.E_INVAL
    assert status([dict(data_off=(1 << 64) - 8, data_len=16, index=1, term=1)], cap=256) == L.E_INVAL
    r = Run(ctx, blob, [], cap=64)
    assert r.save() == [] and r.untouched()
    r.free()
    r = Run(ctx, blob, one)
    assert r.cap == S.save_bound(one)
    r.save()
    r.check()
    r.free()
    # a base pointer off the 16-byte grid, d_out inside d_data
    r = Run(ctx, blob, one)
    recs, u64, unrec = S._save_args(one)
    out = (L.SnapSaved * 1)()
    import ctypes as C
    call = L.lib.esnap_save_packed_device
    assert call(ctx.handle, C.c_void_p(r.d.ptr.value + 4), 32, recs, 1, u64, unrec, L.CASTAGNOLI, r.dout.ptr, r.cap,
                out) == L.E_INVAL
    assert call(ctx.handle, r.d.ptr, len(blob), recs, 1, u64, unrec, L.CASTAGNOLI, C.c_void_p(r.dout.ptr.value + 8),
                r.cap - 8, out) == L.E_INVAL
    assert call(ctx.handle, r.d.ptr, len(blob), recs, 1, u64, unrec, L.CASTAGNOLI, C.c_void_p(r.d.ptr.value + 32), 32,
                out) == L.E_INVAL
    assert r.untouched()
    r.free()


def test_call_history(ctx, lat):
    first = list(lat.res)
    bytes1 = lat.out().tobytes()
    blob, snaps = K.pack([(b"tiny", 7)])
    r = Run(ctx, blob, snaps)
    r.save()
    r.check()
    r.free()
    lat.dout.upload(bytes([PAT]) * lat.cap)
    assert lat.save() == first
    assert lat.out().tobytes() == bytes1
    lat.check()


def test_save_dir(ctx, tmp_path):
    rng = np.random.default_rng(10)
    blob = bytes(3) + rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    d = ctx.alloc(len(blob))
    d.upload(blob)
    s1 = dict(data_off=3, data_len=70000, index=1, term=1, nodes=[1, 2, 3])
    name = S.save_dir(ctx, str(tmp_path), d, len(blob), s1)
    assert name == S.snap_name(1, 1) == "0000000000000001-0000000000000001.snap"
    assert (tmp_path / name).read_bytes() == K.expected(s1, blob)[0]
    assert S.save_dir(ctx, str(tmp_path), d, len(blob), dict(s1, index=0)) is None
    assert sorted(os.listdir(tmp_path)) == [name]
    s2 = dict(data_off=100, data_len=50, index=5, term=2)
    name2 = S.save_dir(ctx, str(tmp_path), d, len(blob), s2)
    assert (tmp_path / name2).read_bytes() == K.expected(s2, blob)[0]
    # an existing file is truncated (ioutil.WriteFile)
    assert S.save_dir(ctx, str(tmp_path), d, len(blob), dict(s1, data_len=10)) == name
    assert (tmp_path / name).read_bytes() == K.expected(dict(s1, data_len=10), blob)[0]
    loaded, snap = S.load_dir(ctx, str(tmp_path))
    assert loaded == name2 and (snap.index, snap.term) == (5, 2)
    assert S.copy_field(ctx, 0, L.SNAP_FIELD_DATA) == blob[100:150]
    d.free()
