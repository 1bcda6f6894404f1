"""Edge-lattice parity of the entry points beside the WAL replay path:
ewal_crc32_update_device, esnap_verify_packed, ecommit_batch_device,
ecommit_batch_rec_device, ewal_save_device and ewal_encode_entries_device
against the oracle, bit-exact, at the lengths, residues, magnitudes and
alignments where their kernels change path (the lattices and what they cover:
tests/test_aux_edge_generators.py)."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

from oracle import oracle as O
from etcd_amd import _lib as L
from etcd_amd import raftcommit as RC
from etcd_amd import snap as S
from etcd_amd import wal as W

import test_aux_edge_generators as GEN
from test_gpu_parity import _oracle_save

pytestmark = pytest.mark.gpu

MiB = 1 << 20


# ---------------------------------------------------------------------------
# 1. ewal_crc32_update_device
# ---------------------------------------------------------------------------
def _crc(ctx, addr, n, poly=L.CASTAGNOLI, seed=0):
    out = C.c_uint32(0xA5A5A5A5)
    rc = L.lib.ewal_crc32_update_device(ctx.handle, seed, poly, C.c_void_p(addr), n, C.byref(out))
    assert rc == 0, (rc, n)
    return out.value


def _no_mismatch(bad):
    assert not bad, "%d mismatches, first (n, got, want): %s" % (len(bad), [(n, hex(g), hex(w)) for n, g, w in bad[:8]])


@pytest.fixture(scope="module")
def pool(ctx):
    """The one random pool, on the host and (with the usual 64 B of slack) on the device."""
    P = GEN.make_pool()
    d = ctx.alloc(len(P) + 64)
    d.upload_ptr(P.ctypes.data, len(P))
    yield P, d
    d.free()


@pytest.fixture(scope="module")
def pool_crcs(pool):
    """crc32.Update(0, Castagnoli, P[:n]) for every length of (b)-(e): one oracle pass over the pool."""
    return GEN.crc_chain(pool[0], GEN.lengths_order())


def test_crc_every_small_length(ctx, pool):
    """(a) every n in 0 .. 2 * 4096 + 512: each count of whole super-pieces
    with each dword / byte tail of prefix_at, one to three units."""
    P, d = pool
    lens = GEN.lengths_small()
    head = P[:lens[-1]].tobytes()
    want = GEN.crc_chain(P, lens, L.CASTAGNOLI)
    _no_mismatch([(n, g, want[n]) for n in lens for g in [_crc(ctx, d.ptr.value, n)] if g != want[n]])
    seeded = lens[::7]
    _no_mismatch([(n, g, w) for n in seeded
                  for g, w in [(_crc(ctx, d.ptr.value, n, seed=0xFFFFFFFF), O.crc32_update(0xFFFFFFFF, head[:n]))]
                  if g != w])
    for poly in (L.KOOPMAN, L.IEEE):
        some = sorted(set(lens[::5]) | set(range(301)))
        want = GEN.crc_chain(P, some, poly)
        _no_mismatch([(n, g, want[n]) for n in some for g in [_crc(ctx, d.ptr.value, n, poly)] if g != want[n]])
        if poly == L.IEEE:
            assert all(want[n] == zlib.crc32(head[:n]) for n in some)


def test_crc_stream_and_scan_edges(ctx, pool, pool_crcs):
    """(b) + (c): lengths around pairs of units, a scan lane's 4 units, a
    workgroup's 24, 1 MiB tiles, 16-tile groups, and the nsafe switch."""
    _, d = pool
    lens = GEN.lengths_edges() + GEN.lengths_nsafe()
    _no_mismatch([(n, g, pool_crcs[n]) for n in lens for g in [_crc(ctx, d.ptr.value, n)] if g != pool_crcs[n]])


def test_crc_large_lengths_and_call_order(ctx, pool, pool_crcs):
    """(d) + (e): one to four pairs per wave through the three-buffer loop,
    then every length of (b)-(d) in a shuffled order and a shrink / grow
    sequence on the one ctx: no call sees an earlier call's v[] / pwave[]."""
    P, d = pool
    large = GEN.lengths_large()
    _no_mismatch([(n, g, pool_crcs[n]) for n in large for g in [_crc(ctx, d.ptr.value, n)] if g != pool_crcs[n]])
    for n, seed in ((large[4], 0x9E3779B9), (large[-1], 0x7F4A7C15)):
        assert _crc(ctx, d.ptr.value, n, seed=seed) == O.crc32_update(seed, P[:n].tobytes()), n
    order = GEN.lengths_order()
    got = [_crc(ctx, d.ptr.value, n) for n in order]
    bad = [(k, n, hex(g), hex(pool_crcs[n])) for k, (n, g) in enumerate(zip(order, got)) if g != pool_crcs[n]]
    assert not bad, "(call, n, got, want): %s" % bad[:8]


def test_crc_base_pointer_and_alignment(ctx, pool):
    """(f) the stream may start at any 16-byte aligned address; (g) any other
    address is refused before anything is launched."""
    P, d = pool
    bad = []
    for off, n in GEN.base_offsets():
        g, w = _crc(ctx, d.ptr.value + off, n), O.crc32_update(0, P[off:off + n].tobytes())
        if g != w:
            bad.append((off, n, hex(g), hex(w)))
    assert not bad, bad[:8]
    out = C.c_uint32(0)
    for mis in (1, 8):
        assert L.lib.ewal_crc32_update_device(ctx.handle, 0, L.CASTAGNOLI, C.c_void_p(d.ptr.value + mis), 64,
                                              C.byref(out)) == L.E_INVAL
        st = (C.c_int32 * 1)()
        assert L.lib.esnap_verify_packed(ctx.handle, C.c_void_p(d.ptr.value + mis), 64, (C.c_uint64 * 1)(0),
                                         (C.c_uint64 * 1)(64), 1, L.CASTAGNOLI, st, None, None) == L.E_INVAL


# ---------------------------------------------------------------------------
# 2. esnap_verify_packed
# ---------------------------------------------------------------------------
def _verify_snaps(ctx, d, sp, buf, poly, fields):
    """esnap_verify_packed over sp's files as they stand in buf (uploaded to
    d) against O.loadsnap per file; returns (status, stored, computed)."""
    buf = bytes(buf)
    d.upload(buf)
    st, sc, cc = S.verify_packed(d, len(buf), sp.offs, sp.lens, poly)
    for i in range(len(sp.offs)):
        o = O.loadsnap(sp.file(i, buf), poly)
        assert st[i] == o["status"], (i, sp.pairs[i], st[i], o["status"])
        if o["status"] in (O.OK, O.ERR_SNAP_CRC):
            assert (sc[i], cc[i]) == (o["stored_crc"], o["computed_crc"]), (i, sp.pairs[i])
        if fields and o["status"] == O.OK:
            s = L.SnapshotDesc()
            assert L.lib.esnap_copy_snapshot(ctx.handle, i, C.byref(s)) == 0
            assert (s.index, s.term, list(s.nodes[:s.n_nodes])) == (o["snap"]["index"], o["snap"]["term"],
                                                                    o["snap"]["nodes"]), (i, sp.pairs[i])
            got = buf[s.data_off:s.data_off + s.data_len] if s.data_len else None
            assert got == o["snap"]["data"], (i, sp.pairs[i])
    return st, sc, cc


@pytest.mark.parametrize("poly", GEN.POLYS, ids=["castagnoli", "koopman", "ieee"])
def test_snapshot_residue_lattice(ctx, poly):
    """One valid file per (Data start, Data end) residue pair mod 256, an
    empty and a 1-byte Data and a Data ending on the buffer's last byte; one
    flipped byte at either end of Data and just outside the file; the same
    buffer again after a smaller batch."""
    sp = GEN.build_snap_lattice(poly)
    d = ctx.alloc(len(sp.buf) + 64)
    small = GEN.small_snap_batch(poly)
    d2 = ctx.alloc(len(small.buf) + 64)
    try:
        clean = _verify_snaps(ctx, d, sp, sp.buf, poly, True)
        assert clean[0][:sp.n_lattice] == [O.OK] * sp.n_lattice
        for kind in GEN.SNAP_DAMAGE:
            res = _verify_snaps(ctx, d, sp, GEN.damage_snap_lattice(sp, kind), poly, False)
            if kind.startswith("pad"):
                assert res == clean, kind
            else:
                assert all(res[0][i] != O.OK for i in range(0, sp.n_lattice, 5)), kind
        _verify_snaps(ctx, d2, small, small.buf, poly, True)
        assert _verify_snaps(ctx, d, sp, sp.buf, poly, True) == clean
    finally:
        d.free()
        d2.free()


# ---------------------------------------------------------------------------
# 3. ecommit_batch_device / ecommit_batch_rec_device
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _soa():
    g = GEN.soa_groups()
    return g, GEN.commit_expect(g)


@functools.lru_cache(maxsize=None)
def _rec():
    g = GEN.rec_groups()
    return g, GEN.commit_expect(g)


def _dev(ctx, arr):
    a = np.ascontiguousarray(arr)
    b = ctx.alloc(a.nbytes + 64)
    if a.nbytes:
        b.upload_ptr(a.ctypes.data, a.nbytes)
    return b


def _triples(c, chg, st):
    return list(zip(c.tolist(), chg.tolist(), st.tolist()))


@pytest.mark.parametrize("G", GEN.SOA_G)
def test_commit_soa_uint64_magnitudes(ctx, G):
    """k_commit and the three quorum selects over Match / committed / offset /
    term values that differ only above bit 31, at the block, grid and
    per-lane group-count edges."""
    groups, expect = _soa()
    match, nv, term, comm, off, ptr, lt = GEN.soa_arrays(groups[:G])
    bufs = [_dev(ctx, x) for x in (match, nv, term, comm, off, ptr, lt)]
    dch, dst = ctx.alloc(G + 64), ctx.alloc(G + 64)
    try:
        assert L.lib.ecommit_batch_device(ctx.handle, G, *[b.ptr for b in bufs], dch.ptr, dst.ptr, None) == 0
        got = _triples(np.frombuffer(bufs[3].download(8 * G), np.uint64), np.frombuffer(dch.download(G), np.uint8),
                       np.frombuffer(dst.download(G), np.uint8))
    finally:
        for b in bufs + [dch, dst]:
            b.free()
    bad = [(g, groups[g], got[g], expect[g]) for g in range(G) if got[g] != expect[g]]
    assert not bad, "%d groups differ, first: %s" % (len(bad), bad[:3])


def _commit_rec(ctx, arrs, with_log=True):
    match, nv, term, comm, off, ptr, lt = arrs
    G = len(nv)
    rec = RC.pack_groups(match, nv, comm, term, off, ptr, lt)
    bufs = [_dev(ctx, rec), _dev(ctx, ptr), _dev(ctx, lt), ctx.alloc(8 * G + 64), ctx.alloc(G + 64), ctx.alloc(G + 64)]
    try:
        assert L.lib.ecommit_batch_rec_device(ctx.handle, G, bufs[0].ptr, bufs[1].ptr if with_log else None,
                                              bufs[2].ptr if with_log else None, bufs[3].ptr, bufs[4].ptr,
                                              bufs[5].ptr, None) == 0
        return (np.frombuffer(bufs[3].download(8 * G), np.uint64), np.frombuffer(bufs[4].download(G), np.uint8),
                np.frombuffer(bufs[5].download(G), np.uint8))
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("G", GEN.REC_G + (GEN.N_REC,))
def test_commit_records_uint64_magnitudes(ctx, G):
    """k_commit_rec over the same magnitudes at the 64-record chunk edges."""
    groups, expect = _rec()
    got = _triples(*_commit_rec(ctx, GEN.soa_arrays(groups[:G])))
    bad = [(g, groups[g], got[g], expect[g]) for g in range(G) if got[g] != expect[g]]
    assert not bad, "%d groups differ, first: %s" % (len(bad), bad[:3])


def test_commit_records_without_log(ctx):
    """log_ptr / log_terms NULL: a group whose quorum index's term lies before
    the 13-term window is reported, every other group is decided as before."""
    groups, expect = _rec()
    got = _triples(*_commit_rec(ctx, GEN.soa_arrays(groups), with_log=False))
    want = [(g[4], 0, L.UNSUPPORTED_ENCODING) if GEN.before_window(g) else e for g, e in zip(groups, expect)]
    assert sum(w[2] == L.UNSUPPORTED_ENCODING for w in want) >= 20
    bad = [(i, groups[i], got[i], want[i]) for i in range(len(groups)) if got[i] != want[i]]
    assert not bad, "%d groups differ, first: %s" % (len(bad), bad[:3])


def test_commit_records_second_round(ctx):
    """More 64-record chunks than the persistent grid has waves: the chunks a
    wave takes after its first carry the same magnitudes."""
    groups, _ = _rec()
    big = GEN.tile_soa(GEN.soa_arrays(groups), GEN.REC_G_BIG)
    c, chg, st = _commit_rec(ctx, big)
    wc, wchg, wst = GEN.batch_expect(big)
    bad = np.nonzero((c != wc) | (chg != wchg) | (st != wst))[0]
    assert bad.size == 0, (bad.size, [(int(g), int(c[g]), int(wc[g]), int(chg[g]), int(wchg[g]), int(st[g]),
                                      int(wst[g])) for g in bad[:5]])


# ---------------------------------------------------------------------------
# 4. write path
# ---------------------------------------------------------------------------
def _ops(seq):
    return [(k, W.Entry(*v) if k == "entry" else W.HardState(*v) if k == "state" else v) for k, v in seq]


def test_save_first_chunk_shorter_than_a_dword(ctx):
    """ewal_save_device when the data-only stream's first chunk is 1, 2, 3, 4
    or 5 bytes and more follows: the chained CRCs at x < 4 and after."""
    for seq in GEN.save_sequences():
        ops = _ops(seq)
        for prev in GEN.SAVE_PREVS:
            assert W.save_device(ctx, ops, prev) == _oracle_save(ops, prev), (seq[0], [k for k, _ in seq], hex(prev))


def test_encode_entries_copy_alignments(ctx):
    """ewal_encode_entries_device with hand-set data_off: every source and
    destination alignment of wave_copy, and entries whose Data ends exactly at
    the end of a source that is not a whole number of dwords."""
    blob = np.random.default_rng(3).integers(0, 256, GEN.ENC_BLOB, dtype=np.uint8).tobytes()
    dd = ctx.alloc(GEN.ENC_BLOB + 64)
    dd.upload(blob)
    try:
        for total, prev in zip(GEN.ENC_TOTALS, (0, 0xDEADBEEF, 1, 0xFFFFFFFF)):
            cases = GEN.encode_cases(total)
            n = len(cases)
            arr = (L.EntryDesc * n)()
            e = O.WalEncoder(prev)
            for a, (ty, term, idx, off, ln) in zip(arr, cases):
                a.type, a.term, a.index, a.data_off, a.data_len = ty, term, idx, off, ln
                e.save_entry(ty, term, idx, blob[off:off + ln])
            cap = sum(c[4] for c in cases) + 80 * n + 64
            de, do = ctx.alloc(C.sizeof(arr) + 64), ctx.alloc(cap + 64)
            try:
                de.upload(bytes(arr))
                out_len, crc = C.c_uint64(), C.c_uint32()
                assert L.lib.ewal_encode_entries_device(ctx.handle, dd.ptr, total, de.ptr, n, prev, do.ptr, cap,
                                                        C.byref(out_len), C.byref(crc)) == 0
                got = do.download(out_len.value)
            finally:
                de.free()
                do.free()
            want = e.getvalue()
            assert len(got) == len(want), total
            if got != want:
                first = next(i for i in range(len(want)) if got[i] != want[i])
                pytest.fail("data_len_total %d: frames differ first at byte %d of %d" % (total, first, len(want)))
            assert crc.value == e.crc, total
    finally:
        dd.free()


def _both_entry_points(ctx, ents, prev):
    """ents through ewal_encode_entries_device and, as entry ops, through
    ewal_save_device: both against the reference writer."""
    ops = [("entry", W.Entry(*e)) for e in ents]
    want, wcrc, woffs = _oracle_save(ops, prev)
    got, crc = W.encode_entries_device(ctx, [x for _, x in ops], prev)
    assert (len(got), crc) == (len(want), wcrc) and got == want, ("encode", len(ents), hex(prev))
    got, crc, offs = W.save_device(ctx, ops, prev)
    assert (len(got), crc) == (len(want), wcrc) and got == want, ("save", len(ents), hex(prev))
    assert offs == woffs, ("save", len(ents), hex(prev))      # the running sum of the reference's frame sizes


def test_write_entry_points_agree_at_varint_widths(ctx):
    """Every Term / Index varint width, Type 0 / 1 / -1 and Data of None, 0 and
    the 1 / 2 / 3-byte length boundaries, at record counts around a wave and a
    block: one pipeline behind both entry points."""
    blob = GEN._wire_blob()
    for n in GEN.WIRE_N:
        ents = GEN.wire_entries(n, blob)
        for prev in GEN.SAVE_PREVS:
            _both_entry_points(ctx, ents, prev)


def test_write_grid_stride_second_trip(ctx):
    """More records than one trip of the wave-per-record grid of k_wr_body /
    k_wr_frame (4 waves x 8 workgroups x CUs)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ents = GEN.stride_entries(cus)
    assert len(ents) > 4 * 8 * cus
    _both_entry_points(ctx, ents, 0x9E3779B1)


def test_save_empty_data_stream(ctx):
    """E == 0: nothing but empty HardStates and nil-metadata Cuts -- no stream
    pass, and the crcType / metadataType frames carry the running CRC."""
    for seq in GEN.empty_stream_sequences():
        ops = _ops(seq)
        for prev in GEN.SAVE_PREVS:
            assert W.save_device(ctx, ops, prev) == _oracle_save(ops, prev), ([k for k, _ in seq], hex(prev))


def _raw_write(ctx, arr, n, payload, total, cap, prev=0x01234567):
    """One raw call (ewal_save_device for SaveRec records, else
    ewal_encode_entries_device) with d_out pre-filled with 0xA5: (status,
    d_out's cap bytes, out_len, last_crc)."""
    dd, dr, do = ctx.alloc(len(payload) + 64), ctx.alloc(C.sizeof(arr) + 64), ctx.alloc(cap + 64)
    try:
        dd.upload(payload)
        dr.upload(bytes(arr))
        do.upload(b"\xa5" * cap)
        out_len, crc = C.c_uint64(77), C.c_uint32(77)
        args = (ctx.handle, dd.ptr, total, dr.ptr, n, prev, do.ptr, cap, C.byref(out_len), C.byref(crc))
        rc = L.lib.ewal_save_device(*args, None) if isinstance(arr[0], L.SaveRec) else \
            L.lib.ewal_encode_entries_device(*args)
        return rc, do.download(cap), out_len.value, crc.value
    finally:
        for b in (dd, dr, do):
            b.free()


def _recs(kind, ranges):
    """Entries (Term 3, Index i + 1) over the (data_off, data_len) ranges, as
    ewal_entry (kind "encode") or as ewal_save_rec entry records."""
    arr = ((L.EntryDesc if kind == "encode" else L.SaveRec) * len(ranges))()
    for i, (a, (off, ln)) in enumerate(zip(arr, ranges)):
        a.data_off, a.data_len = off, ln
        if kind == "encode":
            a.term, a.index = 3, i + 1
        else:
            a.kind, a.a, a.b = L.SAVE_ENTRY, 3, i + 1
    return arr


@pytest.mark.parametrize("kind", ["encode", "save"])
def test_write_errors_leave_the_output_untouched(ctx, kind):
    """A payload one byte past d_data, an empty payload at data_len_total + 1
    and a cap one byte short: the status, and not a byte of d_out written."""
    prev, total = 0x01234567, 100
    payload = bytes(range(total))
    good = [(0, 10), (10, 0), (10, 90)]
    e = O.WalEncoder(prev)
    for i, (off, ln) in enumerate(good):
        e.save_entry(0, 3, i + 1, payload[off:off + ln])
    want = e.getvalue()
    cap = len(want)
    assert _raw_write(ctx, _recs(kind, good), 3, payload, total, cap, prev) == (0, want, cap, e.crc)
    for name, rng in GEN.write_error_ranges(total).items():
        for pos in (0, 1, 2):                                  # the record out of range: first, middle, last
            ranges = good[:pos] + [rng] + good[pos + 1:]
            assert _raw_write(ctx, _recs(kind, ranges), 3, payload, total, cap, prev) == \
                (L.E_INVAL, b"\xa5" * cap, 0, prev), (name, pos)
    assert _raw_write(ctx, _recs(kind, good), 3, payload, total, cap - 1, prev) == \
        (L.E_NOMEM, b"\xa5" * (cap - 1), 0, prev)


def test_save_unknown_kind_and_unread_ranges(ctx):
    """An unknown kind is EWAL_E_INVAL; the data range of a HardState and of a
    nil-metadata Cut is never read, so a wild one is not an error."""
    prev, total = 0x9E3779B1, 16
    payload = bytes(range(total))
    arr = _recs("save", [(0, 4), (4, 12)])
    arr[1].kind = 7
    assert _raw_write(ctx, arr, 2, payload, total, 256, prev) == (L.E_INVAL, b"\xa5" * 256, 0, prev)
    arr = (L.SaveRec * 3)()
    arr[0].kind, arr[0].a, arr[0].b, arr[0].c = L.SAVE_STATE, 4, 2, 1 << 40
    arr[1].kind, arr[1].data_nil = L.SAVE_CUT, 1
    arr[2].kind, arr[2].a, arr[2].b, arr[2].data_off, arr[2].data_len = L.SAVE_ENTRY, 3, 1, 0, total
    for a in arr[:2]:
        a.data_off, a.data_len = (1 << 63) + 5, (1 << 62) + 1
    ops = [("state", W.HardState(4, 2, 1 << 40)), ("cut", None), ("entry", W.Entry(0, 3, 1, payload))]
    want, wcrc, _ = _oracle_save(ops, prev)
    rc, out, out_len, crc = _raw_write(ctx, arr, 3, payload, total, 256, prev)
    assert (rc, out_len, crc) == (0, len(want), wcrc) and out == want + b"\xa5" * (256 - len(want))
