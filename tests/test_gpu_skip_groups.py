"""proto.Skip's group frames at the other sites of the device walker pb_skip:
the WAL decode (a walpb.Record, a raftpb.Entry and a HardState with unknown
groups, in the middle of a WAL; single, and as a shard of the batch, which
replays such a shard on its own) and the snapshot verify (a snappb.Snapshot
envelope and the raftpb.Snapshot inside it).

Nesting up to the walker's boundary is exact -- status, ents, every
XXX_unrecognized, the CRC chain.  One past it Go still accepts the bytes and
the device says EWAL_UNSUPPORTED_ENCODING, in the way include/ewal.h words it
for each call.  The boundary counts pushes on pb_skip's frame stack
(msg_decode_cases.MAX_PUSHES = PB_SKIP_DEPTH; that many pushes are
MAX_NESTED_STARTS = PB_SKIP_DEPTH + 1 start-group tags nested).  The group
shapes are family (f)'s of tests/msg_decode_cases.py.
"""
import random
import struct

import pytest

import msg_decode_cases as K
from oracle import oracle as O
from etcd_amd import _lib as L
from etcd_amd import snap as S
from etcd_amd import wal as W
from test_gpu_framing import MixedWal, nc_record
from test_gpu_parity import assert_parity, build_wal

pytestmark = pytest.mark.gpu

# Field 11 is unknown to every message here.  Each simple wire type inside a
# group; empty; nested to the boundary; siblings that pop and push again.
EXACT = [
    ("holds", K.group(K.fv(12, 300) + K.tag(13, 1) + b"\x01" * 8 + K.fb(14, b"pq") + K.tag(15, 5) + b"\x05" * 4)),
    ("empty", K.group()),
    ("end-only", K.tag(11, 4)),
    ("known-inside", K.group(K.fv(1, 99) + K.fb(2, b"zz") + K.fv(3, 7))),
    ("nest2", K.group(K.fv(12, 2), depth=2)),
    ("boundary", K.group(K.fv(12, 9), depth=K.MAX_NESTED_STARTS)),
    ("siblings", K.group(K.group(depth=K.MAX_PUSHES) * 2 + K.fv(12, 7))),
]
PAST = K.group(K.fv(12, 9), depth=K.MAX_NESTED_STARTS + 1)
SITES = ("record", "entry", "state")


class GroupWal(MixedWal):
    """A WAL whose frames can carry extra bytes after the Record's, the
    Entry's or the HardState's own fields."""

    def __init__(self):
        super().__init__()
        self.offsets = []
        self.index = 0
        self.canonical(4, None)
        self.canonical(1, b"metadata")
        self.plain()

    def canonical(self, type_, data):
        self.offsets.append(len(self.buf))
        super().canonical(type_, data)

    def plain(self):
        self.canonical(2, O.entry_marshal(0, 1, self.index, b"entry %d" % self.index))
        self.index += 1

    def put(self, site, extra):
        if site == "record":   # after the Record's fields: the record's chained CRC covers Data alone
            data = O.entry_marshal(0, 1, self.index, b"in a record with a group")
            self.crc = O.crc32_update(self.crc, data)
            body = nc_record(2, self.crc, data, "crc_first") + extra
            self.offsets.append(len(self.buf))
            self.buf += struct.pack("<q", len(body)) + body
            self.index += 1
        elif site == "entry":
            self.canonical(2, O.entry_marshal(1, 1, self.index, b"with a group") + extra)
            self.index += 1
        else:
            self.canonical(3, O.hardstate_marshal(1, 2, self.index - 1) + extra)
        self.plain()


def exact_wal():
    m = GroupWal()
    for site in SITES:
        for _, g in EXACT:
            m.put(site, g)
    return m


def same_as_oracle(o, g):
    assert g["status"] == o["status"] == O.OK
    for k in ("n_records", "last_crc", "enti", "metadata", "state", "ents"):
        assert g[k] == o[k], k


def test_groups_mid_wal_are_exact(ctx):
    m = exact_wal()
    o, g = assert_parity(ctx, m.buf, 0)   # status, ents with XXX_unrecognized, state, every chained CRC and offset
    assert o["status"] == O.OK and g["n_records"] == len(m.offsets)
    unrec = [e["unrec"] for e in g["ents"] if e["type"] == 1]
    assert unrec == [x for _, x in EXACT]                         # the Entry's own unknown groups, byte for byte
    assert g["state"]["unrec"] == EXACT[-1][1]                    # the last HardState wins, with its group
    # each site alone, so that no frame leans on a neighbour's decode
    for site in SITES:
        for name, x in EXACT:
            w = GroupWal()
            w.put(site, x)
            o, g = assert_parity(ctx, w.buf, 0)
            assert o["status"] == O.OK, (site, name)


def test_groups_in_a_batch_shard_are_exact(ctx):
    m = exact_wal()
    other = build_wal(random.Random(5), 5, 10, big_terms=False)
    r = W.readall_batch_bytes([other, bytes(m.buf), other], [0, 0, 0], ctx)
    same_as_oracle(O.readall(bytes(m.buf), 0), r[1].as_dict())
    assert r[1].flags & L.FLAG_SHARD_FALLBACK
    for k in (0, 2):
        same_as_oracle(O.readall(other, 0), r[k].as_dict())
        assert not r[k].flags & L.FLAG_SHARD_FALLBACK


@pytest.mark.parametrize("site", SITES)
def test_one_past_the_boundary_in_a_wal(ctx, site):
    """Go accepts the frame; ReadAll on the device stops at it with
    EWAL_UNSUPPORTED_ENCODING, fail_record / fail_offset naming the frame,
    as for a frame that failed.  In a batch only that shard stops."""
    m = GroupWal()
    m.put("entry", EXACT[0][1])
    k = len(m.offsets)
    m.put(site, PAST)
    buf = bytes(m.buf)
    o = O.readall(buf, 0)
    assert o["status"] == O.OK and o["n_records"] == len(m.offsets)
    g = W.readall_bytes(buf, 0, ctx).as_dict()
    assert (g["status"], g["fail_record"], g["fail_offset"]) == (L.UNSUPPORTED_ENCODING, k, m.offsets[k])
    other = build_wal(random.Random(6), 5, 10, big_terms=False)
    r = W.readall_batch_bytes([other, buf], [0, 0], ctx)
    assert (r[1].status, r[1].fail_record, r[1].fail_offset) == (L.UNSUPPORTED_ENCODING, k, m.offsets[k])
    same_as_oracle(O.readall(other, 0), r[0].as_dict())
    # the same frame with one group level fewer is exact again
    w = GroupWal()
    w.put("entry", EXACT[0][1])
    w.put(site, K.group(K.fv(12, 9), depth=K.MAX_NESTED_STARTS))
    assert_parity(ctx, w.buf, 0)


def snap_file(inner_extra=b"", outer_extra=b"", split=False):
    body = O.snapshot_marshal(b"snapshot data", [1, 2, 3], 7, 2, removed=[9]) + inner_extra
    crc = O.crc32_update(0, body)
    if split:   # the envelope's Data in two segments with the group between them: pb_each steps over it
        cut = len(body) // 2
        return O.snappb_marshal(crc, body[:cut]) + outer_extra + b"\x12" + K.vint(len(body) - cut) + body[cut:]
    return O.snappb_marshal(crc, body) + outer_extra


def test_groups_in_snapshots(ctx):
    files = [("plain", snap_file(), O.OK)]
    for name, x in EXACT:
        files.append(("inner." + name, snap_file(inner_extra=x), O.OK))
        files.append(("outer." + name, snap_file(outer_extra=x), O.OK))
        files.append(("both." + name, snap_file(x, x), O.OK))
        files.append(("split." + name, snap_file(x, x, split=True), O.OK))
    # one past the boundary: the status alone, for either message
    files.append(("inner.past", snap_file(inner_extra=PAST), L.UNSUPPORTED_ENCODING))
    files.append(("outer.past", snap_file(outer_extra=PAST), L.UNSUPPORTED_ENCODING))
    offs, packed = [], bytearray()
    for k, (_, f, _) in enumerate(files):
        offs.append(len(packed))
        packed += f + b"\0" * (k % 5)
    d = ctx.alloc(len(packed) + 64)
    d.upload(bytes(packed))
    try:
        st, sc, cc = S.verify_packed(d, len(packed), offs, [len(f) for _, f, _ in files])
        for i, (name, f, want) in enumerate(files):
            o = O.loadsnap(f)
            assert o["status"] == O.OK, name            # Go loads every one of them
            assert st[i] == want, (name, st[i])
            if want == O.OK:
                assert (sc[i], cc[i]) == (o["stored_crc"], o["computed_crc"]), name
                assert S.snapshot(ctx, i) == o["snap"], name
    finally:
        d.free()


# ---- a padded unknown tag in front of what a second walk collects -----------
# Unmarshal's default arm restarts Skip at index - sizeOfWire, sizeOfWire from
# the tag's value: after a three-byte tag of field 15 that is its last byte,
# 00, and with 02 behind it the unknown field is (field 0, varint 2) whatever
# wire type the tag named.  The walks that assemble a split bytes field or the
# Snapshot's lists afterwards must frame the following fields the same way.
def padded(wt):
    return K.vpad((15 << 3) | wt, 3) + b"\x02"


def test_padded_unknown_tag_between_split_segments_in_a_wal(ctx):
    m = GroupWal()
    for wt in range(8):
        # Record.Data in two segments, the tag between them: the chained CRC and the Entry come from both
        data = O.entry_marshal(0, 1, m.index, b"split record data %d" % wt)
        m.crc = O.crc32_update(m.crc, data)
        cut = 5 + wt
        body = (b"\x10" + K.vint(m.crc) + b"\x08\x02" + K.fb(3, data[:cut]) + padded(wt) + K.fb(3, data[cut:]))
        m.offsets.append(len(m.buf))
        m.buf += struct.pack("<q", len(body)) + body
        m.index += 1
        # Entry.Data in two segments inside a canonical record
        m.canonical(2, O.entry_marshal(1, 1, m.index, b"he") + padded(wt) + K.fb(4, b"ad%d" % wt))
        m.index += 1
        m.plain()
    o, g = assert_parity(ctx, m.buf, 0)
    assert o["status"] == O.OK and g["n_records"] == len(m.offsets)
    assert [e["data"] for e in g["ents"] if e["type"] == 1] == [b"head%d" % wt for wt in range(8)]
    assert all(e["unrec"] == b"\x00\x02" for e in g["ents"] if e["type"] == 1)
    other = build_wal(random.Random(7), 5, 10, big_terms=False)
    r = W.readall_batch_bytes([other, bytes(m.buf)], [0, 0], ctx)
    same_as_oracle(o, r[1].as_dict())


def test_padded_unknown_tag_between_split_segments_in_snapshots(ctx):
    files = []
    for wt in range(8):
        inner = O.snapshot_marshal(b"snap", [1, 2], 7, 2, removed=[9]) + padded(wt) + K.fv(2, 5) + K.fv(5, 6) + \
            K.fb(1, b"more")
        crc = O.crc32_update(0, inner)
        files.append(("inner.wt%d" % wt, O.snappb_marshal(crc, inner)))
        cut = len(inner) // 2 + wt
        files.append(("both.wt%d" % wt, O.snappb_marshal(crc, inner[:cut]) + padded(wt) + K.fb(2, inner[cut:])))
    offs, packed = [], bytearray()
    for k, (_, f) in enumerate(files):
        offs.append(len(packed))
        packed += f + b"\0" * (k % 3)
    d = ctx.alloc(len(packed) + 64)
    d.upload(bytes(packed))
    try:
        st, sc, cc = S.verify_packed(d, len(packed), offs, [len(f) for _, f in files])
        for i, (name, f) in enumerate(files):
            o = O.loadsnap(f)
            assert o["status"] == O.OK and o["snap"]["nodes"] == [1, 2, 5] and o["snap"]["data"] == b"snapmore", name
            assert (st[i], sc[i], cc[i]) == (O.OK, o["stored_crc"], o["computed_crc"]), (name, st[i])
            assert S.snapshot(ctx, i) == o["snap"], name
    finally:
        d.free()
