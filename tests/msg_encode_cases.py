"""Generators and the expected-bytes helper of the batched raftpb.Message
encode tests (tests/test_msg_encode_host.py, tests/test_gpu_msg_encode.py).

A Batch holds the host copies of emsg_encode_batch_device's arrays: the
payload bytes, the entry descriptors, the uint64 values and the messages.
Its expected() is the oracle's Marshal of every message, nothing of the
engine's."""
import ctypes as C
import random

from oracle import oracle as O
from etcd_amd import _lib as L

U64 = (1 << 64) - 1
# 2^(7k) - 1 and 2^(7k), k = 1..9, and 2^64 - 1: every varint width from both sides
WIDTHS = sorted({(1 << (7 * k)) - 1 for k in range(1, 10)} | {1 << (7 * k) for k in range(1, 10)} | {U64})
DATA_LENS = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257]
FIELDS = ("type", "to", "from_", "term", "log_term", "index", "commit")


def sov(v):
    return max(1, (v.bit_length() + 6) // 7)


class Batch:
    def __init__(self, seed=1):
        self.rng = random.Random(seed)
        self.data = bytearray()
        self.ents = []    # (type, term, index, off, len, nil)
        self.u64 = []
        self.msgs = []    # dicts of emsg_out's fields

    def rand_bytes(self, n):
        return self.rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""

    def add_data(self, b, residue=None):
        """Append b (padding first so that its offset is residue mod 16); its offset."""
        if residue is not None:
            self.data += self.rand_bytes((residue - len(self.data)) % 16)
        off = len(self.data)
        self.data += b
        return off

    def add_entry(self, type_=0, term=0, index=0, data=None, residue=None):
        off = self.add_data(data, residue) if data else 0
        self.ents.append((type_, term, index, off, len(data) if data else 0, 1 if data is None else 0))
        return len(self.ents) - 1

    def add_u64(self, vals):
        off = len(self.u64)
        self.u64 += list(vals)
        return off

    def add_msg(self, ents=None, snap_data=None, nodes=(), removed=(), nodes_at=None, removed_at=None, **f):
        """ents: (first, n) into the entries; snap_data: bytes or an (off, len)
        range; nodes / removed: values, or nodes_at / removed_at = (off, n)
        into the values already added."""
        m = dict.fromkeys(FIELDS + ("snap_index", "snap_term", "reject"), 0)
        m.update(f)
        m["ents_first"], m["n_ents"] = ents if ents is not None else (len(self.ents), 0)
        if isinstance(snap_data, tuple):
            m["snap_data_off"], m["snap_data_len"] = snap_data
        else:
            m["snap_data_off"] = self.add_data(snap_data) if snap_data else 0
            m["snap_data_len"] = len(snap_data or b"")
        m["snap_nodes_off"], m["snap_n_nodes"] = nodes_at if nodes_at else (self.add_u64(nodes), len(nodes))
        m["snap_removed_off"], m["snap_n_removed"] = removed_at if removed_at else (self.add_u64(removed), len(removed))
        self.msgs.append(m)
        return len(self.msgs) - 1

    def add_filler(self, size):
        """A message of exactly `size` bytes (>= 24): Snapshot.Data carries the length."""
        for extra in range(4):
            to = (1 << (7 * extra)) if extra else 0
            for d in range(max(0, size - 24 - extra - 8), size - 24 - extra + 1):
                s = 6 + d + sov(d) - 1
                if 24 + extra + d + (sov(d) - 1) + (sov(s) - 1) == size:
                    return self.add_msg(to=to, snap_data=self.rand_bytes(d))
        raise ValueError(size)

    def total(self):
        return sum(len(b) for b in self.expected())

    def pad_to(self, pos, tile):
        """Fillers so that the next message starts at `pos` modulo the tile."""
        at = self.total()
        gap = (pos - at) % tile
        if gap and gap < 24:
            gap += tile
        if gap:
            self.add_filler(gap)
        assert self.total() % tile == pos % tile

    # -- the oracle's bytes ------------------------------------------------
    def entry_body(self, j):
        t, term, index, off, ln, nil = self.ents[j]
        return O.entry_marshal(t, term, index, None if nil else bytes(self.data[off:off + ln]))

    def expected(self):
        exp = self.__dict__.setdefault("_exp", [])   # messages do not change once added
        while len(exp) < len(self.msgs):
            exp.append(self.expected_one(self.msgs[len(exp)]))
        return exp

    def expected_one(self, m):
        ents = [self.entry_body(j) for j in range(m["ents_first"], m["ents_first"] + m["n_ents"])]
        snap = O.snapshot_marshal(bytes(self.data[m["snap_data_off"]:m["snap_data_off"] + m["snap_data_len"]]),
                                  self.u64[m["snap_nodes_off"]:m["snap_nodes_off"] + m["snap_n_nodes"]],
                                  m["snap_index"], m["snap_term"],
                                  self.u64[m["snap_removed_off"]:m["snap_removed_off"] + m["snap_n_removed"]])
        return O.message_marshal(m["type"], m["to"], m["from_"], m["term"], m["log_term"], m["index"], ents,
                                 m["commit"], snap, bool(m["reject"]))

    # -- the C arrays --------------------------------------------------------
    def c_msgs(self):
        arr = (L.OutMsg * max(len(self.msgs), 1))()
        for a, m in zip(arr, self.msgs):
            for k, v in m.items():
                setattr(a, k, v)
        return arr

    def c_ents(self):
        arr = (L.EntryDesc * max(len(self.ents), 1))()
        for a, (t, term, index, off, ln, nil) in zip(arr, self.ents):
            a.type, a.term, a.index, a.data_off, a.data_len, a.data_nil = t, term, index, off, ln, nil
        return arr

    def c_u64(self):
        return (C.c_uint64 * max(len(self.u64), 1))(*self.u64)

    def host_size(self):
        return L.lib.emsg_encode_size(self.c_msgs(), len(self.msgs), self.c_ents(), len(self.ents), self.c_u64(),
                                      len(self.u64))


def width_lattice():
    """Every varint-carrying field at every width edge, Entry type -1, Reject both ways."""
    b = Batch(11)
    for v in WIDTHS:
        for f in FIELDS:
            b.add_msg(**{f: v})
        e0 = b.add_entry(0, v, 1, b"t")
        b.add_entry(1, 1, v, b"i")
        b.add_msg(ents=(e0, 2), snap_index=v, reject=1)
        b.add_msg(snap_term=v, nodes=[v], removed=[v, 1])
    e = b.add_entry(-1, 2, 3, b"neg")
    b.add_msg(ents=(e, 1))
    b.add_msg(reject=1)
    b.add_msg(reject=0)
    return b


def length_lattice():
    """|E| and |S| at the length varint's edges; n_ents 0, 1, 2, 65."""
    b = Batch(12)
    for want in (127, 128, 16383, 16384):
        # E = 08 00 10 00 18 00 22 v(d) Data
        d = next(d for d in range(want) if 7 + sov(d) + d == want)
        e = b.add_entry(0, 0, 0, b.rand_bytes(d))
        assert len(b.entry_body(e)) == want
        b.add_msg(ents=(e, 1))
        # S = 0a v(d) Data 18 00 20 00
        d = next(d for d in range(want) if 5 + sov(d) + d == want)
        b.add_msg(snap_data=b.rand_bytes(d))
    for n in (0, 1, 2, 65):
        first = len(b.ents)
        for k in range(n):
            b.add_entry(k & 1, k, k + 1, b.rand_bytes(k % 7))
        b.add_msg(ents=(first, n), type=3, commit=n)
    return b


def shared_ranges():
    b = Batch(13)
    for k in range(6):
        b.add_entry(0, 5, 100 + k, b.rand_bytes(10 + 30 * k))
    for to in (2, 3, 1 << 40):
        b.add_msg(type=3, to=to, from_=1, term=5, ents=(1, 3))
    b.add_msg(ents=(0, 4), index=1)
    b.add_msg(ents=(2, 4), index=2)
    b.add_msg(ents=(len(b.ents), 0))
    return b


def rand_mix(n=300, seed=41):
    """Messages drawn like tests/test_gpu_raftmsg._rand_msg."""
    b = Batch(seed)
    rng = b.rng
    for _ in range(n):
        first = len(b.ents)
        for _ in range(rng.choice([0, 0, 1, 3, 20])):
            b.add_entry(rng.choice([0, 1]), rng.randrange(1 << rng.choice([3, 30, 63])), rng.randrange(1 << 40),
                        b.rand_bytes(rng.choice([0, 1, 50, 700])))
        b.add_msg(type=rng.randrange(16), to=rng.randrange(1 << 62), from_=rng.randrange(1 << 62),
                  term=rng.randrange(1 << 30), log_term=rng.randrange(1 << 30), index=rng.randrange(1 << 40),
                  ents=(first, len(b.ents) - first), commit=rng.randrange(1 << 40),
                  snap_data=b.rand_bytes(rng.choice([0, 10, 3000])),
                  nodes=[rng.randrange(1, 1 << 20) for _ in range(rng.randrange(0, 4))],
                  snap_index=rng.randrange(1 << 30), snap_term=rng.randrange(1 << 10),
                  reject=int(rng.random() < 0.5))
    return b
