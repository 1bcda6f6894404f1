"""Edge lattices for the entry points that share the WAL path's prefix
machinery but not its tests (tests/test_gpu_aux_edges.py runs them on the
GPU): ewal_crc32_update_device, esnap_verify_packed, ecommit_batch_device,
ecommit_batch_rec_device, ewal_encode_entries_device, ewal_save_device.

This module holds the generators and, un-marked, their self-checks: every
lattice point the GPU tests rely on is asserted to be present here, from the
oracle's outputs alone (no GPU, no product code)."""
import random
import zlib

import numpy as np

from oracle import oracle as O

KiB, MiB = 1 << 10, 1 << 20
M64 = (1 << 64) - 1
B32 = 1 << 32

# ---------------------------------------------------------------------------
# 1. ewal_crc32_update_device: lengths over one pool
# ---------------------------------------------------------------------------
POOL_BYTES = 80 * MiB + 8 * KiB
POOL_SEED = 20240611
POLYS = (O.CASTAGNOLI, O.KOOPMAN, O.IEEE)

DELTAS = (-4097, -4096, -257, -256, -17, -16, -15, -1, 0, 1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097)
SMALL_MAX = 2 * 4096 + 512          # (a): every n in 0 .. SMALL_MAX
# (d): the stream pass runs 12 waves on each of 256 CUs, a wave takes 8 KiB
# pairs: 24 MiB is one pair per wave.  The ctx does not expose its CU count,
# so the sizes stay those of the 256-CU part.
PAIR_ROUND = 12 * 256 * 8 * KiB
LARGE_BASES = (PAIR_ROUND, PAIR_ROUND + 8 * KiB * 3072, 50 * MiB, 76 * MiB, 80 * MiB)
LARGE_DELTAS = (-1, 0, 1, 4095, 4097, 8191)
ORDER_SEQUENCE = (80 * MiB, 5, 33 * MiB + 17, 4096, 0, 80 * MiB)


def make_pool(nbytes=POOL_BYTES, seed=POOL_SEED):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


def lengths_small():
    return list(range(SMALL_MAX + 1))


def lengths_edges():
    """(b): the unit, pair, scan-lane, workgroup, tile and tile-group edges."""
    bases = [8 * KiB * k for k in (1, 2, 3)] + [16 * KiB * k for k in (1, 3)] + [96 * KiB * k for k in (1, 2)] + \
        [MiB * k for k in (1, 2, 15, 16, 17, 32, 33)]
    return sorted({b + d for b in bases for d in DELTAS})


def lengths_nsafe():
    """(c): around nsafe = (B - 16) / 4096."""
    return [4096 * u + d for u in (1, 2, 3, 4) for d in (15, 16, 17)]


def lengths_large():
    """(d): 1, 2, 3 and 4 pairs per wave."""
    return sorted({b + d for b in LARGE_BASES for d in LARGE_DELTAS})


def lengths_order():
    """(e): the union of (b)-(d) in a fixed shuffled order, then a sequence
    that shrinks and grows."""
    u = sorted(set(lengths_edges()) | set(lengths_nsafe()) | set(lengths_large()))
    random.Random(77).shuffle(u)
    return u + list(ORDER_SEQUENCE)


def base_offsets():
    """(f): (byte offset of the base pointer, n)."""
    return [(16 * j, n) for j in list(range(1, 17)) + [255] for n in (1, 255, 4097, MiB + 17)]


def crc_chain(pool, lengths, poly=O.CASTAGNOLI):
    """{n: crc32.Update(0, poly, pool[:n])} in one pass over the pool."""
    out, prev, a = {}, 0, 0
    for b in sorted(set(lengths)):
        prev = O.crc32_update(prev, pool[a:b].tobytes(), poly)
        out[b] = prev
        a = b
    return out


def test_crc_lengths_cover_prefix_and_stream_edges():
    small = lengths_small()
    # prefix_at: every count of whole super-pieces before x, every tail length
    assert {(n >> 8) & 15 for n in small} == set(range(16))
    assert {n & 255 for n in small} == set(range(256))
    assert {(n & 255, (n >> 8) & 15) for n in small} >= {(t, k) for t in range(256) for k in range(16)}
    # odd and even unit counts, one unit either side of the unguarded path
    units = {n // 4096 + 1 for n in small}
    assert units == {1, 2, 3}
    for u in (1, 2, 3, 4):
        ns = {(n - 16) // 4096 for n in lengths_nsafe() if n // 4096 == u}
        assert ns == {u - 1, u}
    edges = lengths_edges()
    assert min(edges) >= 0 and len(edges) > 200
    for k in (1, 2, 15, 16, 17, 32, 33):       # tiles and 16-tile groups
        assert {k * MiB - 1, k * MiB, k * MiB + 1, k * MiB + 4096} <= set(edges)
    large = lengths_large()
    assert max(large) == POOL_BYTES - 1 and len(large) == 30
    assert {-(-n // PAIR_ROUND) for n in large} == {1, 2, 3, 4}
    order = lengths_order()
    assert order[-6:] == list(ORDER_SEQUENCE)
    ups = sum(1 for a, b in zip(order, order[1:]) if b > a)
    assert ups > 100 and len(order) - 1 - ups > 100           # grows and shrinks
    assert max(o + n for o, n in base_offsets()) < POOL_BYTES
    assert {o % 256 for o, _ in base_offsets()} >= {16 * j for j in range(16)}


def test_crc_chain_is_the_oracle_and_ieee_is_zlib():
    pool = make_pool(3 * MiB + 100, seed=5)
    lens = [0, 1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 70001, MiB, 3 * MiB + 11]
    for poly in POLYS:
        ch = crc_chain(pool, lens, poly)
        for n in lens:
            assert ch[n] == O.crc32_update(0, pool[:n].tobytes(), poly), (hex(poly), n)
    for n in lens:
        b = pool[:n].tobytes()
        assert O.crc32_update(0, b, O.IEEE) == zlib.crc32(b)
        assert O.crc32_update(0xDEADBEEF, b, O.IEEE) == zlib.crc32(b, 0xDEADBEEF)


# ---------------------------------------------------------------------------
# 2. esnap_verify_packed: residues of Data start and Data end mod 256
# ---------------------------------------------------------------------------
RESIDUES = (0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 239, 240, 252, 253, 254, 255)
PAD = 0xA5
SNAP_NODES = [1, 2, 3]


def _vlen(v):
    n = 1
    while v >= 0x80:
        v >>= 7
        n += 1
    return n


def _snap_body(rng, want_len, index, term):
    """A marshalled raftpb.Snapshot of exactly want_len bytes, or None when
    no Data length gives it (a varint length boundary)."""
    fixed = 1 + 2 * len(SNAP_NODES) + 1 + _vlen(index) + 1 + _vlen(term)     # Data tag, Nodes, Index, Term
    for n in range(max(0, want_len - fixed - 10), max(0, want_len - fixed) + 1):
        if fixed + _vlen(n) + n == want_len:
            body = O.snapshot_marshal(rng.randbytes(n), SNAP_NODES, index, term)
            assert len(body) == want_len
            return body
    return None


class SnapPack:
    """Snapshot files packed in one buffer: offs, lens, the bytes, and for the
    lattice files their (start residue, end residue)."""

    def __init__(self):
        self.buf = bytearray()
        self.offs, self.lens, self.pairs, self.doff, self.dlen = [], [], [], [], []

    def add(self, f, header, rs=None, pair=None):
        """Pad (at least one byte) so that the envelope's Data starts at
        residue rs, then append file f whose Data starts header bytes in."""
        pos = len(self.buf)
        pad = 1 if rs is None else (rs - header - pos - 1) % 256 + 1
        self.buf += bytes([PAD]) * pad
        self.offs.append(len(self.buf))
        self.lens.append(len(f))
        self.doff.append(len(self.buf) + header)
        self.dlen.append(len(f) - header)
        self.pairs.append(pair)
        self.buf += f

    def file(self, i, buf=None):
        b = self.buf if buf is None else buf
        return bytes(b[self.offs[i]:self.offs[i] + self.lens[i]])


def _envelope(body, poly):
    f = O.snappb_marshal(O.crc32_update(0, body, poly), body)
    return f, len(f) - len(body)


def build_snap_lattice(poly, seed=31):
    """One valid file per (rs, re) in RESIDUES x RESIDUES, then the extras: an
    empty envelope Data, a 1-byte one, and a file whose Data ends on the
    buffer's last byte.  n_lattice files come first."""
    rng = random.Random(seed)
    sp = SnapPack()
    k = 0
    for rs in RESIDUES:
        for re_ in RESIDUES:
            extra = rng.choice([0, 1, 2, 5, 17])
            want = (re_ - rs) % 256 + 256 * extra
            body = None
            while body is None:
                body = _snap_body(rng, want, 1000 + k, 1 + k % 5) if want >= 12 else None
                want += 256
            f, header = _envelope(body, poly)
            sp.add(f, header, rs, (rs, re_))
            k += 1
    sp.n_lattice = k
    for body in (b"", b"\x18"):
        f, header = _envelope(body, poly)
        sp.add(f, header)
    f, header = _envelope(_snap_body(rng, 700, 7, 7), poly)
    sp.add(f, header, 255)
    return sp


SNAP_DAMAGE = ("data_first", "data_last", "pad_before", "pad_after")


def damage_snap_lattice(sp, kind):
    """A copy of sp's bytes with one flipped byte at every 5th lattice file."""
    b = bytearray(sp.buf)
    for i in range(0, sp.n_lattice, 5):
        p = {"data_first": sp.doff[i], "data_last": sp.doff[i] + sp.dlen[i] - 1, "pad_before": sp.offs[i] - 1,
             "pad_after": sp.offs[i] + sp.lens[i]}[kind]
        b[p] ^= 0x41
    return b


def small_snap_batch(poly):
    rng = random.Random(9)
    sp = SnapPack()
    for n in (0, 33, 5000):
        f, header = _envelope(O.snapshot_marshal(rng.randbytes(n), SNAP_NODES, n + 1, 2), poly)
        sp.add(f, header)
    return sp


def test_snap_lattice_covers_every_residue_pair():
    for poly in POLYS:
        sp = build_snap_lattice(poly)
        assert sp.n_lattice == len(RESIDUES) ** 2 == 484
        got = set()
        for i in range(sp.n_lattice):
            rs, re_ = sp.pairs[i]
            assert sp.doff[i] % 256 == rs and (sp.doff[i] + sp.dlen[i]) % 256 == re_
            assert sp.buf[sp.offs[i] - 1] == PAD and sp.buf[sp.offs[i] + sp.lens[i]] == PAD
            got.add((rs, re_))
            o = O.loadsnap(sp.file(i), poly)
            assert o["status"] == O.OK, (i, o["status"])
            assert o["snap"]["index"] == 1000 + i and o["snap"]["nodes"] == SNAP_NODES
        assert got == {(a, b) for a in RESIDUES for b in RESIDUES}
        assert {(d >> 8) & 15 for d in sp.doff[:sp.n_lattice]} == set(range(16))
        assert {((d + n) >> 8) & 15 for d, n in zip(sp.doff[:484], sp.dlen[:484])} == set(range(16))
        assert len({d >> 12 for d in sp.doff}) > 100                     # ranges cross unit boundaries
        assert any((d >> 12) != ((d + n) >> 12) for d, n in zip(sp.doff, sp.dlen))
        assert sp.dlen[484:] == [0, 1, 700]
        assert sp.offs[-1] + sp.lens[-1] == len(sp.buf) and (len(sp.buf) - 700) % 256 == 255
        assert O.loadsnap(sp.file(486), poly)["status"] == O.OK
        assert len(sp.buf) < MiB
        # the damage: Data flips change the verdict, padding flips change no file
        for kind in SNAP_DAMAGE:
            b = damage_snap_lattice(sp, kind)
            assert np.count_nonzero(np.frombuffer(b, np.uint8) != np.frombuffer(sp.buf, np.uint8)) == 97
            for i in range(sp.n_lattice):
                hit = i % 5 == 0 and kind.startswith("data")
                assert (sp.file(i, b) != sp.file(i)) == hit
                if hit:
                    assert O.loadsnap(sp.file(i, b), poly)["status"] != O.OK


# ---------------------------------------------------------------------------
# 3. raft.maybeCommit over full uint64 magnitudes
# ---------------------------------------------------------------------------
MAG = (0, 1, 2, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 32 + 2, 2 ** 53 + 1, 2 ** 63 - 1, 2 ** 63,
       2 ** 63 + 1, 2 ** 64 - 2, 2 ** 64 - 1)
NLOGS = (0, 1, 3, 12, 13, 14, 30)
SOA_VOTERS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33, 255)
REC_VOTERS = (1, 2, 3, 4, 5, 6, 7)
SOA_G = (1, 255, 256, 257, 1023, 1024, 1025, 4097)
REC_G = (1, 63, 64, 65, 129)
REC_G_BIG = 64 * 12 * 256 + 65      # past one round of the record kernel's persistent grid (12 waves x 256 CUs)
N_SOA, N_REC = 4097, 4800
TAIL = 13


def _near(rng, x):
    return (x + rng.choice([-2, -1, 0, 0, 1, 2])) & M64


def quorum_index(m):
    """mis[q-1] of raft.go:252-255 (the generator steers its inputs by it and
    the self-check classifies by it; expectations come from the oracle)."""
    return sorted(m, reverse=True)[len(m) // 2]


def commit_groups(voters, count, seed):
    """[(matches, log terms, offset, term, committed)] over MAG, its +-1/+-2
    neighbours and low-word twins (x ^ 2^32)."""
    rng = random.Random(seed)
    out = []
    for g in range(count):
        nv = voters[g % len(voters)] if g < 4 * len(voters) else rng.choice(voters)
        base, other = rng.choice(MAG), rng.choice(MAG)
        m = [rng.choice([_near(rng, base), _near(rng, base), _near(rng, base), _near(rng, base ^ B32), other])
             for _ in range(nv)]
        mci = quorum_index(m)
        committed = rng.choice([_near(rng, mci), (mci - 1) & M64, (mci - 2) & M64, _near(rng, mci ^ B32),
                                ((mci ^ B32) - 1) & M64, 0, 0])
        nlog = rng.choice(NLOGS)
        where = rng.choice(["before", "first", "first", "last", "last", "past", "k12", "k13", "k14", "k13", "max", "mag"])
        if nlog == 0 and rng.random() < 0.5:
            where = "zero"
        pos = None                                  # mci - offset when it lies in the log
        if where == "before":
            off = (mci + rng.choice([1, 2, B32])) & M64
        elif where == "first":
            off, pos = mci, 0
        elif where == "last":
            off, pos = (mci - (nlog - 1)) & M64, nlog - 1
        elif where == "past":
            off = (mci - nlog) & M64
        elif where in ("k12", "k13", "k14"):
            pos = max(0, nlog - 1 - int(where[1:]))
            off = (mci - pos) & M64
        elif where == "max":
            off = M64
        elif where == "zero":
            off = 0
        else:
            off = rng.choice(MAG)
        term = rng.choice([1, 5, 7, B32 + 5, B32 + 7, 2 ** 63 + 1, M64])
        pool = [term, term, term ^ B32, (term + 1) & M64, 5, B32 + 5]
        lt = [rng.choice(pool) for _ in range(nlog)]
        if pos is not None and 0 <= pos < nlog and off <= mci:
            lt[pos] = rng.choice([term, term, term, term ^ B32, term ^ B32, (term + 1) & M64])
        out.append((m, lt, off, term, committed))
    return out


def commit_expect(groups):
    """[(new committed, changed, status)] per group from O.maybe_commit."""
    out = []
    for m, lt, off, term, c in groups:
        rc, newc = O.maybe_commit(m, term, c, lt, off)
        out.append((newc, 1 if rc == 1 else 0, O.PANIC_BOUNDS if rc < 0 else 0))
    return out


def before_window(group):
    """The quorum index's term is read and lies before the record's 13-term
    tail window (the record kernel then needs log_terms)."""
    m, lt, off, term, c = group
    mci, nlog = quorum_index(m), len(lt)
    last = (nlog - 1 + off) & M64
    if not mci > c or mci < off or mci > last:
        return False
    k = mci - off
    return k < nlog and nlog - 1 - k >= TAIL


def commit_classes(groups, expect):
    n = dict(commit=0, commit_hi=0, term_twin=0, low_word_above=0, out_of_window=0, panic=0, commit_before_window=0)
    for grp, (newc, chg, st) in zip(groups, expect):
        m, lt, off, term, c = grp
        mci, nlog = quorum_index(m), len(lt)
        last = (nlog - 1 + off) & M64
        if st:
            n["panic"] += 1
        elif chg:
            assert newc == mci
            n["commit"] += 1
            n["commit_hi"] += newc >= B32
            n["commit_before_window"] += before_window(grp)
        else:
            assert newc == c
            if mci <= c:
                n["low_word_above"] += (mci & (B32 - 1)) > (c & (B32 - 1))
            elif mci < off or mci > last:
                n["out_of_window"] += 1
            else:
                t = lt[mci - off]
                assert t != term
                n["term_twin"] += (t ^ term) & (B32 - 1) == 0
    return n


SOA_SEED, REC_SEED = 41, 42


def soa_groups():
    return commit_groups(SOA_VOTERS, N_SOA, SOA_SEED)


def rec_groups():
    return commit_groups(REC_VOTERS, N_REC, REC_SEED)


def soa_arrays(groups, V=None):
    """The SoA arrays of ecommit_batch_device for groups."""
    G = len(groups)
    V = V or max(len(g[0]) for g in groups)
    match = np.zeros((V, G), np.uint64)
    for gi, g in enumerate(groups):
        match[:len(g[0]), gi] = np.array(g[0], np.uint64)
    nv = np.array([len(g[0]) for g in groups], np.uint8)
    ptr = np.concatenate([[0], np.cumsum([len(g[1]) for g in groups])]).astype(np.uint64)
    lt = np.array([t for g in groups for t in g[1]] or [0], np.uint64)
    term = np.array([g[3] for g in groups], np.uint64)
    comm = np.array([g[4] for g in groups], np.uint64)
    off = np.array([g[2] for g in groups], np.uint64)
    return match, nv, term, comm, off, ptr, lt


def tile_soa(arrs, G):
    """G groups taken round-robin from the arrays of N groups (numpy only)."""
    match, nv, term, comm, off, ptr, lt = arrs
    N = len(nv)
    idx = (np.arange(G, dtype=np.int64) * 7 + 3) % N        # 7 and N coprime: every group, in a new order
    nlog = (ptr[1:] - ptr[:-1]).astype(np.int64)[idx]
    nptr = np.concatenate([[0], np.cumsum(nlog)]).astype(np.uint64)
    start = ptr[:-1].astype(np.int64)[idx]
    within = np.arange(int(nptr[-1]), dtype=np.int64) - np.repeat(nptr[:-1].astype(np.int64), nlog)
    nlt = lt[np.repeat(start, nlog) + within]
    return np.ascontiguousarray(match[:, idx]), nv[idx], term[idx], comm[idx], off[idx], nptr, nlt


def batch_expect(arrs):
    """(new committed, changed, status) arrays from O.maybe_commit_batch."""
    match, nv, term, comm, off, ptr, lt = arrs
    G = len(nv)
    c = comm.copy()
    chg, st = np.zeros(G, np.uint8), np.zeros(G, np.uint8)
    O.maybe_commit_batch(G, np.ascontiguousarray(match), nv, term, c, off, ptr, lt, chg, st)
    return c, chg, st


def test_commit_generators_reach_every_class():
    for groups, rec in ((soa_groups(), False), (rec_groups(), True)):
        exp = commit_expect(groups)
        n = commit_classes(groups, exp)
        need = [k for k in n if rec or k != "commit_before_window"]
        assert all(n[k] >= 20 for k in need), n
        assert {len(g[0]) for g in groups} == set(REC_VOTERS if rec else SOA_VOTERS)
        assert {len(g[1]) for g in groups} == set(NLOGS)
        assert any(g[2] == M64 for g in groups)
        # the batch oracle agrees with the per-group one, tiled or not
        arrs = soa_arrays(groups)
        c, chg, st = batch_expect(arrs)
        assert [(int(a), int(b), int(s)) for a, b, s in zip(c, chg, st)] == exp
        if rec:
            assert sum(before_window(g) for g in groups) >= 20
            big = tile_soa(arrs, REC_G_BIG)
            c, chg, st = batch_expect(big)
            idx = (np.arange(REC_G_BIG) * 7 + 3) % len(groups)
            e = np.array([x[0] for x in exp], np.uint64)
            assert (c == e[idx]).all() and (chg == np.array([x[1] for x in exp], np.uint8)[idx]).all()
            assert (st == np.array([x[2] for x in exp], np.uint8)[idx]).all()
            second = slice(64 * 12 * 256, None)                  # what the persistent loop's second round reads
            assert chg[second].any() and not chg[second].all() and (c[second] >= B32).any()


def test_oracle_maybe_commit_takes_full_uint64():
    assert O.maybe_commit([B32 + 1] * 3, 7, B32, [7, 7], B32) == (1, B32 + 1)
    assert O.maybe_commit([B32 + 1] * 3, 7, 2 * B32, [7, 7], B32) == (0, 2 * B32)          # low word above, value not
    assert O.maybe_commit([B32 + 1] * 3, 7 ^ B32, B32, [7, 7], B32) == (0, B32)            # terms agree in the low word
    assert O.maybe_commit([5] * 3, 7, 0, [7, 7], M64) == (0, 0)                           # lastIndex() wraps
    assert O.maybe_commit([5] * 3, 7, 0, [], 0)[0] < 0


# ---------------------------------------------------------------------------
# 4. write path: the first chunk's x < 4 rule, wave_copy's alignments
# ---------------------------------------------------------------------------
SAVE_PREVS = (0, 0xFFFFFFFF, 0x01234567, 0x9E3779B1)


def save_sequences():
    """Lists of ops ("cut", metadata) / ("state", (term, vote, commit)) /
    ("entry", (type, term, index, data)): a first op whose chunk is 1..5 bytes
    (or a HardState), then one follower."""
    rng = random.Random(13)
    firsts = [("cut", bytes([0x61 + k] * k)) for k in (1, 2, 3, 4, 5)] + [("state", (3, 1, 9))]
    follows = [[("entry", (0, 2, 5, b""))], [("entry", (0, 2, 5, b"z"))], [("entry", (1, 2, 5, rng.randbytes(700)))],
               [("state", (4, 2, 1 << 40))], [("cut", b"md")], [("cut", None)], [("cut", b"q")],
               [("cut", b"r"), ("cut", b"s"), ("cut", b"t"), ("cut", b"u"), ("entry", (0, 1, 1, b"abc"))]]
    return [[f] + fl for f in firsts for fl in follows]


def test_save_sequences_put_chunk_ends_inside_the_first_dword():
    ends = set()
    for ops in save_sequences():
        x = 0
        for j, (kind, v) in enumerate(ops):
            if kind == "cut":
                x += len(v or b"")
            elif kind == "state":
                x += len(O.hardstate_marshal(*v))
            else:
                x += len(O.entry_marshal(*v))
            ends.add((j, min(x, 5)))
    assert {(0, k) for k in (1, 2, 3, 4, 5)} <= ends          # the first chunk ends at x = 1, 2, 3, 4, > 4
    assert {(1, 2), (1, 3), (1, 4), (2, 3), (2, 4)} <= ends   # later chunks still inside the first dword


ENC_BLOB = 4096
# data_len_total of each call over the one blob: a copy that ends at the end
# of the source takes wave_copy's byte-wise branch (a + 8 <= send false) only
# when that end is not a multiple of 4
ENC_TOTALS = (ENC_BLOB, ENC_BLOB - 1, ENC_BLOB - 2, ENC_BLOB - 3)
ENC_LENS = tuple(range(10)) + (63, 64, 65, 255, 256, 257)
ENC_TERMS = (1, 200, 70000, 1 << 22)                          # Term varints of 1..4 bytes move the destination


def encode_cases(total=ENC_BLOB):
    """[(type, term, index, data_off, data_len)] over the first `total` bytes
    of one ENC_BLOB-byte source; the last entries end exactly at total."""
    rng = random.Random(17)
    out = []
    i = 1
    for L in ENC_LENS:
        for s in range(4):
            for t in ENC_TERMS:
                off = 4 * rng.randrange(0, (ENC_BLOB - 300) // 4) + s
                out.append((0, t, i, off, L))
                i += 1
    for L in range(4, 13):
        for t in ENC_TERMS:
            out.append((1, t, i, total - L, L))
            i += 1
    return out


def test_encode_cases_cover_source_and_destination_alignments():
    pairs, tail, end_branch = set(), set(), 0
    for total in ENC_TOTALS:
        cases = encode_cases(total)
        x = 0
        for ty, t, idx, off, L in cases:
            assert off + L <= total
            e = O.entry_marshal(ty, t, idx, b"\0" * L)
            dst = x + len(e) - L                               # where Data lands in the data-only stream
            if L >= 8:
                pairs.add((off % 4, dst % 4))
            if off + L == total:
                tail.add((off % 4, L))
                # wave_copy's last output dword reads the source at p = off + head + 4 (m - 1)
                head = min(L, (4 - dst % 4) % 4)
                m = (L - head) // 4
                if m:
                    p = off + head + 4 * (m - 1)
                    end_branch += p % 4 != 0 and (p & ~3) + 8 > total
            x += len(e)
        for L in ENC_LENS:
            assert {c[3] % 4 for c in cases if c[4] == L} == {0, 1, 2, 3}
    assert pairs == {(a, b) for a in range(4) for b in range(4)}
    assert tail == {(s, L) for s in range(4) for L in range(4, 13)}      # misalignment 1, 2, 3 (and 0) at every length
    assert end_branch >= 20


# ---------------------------------------------------------------------------
# 5. write path: the two entry points over the one pipeline (k_wr_*)
# ---------------------------------------------------------------------------
WIRE_N = (1, 2, 63, 64, 65, 255, 256, 257)                    # around a wave's 64 lanes and a 256-thread block
WIRE_TYPES = (0, 1, -1)
WIRE_BOUNDS = tuple(v for k in range(1, 10) for v in ((1 << 7 * k) - 1, 1 << 7 * k))
WIRE_DLENS = (None, 0, 1, 127, 128, 16383, 16384)


def _wire_blob():
    return make_pool(16384 + 256, seed=23).tobytes()


def wire_entries(n, blob=None):
    """n entries (type, term, index, data): Type over WIRE_TYPES, Term and
    Index walking the varint width boundaries, Data over WIRE_DLENS."""
    blob = blob or _wire_blob()
    out = []
    for i in range(n):
        dl = WIRE_DLENS[i % len(WIRE_DLENS)]
        data = None if dl is None else blob[i % 251:i % 251 + dl]
        out.append((WIRE_TYPES[i % 3], WIRE_BOUNDS[i % 18], WIRE_BOUNDS[(7 * i + 3) % 18], data))
    return out


def test_wire_entries_cover_every_varint_width():
    blob = _wire_blob()
    for n in WIRE_N:
        ents = wire_entries(n, blob)
        assert len(ents) == n
        if n < 63:      # 1 and 2 entries cannot hold ten widths: the coverage below is that of the six larger counts
            continue
        assert {_vlen(e[1]) for e in ents} == set(range(1, 11))           # Term
        assert {_vlen(e[2]) for e in ents} == set(range(1, 11))           # Index
        assert {_vlen(len(e[3] or b"")) for e in ents} == {1, 2, 3}       # len(Data)
        assert {e[0] for e in ents} == set(WIRE_TYPES)
        assert {None if e[3] is None else len(e[3]) for e in ents} == set(WIRE_DLENS)
    # a negative Type is the 10-byte varint of its sign extension
    assert O.entry_marshal(-1, 1, 1, None)[:11] == b"\x08" + b"\xff" * 9 + b"\x01"


def stride_entries(cus):
    """4 * 8 * cus + 5 entries of 0..3 Data bytes: five more than one trip of
    the wave-per-record grid (8 workgroups of 4 waves on each of cus CUs)."""
    return [(0, 1 + (i >> 12), i + 1, bytes([i & 0xff] * (i & 3))) for i in range(4 * 8 * cus + 5)]


def test_stride_entries_exceed_one_grid_trip():
    for cus in (1, 64, 256, 304):
        ents = stride_entries(cus)
        assert len(ents) == 4 * 8 * cus + 5 > 4 * 8 * cus
        assert {len(e[3]) for e in ents} == {0, 1, 2, 3}


def stream_len(ops):
    """Bytes of the data-only stream of a save sequence: Entry and HardState
    marshals and Cut metadata; an empty HardState writes nothing."""
    x = 0
    for kind, v in ops:
        if kind == "cut":
            x += len(v or b"")
        elif kind == "state":
            x += len(O.hardstate_marshal(*v)) if any(v) else 0
        else:
            x += len(O.entry_marshal(*v))
    return x


def empty_stream_sequences():
    """Save sequences whose data-only stream is empty (E == 0)."""
    st, cut = ("state", (0, 0, 0)), ("cut", None)
    return [[st], [cut], [st, cut, st, cut]]


def test_empty_stream_sequences_have_no_data_bytes():
    for ops in empty_stream_sequences():
        assert stream_len(ops) == 0
    assert stream_len([("state", (0, 0, 1))]) == 6 and stream_len([("cut", b"")]) == 0
    for prev in SAVE_PREVS:                    # the reference: an empty HardState leaves no frame
        e = O.WalEncoder(prev)
        e.save_state(0, 0, 0)
        assert e.getvalue() == b"" and e.crc == prev


def write_error_ranges(total):
    """(data_off, data_len) outside a d_data of total bytes."""
    return {"past_end": (total - 3, 4), "empty_past_end": (total + 1, 0)}


def test_write_error_ranges_miss_by_one():
    for total in (0 + 3, 100, 4096):
        r = write_error_ranges(total)
        assert sum(r["past_end"]) == total + 1 and r["past_end"][1] > 0
        assert r["empty_past_end"] == (total + 1, 0)
