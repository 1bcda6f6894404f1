"""The edge lattice for the raftpb.Message decode (emsg_decode_batch_device).

Deterministic generators of POST /raft bodies: every family is a list of
(name, body).  Nothing here needs a GPU or the oracle; tests/
test_msg_decode_host.py checks the two references against each other over
these bodies and tests/test_gpu_msg_decode_edges.py sends them to the device.

All bodies are variations of one seed message S (61 bytes): ten non-default
fields, a two-byte varint at each of the three levels (Message.To, Entry.Index,
Snapshot.Index), two Entries (Type 1 with Data, Type 0 with empty Data), a
Snapshot with Data, two Nodes, Index, Term and one RemovedNodes, Reject true.
A body is put together from four lists of chunks, one per level: "msg" (the
Message, with markers where the sub-messages go), "ent" (the first Entry),
"ent2" (the second) and "snap".  "Each level" below means msg, ent and
snap: the Message, an Entry inside it, the Snapshot inside it.
"""
import os
import random
import re

M64 = (1 << 64) - 1
LEVELS = ("msg", "ent", "snap")

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "etcd_amd", "csrc", "ewal_device.h")
with open(_HDR) as _f:
    PB_SKIP_DEPTH = int(re.search(r"#define\s+PB_SKIP_DEPTH\s+(\d+)", _f.read()).group(1))
# pb_skip handles the outermost group in place and pushes one frame for every
# group opened inside a group; the push is refused when PB_SKIP_DEPTH frames
# are already on the stack.  So the boundary counts PUSHES: PB_SKIP_DEPTH
# pushes are exact, which is PB_SKIP_DEPTH + 1 start-group tags nested.
MAX_PUSHES = PB_SKIP_DEPTH
MAX_NESTED_STARTS = PB_SKIP_DEPTH + 1


def vint(v):
    """The minimal varint of v mod 2^64."""
    v &= M64
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def vpad(v, n, late=0):
    """v mod 2^64 in exactly n bytes: padded with 80...00 past its minimal
    length.  Bytes past the tenth sit at shifts >= 70, which Go shifts away;
    they carry the bits of `late`."""
    v &= M64
    out = bytearray()
    for k in range(n):
        c = (v >> (7 * k)) & 0x7F if k < 10 else late & 0x7F
        out.append(c | (0x80 if k < n - 1 else 0))
    return bytes(out)


def v10(low, last):
    """A ten-byte varint: the low 63 bits of `low`, then `last` (of which only bit 0 survives, as bit 63)."""
    return vpad(low & ((1 << 63) - 1), 10)[:9] + bytes([last])


def tag(fn, wt):
    return vint((fn << 3) | wt)


def fv(fn, v):
    return tag(fn, 0) + vint(v)


def fb(fn, d):
    return tag(fn, 2) + vint(len(d)) + d


# (field number, value): an int is a varint field, bytes a bytes field, a str the sub-message of that level
SPEC = {
    "msg": [(1, 3), (2, 150), (3, 2), (4, 5), (5, 4), (6, 7), (7, "ent"), (7, "ent2"), (8, 6), (9, "snap"), (10, 1)],
    "ent": [(1, 1), (2, 5), (3, 300), (4, b"abc")],
    "ent2": [(1, 0), (2, 5), (3, 301), (4, b"")],
    "snap": [(1, b"snap"), (2, 1), (2, 2), (3, 200), (4, 4), (5, 9)],
}


def seed(level):
    """The seed's chunks of one level; in "msg" a sub-message is a (field, level) marker."""
    out = []
    for fn, v in SPEC[level]:
        out.append(fv(fn, v) if isinstance(v, int) else fb(fn, v) if isinstance(v, bytes) else (fn, v))
    return out


def build(msg=None, ent=None, ent2=None, snap=None):
    subs = dict(ent=ent, ent2=ent2, snap=snap)
    out = []
    for c in seed("msg") if msg is None else msg:
        if isinstance(c, tuple):
            parts = subs[c[1]]
            out.append(fb(c[0], b"".join(seed(c[1]) if parts is None else parts)))
        else:
            out.append(c)
    return b"".join(out)


S = build()
assert len(S) <= 96


def put(level, chunk, pos=None):
    """The seed with `chunk` inserted into `level` before chunk `pos` (default: at its end)."""
    parts = seed(level)
    parts.insert(len(parts) if pos is None else pos, chunk)
    return build(**{level: parts})


def swap(level, idx, chunk):
    parts = seed(level)
    parts[idx] = chunk
    return build(**{level: parts})


def site(level, idx):
    """(tag value, value or length, payload) of chunk idx of the seed's level."""
    fn, v = SPEC[level][idx]
    if isinstance(v, int):
        return (fn << 3), v, b""
    d = v if isinstance(v, bytes) else b"".join(seed(v))
    return (fn << 3) | 2, len(d), d


def with_site(level, idx, tagb=None, enc=None):
    t, v, d = site(level, idx)
    return swap(level, idx, (vint(t) if tagb is None else tagb) + (vint(v) if enc is None else enc) + d)


VARINT_SITES = [("msg", i) for i in (0, 1, 2, 3, 4, 5, 8, 10)] + [("ent", i) for i in (0, 1, 2)] + \
    [("snap", i) for i in (1, 2, 3, 4, 5)]
LENGTH_SITES = [("msg", 6), ("msg", 9), ("ent", 3), ("snap", 0)]
KNOWN_SITES = [(lv, i) for lv in LEVELS for i in range(len(SPEC[lv]))]


def seed_marks():
    """Positions in S of every tag byte and every length-prefix byte (all are one byte long in S)."""
    tags, lens = [], []

    def walk(lo, hi, level):
        i = lo
        while i < hi:
            tags.append(i)
            fn, wt = S[i] >> 3, S[i] & 7
            i += 1
            if wt == 0:
                while S[i] >= 0x80:
                    i += 1
                i += 1
                continue
            lens.append(i)
            n = S[i]
            i += 1
            if level == "msg":
                walk(i, i + n, "ent" if fn == 7 else "snap")
            i += n

    walk(0, len(S), "msg")
    return tags, lens


def sub_span(which):
    """(position of the length byte, start, end) in S of sub-message "ent", "ent2" or "snap"."""
    idx = [c for c in seed("msg")].index((7 if which != "snap" else 9, which))
    at = len(build(msg=seed("msg")[:idx]))
    n = S[at + 1]
    return at + 1, at + 2, at + 2 + n


# ---- (a) single-fault exhaustion of S --------------------------------------
FAULT_BYTES = (0x00, 0x7F, 0x80, 0xFF, 0x0B, 0x0C, 0x3A, 0x4A)


def prefixes():
    return [("a/prefix%d" % p, S[:p]) for p in range(len(S) + 1)]


def family_a():
    out = []
    for p in range(len(S)):
        for bit in range(8):
            b = bytearray(S)
            b[p] ^= 1 << bit
            out.append(("a/flip%d.%d" % (p, bit), bytes(b)))
    out += prefixes()
    for p in range(len(S)):
        for v in FAULT_BYTES:
            b = bytearray(S)
            b[p] = v
            out.append(("a/set%d=%02x" % (p, v), bytes(b)))
    tags, lens = seed_marks()
    for kind, marks in (("tag", tags), ("len", lens)):
        for p in marks:
            for v in range(256):
                b = bytearray(S)
                b[p] = v
                out.append(("a/%s%d=%02x" % (kind, p, v), bytes(b)))
    return out


# ---- (b) moving sub-message boundaries -------------------------------------
def family_b():
    out = []
    for which in ("ent", "ent2", "snap"):
        whole = b"".join(seed(which))
        for k in range(len(whole) + 1):   # cut the sub-message, the outer length follows
            parts = [whole[:k]]
            out.append(("b/%s.cut%d" % (which, k), build(**{which: parts})))
        lp, lo, _ = sub_span(which)
        for n in range(len(S) - lo + 3):   # the outer length alone, from 0 to two past the end of S
            b = bytearray(S)
            b[lp] = n
            out.append(("b/%s.len%d" % (which, n), bytes(b)))
    return out


# ---- (c) varints -----------------------------------------------------------
def encodings(v):
    """(name, bytes) encodings of a varint whose seed value is v."""
    out = [("n1", vint(v & 0x7F))]
    out += [("n%d" % n, vint(v | (1 << (7 * (n - 1))))) for n in range(2, 11)]   # minimal forms of 2..10 bytes
    out += [("pad%d" % n, vpad(v, n)) for n in range(len(vint(v)) + 1, 13)]      # 80...00 up to 12 bytes
    out += [("late11", vpad(v, 11, 0x7F)), ("late12", vpad(v, 12, 0x55)),         # bits at shifts 70 and 77
            ("late12b", vpad(v, 10)[:9] + bytes([0xFE, 0xFF, 0x7F]))]             # and 0x7e at shift 63
    out += [("ten%02x" % last, v10(v, last)) for last in (0x01, 0x02, 0x7F)]
    return out


def family_c():
    out = []
    for lv, i in VARINT_SITES + LENGTH_SITES:
        for name, enc in encodings(site(lv, i)[1]):
            out.append(("c/%s%d.val.%s" % (lv, i, name), with_site(lv, i, enc=enc)))
    for lv, i in KNOWN_SITES:
        for name, enc in encodings(site(lv, i)[0]):
            out.append(("c/%s%d.tag.%s" % (lv, i, name), with_site(lv, i, tagb=enc)))
    for lv, i in VARINT_SITES:   # the same field twice
        t, v, _ = site(lv, i)
        out.append(("c/%s%d.twice.disjoint" % (lv, i), put(lv, vint(t) + vint(1 << 40), i + 1)))
        out.append(("c/%s%d.twice.overlap" % (lv, i), put(lv, vint(t) + vint(v | 0x81), i + 1)))
        out.append(("c/%s%d.twice.truncated" % (lv, i), put(lv, vint(t) + b"\xff\xff")))   # partial bits stay
    for bit in range(28, 35):
        out.append(("c/ent0.type.bit%d" % bit, swap("ent", 0, b"\x08" + vint(1 << bit))))
        out.append(("c/ent0.type.bit%d+1" % bit, swap("ent", 0, b"\x08" + vint((1 << bit) | 1))))
    out.append(("c/ent0.type.minus1", swap("ent", 0, b"\x08" + vint(M64))))
    for name, enc in (("00", b"\x00"), ("01", b"\x01"), ("02", b"\x02"), ("8000", b"\x80\x00"),
                      ("2^63", v10(0, 0x01)), ("2^64", vpad(0, 11, 0x01))):
        out.append(("c/reject.%s" % name, swap("msg", 10, b"\x50" + enc)))
    out.append(("c/reject.true-then-false", put("msg", b"\x50\x00")))
    out.append(("c/reject.false-then-true", build(msg=seed("msg")[:10] + [b"\x50\x00", b"\x50\x02"])))
    return out


# ---- (d) lengths -----------------------------------------------------------
def _length_site(name):
    """A bytes field that is the last thing in its level: (level parts before
    it, tag bytes, payload, rebuild(level parts))."""
    if name in ("msg7", "msg9"):
        mk = (7, "ent") if name == "msg7" else (9, "snap")
        rest = [c for c in seed("msg") if c != mk]
        return rest, tag(mk[0], 2), b"".join(seed(mk[1])), lambda parts: build(msg=parts)
    if name == "ent.data":
        return seed("ent")[:3], b"\x22", b"abc", lambda parts: build(ent=parts)
    if name == "snap.data":
        return seed("snap")[1:], b"\x0a", b"snap", lambda parts: build(snap=parts)
    lv = name.split(".")[1]   # unknown.<level>: field 15, bytes
    return seed(lv), b"\x7a", b"xyz", lambda parts: build(**{lv: parts})


def _level_len(parts):
    return len(build(msg=parts)) if any(isinstance(c, tuple) for c in parts) else len(b"".join(parts))


def family_d():
    out = []
    for name in ("msg7", "msg9", "ent.data", "snap.data", "unknown.msg", "unknown.ent", "unknown.snap"):
        before, tg, payload, rebuild = _length_site(name)
        at = _level_len(before) + len(tg)   # where the length prefix starts in its level
        r = len(payload)
        lengths = [("to-l", r), ("to-l+1", r + 1), ("0", 0), ("2^31", 1 << 31), ("2^32", 1 << 32),
                   ("2^63-1-i", (1 << 63) - 1 - (at + 9)), ("2^63-i", (1 << 63) - (at + 9)), ("2^63", 1 << 63)]
        lengths += [("2^64-%d" % k, (1 << 64) - k) for k in range(1, 17)]
        for ln, v in lengths:
            out.append(("d/%s.%s" % (name, ln), rebuild(before + [tg + vint(v) + payload])))
    # The same lengths behind values the device collects in a second walk of
    # the sub-message (pb_each): a split Entry.Data, the Snapshot's Nodes.  The
    # first walk refuses the length; the second must stop there too, and not
    # step to tag + skippy, which for these lengths lies far outside the body.
    for lv, head in (("ent", seed("ent")[:3] + [fb(4, b"he"), fb(4, b"ad")]), ("snap", seed("snap"))):
        at = len(b"".join(head)) + 1
        for fn in (15, 4 if lv == "ent" else 1):
            for ln, v in [("2^63-1-i", (1 << 63) - 1 - (at + 9)), ("2^63-i", (1 << 63) - (at + 9)),
                          ("2^63", 1 << 63), ("2^64-1", M64), ("2^64-11", (1 << 64) - 11), ("2^62", 1 << 62)]:
                out.append(("d/%s.second-walk.fn%d.%s" % (lv, fn, ln), build(**{lv: head + [tag(fn, 2) + vint(v) + b"xyz"]})))
    for lv in LEVELS:   # unknown fixed-width fields that run past the end of their level
        for k in range(9):
            out.append(("d/fixed64.%s.%d" % (lv, k), put(lv, tag(15, 1) + b"\x11" * k)))
        for k in range(5):
            out.append(("d/fixed32.%s.%d" % (lv, k), put(lv, tag(15, 5) + b"\x22" * k)))
    return out


# ---- (e) tags --------------------------------------------------------------
def _payload(wt):
    """A well-formed body for an unknown field of a simple wire type."""
    return {0: vint(300), 1: b"\x01" * 8, 2: b"\x02pq", 5: b"\x05" * 4}.get(wt, b"")


ALIAS_K = (1, 3, 1 << 28)   # wire |= k << 35: bits int32(wire >> 3) drops


def family_e():
    out = []
    for lv in LEVELS:
        for fn in (0, 11, 15, 16, 1 << 28, (1 << 31) | 1, (1 << 31) | 7):
            for wt in (0, 1, 2, 5):
                out.append(("e/%s.fn%x.wt%d" % (lv, fn, wt), put(lv, tag(fn, wt) + _payload(wt))))
                out.append(("e/%s.fn%x.wt%d.mid" % (lv, fn, wt), put(lv, tag(fn, wt) + _payload(wt), 1)))
        for wt in range(8):   # non-minimal tags on unknown fields: Skip restarts inside the tag
            for n in (2, 3, 10, 11):
                out.append(("e/%s.unknown.wt%d.pad%d" % (lv, wt, n),
                            put(lv, vpad((15 << 3) | wt, n) + _payload(wt) + b"\x00\x00")))
    # A padded tag in front of values the device collects in a second walk of
    # the sub-message (Nodes, RemovedNodes, the segments of a split Data).
    # After a padded UNKNOWN tag Skip restarts on the tag's last byte, 00: with
    # 02 behind it that is field 0, varint 2, whatever wire type the tag
    # named, and the fields that follow are the message's own.  A padded or
    # aliased KNOWN tag is read whole.  Both walks must frame what follows
    # alike, or the second loses or invents values.
    def followed(lv, chunk):
        if lv == "snap":
            return build(snap=seed("snap") + [chunk, fv(2, 5), fv(5, 6), fb(1, b"more")])
        return build(ent=seed("ent")[:3] + [fb(4, b"he"), fb(4, b"ad"), chunk, fb(4, b"z")])

    for lv in ("snap", "ent"):
        for wt in range(8):
            for n in (2, 3, 10, 11):
                out.append(("e/%s.second-walk.wt%d.pad%d" % (lv, wt, n), followed(lv, vpad((15 << 3) | wt, n) + b"\x02")))
            out.append(("e/%s.second-walk.wt%d.payload" % (lv, wt),
                        followed(lv, vpad((15 << 3) | wt, 3) + _payload(wt) + b"\x00")))
        known = (3 << 3, vint(7)) if lv == "snap" else (2 << 3, vint(9))
        for n in (2, 3, 10, 11):
            out.append(("e/%s.second-walk.known.pad%d" % (lv, n), followed(lv, vpad(known[0], n) + known[1])))
        for k in ALIAS_K:
            out.append(("e/%s.second-walk.known.alias%x" % (lv, k), followed(lv, vint(known[0] | (k << 35)) + known[1])))
    for lv, i in KNOWN_SITES:
        t, v, d = site(lv, i)
        for k in ALIAS_K:
            out.append(("e/%s%d.alias%x" % (lv, i, k), with_site(lv, i, tagb=vint(t | (k << 35)))))
        for wt in range(8):
            out.append(("e/%s%d.wt%d" % (lv, i, wt), with_site(lv, i, tagb=vint((t & ~7) | wt))))
        for n in (2, 3, 10, 11):
            out.append(("e/%s%d.pad%d" % (lv, i, n), with_site(lv, i, tagb=vpad(t, n))))
    return out


# ---- (f) groups ------------------------------------------------------------
def group(inner=b"", fn=11, depth=1):
    """`depth` start-group tags, inner, `depth` end-group tags."""
    return tag(fn, 3) * depth + inner + tag(fn, 4) * depth


NEST = list(range(1, MAX_NESTED_STARTS + 3))   # start-group tags nested: 1 .. two past the boundary


def family_f():
    out = []
    for lv in LEVELS:
        for wt in (0, 1, 2, 5, 6, 7):
            out.append(("f/%s.holds.wt%d" % (lv, wt), put(lv, group(tag(12, wt) + _payload(wt)))))
        out.append(("f/%s.empty" % lv, put(lv, group())))
        out.append(("f/%s.empty.mid" % lv, put(lv, group(), 1)))
        out.append(("f/%s.end-only" % lv, put(lv, tag(11, 4))))
        out.append(("f/%s.end-only.mid" % lv, put(lv, tag(11, 4), 1)))
        out.append(("f/%s.unclosed" % lv, put(lv, tag(11, 3) + fv(12, 5))))
        out.append(("f/%s.unclosed.mid" % lv, put(lv, tag(11, 3) + fv(12, 5), 1)))
        out.append(("f/%s.two-groups" % lv, put(lv, group(fv(12, 1)) + group(group(), depth=2))))
        for n in NEST:
            out.append(("f/%s.nest%d" % (lv, n), put(lv, group(fv(12, n), depth=n))))
            out.append(("f/%s.nest%d.mid" % (lv, n), put(lv, group(depth=n), 1)))
        # siblings at the boundary: frames are popped and pushed again, the depth never passes it
        out.append(("f/%s.siblings" % lv, put(lv, group(group(depth=MAX_PUSHES) * 2 + fv(12, 7)))))
        # an inner bytes field whose length sends Skip back: to itself (k = 11: a
        # cycle), to the group's own start tag (12: the call re-enters itself),
        # before the slice (13..: index < 0) or a few bytes forward (8..10)
        for k in range(8, 17):
            out.append(("f/%s.back%d" % (lv, k), put(lv, tag(11, 3) + b"\x7a" + vint((1 << 64) - k) + tag(11, 4))))
        # the same cycle led through a nested group (k = 13 lands on the inner
        # group's start tag at local 1).  Every round pushes and pops a frame,
        # so only a walker that gives the outer frame its own loop count back
        # on the pop ever sees the outer loop run out of positions.  Bounded
        # by construction: at most l + 2 rounds of two iterations each.
        out.append(("f/%s.back-over-group" % lv,
                    put(lv, tag(11, 3) + group() + b"\x7a" + vint((1 << 64) - 13) + tag(11, 4))))
        out.append(("f/%s.known-inside" % lv, put(lv, group(fv(1, 99) + fb(4, b"zz") + fb(1, b"yy")))))
    for lv, fn, i in (("ent", 4, 3), ("snap", 1, 0)):   # a bytes field split by a group: pb_each steps over it
        for n in (1, 2, MAX_NESTED_STARTS, MAX_NESTED_STARTS + 1):
            parts = seed(lv)
            parts[i:i + 1] = [fb(fn, b"he"), group(fv(12, 3), depth=n), fb(fn, b"ad")]
            out.append(("f/%s.split.nest%d" % (lv, n), build(**{lv: parts})))
    return out


# ---- (g) seeded mutation ---------------------------------------------------
MUTATION_BYTES = (0x0B, 0x0C, 0x5B, 0x5C, 0x80, 0xFF, 0x7A, 0x3A, 0x4A, 0x01)
N_MUTATIONS = 20000


def family_g():
    rng = random.Random(0x6d7367)
    out = []
    for k in range(N_MUTATIONS):
        b = bytearray(S)
        for _ in range(rng.randrange(1, 4)):
            op = rng.randrange(3)
            if op == 0 and b:
                b[rng.randrange(len(b))] = rng.choice(MUTATION_BYTES)
            elif op == 1 and b:
                del b[rng.randrange(len(b))]
            else:
                b.insert(rng.randrange(len(b) + 1), rng.choice(MUTATION_BYTES))
        out.append(("g/%d" % k, bytes(b)))
    return out


FAMILIES = dict(a=family_a, b=family_b, c=family_c, d=family_d, e=family_e, f=family_f, g=family_g)
STRUCTURED = "abcdef"
_cache = {}


def family(k):
    if k not in _cache:
        _cache[k] = FAMILIES[k]()
    return _cache[k]
