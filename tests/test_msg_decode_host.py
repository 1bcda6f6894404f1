"""The two references for raftpb.Message.Unmarshal against each other (CPU).

tests/pb_model.py restates the generated Go code field by field in Python;
the oracle's or_message_unmarshal runs Entry and Snapshot through a table
engine in C.  Neither is pinned by a Go vector (the reference has none for
Message), so they pin each other over the whole lattice of
tests/msg_decode_cases.py, and this module asserts that the lattice reaches
what it is for: every verdict class, each way of never terminating, a bounds
panic at every level, the device walker's nesting boundary from both sides.
The same bodies then go to the device (tests/test_gpu_msg_decode_edges.py),
so the iteration cap on proto.Skip's loops is asserted here too.
"""
import collections

import pytest

import msg_decode_cases as K
import pb_model as P
from oracle import oracle as O

OKS = (O.OK, O.ERR_UNEXPECTED_EOF, O.ERR_WRONG_TYPE)
MSG_KEYS = ("type", "to", "from_", "term", "log_term", "index", "commit", "reject", "unrec", "unrec_len")
ENT_KEYS = ("type", "term", "index", "data", "unrec", "unrec_len")
SNAP_KEYS = ("data", "index", "term", "n_nodes", "n_removed", "unrec", "unrec_len", "nodes", "removed")
SKIP_ITER_CAP = 4096

# The oracle's verdicts per family: {status: bodies}.
HISTOGRAM = {
    "a": {0: 4294, 2: 1976, 7: 2704},
    "b": {0: 65, 2: 42, 7: 40},
    "c": {0: 1126, 2: 37, 33: 12},
    "d": {0: 50, 2: 53, 7: 21, 33: 105, 37: 5},
    "e": {0: 518, 2: 36, 7: 119},
    "f": {0: 162, 2: 4, 7: 10, 33: 12, 37: 9},
    "g": {0: 3664, 2: 5648, 7: 10688},
}
G_DROPPED = 0   # bodies of family (g) over the iteration cap, which the device never sees


def same_fields(a, b):
    """The first field in which two decode results differ, or None."""
    for k in MSG_KEYS:
        if a[k] != b[k]:
            return k
    if len(a["ents"]) != len(b["ents"]):
        return "len(ents)"
    for i, (x, y) in enumerate(zip(a["ents"], b["ents"])):
        for k in ENT_KEYS:
            if x[k] != y[k]:
                return "ents[%d].%s" % (i, k)
    for k in SNAP_KEYS:
        if a["snap"][k] != b["snap"][k]:
            return "snap." + k
    return None


_both = {}


def both(body):
    if body not in _both:
        _both[body] = (P.message_unmarshal(body), O.message_unmarshal(body))
    return _both[body]


@pytest.fixture(scope="module")
def by_name():
    return {name: body for f in K.FAMILIES for name, body in K.family(f)}


@pytest.mark.parametrize("fam", list(K.FAMILIES))
def test_model_and_oracle_agree(fam):
    bad = []
    hist = collections.Counter()
    for name, body in K.family(fam):
        m, o = both(body)
        hist[o["status"]] += 1
        why = "status" if m["status"] != o["status"] else same_fields(m, o) if o["status"] in OKS else None
        if why:
            bad.append((name, why, body.hex()))
    print(fam, len(K.family(fam)), dict(sorted(hist.items())))
    assert not bad, (len(bad), bad[:5])
    assert dict(hist) == HISTOGRAM[fam]


def test_seed_is_what_the_lattice_assumes():
    m, o = both(K.S)
    assert len(K.S) <= 96 and o["status"] == O.OK and same_fields(m, o) is None
    assert all(o[k] for k in ("type", "to", "from_", "term", "log_term", "index", "commit", "reject"))
    assert o["to"] >= 0x80 and o["ents"][0]["index"] >= 0x80 and o["snap"]["index"] >= 0x80   # multi-byte, each level
    assert [(e["type"], e["data"]) for e in o["ents"]] == [(1, b"abc"), (0, None)]
    s = o["snap"]
    assert s["data"] and len(s["nodes"]) == 2 and s["index"] and s["term"] and len(s["removed"]) == 1
    names = [n for f in K.FAMILIES for n, _ in K.family(f)]
    assert len(names) == len(set(names))
    assert len(K.family("g")) == 20000


def test_every_verdict_class_and_each_way_to_it(by_name):
    seen = {both(b)[1]["status"] for f in K.FAMILIES for _, b in K.family(f)}
    assert seen == {O.OK, O.ERR_UNEXPECTED_EOF, O.ERR_WRONG_TYPE, O.PANIC_BOUNDS, O.NONTERMINATING}

    def verdict(name):
        m, o = both(by_name[name])
        return o["status"], m["why"]

    # skippy == 0: Skip's local index is 11 after a one-byte tag and a ten-byte length, so k = 11
    assert verdict("d/unknown.msg.2^64-11") == (O.NONTERMINATING, "msg:skippy")
    assert verdict("d/unknown.ent.2^64-11") == (O.NONTERMINATING, "ent:skippy")    # inside an Entry: it propagates
    assert verdict("d/unknown.snap.2^64-11") == (O.NONTERMINATING, "snap:skippy")
    for k in range(1, 17):
        if k != 11:
            assert verdict("d/unknown.msg.2^64-%d" % k)[0] != O.NONTERMINATING
    for lv in K.LEVELS:
        assert verdict("f/%s.back11" % lv) == (O.NONTERMINATING, lv + ":cycle")       # the group loop revisits its field
        assert verdict("f/%s.back12" % lv) == (O.NONTERMINATING, lv + ":recursion")   # the group re-enters itself
        assert verdict("f/%s.back13" % lv) == (O.PANIC_BOUNDS, lv + ":index")         # data[-1]
        m, o = both(by_name["f/%s.back-over-group" % lv])   # the cycle passes through a nested group
        assert (o["status"], m["why"], m["pushes"]) == (O.NONTERMINATING, lv + ":cycle", 1)
        assert m["skip_iters"] <= 2 * (len(by_name["f/%s.back-over-group" % lv]) + 2)
        assert len(by_name["f/%s.back11" % lv]) < 128 and len(by_name["f/%s.back-over-group" % lv]) < 128
    # a bounds panic at each level: post < index in a known bytes field
    assert verdict("d/msg7.2^63") == (O.PANIC_BOUNDS, "msg:slice")
    assert verdict("d/msg9.2^64-1") == (O.PANIC_BOUNDS, "msg:slice")
    assert verdict("d/ent.data.2^63") == (O.PANIC_BOUNDS, "ent:slice")
    assert verdict("d/snap.data.2^64-16") == (O.PANIC_BOUNDS, "snap:slice")
    assert verdict("d/msg7.2^63-1-i")[0] == O.ERR_UNEXPECTED_EOF and verdict("d/msg7.2^63-i")[0] == O.PANIC_BOUNDS
    assert verdict("d/msg7.to-l")[0] == O.OK and verdict("d/msg7.to-l+1")[0] == O.ERR_UNEXPECTED_EOF


def test_nesting_reaches_the_device_boundary_from_both_sides(by_name):
    assert K.MAX_PUSHES == K.PB_SKIP_DEPTH and K.MAX_NESTED_STARTS == K.MAX_PUSHES + 1
    for lv in K.LEVELS:
        for n in K.NEST:
            m, o = both(by_name["f/%s.nest%d" % (lv, n)])
            assert o["status"] == O.OK and m["pushes"] == n - 1   # n start tags nested: n - 1 pushes
        assert both(by_name["f/%s.siblings" % lv])[0]["pushes"] == K.MAX_PUSHES
    assert K.NEST[-1] - 1 == K.MAX_PUSHES + 2
    # past the boundary only bodies Go accepts: the device answers those, and only those, with 48
    for f in K.FAMILIES:
        for name, b in K.family(f):
            m, o = both(b)
            assert m["pushes"] <= K.MAX_PUSHES or o["status"] == O.OK, name


def test_go_quirks_are_exercised(by_name):
    seed = both(K.S)[1]
    # int32(wire >> 3): a tag with bits above bit 34 is still the known field
    for lv, i in K.KNOWN_SITES:
        for k in K.ALIAS_K:
            body = by_name["e/%s%d.alias%x" % (lv, i, k)]
            assert len(body) > len(K.S) and same_fields(both(body)[1], seed) is None
    # Entry.Type is an int32: what a 64-bit-clean reading of the same varint would give is something else
    for bit in range(28, 35):
        e = both(by_name["c/ent0.type.bit%d+1" % bit])[1]["ents"][0]
        clean = (1 << bit) | 1
        assert e["type"] == P.i32(clean) and (e["type"] != clean) == (bit >= 31)
    assert both(by_name["c/ent0.type.minus1"])[1]["ents"][0]["type"] == -1
    # bits shifted past 64 vanish; a clean reader would see 2^64 + ... or reject eleven bytes
    assert both(by_name["c/msg1.val.late12"])[1]["to"] == seed["to"]
    assert both(by_name["c/msg1.val.ten02"])[1]["to"] == seed["to"]            # 2 << 63 == 0
    assert both(by_name["c/msg1.val.ten7f"])[1]["to"] == seed["to"] | 1 << 63
    # a truncated varint leaves its partial bits: ff ff is 0x3fff so far
    o = both(by_name["c/msg1.twice.truncated"])[1]
    assert o["status"] == O.ERR_UNEXPECTED_EOF and o["to"] == seed["to"] | 0x3FFF
    o = both(by_name["c/ent1.twice.truncated"])[1]
    assert o["status"] == O.OK and o["ents"][0]["term"] == 5 | 0x3FFF             # the Entry's error is dropped
    o = both(by_name["c/snap3.twice.truncated"])[1]
    assert o["status"] == O.ERR_UNEXPECTED_EOF and o["snap"]["nodes"] == [1, 2]     # the Snapshot's is not
    # Reject is assigned
    assert [both(by_name["c/reject." + n])[1]["reject"] for n in
            ("00", "01", "02", "8000", "2^63", "2^64", "true-then-false", "false-then-true")] == \
        [False, True, True, False, True, False, False, True]
    # sizeOfWire comes from the tag's value: after a padded tag Skip restarts on its last byte
    o = both(by_name["e/msg.unknown.wt0.pad3"])[1]
    assert o["status"] == O.OK and o["unrec"] == b"\x00\xac\x02" + b"\x00\x00"
    # what follows a padded tag: after an unknown one Skip restarts on the tag's last byte (00, then 02),
    # whatever its wire type, and the Nodes, RemovedNodes and Data segments behind it are the message's own
    for wt in range(8):
        for n in (2, 3, 10, 11):
            o = both(by_name["e/snap.second-walk.wt%d.pad%d" % (wt, n)])[1]
            s = o["snap"]
            assert (o["status"], s["nodes"], s["removed"], s["data"], s["unrec"]) == \
                (O.OK, [1, 2, 5], [9, 6], b"snapmore", b"\x00\x02")
            o = both(by_name["e/ent.second-walk.wt%d.pad%d" % (wt, n)])[1]
            assert (o["status"], o["ents"][0]["data"], o["ents"][0]["unrec"]) == (O.OK, b"headz", b"\x00\x02")
    for n in ("pad2", "pad3", "pad10", "pad11", "alias1", "alias3", "alias10000000"):
        o = both(by_name["e/snap.second-walk.known." + n])[1]
        assert (o["status"], o["snap"]["nodes"], o["snap"]["index"], o["snap"]["unrec"]) == (O.OK, [1, 2, 5], 200 | 7, None)
        o = both(by_name["e/ent.second-walk.known." + n])[1]
        assert (o["ents"][0]["data"], o["ents"][0]["term"], o["ents"][0]["unrec"]) == (b"headz", 5 | 9, None)
    # a known field number inside a group stays unrecognized
    for lv in K.LEVELS:
        o = both(by_name["f/%s.known-inside" % lv])[1]
        t = dict(msg=o, ent=o["ents"][0] if o["ents"] else None, snap=o["snap"])[lv]
        assert o["status"] == O.OK and t["unrec"] == K.group(K.fv(1, 99) + K.fb(4, b"zz") + K.fb(1, b"yy"))
        assert o["type"] == seed["type"] and o["ents"][0]["data"] == b"abc" and o["snap"]["data"] == b"snap"
    # a bytes field split by a group: the halves concatenate
    assert both(by_name["f/ent.split.nest1"])[1]["ents"][0]["data"] == b"head"
    assert both(by_name["f/snap.split.nest%d" % K.MAX_NESTED_STARTS])[1]["snap"]["data"] == b"head"


def device_bodies(fam):
    """The bodies of a family that go to the device: those within the iteration cap."""
    return [(n, b) for n, b in K.family(fam) if both(b)[0]["skip_iters"] <= SKIP_ITER_CAP]


def test_iteration_cap():
    """No lane runs long: pb_skip's loops have the model's shape and bound, and
    the model's count is small for every body sent.  A condition, not a
    measurement."""
    for f in K.STRUCTURED:
        assert len(device_bodies(f)) == len(K.family(f)), f
    assert len(K.family("g")) - len(device_bodies("g")) == G_DROPPED
    assert G_DROPPED * 100 <= len(K.family("g"))
    worst = max(both(b)[0]["skip_iters"] for f in K.FAMILIES for _, b in K.family(f))
    print("most Skip group-loop iterations in one body:", worst)
    assert worst <= 66   # the figure DESIGN quotes
