"""A second reference for the /raft ingress decode, beside the C oracle.

Plain-Python restatements of raftpb.Message.Unmarshal (raft/raftpb/raft.pb.go:
407-617), Entry.Unmarshal (:170-278), Snapshot.Unmarshal (:279-406) and
proto.Skip (third_party/code.google.com/p/gogoprotobuf/proto/skip_gogo.go:
33-116), written field by field in the order the generated code goes, not as
a table engine (the oracle is one).  Go's `int`, `uint64` and `int32` are
Python integers under explicit masks; an index below zero is a bounds panic,
never Python's wrap-around; Skip's groups recurse as Go's do.

`message_unmarshal(b)` returns the dict `oracle.message_unmarshal` returns,
plus what the decode tests need to know about the run:

  skip_iters  iterations of Skip's group loops, summed over the call
  pushes      the deepest chain of Skip calls that entered a group from
              inside a group (0: no group, or groups not nested)
  why         for a panic or a never-terminating run, where it arose:
              "<level>:<what>", level one of msg / ent / snap

A run that never terminates is recognised as the oracle and the device
recognise it: a group loop that runs more often than its slice has positions
revisits one and so cycles; a group met at local position 0 is the call that
is already running; an unknown field Skip measures as 0 bytes long leaves the
caller's index where it was.
"""

OK, ERR_UNEXPECTED_EOF, ERR_WRONG_TYPE, PANIC_BOUNDS, NONTERMINATING = 0, 2, 7, 33, 37

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1


def i64(x):
    """Go's int: the low 64 bits, signed."""
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def i32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def shl64(x, s):
    return (x << s) & M64 if s < 64 else 0


def shl32(x, s):
    return (x << s) & M32 if s < 32 else 0


class GoPanic(Exception):
    pass


class NeverReturns(Exception):
    pass


class Run:
    """What one Message.Unmarshal call did besides its result."""

    def __init__(self):
        self.skip_iters = 0
        self.pushes = 0
        self.level = "msg"


def at(data, index):
    """data[index]"""
    if index < 0 or index >= len(data):
        raise GoPanic("index")
    return data[index]


def cut(data, lo, hi):
    """data[lo:hi]"""
    if lo < 0 or hi < lo or hi > len(data):
        raise GoPanic("slice")
    return data[lo:hi]


def skip(data, run, pushes=0):
    """proto.Skip: (n, err)."""
    l = len(data)
    index = 0
    while index < l:
        wire = 0
        shift = 0
        while True:
            if index >= l:
                return 0, ERR_UNEXPECTED_EOF
            b = at(data, index)
            index += 1
            wire |= shl64(b & 0x7F, shift)
            if b < 0x80:
                break
            shift += 7
        wire_type = wire & 0x7
        if wire_type == 0:
            while True:
                if index >= l:
                    return 0, ERR_UNEXPECTED_EOF
                index += 1
                if at(data, index - 1) < 0x80:
                    break
            return index, None
        if wire_type == 1:
            index = i64(index + 8)
            return index, None
        if wire_type == 2:
            length = 0
            shift = 0
            while True:
                if index >= l:
                    return 0, ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                length = i64(length | shl64(b & 0x7F, shift))
                if b < 0x80:
                    break
                shift += 7
            index = i64(index + length)
            return index, None
        if wire_type == 3:
            run.pushes = max(run.pushes, pushes)
            iters = 0
            while True:
                iters += 1
                run.skip_iters += 1
                if iters > l + 1:
                    raise NeverReturns("cycle")
                wire = 0
                start = index
                shift = 0
                while True:
                    if index >= l:
                        return 0, ERR_UNEXPECTED_EOF
                    b = at(data, index)
                    index += 1
                    wire |= shl64(b & 0x7F, shift)
                    if b < 0x80:
                        break
                    shift += 7
                inner_type = wire & 0x7
                if inner_type == 4:
                    break
                if start == 0:
                    raise NeverReturns("recursion")   # Skip(data[0:]) is this very call
                nxt, err = skip(cut(data, start, l), run, pushes + (1 if inner_type == 3 else 0))
                if err is not None:
                    return 0, err
                index = i64(start + nxt)
            return index, None
        if wire_type == 4:
            return index, None
        if wire_type == 5:
            index = i64(index + 4)
            return index, None
        return 0, ERR_WRONG_TYPE
    raise GoPanic("unreachable")


def _unknown(data, index, wire, l, run):
    """The default arm the three Unmarshals share word for word: (index, err,
    the bytes appended to XXX_unrecognized)."""
    size_of_wire = 0
    while True:
        size_of_wire += 1
        wire >>= 7
        if wire == 0:
            break
    index -= size_of_wire
    skippy, err = skip(cut(data, index, l), run)
    if err is not None:
        return index, err, b""
    if i64(index + skippy) > l:
        return index, ERR_UNEXPECTED_EOF, b""
    seg = cut(data, index, i64(index + skippy))
    if skippy == 0:
        raise NeverReturns("skippy")
    return i64(index + skippy), None, seg


def _wire(data, index, l):
    """The tag loop every Unmarshal opens with: (wire, index) or (None, index) at EOF."""
    wire = 0
    shift = 0
    while True:
        if index >= l:
            return None, index
        b = at(data, index)
        index += 1
        wire |= shl64(b & 0x7F, shift)
        if b < 0x80:
            return wire, index
        shift += 7


def entry_unmarshal(data, m, run):
    """Entry.Unmarshal into the dict m: err or None."""
    l = len(data)
    index = 0
    while index < l:
        wire, index = _wire(data, index, l)
        if wire is None:
            return ERR_UNEXPECTED_EOF
        field_num = i32(wire >> 3)
        wire_type = wire & 0x7
        if field_num == 1:
            if wire_type != 0:
                return ERR_WRONG_TYPE
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                m["type"] = i32(m["type"] | shl32(b & 0x7F, shift))
                if b < 0x80:
                    break
                shift += 7
        elif field_num == 2:
            if wire_type != 0:
                return ERR_WRONG_TYPE
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                m["term"] |= shl64(b & 0x7F, shift)
                if b < 0x80:
                    break
                shift += 7
        elif field_num == 3:
            if wire_type != 0:
                return ERR_WRONG_TYPE
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                m["index"] |= shl64(b & 0x7F, shift)
                if b < 0x80:
                    break
                shift += 7
        elif field_num == 4:
            if wire_type != 2:
                return ERR_WRONG_TYPE
            byte_len = 0
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                byte_len = i64(byte_len | shl64(b & 0x7F, shift))
                if b < 0x80:
                    break
                shift += 7
            post_index = i64(index + byte_len)
            if post_index > l:
                return ERR_UNEXPECTED_EOF
            seg = cut(data, index, post_index)
            if seg:
                m["data"] = (m["data"] or b"") + seg
            index = post_index
        else:
            index, err, seg = _unknown(data, index, wire, l, run)
            if err is not None:
                return err
            m["unrec"] = (m["unrec"] or b"") + seg
    return None


def snapshot_unmarshal(data, m, run):
    """Snapshot.Unmarshal into the dict m (it accumulates over calls): err or None."""
    l = len(data)
    index = 0
    while index < l:
        wire, index = _wire(data, index, l)
        if wire is None:
            return ERR_UNEXPECTED_EOF
        field_num = i32(wire >> 3)
        wire_type = wire & 0x7
        if field_num == 1:
            if wire_type != 2:
                return ERR_WRONG_TYPE
            byte_len = 0
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                byte_len = i64(byte_len | shl64(b & 0x7F, shift))
                if b < 0x80:
                    break
                shift += 7
            post_index = i64(index + byte_len)
            if post_index > l:
                return ERR_UNEXPECTED_EOF
            seg = cut(data, index, post_index)
            if seg:
                m["data"] = (m["data"] or b"") + seg
            index = post_index
        elif field_num == 2:
            if wire_type != 0:
                return ERR_WRONG_TYPE
            v = 0
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                v |= shl64(b & 0x7F, shift)
                if b < 0x80:
                    break
                shift += 7
            m["nodes"].append(v)
        elif field_num == 3:
            if wire_type != 0:
                return ERR_WRONG_TYPE
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                m["index"] |= shl64(b & 0x7F, shift)
                if b < 0x80:
                    break
                shift += 7
        elif field_num == 4:
            if wire_type != 0:
                return ERR_WRONG_TYPE
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                m["term"] |= shl64(b & 0x7F, shift)
                if b < 0x80:
                    break
                shift += 7
        elif field_num == 5:
            if wire_type != 0:
                return ERR_WRONG_TYPE
            v = 0
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                v |= shl64(b & 0x7F, shift)
                if b < 0x80:
                    break
                shift += 7
            m["removed"].append(v)
        else:
            index, err, seg = _unknown(data, index, wire, l, run)
            if err is not None:
                return err
            m["unrec"] = (m["unrec"] or b"") + seg
    return None


def _message(data, m, run):
    l = len(data)
    index = 0
    while index < l:
        wire, index = _wire(data, index, l)
        if wire is None:
            return ERR_UNEXPECTED_EOF
        field_num = i32(wire >> 3)
        wire_type = wire & 0x7
        if field_num == 1:
            if wire_type != 0:
                return ERR_WRONG_TYPE
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                m["type"] |= shl64(b & 0x7F, shift)
                if b < 0x80:
                    break
                shift += 7
        elif field_num == 2:
            if wire_type != 0:
                return ERR_WRONG_TYPE
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                m["to"] |= shl64(b & 0x7F, shift)
                if b < 0x80:
                    break
                shift += 7
        elif field_num == 3:
            if wire_type != 0:
                return ERR_WRONG_TYPE
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                m["from_"] |= shl64(b & 0x7F, shift)
                if b < 0x80:
                    break
                shift += 7
        elif field_num == 4:
            if wire_type != 0:
                return ERR_WRONG_TYPE
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                m["term"] |= shl64(b & 0x7F, shift)
                if b < 0x80:
                    break
                shift += 7
        elif field_num == 5:
            if wire_type != 0:
                return ERR_WRONG_TYPE
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                m["log_term"] |= shl64(b & 0x7F, shift)
                if b < 0x80:
                    break
                shift += 7
        elif field_num == 6:
            if wire_type != 0:
                return ERR_WRONG_TYPE
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                m["index"] |= shl64(b & 0x7F, shift)
                if b < 0x80:
                    break
                shift += 7
        elif field_num == 7:
            if wire_type != 2:
                return ERR_WRONG_TYPE
            msglen = 0
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                msglen = i64(msglen | shl64(b & 0x7F, shift))
                if b < 0x80:
                    break
                shift += 7
            post_index = i64(index + msglen)
            if post_index > l:
                return ERR_UNEXPECTED_EOF
            e = dict(type=0, term=0, index=0, data=None, unrec=None)
            m["ents"].append(e)
            sub = cut(data, index, post_index)
            run.level = "ent"
            entry_unmarshal(sub, e, run)   # the error is dropped; a panic is not
            run.level = "msg"
            index = post_index
        elif field_num == 8:
            if wire_type != 0:
                return ERR_WRONG_TYPE
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                m["commit"] |= shl64(b & 0x7F, shift)
                if b < 0x80:
                    break
                shift += 7
        elif field_num == 9:
            if wire_type != 2:
                return ERR_WRONG_TYPE
            msglen = 0
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                msglen = i64(msglen | shl64(b & 0x7F, shift))
                if b < 0x80:
                    break
                shift += 7
            post_index = i64(index + msglen)
            if post_index > l:
                return ERR_UNEXPECTED_EOF
            sub = cut(data, index, post_index)
            run.level = "snap"
            err = snapshot_unmarshal(sub, m["snap"], run)
            if err is not None:
                return err
            run.level = "msg"
            index = post_index
        elif field_num == 10:
            if wire_type != 0:
                return ERR_WRONG_TYPE
            v = 0
            shift = 0
            while True:
                if index >= l:
                    return ERR_UNEXPECTED_EOF
                b = at(data, index)
                index += 1
                v = i64(v | shl64(b & 0x7F, shift))
                if b < 0x80:
                    break
                shift += 7
            m["reject"] = v != 0
        else:
            index, err, seg = _unknown(data, index, wire, l, run)
            if err is not None:
                return err
            m["unrec"] = (m["unrec"] or b"") + seg
    return None


def message_unmarshal(b):
    """Message.Unmarshal(b) on a zero Message: the oracle's dict, and the run's record."""
    b = bytes(b)
    run = Run()
    m = dict(type=0, to=0, from_=0, term=0, log_term=0, index=0, commit=0, reject=False, ents=[], unrec=None,
             snap=dict(data=None, index=0, term=0, nodes=[], removed=[], unrec=None))
    why = None
    try:
        err = _message(b, m, run)
        status = OK if err is None else err
    except GoPanic as e:
        status, why = PANIC_BOUNDS, "%s:%s" % (run.level, e)
    except NeverReturns as e:
        status, why = NONTERMINATING, "%s:%s" % (run.level, e)
    for e in m["ents"]:
        e["unrec_len"] = len(e["unrec"] or b"")
    s = m["snap"]
    s.update(n_nodes=len(s["nodes"]), n_removed=len(s["removed"]), unrec_len=len(s["unrec"] or b""))
    m.update(status=status, unrec_len=len(m["unrec"] or b""), skip_iters=run.skip_iters, pushes=run.pushes, why=why)
    return m
