"""The host side of the batched raftpb.Message encode (no GPU): the ABI's
struct sizes and symbols, emsg_encode_size against the oracle's Marshal on
the width and length lattices, its saturation, and the argument check that
needs no device."""
import ctypes as C

from etcd_amd import _lib as L
from etcd_amd import raftmsg as M

import msg_encode_cases as K


def test_abi_sizes_and_symbols():
    assert C.sizeof(L.OutMsg) == L.lib.emsg_out_size() == 144
    assert C.sizeof(L.Encoded) == L.lib.emsg_encoded_size() == 16
    for name in ("emsg_encode_batch_device", "emsg_encode_size", "emsg_encode_tile_bytes", "emsg_out_size",
                 "emsg_encoded_size"):
        assert name in L.header_symbols() and hasattr(L.lib, name), name


def test_tile_bytes():
    t = L.lib.emsg_encode_tile_bytes()
    assert t > 0 and t % 16 == 0 and M.ENCODE_TILE == t


def test_empty_message_is_24_bytes():
    b = K.Batch()
    b.add_msg()
    assert b.expected()[0].hex() == "0800100018002000280030004000" + "4a060a0018002000" + "5000"
    assert b.host_size() == 24


def test_size_matches_oracle_on_lattices():
    for b in (K.width_lattice(), K.length_lattice(), K.shared_ranges(), K.rand_mix(60, 7)):
        want = [len(x) for x in b.expected()]
        assert b.host_size() == sum(want)
        # message by message, sharing the arrays
        msgs = b.c_msgs()
        for i, w in enumerate(want):
            one = (L.OutMsg * 1)(msgs[i])
            assert L.lib.emsg_encode_size(one, 1, b.c_ents(), len(b.ents), b.c_u64(), len(b.u64)) == w, i


def test_size_of_dicts():
    msgs = [dict(type=3, to=2, ents=[dict(term=1, index=2, data=b"abc"), dict(type=1, data=None)],
                 snap=dict(data=b"snap", index=9, term=1, nodes=[1, 300], removed=[7])), {}]
    b = K.Batch()
    e = b.add_entry(0, 1, 2, b"abc")
    b.add_entry(1, 0, 0, None)
    b.add_msg(type=3, to=2, ents=(e, 2), snap_data=b"snap", snap_index=9, snap_term=1, nodes=[1, 300], removed=[7])
    b.add_msg()
    assert M.encode_size(msgs) == b.total()


def test_size_saturates():
    b = K.Batch()
    b.add_msg(snap_data=(0, 1 << 63))
    b.add_msg(snap_data=(0, 1 << 63))
    assert b.host_size() == K.U64
    b = K.Batch()
    b.ents.append((0, 0, 0, 0, K.U64 - 8, 0))
    b.add_msg(ents=(0, 1))
    assert b.host_size() == K.U64
    # a range outside its array
    b = K.Batch()
    b.add_msg(ents=(1, 1))
    assert b.host_size() == K.U64
    b = K.Batch()
    b.add_msg(nodes_at=(K.U64, 2))
    assert b.host_size() == K.U64


def test_null_ctx_is_inval():
    tot = C.c_uint64(7)
    assert L.lib.emsg_encode_batch_device(None, None, 0, None, 0, None, 0, None, 0, None, 0, None,
                                          C.byref(tot)) == L.E_INVAL
