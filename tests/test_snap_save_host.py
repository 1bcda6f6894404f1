"""Host side of the batched Snapshotter.save (no GPU): the file-name helper,
the capacity bound against the oracle's exact file lengths, and the struct
layouts the ctypes binding assumes."""
import ctypes as C

from etcd_amd import _lib as L
from etcd_amd import snap as S

import snap_save_cases as K


def test_snap_name_table():
    # snap/snapshotter.go:47: fmt.Sprintf("%016x-%016x%s", Term, Index, ".snap")
    for term, index in ((0, 0), (1, 1), (2, 5), (0xabc, 0xdef0), (1 << 32, 1 << 63), ((1 << 64) - 1, (1 << 64) - 1)):
        assert S.snap_name(term, index) == "%016x-%016x.snap" % (term, index)
    assert S.snap_name((1 << 64) - 1, 0) == "ffffffffffffffff-0000000000000000.snap"
    assert len(S.snap_name(1, 1)) == 38


def test_bound_covers_the_lattice():
    T = S.SAVE_TILE
    assert T > 0 and T % 16 == 0
    blob, snaps = K.lattice(T)
    n = len(snaps)
    exact = sum(len(K.expected(s, blob)[0]) for s in snaps)
    bound = S.save_bound(snaps)
    assert exact <= bound <= exact + 64 * n, (exact, bound, n)
    # per record too, and with every field at its widest
    wide = dict(data_off=0, data_len=0, index=(1 << 64) - 1, term=(1 << 64) - 1, nodes=[(1 << 64) - 1] * 70,
                removed=[1 << 63] * 70, unrec=b"\x38\x01")
    for s in (snaps[0], snaps[-1], wide):
        e = len(K.expected(s, blob)[0])
        assert e <= S.save_bound([s]) <= e + 64
    assert S.save_bound([]) == 0
    # a length that cannot be added up saturates instead of wrapping
    assert S.save_bound([dict(data_off=0, data_len=(1 << 64) - 1)]) == (1 << 64) - 1


def test_struct_sizes_match_the_library():
    assert C.sizeof(L.SnapSaveRec) == L.lib.esnap_save_rec_size() == 80
    assert C.sizeof(L.SnapSaved) == L.lib.esnap_saved_size() == 24
    for name in ("esnap_save_bound", "esnap_save_packed_device", "esnap_snap_name", "esnap_save_dir",
                 "esnap_save_tile_bytes"):
        assert name in L.header_symbols() and hasattr(L.lib, name), name
