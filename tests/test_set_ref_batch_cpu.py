"""CPU tests of the batched setCoarseTrackingRef (dmvio_hip_tracker_set_ref_batch): the entry points are declared in include/dmvio_hip.h next to the track-multi block under a
comment that cites what they replace, exported by the library, bound in the Python harness, and refuse NULL handles before they touch a device.  No GPU needed."""
import ctypes as C

SYMBOLS = ["dmvio_hip_set_ref_batch_create", "dmvio_hip_set_ref_batch_destroy", "dmvio_hip_tracker_set_ref_batch", "dmvio_hip_set_ref_batch_last_work"]


def test_set_ref_batch_entry_points_declared_exported_and_bound(pkg):
    syms = pkg.declared_symbols()
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in syms, s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s + ": no ctypes signature"
    hdr = open(pkg.INCLUDE_PATH).read()
    first = hdr.index("typedef struct dmvio_hip_set_ref_batch dmvio_hip_set_ref_batch;")
    assert hdr.index("int dmvio_hip_track_multi_last_work(") < first < hdr.index("int dmvio_hip_make_track_hypotheses(")
    end = hdr.rindex("*/", 0, first)
    assert not hdr[end + 2:first].strip()
    comment = hdr[hdr.rindex("/*", 0, end):end]
    for cite in ("CoarseTracker.cpp:524-538, 138-295", "NOT counted", "named twice"):
        assert cite in comment, cite
    for meth in ("set_ref", "pack", "last_work", "close"):
        assert hasattr(pkg.SetRefBatchHip, meth), meth


def test_window_record_matches_the_header(pkg):
    """dmvio_hip_set_ref_window as the header lays it out on x86-64: pointer, int, float, two doubles, int, four pointers"""
    W = pkg.SetRefWindow
    assert [f[0] for f in W._fields_] == ["trk", "ref_slot", "ref_exposure", "ref_aff_a", "ref_aff_b", "n", "u", "v", "idepth", "hdiF"]
    assert (W.trk.offset, W.ref_slot.offset, W.ref_exposure.offset, W.ref_aff_a.offset, W.ref_aff_b.offset, W.n.offset, W.u.offset) == (0, 8, 12, 16, 24, 32, 40)
    assert C.sizeof(W) == 72


def test_null_handles_are_refused_with_a_message(pkg):
    lib = pkg.load_library()
    err = lambda: lib.dmvio_hip_last_error().decode()
    assert not lib.dmvio_hip_set_ref_batch_create(None, 2, 100) and "null context" in err()
    assert lib.dmvio_hip_tracker_set_ref_batch(None, 0, None) != 0 and "null handle" in err()
    a = C.c_int(7)
    assert lib.dmvio_hip_set_ref_batch_last_work(None, C.byref(a), None, None, None) != 0 and a.value == 7 and "null handle" in err()
    lib.dmvio_hip_set_ref_batch_destroy(None)
