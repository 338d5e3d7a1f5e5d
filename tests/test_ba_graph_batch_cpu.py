"""CPU tests of the batched window hand-over (dmvio_hip_ba_set_graph_from_batch): the three entry points and the window structure are declared in include/dmvio_hip.h next
to the other dmvio_hip_ba_*_batch calls, exported by the library, bound in the Python harness, and refuse NULL handles before they touch a device.  No GPU needed."""
import ctypes as C

SYMBOLS = ["dmvio_hip_ba_set_graph_from_batch", "dmvio_hip_ba_batch_last_graph_work", "dmvio_hip_ba_batch_last_graph_ms"]


def test_entry_points_declared_exported_and_bound(pkg):
    syms = pkg.declared_symbols()
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in syms, s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s + ": no ctypes signature"
    hdr = open(pkg.INCLUDE_PATH).read()
    first = hdr.index("typedef struct dmvio_hip_ba_graph_window { dmvio_hip_ba* ba; dmvio_hip_graph* graph; } dmvio_hip_ba_graph_window;")
    assert hdr.index("int dmvio_hip_ba_marginalize_frame_batch(") < first < hdr.index("int dmvio_hip_ba_set_graph_from_batch(") < hdr.index("int dmvio_hip_ba_batch_set_exact_backsub(")
    end = hdr.rindex("*/", 0, first)
    assert not hdr[end + 2:first].strip()
    comment = hdr[hdr.rindex("/*", 0, end):end]
    for cite in ("dmvio_hip_ba_set_graph_from(win[i].ba, win[i].graph)", "ONE upload", "SIX kernel launches", "ONE wait", "names the window", "observes one keyframe twice"):
        assert cite in comment, cite
    for meth in ("set_graph_from", "last_graph_work", "last_graph_ms"):
        assert hasattr(pkg.BundleAdjusterBatch, meth), meth


def test_window_record_matches_the_header(pkg):
    """dmvio_hip_ba_graph_window on x86-64: two pointers"""
    W = pkg.BAGraphWindow
    assert [f[0] for f in W._fields_] == ["ba", "graph"]
    assert (W.ba.offset, W.graph.offset, C.sizeof(W)) == (0, 8, 16)


def test_null_handles_are_refused_with_a_message(pkg):
    lib = pkg.load_library()
    err = lambda: lib.dmvio_hip_last_error().decode()
    assert lib.dmvio_hip_ba_set_graph_from_batch(None, 0, None) != 0 and "null batch" in err()
    a = C.c_int(7)
    assert lib.dmvio_hip_ba_batch_last_graph_work(None, C.byref(a), None, None, None) != 0 and a.value == 7 and "null batch" in err()
    ms = C.c_float(3.0)
    assert lib.dmvio_hip_ba_batch_last_graph_ms(None, C.byref(ms)) != 0 and ms.value == 3.0 and "null argument" in err()
