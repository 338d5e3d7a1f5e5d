"""CPU tests of multi-window tracking (dmvio_hip_tracker_track_multi): the entry points are declared in include/dmvio_hip.h next to dmvio_hip_tracker_track_batch under a
comment that cites the reference lines they replace, exported by the library and bound by the Python wrapper and the C++ mirror; the header still compiles as C99 and
C++11; NULL arguments are refused without a device; the new kernel instantiations touch memory through global instructions only."""
import json
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

MULTI_SYMBOLS = ["dmvio_hip_track_multi_create", "dmvio_hip_track_multi_destroy", "dmvio_hip_tracker_track_multi", "dmvio_hip_track_multi_set_launch_shape",
                 "dmvio_hip_track_multi_set_residual_only_evals", "dmvio_hip_track_multi_last_launch", "dmvio_hip_track_multi_last_work"]


def test_multi_entry_points_declared_exported_and_bound(pkg):
    syms = pkg.declared_symbols()
    lib = pkg.load_library()
    for s in MULTI_SYMBOLS:
        assert s in syms, s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s + ": no ctypes signature"
    hdr = open(pkg.INCLUDE_PATH).read()
    # the declarations stand with the batch entries of the tracker, under a comment that cites what they replace
    first = hdr.index("typedef struct dmvio_hip_track_multi dmvio_hip_track_multi;")
    assert hdr.index("int dmvio_hip_tracker_track_batch(") < first < hdr.index("int dmvio_hip_make_track_hypotheses(")
    end = hdr.rindex("*/", 0, first)
    assert not hdr[end + 2:first].strip()
    comment = hdr[hdr.rindex("/*", 0, end):end]
    for cite in ("CoarseTracker.cpp:539-770", "FullSystem.cpp:364-402"):
        assert cite in comment, cite
    assert hasattr(pkg, "TrackMultiHip")
    for meth in ("track", "set_launch_shape", "set_residual_only_evals", "last_launch", "last_work", "close"):
        assert hasattr(pkg.TrackMultiHip, meth), meth
    hpp = open(os.path.join(os.path.dirname(pkg.INCLUDE_PATH), "dmvio_hip.hpp")).read()
    assert re.search(r"class TrackMulti\b", hpp)
    for s in MULTI_SYMBOLS:
        assert s in hpp, s


def test_header_with_the_multi_entries_is_plain_c_and_cxx(pkg, tmp_path):
    hdr = pkg.INCLUDE_PATH
    subprocess.check_call(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", hdr])
    subprocess.check_call(["g++", "-fsyntax-only", "-x", "c++", "-std=c++11", "-Wall", "-Werror", hdr])
    src = tmp_path / "use_track_multi.c"
    src.write_text('#include <string.h>\n#include "%s"\nint main(void) {\n  int win[2] = {0, 0}, slots[2] = {0, 0}, a = 7, b = 7;\n  long long e = 7, pe = 7;\n'
                   '  double pose[14], aff[4];\n  dmvio_hip_tracker* trk[1] = {0};\n  int r;\n'
                   '  memset(pose, 0, sizeof(pose)); memset(aff, 0, sizeof(aff));\n'
                   '  r = dmvio_hip_tracker_track_multi(0, 1, trk, 2, win, slots, 0, pose, aff, 2, 0, 0, 0, 0, 0, 0, 0);\n'
                   '  if (r == 0 || !strstr(dmvio_hip_last_error(), "null handle")) return 1;\n'
                   '  if (dmvio_hip_track_multi_create(0, 2, 2) || !strstr(dmvio_hip_last_error(), "null context")) return 2;\n'
                   '  if (dmvio_hip_track_multi_set_launch_shape(0, 0) == 0 || !strstr(dmvio_hip_last_error(), "null handle")) return 3;\n'
                   '  if (dmvio_hip_track_multi_set_residual_only_evals(0, 1) == 0 || !strstr(dmvio_hip_last_error(), "null handle")) return 4;\n'
                   '  if (dmvio_hip_track_multi_last_launch(0, &a, &b) == 0 || a != 7 || b != 7) return 5;\n'
                   '  if (dmvio_hip_track_multi_last_work(0, &e, &pe) == 0 || e != 7 || pe != 7) return 6;\n'
                   '  dmvio_hip_track_multi_destroy(0);\n  return 0;\n}\n' % hdr)
    exe = tmp_path / "use_track_multi"
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", str(src), "-o", str(exe), "-L" + libdir, "-ldmvio_hip", "-Wl,-rpath," + libdir,
                           "-Wl,--allow-shlib-undefined"])
    # NULL handles are refused with a message, without a device
    assert subprocess.call([str(exe)]) == 0
    lib = pkg.load_library()
    assert lib.dmvio_hip_tracker_track_multi(None, 0, None, 0, None, None, None, None, None, 0, None, None, None, None, None, None, None) != 0
    assert b"null handle" in lib.dmvio_hip_last_error()


def test_cxx_wrapper_compiles(pkg, tmp_path):
    src = tmp_path / "use_track_multi.cpp"
    src.write_text('#include "dmvio_hip.hpp"\nint main() {\n  dmvio_hip::TrackMulti m(nullptr, 2, 4);\n  std::vector<const dmvio_hip::CoarseTracker*> t;\n'
                   '  std::vector<dmvio_hip::TrackMulti::Problem> p(1);\n  int c = 0, th = 0;\n  long long e = 0, pe = 0;\n'
                   '  return (m.valid() || m.track(t, p, 2) || m.setLaunchShape(0) || m.setResidualOnlyEvals(true) || m.lastLaunch(c, th) || m.lastWork(e, pe)) ? 1 : 0;\n}\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.dirname(pkg.INCLUDE_PATH), str(src)])


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_isa_check_lists_the_multi_kernels_without_flat_accesses():
    """both instantiations of k_track_lm_w are built, and the reference that now comes out of a table is still reached through global (not generic) pointers"""
    r = json.loads(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "isa_check.py"), "--json"]))
    hits = [n for n in r if n.startswith("capi:k_track_lm_w")]
    assert len(hits) == 2, hits
    for n in hits:
        assert r[n]["flat_load"] + r[n]["flat_store"] + r[n]["flat_atomic"] == 0, (n, r[n])
        assert r[n]["global_load"] > 0 and r[n]["global_store"] > 0, n
