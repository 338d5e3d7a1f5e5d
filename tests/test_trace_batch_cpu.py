"""CPU tests of batched tracing: the entry points are declared in include/dmvio_hip.h with the reference lines they replace, exported by the library and bound by the
Python wrapper and the C++ mirror; the ctypes structures follow the header; the header still compiles as C99 and C++11; NULL handles are refused without a device; the
batched kernels touch memory through global instructions only."""
import json
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

BATCH_SYMBOLS = ["dmvio_hip_trace_batch_create", "dmvio_hip_trace_batch_destroy", "dmvio_hip_immature_trace_batch", "dmvio_hip_trace_new_coarse_batch"]
BATCH_TYPES = ["dmvio_hip_trace_tables_window", "dmvio_hip_trace_window"]
TRACE_KERNELS = ["k_immature_trace_b", "k_status_hist_b"]


def test_batch_entry_points_declared_exported_and_bound(pkg):
    syms = pkg.declared_symbols()
    lib = pkg.load_library()
    for s in BATCH_SYMBOLS:
        assert s in syms, s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s + ": no ctypes signature"
    hdr = open(pkg.INCLUDE_PATH).read()
    for t in BATCH_TYPES:
        assert "typedef struct %s {" % t in hdr, t
    assert "typedef struct dmvio_hip_trace_batch dmvio_hip_trace_batch;" in hdr
    # the declarations stand with the immature-point entries, under a comment that cites what they replace
    first = hdr.index("typedef struct dmvio_hip_trace_batch dmvio_hip_trace_batch;")
    assert hdr.index("dmvio_hip_trace_new_coarse(") < first < hdr.index("typedef struct dmvio_hip_initializer dmvio_hip_initializer;")
    end = hdr.rindex("*/", 0, first)
    assert not hdr[end + 2:first].strip()
    comment = hdr[hdr.rindex("/*", 0, end):end]
    for cite in ("FullSystem.cpp:541-584", "ImmaturePoint.cpp:76-437"):
        assert cite in comment, cite
    assert hasattr(pkg, "TraceBatchHip") and hasattr(pkg, "TraceTablesWindow") and hasattr(pkg, "TraceWindow")
    for meth in ("trace", "trace_new_coarse"):
        assert hasattr(pkg.TraceBatchHip, meth), meth
    hpp = open(os.path.join(os.path.dirname(pkg.INCLUDE_PATH), "dmvio_hip.hpp")).read()
    assert re.search(r"class TraceBatch\b", hpp)
    for s in BATCH_SYMBOLS:
        assert s in hpp, s


def test_wrapper_structures_match_the_header(pkg):
    """the ctypes mirrors list the members of the C structures in the header's order"""
    hdr = open(pkg.INCLUDE_PATH).read()
    for name, cls in (("dmvio_hip_trace_tables_window", pkg.TraceTablesWindow), ("dmvio_hip_trace_window", pkg.TraceWindow)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        members = []
        for decl in body.split(";"):
            for piece in decl.split(","):
                m = re.search(r"(\w+)\s*(\[\d+\])?\s*$", piece.strip())
                if m:
                    members.append(m.group(1))
        assert members == [f[0] for f in cls._fields_], name
    assert pkg.TraceWindow.new_w2c7.size == 56 and pkg.TraceWindow.new_aff.size == 16 and pkg.TraceWindow.counts6.size == 24


def test_header_with_the_batch_entries_is_plain_c_and_cxx(pkg, tmp_path):
    hdr = pkg.INCLUDE_PATH
    subprocess.check_call(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", hdr])
    subprocess.check_call(["g++", "-fsyntax-only", "-x", "c++", "-std=c++11", "-Wall", "-Werror", hdr])
    src = tmp_path / "use_trace_batch.c"
    src.write_text('#include <string.h>\n#include "%s"\nint main(void) {\n  dmvio_hip_trace_tables_window t[2];\n  dmvio_hip_trace_window w[2];\n'
                   '  double K[4] = {100, 100, 64, 64};\n  int r;\n'
                   '  memset(t, 0, sizeof(t)); memset(w, 0, sizeof(w));\n'
                   '  r = dmvio_hip_immature_trace_batch(0, 2, t);\n  if (r >= 0 || !strstr(dmvio_hip_last_error(), "null batch handle")) return 1;\n'
                   '  r = dmvio_hip_trace_new_coarse_batch(0, 2, w, K, 1);\n  if (r >= 0 || !strstr(dmvio_hip_last_error(), "null batch handle")) return 2;\n'
                   '  if (dmvio_hip_trace_batch_create(0, 2) || !strstr(dmvio_hip_last_error(), "null context")) return 3;\n'
                   '  dmvio_hip_trace_batch_destroy(0);\n  return 0;\n}\n' % hdr)
    exe = tmp_path / "use_trace_batch"
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", str(src), "-o", str(exe), "-L" + libdir, "-ldmvio_hip", "-Wl,-rpath," + libdir,
                           "-Wl,--allow-shlib-undefined"])
    # NULL handles are refused with a message, without a device
    assert subprocess.call([str(exe)]) == 0
    lib = pkg.load_library()
    assert lib.dmvio_hip_immature_trace_batch(None, 0, None) < 0 and b"null batch handle" in lib.dmvio_hip_last_error()
    assert lib.dmvio_hip_trace_new_coarse_batch(None, 0, None, None, 0) < 0 and b"null batch handle" in lib.dmvio_hip_last_error()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_isa_check_lists_the_batched_kernels_without_flat_or_scratch_accesses():
    r = json.loads(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "isa_check.py"), "--json"]))
    for k in TRACE_KERNELS:
        hits = [n for n in r if n.startswith("capi_immature:" + k)]
        assert hits, k
        for n in hits:
            assert r[n]["flat_load"] + r[n]["flat_store"] + r[n]["flat_atomic"] + r[n]["scratch_load"] + r[n]["scratch_store"] == 0, (n, r[n])
            assert r[n]["global_load"] + r[n]["global_store"] + r[n]["global_atomic"] > 0, n
