"""CPU tests of batched point activation: the entry points are declared in include/dmvio_hip.h with the reference lines they replace, exported by the library and bound
by the Python wrapper and the C++ mirror; the header still compiles as C99 and C++11; the batched kernels touch memory through global instructions only."""
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

BATCH_SYMBOLS = ["dmvio_hip_activation_batch_create", "dmvio_hip_activation_batch_destroy", "dmvio_hip_distance_map_make_batch",
                 "dmvio_hip_immature_select_for_activation_batch", "dmvio_hip_immature_optimize_selected_batch", "dmvio_hip_immature_remove_marked_batch"]
BATCH_KERNELS = ["k_dm_fill_b", "k_dm_seed_b", "k_dm_grow_b", "k_act_classify_b", "k_act_ordered_walk_b", "k_act_gather_b", "k_rm_plan_b", "k_rm_apply_b"]


def test_batch_entry_points_declared_exported_and_bound(pkg):
    syms = pkg.declared_symbols()
    lib = pkg.load_library()
    for s in BATCH_SYMBOLS:
        assert s in syms, s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s + ": no ctypes signature"
    hdr = open(pkg.INCLUDE_PATH).read()
    part = hdr[hdr.index("dmvio_hip_activation_batch"):]
    for cite in ("CoarseTracker.cpp:931-967", "CoarseTracker.cpp:979-1073", "CoarseTracker.cpp:1076-1082", "FullSystem.cpp:646-717", "FullSystem.cpp:723-756",
                 "FullSystem.cpp:759-770"):
        assert cite in part, cite
    assert "struct dmvio_hip_activation_window" in hdr and "struct dmvio_hip_activation_optimize" in hdr
    assert hasattr(pkg, "ActivationBatchHip") and hasattr(pkg, "activate_points_batch") and hasattr(pkg, "ActivationWindow")
    for meth in ("make", "select", "optimize_selected", "remove_marked"):
        assert hasattr(pkg.ActivationBatchHip, meth), meth
    hpp = open(os.path.join(os.path.dirname(pkg.INCLUDE_PATH), "dmvio_hip.hpp")).read()
    assert re.search(r"class ActivationBatch\b", hpp)
    for s in BATCH_SYMBOLS:
        assert s in hpp, s


def test_wrapper_structures_match_the_header(pkg):
    """the ctypes mirrors list the members of the C structures in the header's order"""
    hdr = open(pkg.INCLUDE_PATH).read()
    for name, cls in (("dmvio_hip_activation_window", pkg.ActivationWindow), ("dmvio_hip_activation_optimize", pkg.ActivationOptimize)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        members = []
        for decl in body.split(";"):
            for piece in decl.split(","):
                m = re.search(r"(\w+)\s*$", piece.strip())
                if m:
                    members.append(m.group(1))
        assert members == [f[0] for f in cls._fields_], name


def test_header_with_the_batch_entries_is_plain_c_and_cxx(pkg, tmp_path):
    hdr = pkg.INCLUDE_PATH
    subprocess.check_call(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", hdr])
    subprocess.check_call(["g++", "-fsyntax-only", "-x", "c++", "-std=c++11", "-Wall", "-Werror", hdr])
    src = tmp_path / "use_batch.c"
    src.write_text('#include "%s"\nint main(void) {\n  dmvio_hip_activation_window w[2] = {{0}};\n  dmvio_hip_activation_optimize o[2] = {{0}};\n'
                   '  dmvio_hip_immature* m[2] = {0, 0};\n  int left[2];\n  int r = dmvio_hip_distance_map_make_batch(0, 2, w);\n'
                   '  r += dmvio_hip_immature_select_for_activation_batch(0, 2, w);\n  r += dmvio_hip_immature_optimize_selected_batch(0, 2, o, 0);\n'
                   '  r += dmvio_hip_immature_remove_marked_batch(0, 2, m, left);\n  dmvio_hip_activation_batch_destroy(dmvio_hip_activation_batch_create(0, 2));\n'
                   '  return r == -8 ? 0 : 1;\n}\n' % hdr)
    exe = tmp_path / "use_batch"
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", str(src), "-o", str(exe), "-L" + libdir, "-ldmvio_hip", "-Wl,-rpath," + libdir,
                           "-Wl,--allow-shlib-undefined"])
    # NULL handles are refused with a message, without a device
    assert subprocess.call([str(exe)]) == 0
    lib = pkg.load_library()
    assert lib.dmvio_hip_immature_remove_marked_batch(None, 1, None, None) < 0 and b"null batch handle" in lib.dmvio_hip_last_error()
    assert not lib.dmvio_hip_activation_batch_create(None, 4) and b"null context" in lib.dmvio_hip_last_error()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_isa_check_lists_the_batched_kernels_without_flat_or_scratch_accesses():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "isa_check.py"), "--json"])
    r = __import__("json").loads(out)
    for k in BATCH_KERNELS:
        hits = [n for n in r if n.startswith("capi_activate:" + k)]
        assert hits, k
        for n in hits:
            assert r[n]["flat_load"] + r[n]["flat_store"] + r[n]["flat_atomic"] + r[n]["scratch_load"] + r[n]["scratch_store"] == 0, (n, r[n])
            assert r[n]["global_load"] + r[n]["global_store"] + r[n]["global_atomic"] > 0, n
    assert len([n for n in r if n.startswith("capi_activate:k_act_ordered_walk_b")]) == 2      # the LDS walk and the global-memory walk

