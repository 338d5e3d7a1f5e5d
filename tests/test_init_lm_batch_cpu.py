"""The batched form of the initializer's LM loop (include/dmvio_hip_init_lm_batch.h) without a GPU: the extension header against its signature table and its struct against
the ctypes mirror as gcc lays it out, the exports and their bindings, the head refusals (which need no device), and the reference lines the header cites."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "dmvio_hip_init_lm_batch.h"
PATH = os.path.join(ROOT, "include", HEADER)
ENTRIES = ("dmvio_hip_initializer_lm_batch_create", "dmvio_hip_initializer_lm_batch_destroy", "dmvio_hip_initializer_resident_track_frame_batch",
           "dmvio_hip_initializer_lm_batch_last_work")
HANDLES = ("dmvio_hip_initializer", "dmvio_hip_ctx", "dmvio_hip_initializer_lm_batch")


@pytest.fixture(scope="module")
def abi(pkg):
    import dmvio_amd._abi as m
    return m


@pytest.fixture(scope="module")
def parsed(pkg):
    import test_python_binding_cpu as B
    return B.parse_header(PATH)


def test_extension_header_matches_its_table(pkg, abi, parsed):
    """under the rules of test_init_lm_cpu.py::test_extension_header_matches_its_table; a pointer to the header's own struct is POINTER(its mirror in EXTENSION_MIRRORS)"""
    import test_python_binding_cpu as B
    protos, structs, opaque, fn_types = parsed
    table = abi.EXTENSION_SIGNATURES[HEADER]
    mirrors = abi.EXTENSION_MIRRORS[HEADER]
    assert sorted(table) == sorted(protos) == sorted(ENTRIES)
    assert not set(table) & set(abi.SIGNATURES)
    for other, t in abi.EXTENSION_SIGNATURES.items():
        assert other == HEADER or not set(table) & set(t), other
    assert sorted(structs) == sorted(mirrors) == ["dmvio_hip_initializer_lm_window"] and not set(mirrors) & set(abi.MIRRORS)
    assert "dmvio_hip_initializer_lm_batch" in opaque and not fn_types
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        base, depth = B.c_type(ret + " _")
        if depth:
            assert base in HANDLES and restype is C.c_void_p, name
        elif base == "void":
            assert restype is None, name
        else:
            assert restype is B.SCALARS[base], name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, (t, decl) in enumerate(zip(argtypes, params)):
            base, depth = B.c_type(decl)
            where = "%s, parameter %d (%s)" % (name, k, decl)
            if depth == 0:
                assert t is B.SCALARS[base], "%s: %r" % (where, t)
            elif base in HANDLES:
                assert t is (C.c_void_p if depth == 1 else C.POINTER(C.c_void_p)), where
            elif base in structs:
                assert depth == 1 and t is C.POINTER(mirrors[base]), where
            else:
                B._check_pointer(pkg, parsed, t, base, depth, where)
    main = open(os.path.join(ROOT, "include", "dmvio_hip.h")).read()
    assert HEADER in main


def test_struct_mirror_has_the_headers_layout(pkg, abi, parsed, tmp_path):
    """sizeof and, per field, name, offsetof and size as gcc lays the struct out, against the ctypes mirror; and every pointer field's pointee"""
    import test_python_binding_cpu as B
    protos, structs, opaque, fn_types = parsed
    src = ['#include "%s"' % PATH, "#include <stdio.h>", "#include <stddef.h>", "int main(void) {"]
    for s, fields in structs.items():
        src.append('  printf("S %s %%zu\\n", sizeof(%s));' % (s, s))
        for f, _decl in fields:
            src.append('  printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, f, s, f, s, f))
    src += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")])
    sizes, layout = {}, {s: [] for s in structs}
    for line in subprocess.check_output([str(tmp_path / "layout")]).decode().split("\n"):
        w = line.split()
        if w and w[0] == "S":
            sizes[w[1]] = int(w[2])
        elif w:
            layout[w[1]].append((w[2], int(w[3]), int(w[4])))
    for s, fields in structs.items():
        M = abi.EXTENSION_MIRRORS[HEADER][s]
        assert issubclass(M, C.Structure) and C.sizeof(M) == sizes[s], (s, C.sizeof(M), sizes[s])
        mine = [(f, getattr(M, f).offset, getattr(M, f).size) for f, _t in M._fields_]
        assert mine == layout[s] and len(mine) == 25, (s, mine, layout[s])
        assert [f for f, _d in fields] == [f for f, _o, _n in layout[s]]
        for (f, decl), (_f, t) in zip(fields, M._fields_):
            base, depth = B.c_type(decl)
            where = "%s.%s (%s)" % (s, f, decl)
            if depth == 0:
                assert t is B.SCALARS[base], where
            elif base in HANDLES:
                assert t is (C.c_void_p if depth == 1 else C.POINTER(C.c_void_p)), where
            else:
                B._check_pointer(pkg, parsed, t, base, depth, where)


def test_library_exports_every_entry_and_the_wrapper_binds_it(pkg, abi):
    import dmvio_amd.initializer as INI
    lib = pkg.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name, (restype, argtypes) in abi.EXTENSION_SIGNATURES[HEADER].items():
        assert name in exported, name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    cls = INI.InitializerLmBatch
    assert issubclass(cls, abi._Handle) and cls._destroy == "dmvio_hip_initializer_lm_batch_destroy"
    for m in ("track_frame_batch", "last_work", "pack", "close"):
        assert callable(getattr(cls, m)), m


def test_head_refusals_need_no_device(pkg, abi):
    lib = pkg.load_library()
    err = lambda: (lib.dmvio_hip_last_error() or b"").decode()
    Win = abi.EXTENSION_MIRRORS[HEADER]["dmvio_hip_initializer_lm_window"]
    arr = (Win * 2)()
    assert lib.dmvio_hip_initializer_resident_track_frame_batch(None, 1, arr) != 0 and "null batch handle" in err()
    assert lib.dmvio_hip_initializer_resident_track_frame_batch(None, 0, None) != 0 and "null batch handle" in err()
    assert not lib.dmvio_hip_initializer_lm_batch_create(None, 4) and "bad argument" in err()
    out = [C.c_int(7) for _ in range(4)]
    assert lib.dmvio_hip_initializer_lm_batch_last_work(None, *[C.byref(x) for x in out]) != 0 and [x.value for x in out] == [7] * 4
    lib.dmvio_hip_initializer_lm_batch_destroy(None)
    # W < 0, W > max_windows and a NULL array: refused too, by the same head check (dmvBatchHead: tests/batch_slab_harness.cpp holds its order, in which the missing
    # handle comes first — a batch handle needs a context, hence a device; tests/test_init_lm_batch_gpu.py makes the three calls on a live batch and reads their messages)
    for W, a in ((-1, arr), (65536, arr), (3, arr), (1, None)):
        assert lib.dmvio_hip_initializer_resident_track_frame_batch(None, W, a) != 0 and "initializer_resident_track_frame_batch" in err(), (W, a)
    # and the creation fails cleanly, with a message, for every size outside [1, 65535]
    for mw in (0, -1, 65536):
        assert not lib.dmvio_hip_initializer_lm_batch_create(None, mw) and "max_windows" in err()


def test_header_cites_the_reference_lines():
    txt = open(PATH).read()
    assert "CoarseInitializer.cpp:100-114, 126-263, 708-747, 749-777" in txt
    for lines in ("100-114", "126-263", "708-747", "749-777"):
        assert lines in txt, lines


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_batch_unit_has_no_generic_access_and_no_scratch():
    """the new unit's ISA under the rules tests/test_init_lm_cpu.py applies to the single call's: every pointer of a record is read through initGl(), so no kernel of the unit
    makes a flat_* access; the frame kernel keeps the level loop's MFMA evaluation and uses no scratch"""
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check
    with tempfile.TemporaryDirectory() as d:
        lines = isa_check.unit_isa("capi_init_lm_batch", d)
    kinds = isa_check.kernels(lines)
    assert sum("k_init_lm_frame_bE" in k for k in kinds) == 1, sorted(kinds)
    for k, c in kinds.items():
        assert c["flat_load"] + c["flat_store"] + c["flat_atomic"] == 0, (k, dict(c))
    loops = [v for k, v in isa_check.loop_report(lines).items() if "k_init_lm_frame_bE" in k]
    assert len(loops) == 1 and loops[0]["mfma_loop_blocks"] >= 1 and loops[0]["loop_blocks"] > 100
    assert not loops[0]["scratch_in_loop"] and loops[0]["scratch_bytes"] == 0, loops[0]["scratch_in_loop"][:4]
