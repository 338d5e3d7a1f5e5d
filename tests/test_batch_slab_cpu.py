"""The host layer under every W-windows-per-call entry point (dm-vio_amd/csrc/batch_slab.hpp): where the parts of a slab lie, that a slab sized at creation holds what a
call packs, the head check's refusals, and the first-repeated-handle test at the largest batch the create functions accept.  tests/batch_slab_harness.cpp is compiled by
g++ alone — the layer's first part makes no HIP call — and run as its own program; with AddressSanitizer and UBSan where g++ has their runtimes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_slab_harness(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "batch_slab_harness.cpp")
    exe = str(tmp_path / "batch_slab_harness")
    base = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-I" + os.path.join(ROOT, "dm-vio_amd", "csrc"), src, "-o", exe]
    sanitized = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 0
    if not sanitized:   # no sanitizer runtime on this machine: the same checks, unsanitized
        subprocess.check_call(base)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    print("sanitized" if sanitized else "not sanitized (no runtime)", out)
    assert p.returncode == 0 and "\nok " in "\n" + out, out


def test_the_units_keep_no_alignment_or_slab_allocation_of_their_own():
    """what the layer replaced stays replaced: the batched units compute no 256-byte alignment and pin no slab themselves"""
    csrc = os.path.join(ROOT, "dm-vio_amd", "csrc")
    for unit in ("capi_activate.hip", "capi_select.hip", "capi_immature.hip", "immature_handle.h", "capi_ref.hip", "capi_init.hip", "ba_batch_host.hpp", "ba_marg_frame_host.hpp", "ba_graph_batch_host.hpp"):
        text = open(os.path.join(csrc, unit)).read()
        assert "~(size_t)255" not in text, unit
    for unit in ("capi_activate.hip", "capi_ref.hip", "ba_marg_frame_host.hpp", "ba_graph_batch_host.hpp"):
        assert "hipHostMalloc" not in open(os.path.join(csrc, unit)).read(), unit
    assert "~(size_t)255" in open(os.path.join(csrc, "batch_slab.hpp")).read()
