#!/usr/bin/env python
"""Address-space check of the device code: compiles every translation unit of dm-vio_amd/csrc to gfx950 ISA (hipcc -S --cuda-device-only, the Makefile's flags) and counts, per
kernel, the memory instructions by address space.  A pointer that does not arrive as a kernel argument is a GENERIC pointer to the compiler: accesses through it become flat_load /
flat_store, which count on BOTH wait counters (an s_waitcnt lgkmcnt(0) in front of an LDS read then also waits for every outstanding global load) — round 6 found the tracker's
image taps and every batched BA kernel in that state.  usage: python tools/isa_check.py [--json]; tests/test_isa_cpu.py asserts on the result.
--loops [--all] [--json]: per kernel (of capi.hip, or of every unit), the scratch_ instructions and s_loads inside blocks the assembler marks as part of a loop, beside the resource
summary (loop_report(); tests/test_tracker_loop_scratch_cpu.py asserts on it)."""
import json, os, re, subprocess, sys, tempfile
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dm-vio_amd", "csrc")
UNITS = ["capi", "capi_ref", "capi_frames", "capi_ba", "capi_immature", "capi_init", "capi_init_resident", "capi_init_first", "capi_select", "capi_activate"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics", "-fno-slp-vectorize", "-mllvm", "-amdgpu-sched-strategy=max-ilp"]
KINDS = ("global_load", "global_store", "global_atomic", "flat_load", "flat_store", "flat_atomic", "scratch_load", "scratch_store")


def unit_isa(unit, outdir):
    out = os.path.join(outdir, unit + ".s")
    subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-S", "--cuda-device-only", "-o", out, unit + ".hip"], cwd=CSRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out).read().splitlines()


def kernels(lines):
    """{demangled-ish kernel name: Counter of memory instruction kinds}"""
    res = {}
    starts = [(i, l) for i, l in enumerate(lines) if re.match(r"^_ZN3dmv\d+k_\w+:", l)]
    for i, l in starts:
        sym = l.split(":")[0]
        m = re.match(r"^_ZN3dmv(\d+)(k_\w+)", sym)
        name = m.group(2)[:int(m.group(1))] + sym[len("_ZN3dmv") + len(m.group(1)) + int(m.group(1)):][:24]
        c = Counter()
        for x in lines[i:]:
            if x.startswith(".Lfunc_end"):
                break
            mm = re.match(r"\s+(global_load|global_store|global_atomic|flat_load|flat_store|flat_atomic|scratch_load|scratch_store)", x)
            if mm:
                c[mm.group(1)] += 1
        res[name] = c
    return res


def loop_report(lines):
    """{mangled kernel symbol: per-kernel figures of the blocks the assembler marks as part of a loop (`in Loop:` in the label comment, or a `Loop Header`)}: the
    scratch_ instructions and s_loads inside such blocks with their line numbers, the number of loop-marked blocks that hold v_mfma instructions (0 = the comment format has
    changed, or the kernel has no matrix-core loop: a caller that expects one must fail), and the resource summary (vgprs, occupancy, lds, scratch bytes)."""
    res = {}
    starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_ZN3dmv\d+k_\w+:", l)]
    for i, sym in starts:
        d = dict(scratch_in_loop=[], s_load_in_loop=0, mfma_loop_blocks=0, loop_blocks=0, scratch_total=0)
        in_loop, label_open, block_has_mfma = False, False, False
        j = i + 1
        while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
            x = lines[j]
            if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", x):
                if in_loop and block_has_mfma:
                    d["mfma_loop_blocks"] += 1
                in_loop, label_open, block_has_mfma = ("in Loop:" in x or "Loop Header" in x), True, False
                d["loop_blocks"] += in_loop
            elif label_open and re.match(r"^\s*;", x):   # continuation lines of the label comment
                if not in_loop and ("in Loop:" in x or "Loop Header" in x):
                    in_loop = True
                    d["loop_blocks"] += 1
            else:
                label_open = False
                ins = x.strip()
                if ins.startswith("scratch_"):
                    d["scratch_total"] += 1
                    if in_loop:
                        d["scratch_in_loop"].append((j + 1, ins.split(";")[0].strip()))
                elif in_loop and ins.startswith("s_load_"):
                    d["s_load_in_loop"] += 1
                elif ins.startswith("v_mfma"):
                    block_has_mfma = True
            j += 1
        if in_loop and block_has_mfma:
            d["mfma_loop_blocks"] += 1
        for x in lines[j:j + 80]:   # the resource summary follows the function
            for key, pat in (("vgprs", r"^; TotalNumVgprs: (\d+)"), ("occupancy", r"^; Occupancy: (\d+)"), ("lds", r"^; LDSByteSize: (\d+)"), ("scratch_bytes", r"^; ScratchSize: (\d+)")):
                m = re.match(pat, x)
                if m and key not in d:
                    d[key] = int(m.group(1))
        res[sym] = d
    return res


def run_loops(units=("capi",)):
    """loop_report() of the given translation units, keyed unit:mangled symbol"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for u in units:
            for k, v in loop_report(unit_isa(u, d)).items():
                out[u + ":" + k] = v
    return out


def run():
    with tempfile.TemporaryDirectory() as d:
        with ThreadPoolExecutor(len(UNITS)) as ex:
            isa = list(ex.map(lambda u: unit_isa(u, d), UNITS))
    out = {}
    for u, lines in zip(UNITS, isa):
        for k, c in kernels(lines).items():
            out[u + ":" + k] = {kk: c.get(kk, 0) for kk in KINDS}
    return out


if __name__ == "__main__":
    if "--loops" in sys.argv:
        r = run_loops(UNITS if "--all" in sys.argv else ("capi",))
        if "--json" in sys.argv:
            print(json.dumps(r))
        else:
            print("| kernel | VGPRs | occupancy | LDS B | scratch B | scratch_ total | scratch_ in loops | s_load in loops |\n|---|---|---|---|---|---|---|---|")
            for k, c in sorted(r.items()):
                print("| %s | %s | %s | %s | %s | %d | %d | %d |" % (k[:72], c.get("vgprs"), c.get("occupancy"), c.get("lds"), c.get("scratch_bytes"), c["scratch_total"],
                                                                  len(c["scratch_in_loop"]), c["s_load_in_loop"]))
        sys.exit(0)
    r = run()
    if "--json" in sys.argv:
        print(json.dumps(r))
    else:
        print("| kernel | global ld / st / atomic | flat ld / st / atomic | scratch ld / st |\n|---|---|---|---|")
        for k, c in sorted(r.items()):
            print("| %s | %d / %d / %d | %d / %d / %d | %d / %d |" % (k, c["global_load"], c["global_store"], c["global_atomic"], c["flat_load"], c["flat_store"], c["flat_atomic"],
                                                                     c["scratch_load"], c["scratch_store"]))
