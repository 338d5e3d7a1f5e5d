#!/usr/bin/env python
"""Is the device code of two trees the same?  Compares, kernel by kernel, the gfx950 ISA of every translation unit tools/isa_check.py knows: the instruction stream (block
labels .LBB<n>_<m> / .Ltmp<n> renumbered in order of appearance, `;` comments stripped) and the kernel's .amdhsa_* block.  What a refactor that must not touch the kernels
checks itself with: every kernel of A must be in B and identical, and B must not add one.  Kernels are matched by symbol over the union of all units, so a kernel that
changed its translation unit is compared all the same and reported as moved (which alone is no difference).

usage: python tools/isa_diff.py [--explain] <dirA> <dirB>   directories of <unit>.s files; --explain: per differing kernel, the .amdhsa_ lines and the opcode counts that differ
       python tools/isa_diff.py --dump <dir> [csrc]  compile the units of dm-vio_amd/csrc (or of another tree's csrc) into <dir> first (hipcc -S --cuda-device-only, the Makefile's flags)
exit status 0: identical; 1: differences (listed)."""
import os, re, subprocess, sys
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_check import CSRC, FLAGS, UNITS


def dump(outdir, csrc=CSRC):
    os.makedirs(outdir, exist_ok=True)
    def one(u):
        subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-S", "--cuda-device-only", "-o", os.path.join(os.path.abspath(outdir), u + ".s"), u + ".hip"], cwd=csrc, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    units = [u for u in UNITS if os.path.exists(os.path.join(csrc, u + ".hip"))]   # (another tree may not have every unit)
    with ThreadPoolExecutor(len(units)) as ex:
        list(ex.map(one, units))


def kernels(path):
    """{kernel symbol: (normalised instruction lines, .amdhsa_ lines)}"""
    lines = open(path).read().splitlines()
    hsa, sym = {}, None
    for l in lines:   # .amdhsa_kernel <sym> ... .end_amdhsa_kernel
        t = l.strip()
        if t.startswith(".amdhsa_kernel "):
            sym = t.split()[1]; hsa[sym] = []
        elif t == ".end_amdhsa_kernel":
            sym = None
        elif sym and t.startswith(".amdhsa_"):
            hsa[sym].append(t)
    start = {l.split(":")[0]: i for i, l in enumerate(lines) if l[:1] == "_" and ":" in l}   # "<sym>:   ; @<sym>"
    res = {}
    for k in hsa:
        i = start[k]
        body, names = [], {}
        def renum(m):
            return names.setdefault(m.group(0), "L%d" % len(names))
        for l in lines[i + 1:]:
            if l.startswith(".Lfunc_end") or l.strip().startswith((".section", ".amdhsa_kernel")):   # (the descriptor block stands between the code and .Lfunc_end)
                break
            t = l.split(";")[0].strip()
            if not t or t.startswith((".p2align", ".loc", ".cfi", ".file")):
                continue
            body.append(re.sub(r"\.(LBB\d+_\d+|Ltmp\d+)", renum, t))
        res[k] = (body, hsa[k])
    return res


def tree(d):
    """{kernel symbol: (unit, normalised instruction lines, .amdhsa_ lines)} over every <unit>.s of the directory"""
    res = {}
    for f in sorted(os.listdir(d)):
        if f.endswith(".s"):
            for k, v in kernels(os.path.join(d, f)).items():
                assert k not in res, "%s is in two units: %s and %s" % (k, res[k][0], f[:-2])
                res[k] = (f[:-2],) + v
    return res


def explain(va, vb):
    """what differs between two versions of a kernel: the .amdhsa_ lines (registers, LDS, scratch) and the opcodes whose counts differ, as (A, B)"""
    for t in sorted(set(va[2]) ^ set(vb[2])):
        print("    %s %s" % ("A" if t in va[2] else "B", t))
    ca, cb = (Counter("label" if l.endswith(":") else l.split()[0] for l in v[1]) for v in (va, vb))
    print("    " + (", ".join("%s (%d, %d)" % (o, ca[o], cb[o]) for o in sorted(set(ca) | set(cb)) if ca[o] != cb[o]) or "same opcode counts: order or operands differ"))


def main(a, b, why=False):
    ka, kb = tree(a), tree(b)
    bad = moved = 0
    for k in sorted(set(ka) | set(kb)):
        if k in ka and k in kb and ka[k][0] != kb[k][0]:
            moved += 1
            print("%s: moved from %s to %s" % (k, ka[k][0], kb[k][0]))
        if k not in kb: what = "missing in B"
        elif k not in ka: what = "added in B"
        elif ka[k][1] != kb[k][1]: what = "instructions differ (%d vs %d lines)" % (len(ka[k][1]), len(kb[k][1]))
        elif ka[k][2] != kb[k][2]: what = ".amdhsa block differs"
        else: continue
        bad += 1
        print("%s: %s: %s" % ((ka.get(k) or kb[k])[0], k, what))
        if why and k in ka and k in kb: explain(ka[k], kb[k])
    for u in sorted(set(v[0] for v in ka.values()) | set(v[0] for v in kb.values())):
        print("%s: %d kernels in A, %d in B" % (u, sum(v[0] == u for v in ka.values()), sum(v[0] == u for v in kb.values())))
    print("%d kernels in A, %d in B, %d moved; %s" % (len(ka), len(kb), moved, "identical" if not bad else "%d kernels differ" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--dump":
        dump(sys.argv[2], *sys.argv[3:4])
    elif len(sys.argv) == 4 and sys.argv[1] == "--explain":
        sys.exit(main(sys.argv[2], sys.argv[3], True))
    elif len(sys.argv) == 3:
        sys.exit(main(sys.argv[1], sys.argv[2]))
    else:
        sys.exit(__doc__)
