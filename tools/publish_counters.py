#!/usr/bin/env python
"""profiles/<round>_counters_k_track_lm.md from the outputs of tools/profile_counters.sh (gpurun_out/prof_<round>/counters_*.md) and the round's bench line
(gpurun_out/prof_<round>/bench_n1.json).   usage: python tools/publish_counters.py r04"""
import glob, json, os, sys

R = sys.argv[1] if len(sys.argv) > 1 else "r04"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O = os.path.join(ROOT, "gpurun_out", "prof_" + R) + "/"
P = os.path.join(ROOT, "profiles") + "/"
d = json.loads(open(O + "bench_n1.json").read().strip().splitlines()[-1])
rf = d["roofline"]


def rows(path, names):
    out = []
    for l in open(path):
        if any(n in l for n in names):
            p = [x.strip() for x in l.strip().strip("|").split("|")]
            out.append(p)
    return out


# ---- counters of the headline kernel
cf = sorted(glob.glob(O + "counters_*.md"))
if cf:
    C = {}
    raw = []
    for f in cf:
        for p in rows(f, ["k_track_lm<256", "k_build_pyramids"]):
            k = "k_track_lm<256,4>" if "k_track_lm" in p[0] else "k_build_pyramids"
            raw.append((k, p[1], p[2], p[3], p[4], p[5]))
            if k.startswith("k_track"):
                C[p[1]] = float(p[3])
    pe = rf["point_evals_per_launch"]
    cyc = C["GRBM_GUI_ACTIVE"] / 8.0
    valu_busy = 4 * C["SQ_ACTIVE_INST_VALU"] / (1024 * cyc)
    out = ["# %s — hardware counters of the headline step (`tools/profile_counters.sh %s`: one `rocprofv3 --kernel-trace --pmc <group>` run per group of" % (R, R),
           "`python bench.py --full --no-cpu --no-ba --steps 3 --warmup 1`, batch 4096, 1x MI355X; per-dispatch values summed over the device)", "",
           "## What they say about `k_track_lm<256,4>` (%d alignment problems, %.1f M point-evaluations, %.2f ms per launch by HIP events)" % (d["config"]["frames_per_step_per_gpu"], pe / 1e6, rf["kernel_ms"]), "",
           "* `GRBM_GUI_ACTIVE` %.1f M = 8 XCDs x %.2f M cycles; `SQ_BUSY_CU_CYCLES` %.0f M = 256 CUs x %.2f M: every CU is busy for the whole launch."
           % (C["GRBM_GUI_ACTIVE"] / 1e6, cyc / 1e6, C["SQ_BUSY_CU_CYCLES"] / 1e6, C["SQ_BUSY_CU_CYCLES"] / 256e6),
           "* **VALU**: %.0f M wavefront instructions = %.0f per 64 point-evaluations (evaluation loop + LM control); `SQ_ACTIVE_INST_VALU` %.0f M quad-cycles"
           % (C["SQ_INSTS_VALU"] / 1e6, C["SQ_INSTS_VALU"] * 64 / pe, C["SQ_ACTIVE_INST_VALU"] / 1e6),
           "  → VALUBusy = 4 x %.0f M / (1024 SIMDs x %.2f M cycles) = **%.0f %%**.  %.1f M MFMA instructions (the 9x9 outer products) are %.0f %% of them."
           % (C["SQ_ACTIVE_INST_VALU"] / 1e6, cyc / 1e6, 100 * valu_busy, C["SQ_INSTS_MFMA"] / 1e6, 100 * C["SQ_INSTS_MFMA"] / C["SQ_INSTS_VALU"]),
           "* **Vector L1 (TCP)**: %.1f M wavefront loads (%.1f per point-evaluation: 4 taps + the template record) make %.1f M tag look-ups = %.0f cache lines per"
           % (C["SQ_INSTS_VMEM_RD"] / 1e6, C["SQ_INSTS_VMEM_RD"] * 64 / pe, C["TCP_TOTAL_CACHE_ACCESSES_sum"] / 1e6, C["TCP_TOTAL_CACHE_ACCESSES_sum"] / C["SQ_INSTS_VMEM_RD"]),
           "  64-lane load (%.1f per point-evaluation); the TCP is active in **%.0f %%** of the CU cycles (`TCP_GATE_EN2 / TCP_GATE_EN1`), stalled on outstanding misses in %.0f %%"
           % (C["TCP_TOTAL_CACHE_ACCESSES_sum"] / pe, 100 * C["TCP_GATE_EN2_sum"] / C["TCP_GATE_EN1_sum"], 100 * C["TCP_PENDING_STALL_CYCLES_sum"] / C["SQ_BUSY_CU_CYCLES"]),
           "  (`TCP_PENDING_STALL_CYCLES`); tag-conflict stalls %.0f %%.  L1 hit rate %.0f %% (%.1f M requests go on to the L2)."
           % (100 * C["TCP_READ_TAGCONFLICT_STALL_CYCLES_sum"] / C["SQ_BUSY_CU_CYCLES"], 100 * (1 - C["TCP_TCC_READ_REQ_sum"] / C["TCP_TOTAL_CACHE_ACCESSES_sum"]), C["TCP_TCC_READ_REQ_sum"] / 1e6),
           "* **L2 (TCC)**: %.1f M requests, %.1f %% hits; %.1f M reads go to the fabric = %.2f GB of 128-B lines per launch — the same figure as 2 x FETCH_SIZE"
           % (C["TCC_REQ_sum"] / 1e6, 100 * C["TCC_HIT_sum"] / C["TCC_REQ_sum"], C["TCC_EA0_RDREQ_sum"] / 1e6, C["TCC_EA0_RDREQ_sum"] * 128 / 1e9),
           "  (profiles/%s_pmc_hbm_traffic.md): %.1f TB/s, far below the HBM peak." % (R, C["TCC_EA0_RDREQ_sum"] * 128 / 1e9 / rf["kernel_ms"]),
           "* **TLB**: %.0f M UTCL1 requests, %.0f misses — address translation is not a factor (1.4 GB of pyramids in 2-MB fragments)."
           % (C["TCP_UTCL1_REQUEST_sum"] / 1e6, C["TCP_UTCL1_TRANSLATION_MISS_sum"]),
           "", "Conclusion: no single unit is the limiter — the SIMDs issue VALU work %.0f %% of the time while the vector L1 is busy %.0f %% of the time (one tag look-up per"
           % (100 * valu_busy, 100 * C["TCP_GATE_EN2_sum"] / C["TCP_GATE_EN1_sum"]),
           "clock per CU, each tap row its own 128-B line because the template is semi-dense).  HBM, L2 bandwidth, LDS and the TLB are far from their limits.  Cutting the",
           "VALU count is what has paid (DESIGN.md §4: shared-reciprocal division, pipeline hand-over without moves); layout changes that cut the line count are listed in §7.", "",
           "## Raw values (avg / min / max per dispatch)", "", "| kernel | counter | dispatches | avg | min | max |", "|---|---|---|---|---|---|"]
    out += ["| %s | %s | %s | %s | %s | %s |" % r for r in raw]
    open(P + R + "_counters_k_track_lm.md", "w").write("\n".join(out) + "\n")
print("published counters", R)
