#!/usr/bin/env python3
"""Copy the judged summaries of a tools/prof_r06.sh run from $PROF_OUT/<tag>_* (default prof_out/) into profiles/ (tracked):
kernel-stats CSVs as they are, PMC counter CSVs reduced to one averaged row per kernel, plus two small JSON digests
(profiles/psf_kernel_pmc.json, profiles/conv_traffic.json) that bench.py quotes as static context."""
import collections, csv, glob, json, os, shutil, sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tag = sys.argv[1] if len(sys.argv) > 1 else "r02_a"
G, P = os.environ.get("PROF_OUT") or os.path.join(REPO, "prof_out"), os.path.join(REPO, "profiles")


def code_sha256(*sources):
    """sha256 of the kernel sources a digest belongs to: bench.py quotes a digest only while the tree still holds these sources.
    Taken from $PROF_OUT/<tag>_code_sha256.json when the collection script wrote it AT COLLECTION TIME (tools/prof_r05.sh: the
    sources, common.h, include/aadff.h and the libaadff.so that ran - ADVICE r4: a digest summarised after an edit must not be
    stamped with the new hash); hashing the tree now is the fallback for older collections."""
    import hashlib
    stamp = os.path.join(G, f"{tag}_code_sha256.json")
    if os.path.exists(stamp):
        rec = json.load(open(stamp))
        out = {src: rec[src] for src in sources if src in rec}
        out.update({k: rec[k] for k in ("common.h", "aadff.h", "libaadff.so") if k in rec})
        if all(src in out for src in sources):
            return out
    out = {}
    for src in sources:
        with open(os.path.join(REPO, "aberration-aware-depth-from-focus_amd", "csrc", src), "rb") as f:
            out[src] = hashlib.sha256(f.read()).hexdigest()
    return out


def one(pattern):
    f = glob.glob(os.path.join(G, pattern), recursive=True)
    return max(f, key=os.path.getmtime) if f else None           # a tag collected twice: the latest run


def pmc_rows(path):
    acc = collections.defaultdict(lambda: collections.defaultdict(list))
    meta = {}
    for r in csv.DictReader(open(path)):
        k = r["Kernel_Name"]
        acc[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
        meta[k] = (r["VGPR_Count"], r["SGPR_Count"], r["LDS_Block_Size"], r["Workgroup_Size"], r["Grid_Size"])
    return {k: ({c: sum(v) / len(v) for c, v in cs.items()}, len(next(iter(cs.values()))), meta[k]) for k, cs in acc.items()}


def write_pmc(dst, sources, keep):
    rows = {}
    for src in sources:
        if not src:
            continue
        for k, (vals, n, meta) in pmc_rows(src).items():
            if any(s in k for s in keep):
                rows.setdefault(k, [{}, n, meta])[0].update(vals)
    with open(dst, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["kernel", "launches_averaged", "vgpr", "sgpr", "lds_bytes", "workgroup", "grid", "counter", "mean_value_per_launch"])
        for k, (vals, n, meta) in rows.items():
            for c, v in sorted(vals.items()):
                w.writerow([k[:100], n, *meta, c, f"{v:.3f}"])
    return rows


for name, sub in (("kernel_stats", "stats"), ("kernel_stats_1stream", "stats_s1"), ("fit_kernel_stats", "fit_stats"), ("local_psf_kernel_stats", "lp_stats"),
                  ("single_kernel_stats", "single_stats"), ("strict_kernel_stats", "strict_stats"), ("m1l_kernel_stats", "m1l_stats"),
                  ("dropin_kernel_stats", "dropin_stats"), ("edge_kernel_stats", "edge_stats")):
    src = one(f"{tag}_{sub}/**/*_kernel_stats.csv")
    if src:
        shutil.copy(src, os.path.join(P, f"{tag}_{name}.csv"))
for name in ("bench", "bench_fit", "bench_m2", "bench_2streams", "bench_refocus_overlap", "bench_1stream", "bench_c3", "bench_under_rocprof",
             "conv_timeline", "conv_timeline_paired", "parity_per_slice_shipped", "parity_per_slice_literal", "parity_per_slice_strict",
             "conv_single_timeline", "conv_single_timeline_toeplitz", "bench_rccl1_gather", "bench_m1l", "code_sha256",
             "conv_blkw_timeline_ks21", "conv_blkw_timeline_ks21_rb24"):
    src = os.path.join(G, f"{tag}_{name}.json")
    if os.path.exists(src) and os.path.getsize(src):
        shutil.copy(src, os.path.join(P, f"{tag}_{name}.json"))

for name in ("conv_ks_sweep", "strict_profile", "kbench", "dropin", "conv_blkw_probe", "strict_pipe_probe", "dropin_with_copies", "edge_bench",
             "edge_bench_under_rocprof"):
    src = os.path.join(G, f"{tag}_{name}.txt")
    if os.path.exists(src) and os.path.getsize(src):
        shutil.copy(src, os.path.join(P, f"{tag}_{name}.txt"))
STRICT_SOURCES = ("strict_fused.hip", "strict_math2.h", "strict_math.h", "strict.hip")
sp_ = one(f"{tag}_strict_pmc/**/*counter_collection.csv")
if sp_:
    srows = write_pmc(os.path.join(P, f"{tag}_strict_kernel_pmc.csv"), [sp_], ("fused_psf_kernel", "fused_flat_kernel"))
    # digest of the strict psf_map kernel, stamped with the hashes of EVERY source it is compiled from: bench.py quotes
    # it under parity.strict_mode only while the tree still holds those sources
    sstats = one(f"{tag}_strict_stats/**/*_kernel_stats.csv")
    us = None
    if sstats:
        for r in csv.DictReader(open(sstats)):
            if "fused_psf_kernel<256>" in r["Name"]:
                us = float(r["AverageNs"]) / 1e3
    for k, (v, n, meta) in srows.items():
        if "fused_psf_kernel<256>" in k and "SQ_INSTS_VALU" in v:
            json.dump({"kernel": "strict::fused_psf_kernel<256> (psf_map level of a strict stack: S=10, N=121, L=3, spp 2048 + 2048 chief)",
                       "code_sha256": code_sha256(*STRICT_SOURCES), "source": f"profiles/{tag}_strict_kernel_pmc.csv, profiles/{tag}_strict_kernel_stats.csv",
                       "us_per_launch_rocprof": us, "SQ_INSTS_VALU": v["SQ_INSTS_VALU"], "SQ_INSTS_VALU_TRANS": v.get("SQ_INSTS_VALU_TRANS"),
                       "valu_busy": round(min(1.0, v["SQ_ACTIVE_INST_VALU"] * 4 / (us * 1e-6 * 2.4e9 * 1024)), 3) if us and "SQ_ACTIVE_INST_VALU" in v else None},
                      open(os.path.join(P, "strict_kernel_pmc.json"), "w"), indent=1)

rows = write_pmc(os.path.join(P, f"{tag}_psf_kernel_pmc.csv"),
                 [one(f"{tag}_psf_pmc1/**/*counter_collection.csv"), one(f"{tag}_psf_pmc2/**/*counter_collection.csv")], ("psf_points_kernel",))
for k, (v, n, meta) in rows.items():
    if "SQ_INSTS_VALU" in v:
        stats = one(f"{tag}_stats_s1/**/*_kernel_stats.csv") or one(f"{tag}_stats/**/*_kernel_stats.csv")
        us = None
        for r in csv.DictReader(open(stats)):
            if "psf_points_kernel" in r["Name"]:
                us = float(r["AverageNs"]) / 1e3
        simd_cycles = us * 1e-6 * 2.4e9 * 1024 if us else None          # 256 CUs x 4 SIMDs at the 2.4 GHz peak clock
        json.dump({"kernel": "psf_points_kernel (S=10, N=121, L=3, spp 2048 + 2048 chief)", "code_sha256": code_sha256("trace.hip"), "source": f"profiles/{tag}_psf_kernel_pmc.csv, profiles/{tag}_{'kernel_stats_1stream' if one(f'{tag}_stats_s1/**/*_kernel_stats.csv') else 'kernel_stats'}.csv",
                   "us_per_launch_rocprof": us, "SQ_INSTS_VALU": v["SQ_INSTS_VALU"], "SQ_ACTIVE_INST_VALU_quadcycles": v.get("SQ_ACTIVE_INST_VALU"),
                   "valu_wave_instructions_per_surface_per_lane": round(v["SQ_INSTS_VALU"] / (178421760 / 128), 1),
                   "note": "a lane carries two rays (packed fp32), so one surface step of a lane = 2 ray-surface steps; 178 421 760 ray-surface steps per launch (SURVEY.md 8d); includes sampling, chief-ray reduction, compaction and splat",
                   "valu_busy": round(min(1.0, v["SQ_ACTIVE_INST_VALU"] * 4 / simd_cycles), 3) if simd_cycles else None,
                   "valu_busy_definition": "SQ_ACTIVE_INST_VALU (quad-cycles) x 4 / (kernel time x 2.4 GHz x 1024 SIMDs); the chip clocks below 2.4 GHz under load, so this is a lower bound",
                   "cycles_per_valu_instruction": round(simd_cycles / v["SQ_INSTS_VALU"], 2) if simd_cycles else None}, open(os.path.join(P, "psf_kernel_pmc.json"), "w"), indent=1)

f, w = one(f"{tag}_fetch/**/*counter_collection.csv"), one(f"{tag}_write/**/*counter_collection.csv")
if f and w:
    rows = write_pmc(os.path.join(P, f"{tag}_conv_traffic_pmc.csv"), [f, w], ("conv_psf_map_sbatch",))
    for k, (v, n, meta) in rows.items():
        fetch, write = v["FETCH_SIZE"] * 1024, v["WRITE_SIZE"] * 1024
        requested = 1452 * (34 * 108 * 4) + 1452 * 12 * 121 * 4          # what the workgroups ask L2 for: staged rows (with halo) + taps
        json.dump({"kernel": "conv_psf_map_sbatch_kernel (S=10 stack, 1024x1024x3)", "code_sha256": code_sha256("conv.hip"),
                   "source": f"rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE, separate passes on bench.py --streams 1 (tools/prof_r03.sh), profiles/{tag}_conv_traffic_pmc.csv",
                   "FETCH_SIZE_KB": v["FETCH_SIZE"], "WRITE_SIZE_KB": v["WRITE_SIZE"],
                   "correction": "MI355X_MICROARCH.md (HBM): the x2 FETCH_SIZE rule is calibrated for 16 B/lane streaming reads only; this kernel stages its "
                                 "band with 4 B/lane loads and stores 8 B/lane, both uncalibrated widths.  Calibration by bound: the counter tallies L2 "
                                 f"misses, which cannot exceed what the workgroups request from L2 ({requested / 1e6:.1f} MB: 1452 bands x (34 rows x 108 "
                                 "floats) + taps); x2 would read "
                                 f"{2 * fetch / 1e6:.1f} MB > that, so FETCH_SIZE is taken AS COUNTED here (x1; round 2 doubled it).  WRITE_SIZE as counted "
                                 "(output 125.8 MB -> 1.05x: consistent).  Both include Infinity-Cache hits.",
                   "l2_requested_bytes_per_launch": requested, "fetch_bytes_x2_for_reference": int(2 * fetch),
                   "hbm_bytes_per_launch": int(fetch + write), "unique_bytes_per_launch": 138412032, "algorithmic_bytes_per_launch": 251658240},
                  open(os.path.join(P, "conv_traffic.json"), "w"), indent=1)
cp = one(f"{tag}_conv_pmc/**/*counter_collection.csv")
if cp:
    write_pmc(os.path.join(P, f"{tag}_conv_kernel_pmc.csv"), [cp], ("conv_psf_map_sbatch",))
sp = one(f"{tag}_single_pmc/**/*counter_collection.csv")
if sp:
    write_pmc(os.path.join(P, f"{tag}_conv_single_kernel_pmc.csv"), [sp, one(f"{tag}_single_fetch/**/*counter_collection.csv"), one(f"{tag}_single_write/**/*counter_collection.csv")],
              ("conv_psf_map_blk", "conv_psf_map_mfma"))
for txt in ("latency_breakdown.txt", "soak.txt", "kbench.txt", "kbench_toeplitz.txt", "strict_profile.txt"):
    src = os.path.join(G, f"{tag}_{txt}")
    if os.path.exists(src) and os.path.getsize(src):
        shutil.copy(src, os.path.join(P, f"{tag}_{txt}"))
lp = one(f"{tag}_lp_fetch/**/*counter_collection.csv")
if lp:
    write_pmc(os.path.join(P, f"{tag}_local_psf_fetch_pmc.csv"), [lp], ("local_psf",))
print(sorted(f for f in os.listdir(P) if f.startswith(tag)))
