#!/usr/bin/env python3
"""The point-cloud ray tracer (IP 3, jur_cloud_trace_kernel) beside the 1-D and 2-D tracers on the same rays: the first
1e5 of bench.py's limb rays (4 channels, 5 emitters) and its 1e5 nadir rays, on clouds of 256, 1024 and
cloud_lds_points() + 1 points in one time block under IP 3, against the same rays under IP 1 on one profile and under
IP 2 on a track of as many profiles as the cloud has columns.  Writes profiles/cloud.json; asserts no threshold -- nobody
has measured these before.

  trace             the tracer's event time (slot [0] of jur_model_last_kernel_ms, summed over the call's launches) of
                    one device-resident jur_formod_device call: --rounds alternating rounds over all configurations,
                    each a fresh model, one warm-up call and one timed call; median and range.  The cloud: columns of
                    the case's profile spread over the latitudes the rays cross, every point moved by a seeded
                    +-0.2 km and +-0.05 degrees, cut to the number of points; cx = 4000 km, cz = 3 km, so that no
                    position is a hole and every scan applies all three gates to every point.
  estimate          counted before anything ran: scans = 5 evaluations x points x steps per ray
  resources         VGPRs, SGPRs, scratch and static LDS of the tracer kernels from the compiler's metadata
  bench             with --parent-so: `python bench.py` on this commit's library and on a library built from the parent
                    commit, --rounds alternating rounds in processes of their own -- the 1-D kernels must not move.
                    --bench-only adds the rounds of its order (--parent-first or not) to the file --out holds already

  python tools/bench_cloud.py [--rounds 5] [--parent-so path/to/libjurassic_hip.so] [--parent-first]
  python tools/bench_cloud.py --resources-only --out file.json      (no GPU: compiles the kernels to assembly)"""
import argparse, json, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
from bench_cga import bench_rounds

NRAYS = 100000
CX, CZ = 4000.0, 3.0


def resources():
    """{tracer kernel: vgprs, sgprs, scratch_bytes, static_lds_bytes}"""
    csrc = os.path.join(ROOT, "jurassic-gpu_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "k.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-ffp-contract=off", "-std=c++17",
                               "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-DJUR_ND=100", "-DJUR_NG=30", "-S",
                               "--cuda-device-only", "-o", asm, os.path.join(csrc, "jur_kernels.hip")], stderr=subprocess.DEVNULL)
        text = open(asm).read()
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for block in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.search(r"\d+(jur_trace_(?:slice_|lanes_)?kernel|jur_track_trace_kernel|jur_cloud_trace_kernel)", name)
        if not m:
            continue
        out[m.group(1)] = {"vgprs": int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)),
                           "sgprs": int(re.search(r"\.sgpr_count:\s+(\d+)", block).group(1)),
                           "scratch_bytes": int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)),
                           "static_lds_bytes": int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))}
    lds = out.get("jur_cloud_trace_kernel", {}).get("static_lds_bytes", 0)
    return {"kernels": out, "lds_per_cu_bytes": 163840,
            "jur_cloud_trace_kernel_workgroups_per_cu_by_lds": (163840 // lds) if lds else None,
            "note": "scratch of jur_cloud_trace_kernel includes the frames of track_geo, cloud_probe, cloud_point (the means of "
                    "a point: 2 + JUR_NG + JUR_NW doubles) and redo_columns_cloud, which it calls out of line; launch bounds "
                    "(256, 2): two workgroups of 256 lanes per CU, two waves per SIMD"}


def trace(workload, rounds, sizes):
    import torch
    import bench
    import common
    import cloud_model as CM
    import track_model as T
    from jurassic_hip import abi, lib
    dev = torch.device("cuda", 0)
    n = min(NRAYS, bench.WORKLOADS[workload]["total"])
    geom = bench.workload_rays(workload, np.arange(n))
    geom[:, 0] = 0.0                                         # one time block
    limb = bench.WORKLOADS[workload]["kind"] == "limb"
    case = common.limb_case(geom=geom, nu=common.CTM4_NU) if limb else common.nadir_case(geom=geom)
    lo, hi = (8.0, 46.0) if limb else (-19.0, 19.0)          # the latitudes the rays cross (tools/bench_track.py)
    nd = case.ctl.nd
    tables = case.lib_tables()
    d_geom = torch.from_numpy(np.ascontiguousarray(case.geom.T)).to(dev)
    d_rad = torch.zeros((n, nd), dtype=torch.float64, device=dev)
    d_tau, d_tp = torch.zeros_like(d_rad), torch.zeros((3, n), dtype=torch.float64, device=dev)
    d_np = torch.zeros(n, dtype=torch.int32, device=dev)
    d_status = torch.zeros(1, dtype=torch.int32, device=dev)
    atms, columns = {}, {}
    for npts in sizes:
        ncol = max(2, -(-npts // case.atm.np))
        lats = tuple(np.linspace(lo, hi, ncol).tolist())
        columns[npts] = ncol
        atms[(3, npts)] = CM.join(CM.columns(case.ctl, case.atm, lats, seed=npts, npoints=npts))
        # (IP 2 refuses neighbours more than 10 degrees apart: the track keeps the number of profiles and, where it must,
        # gives up the span -- beyond its ends a point takes the end profile, and the scan costs the same)
        step = min((hi - lo) / (ncol - 1), 9.5)
        lats2 = tuple((0.5 * (lo + hi) + step * (i - 0.5 * (ncol - 1))) for i in range(ncol))
        atms[(2, npts)] = T.track_atmosphere(case.ctl, case.atm, lats=lats2, graded=False, thinned=None, second_block=False)
    atms[(1, 0)] = case.atm
    steps = {}

    def one(ip, npts):
        ctl = abi.ctl_t.from_buffer_copy(bytes(case.ctl))
        ctl.ip, ctl.cx, ctl.cz = ip, CX, CZ
        model = lib.Model(ctl, tables, device=0)
        model.set_atm(atms[(ip, npts)])
        model.reserve(n)
        res = None
        for timed in (False, True):
            model.enable_timing(timed)
            d_rad.zero_()
            model.formod_device(n, d_geom.data_ptr(), d_rad.data_ptr(), d_tau.data_ptr(), d_tp.data_ptr(), d_np.data_ptr(),
                                d_status.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            if timed:
                res = model.kernel_ms()
        ok = int(d_status.item()) == 0 and bool(torch.isfinite(d_rad).all())
        steps[(ip, npts)] = float(d_np.double().mean().item())
        model.close()
        if not ok:
            raise SystemExit("%s IP %d, %d points: NLOS overflow or a non-finite radiance" % (workload, ip, npts))
        return res

    configs = [(3, s) for s in sizes] + [(2, s) for s in sizes] + [(1, 0)]
    series = {c: [] for c in configs}
    for _ in range(rounds):
        for c in configs:
            series[c].append(one(*c))
            print("%s IP %d points %d %s" % (workload, c[0], c[1], json.dumps(series[c][-1])), flush=True)
    out = {"rays": n, "channels": nd, "emitters": case.ctl.ng, "rounds": rounds, "levels_per_column": case.atm.np, "cx_km": CX, "cz_km": CZ,
           "refraction": int(case.ctl.refrac)}

    def stats(c):
        ms = [r["trace_ms"] for r in series[c]]
        return {"trace_ms": ms, "trace_ms_median": float(np.median(ms)), "trace_ms_range": [min(ms), max(ms)],
                "trace_launches": series[c][0]["trace_launches"], "mean_points_per_ray": steps[c]}
    out["ip1_profile"] = stats((1, 0))
    for s in sizes:
        e = {"columns": columns[s], "ip3_cloud": stats((3, s)), "ip2_track_of_as_many_profiles": stats((2, s))}
        e["ip3_over_ip1_trace_time"] = e["ip3_cloud"]["trace_ms_median"] / out["ip1_profile"]["trace_ms_median"]
        e["ip3_over_ip2_trace_time"] = e["ip3_cloud"]["trace_ms_median"] / e["ip2_track_of_as_many_profiles"]["trace_ms_median"]
        evals = (5 if case.ctl.refrac else 1) * steps[(3, s)] * n
        e["scans_counted"] = {"evaluations": evals, "point_gates": evals * s}
        e["wall_ps_per_point_gate"] = 1e9 * e["ip3_cloud"]["trace_ms_median"] / (evals * s)
        out["points_%d" % s] = e
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-so", help="a libjurassic_hip.so built from the parent commit: bench.py alternates between the two")
    ap.add_argument("--resources", help="a file written by --resources-only (default: compile here)")
    ap.add_argument("--resources-only", action="store_true", help="write the kernels' resource usage and stop (needs no GPU)")
    ap.add_argument("--bench-only", action="store_true", help="only the bench.py rounds against --parent-so")
    ap.add_argument("--parent-first", action="store_true", help="the parent's library runs first in every bench.py round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud.json"))
    args = ap.parse_args()
    if args.resources_only:
        with open(args.out, "w") as f:
            json.dump(resources(), f, indent=1)
            f.write("\n")
        return
    order = "parent_commit_first" if args.parent_first else "this_commit_first"

    def write(doc):
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    def add_bench(doc):
        """the rounds of this order go beside whatever the file holds already, the other order's rounds included"""
        b = doc.get("bench_py")
        b = dict(b) if isinstance(b, dict) else {}
        b[order] = bench_rounds(args.parent_so, args.rounds, args.parent_first)
        both = [b[o] for o in ("this_commit_first", "parent_commit_first") if o in b]
        if len(both) == 2:
            this, parent = both[0]["this_commit"] + both[1]["this_commit"], both[0]["parent_commit"] + both[1]["parent_commit"]
            med = sorted(this)[len(this) // 2]
            b["both_runs_together"] = {"this_commit_median": med, "parent_commit_median": sorted(parent)[len(parent) // 2],
                                       "parent_commit_spread": [min(parent), max(parent)],
                                       "median_of_this_commit_at_or_above_the_parents_minimum": bool(med >= min(parent))}
        doc["bench_py"] = b
        print("bench_py " + json.dumps(b[order]), flush=True)

    if args.bench_only:                                  # merged into the file a full run has written, if there is one
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        add_bench(doc)
        write(doc)
        return
    import torch
    assert torch.cuda.is_available()                 # torch's HIP runtime first: the one loaded first serves both
    from jurassic_hip import lib
    limit = lib.cloud_lds_points()
    sizes = sorted({256, 1024, limit + 1})
    doc = {"what": "point-cloud ray tracer (IP 3, jur_cloud_trace_kernel: full scan of the block's points at every evaluation, no "
                   "warm start, no pruning) beside the 1-D and 2-D tracers on the same rays: event time of the tracer of one "
                   "device-resident forward-model call, resource usage of the tracer kernels, and bench.py on this commit and on "
                   "the parent (tools/bench_cloud.py)",
           "timing": "HIP events around every launch of the call (jur_model_enable_timing); %d alternating rounds over all "
                     "configurations, each a fresh model with one warm-up call; no target was set for any of these numbers" % args.rounds,
           "staging_limit_points": limit,
           "estimate_before_measuring": "scans = 5 evaluations x points x steps per ray: a limb ray of some 180 steps on 1024 points "
                                        "applies 9e5 point gates, 1e5 such rays 9e10; at some 12 fp64 instructions a gate and 2 "
                                        "cycles an instruction on 16 384 lanes at 2.4 GHz that is about 55 ms per 1e5 limb rays, a "
                                        "quarter of it on 256 points, and the same again beyond the staging limit if the L2 serves the "
                                        "gates as fast as LDS does",
           "device": lib.device_info(0)["pci_bus_id"]}
    doc["resources"] = json.load(open(args.resources)) if args.resources else resources()
    for workload in ("limb_1e6", "nadir_1e5"):
        doc[workload.replace("limb_1e6", "limb_1e5")] = trace(workload, args.rounds, sizes)
        print(workload + " " + json.dumps(doc[workload.replace("limb_1e6", "limb_1e5")]), flush=True)
        write(doc)                                       # (what has been measured so far is kept if a later stage ends the run)
    if args.parent_so:
        add_bench(doc)
    else:
        doc["bench_py"] = "not measured: no --parent-so given"
    write(doc)


if __name__ == "__main__":
    main()
