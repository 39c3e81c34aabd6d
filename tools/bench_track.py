#!/usr/bin/env python3
"""The 2-D ray tracer (IP 2, jur_track_trace_kernel) beside the 1-D tracers on the same rays: bench.py's limb rays (1e6,
4 channels, 5 emitters) on a homogeneous track of 64 profiles in one time block under IP 2 against the same rays under
IP 1 on one profile, and 1e5 nadir rays the same way.  Writes profiles/track.json; asserts no threshold -- nobody has
measured these before.

  trace             the tracer's event time (slot [0] of jur_model_last_kernel_ms, summed over the call's launches) of
                    one device-resident jur_formod_device call under IP 2 and under IP 1: --rounds alternating rounds,
                    each a fresh model, one warm-up call and one timed call; median and range, the other two kernels'
                    times of the same calls, and the largest relative difference of the radiances (a homogeneous
                    track is the one profile, up to the rounding of (1 - r) y + r y)
  resources         VGPRs, SGPRs, scratch and static LDS of the tracer kernels from the compiler's metadata
  bench             with --parent-so: `python bench.py` on this commit's library and on a library built from the parent
                    commit, --rounds alternating rounds in processes of their own -- the 1-D kernels must not move

  python tools/bench_track.py [--rounds 5] [--parent-so path/to/libjurassic_hip.so] [--parent-first]
  python tools/bench_track.py --resources-only --out file.json      (no GPU: compiles the kernels to assembly)"""
import argparse, json, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
from bench_cga import bench_rounds

NPROFILES = 64


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
        m = re.search(r"\d+(jur_trace_(?:slice_|lanes_)?kernel|jur_track_trace_kernel)", name)
        if not m:
            continue
        out[m.group(1)] = {"vgprs": int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)),
                           "sgprs": int(re.search(r"\.sgpr_count:\s+(\d+)", block).group(1)),
                           "scratch_bytes": int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)),
                           "static_lds_bytes": int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))}
    return {"kernels": out, "note": "scratch of jur_track_trace_kernel includes the frames of track_geo and redo_columns_track, "
                                    "which it calls out of line"}


def trace(workload, rounds):
    import torch
    import bench
    import common
    import track_model as T
    from jurassic_hip import abi, lib
    dev = torch.device("cuda", 0)
    n = bench.WORKLOADS[workload]["total"]
    geom = bench.workload_rays(workload, np.arange(n))
    geom[:, 0] = 0.0                                         # one time block
    limb = bench.WORKLOADS[workload]["kind"] == "limb"
    case = common.limb_case(geom=geom, nu=common.CTM4_NU) if limb else common.nadir_case(geom=geom)
    nprof = min(NPROFILES, abi.NP // case.atm.np)
    lats = np.linspace(8.0, 46.0, nprof) if limb else np.linspace(-19.0, 19.0, nprof)     # the paths stay inside the track
    track = T.track_atmosphere(case.ctl, case.atm, lats=tuple(lats.tolist()), graded=False, thinned=None, second_block=False)
    nd = case.ctl.nd
    tables = case.lib_tables()
    d_geom = torch.from_numpy(np.ascontiguousarray(case.geom.T)).to(dev)
    d_rad = torch.zeros((n, nd), dtype=torch.float64, device=dev)
    d_tau, d_tp = torch.zeros_like(d_rad), torch.zeros((3, n), dtype=torch.float64, device=dev)
    d_status = torch.zeros(1, dtype=torch.int32, device=dev)
    rad = {}

    def one(ip):
        ctl = abi.ctl_t.from_buffer_copy(bytes(case.ctl))
        ctl.ip = ip
        model = lib.Model(ctl, tables, device=0)
        model.set_atm(track if ip == 2 else case.atm)
        model.reserve(n)
        res = None
        for timed in (False, True):
            model.enable_timing(timed)
            d_rad.zero_()
            model.formod_device(n, d_geom.data_ptr(), d_rad.data_ptr(), d_tau.data_ptr(), d_tp.data_ptr(), 0,
                                d_status.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            if timed:
                res = model.kernel_ms()
        ok = int(d_status.item()) == 0 and bool(torch.isfinite(d_rad).all())
        rad[ip] = d_rad.clone()
        model.close()
        if not ok:
            raise SystemExit("%s IP %d: NLOS overflow or a non-finite radiance" % (workload, ip))
        return res

    series = {1: [], 2: []}
    for _ in range(rounds):
        for ip in (2, 1):
            series[ip].append(one(ip))
            print("%s IP %d %s" % (workload, ip, json.dumps(series[ip][-1])), flush=True)
    out = {"rays": n, "channels": nd, "emitters": case.ctl.ng, "rounds": rounds, "profiles_of_the_track": nprof,
           "levels_per_profile": case.atm.np,
           "largest_relative_radiance_difference_ip2_ip1": float(((rad[2] - rad[1]).abs() / rad[1].abs().clamp_min(1e-300)).max().item())}
    for ip, name in ((2, "ip2_track"), (1, "ip1_profile")):
        ms = [r["trace_ms"] for r in series[ip]]
        out[name] = {"trace_ms": ms, "trace_ms_median": float(np.median(ms)), "trace_ms_range": [min(ms), max(ms)],
                     "trace_launches": series[ip][0]["trace_launches"], "pencil_launches": series[ip][0]["pencil_launches"],
                     "lookup_ms_median": float(np.median([r["ega_ms"] for r in series[ip]])),
                     "combine_ms_median": float(np.median([r["combine_ms"] for r in series[ip]]))}
    out["ip2_over_ip1_trace_time"] = out["ip2_track"]["trace_ms_median"] / out["ip1_profile"]["trace_ms_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-so", help="a libjurassic_hip.so built from the parent commit: bench.py alternates between the two")
    ap.add_argument("--resources", help="a file written by --resources-only (default: compile here)")
    ap.add_argument("--resources-only", action="store_true", help="write the kernels' resource usage and stop (needs no GPU)")
    ap.add_argument("--bench-only", action="store_true", help="only the bench.py rounds against --parent-so")
    ap.add_argument("--parent-first", action="store_true", help="the parent's library runs first in every bench.py round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track.json"))
    args = ap.parse_args()
    if args.resources_only:
        with open(args.out, "w") as f:
            json.dump(resources(), f, indent=1)
            f.write("\n")
        return
    if args.bench_only:
        with open(args.out, "w") as f:
            json.dump({"bench_py": bench_rounds(args.parent_so, args.rounds, args.parent_first)}, f, indent=1)
            f.write("\n")
        return
    import torch
    assert torch.cuda.is_available()                 # torch's HIP runtime first: the one loaded first serves both
    from jurassic_hip import lib
    doc = {"what": "2-D ray tracer (IP 2, jur_track_trace_kernel: full scan of the block's profiles at every evaluation, no warm "
                   "start) beside the 1-D tracers on the same rays: event time of the tracer of one device-resident forward-model "
                   "call, resource usage of the tracer kernels, and bench.py on this commit and on the parent (tools/bench_track.py)",
           "timing": "HIP events around every launch of the call (jur_model_enable_timing); %d alternating rounds, each a fresh model "
                     "with one warm-up call; no target was set for any of these numbers" % args.rounds,
           "device": lib.device_info(0)["pci_bus_id"]}
    doc["resources"] = json.load(open(args.resources)) if args.resources else resources()
    for workload in ("limb_1e6", "nadir_1e5"):
        doc[workload] = trace(workload, args.rounds)
        print(workload + " " + json.dumps(doc[workload]), flush=True)
    if args.parent_so:
        doc["bench_py"] = bench_rounds(args.parent_so, args.rounds, args.parent_first)
        print("bench_py " + json.dumps(doc["bench_py"]), flush=True)
    else:
        doc["bench_py"] = "not measured: no --parent-so given"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
