#!/usr/bin/env python3
"""The Curtis-Godson look-up (FORMOD 1, jur_cga_kernel) beside the emissivity-growth look-up (FORMOD 2, jur_ega_kernel)
on bench.py's limb workload (1e6 rays, 4 channels, 5 emitters) and on nadir 1e5 x 3.  Writes profiles/cga.json; asserts
no threshold -- nobody has measured these before.

  lookup            the look-up kernel's event time (slot [1] of jur_model_last_kernel_ms, summed over the call's
                    launches) of one device-resident jur_formod_device call under FORMOD 1 and under FORMOD 2 on the same
                    atmosphere, rays and tables: --rounds alternating rounds, each a fresh model, one warm-up call and
                    one timed call; median and range, and the other two kernels' times of the same calls
  resources         VGPRs, SGPRs, scratch of every jur_cga_kernel / jur_ega_kernel instance from the compiler's metadata,
                    the dynamic LDS of the launch, and the vector-ALU instructions in each kernel's TEXT (a static count:
                    the executed count was not measured)
  bench             with --parent-so: `python bench.py` on this commit's library and on a library built from the parent
                    commit, --rounds alternating rounds in processes of their own -- the emissivity-growth side must not
                    move

  python tools/bench_cga.py [--rounds 5] [--parent-so path/to/libjurassic_hip.so] [--resources file.json]
  python tools/bench_cga.py --resources-only --out file.json      (no GPU: compiles the kernels to assembly)"""
import argparse, json, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np


def resources():
    """{kernel instance: vgprs, sgprs, scratch_bytes, static_lds_bytes, valu_instructions_in_text}"""
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
        m = re.search(r"14jur_(cga|ega)_kernelILb([01])ELb([01])ELb([01])E", name)
        if not m:
            continue
        key = "jur_%s_kernel<%s>" % (m.group(1), ", ".join("true" if b == "1" else "false" for b in m.groups()[1:]))
        start = text.index("\n" + name + ":")
        body = text[start:text.index("s_endpgm", start)]
        out[key] = {"vgprs": int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)),
                    "sgprs": int(re.search(r"\.sgpr_count:\s+(\d+)", block).group(1)),
                    "scratch_bytes": int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)),
                    "static_lds_bytes": int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1)),
                    "valu_instructions_in_text": len(re.findall(r"^\s+v_\w+", body, re.M)),
                    "fp64_valu_instructions_in_text": len(re.findall(r"^\s+v_\w+_f64", body, re.M))}
    return {"template_arguments": "WARM, LDS, RCPB (bench.py's tables take <true, true, true>)", "kernels": out,
            "note": "instruction counts are of the kernel's text, loops counted once -- the executed count was not measured"}


def lookup(workload, rounds):
    import torch
    import bench
    from jurassic_hip import abi, lib
    dev = torch.device("cuda", 0)
    n = bench.WORKLOADS[workload]["total"]
    case = bench.build_case(workload, bench.workload_rays(workload, np.arange(n)))
    nd = case.ctl.nd
    tables = case.lib_tables()
    d_geom = torch.from_numpy(np.ascontiguousarray(case.geom.T)).to(dev)
    d_rad = torch.zeros((n, nd), dtype=torch.float64, device=dev)
    d_tau, d_tp = torch.zeros_like(d_rad), torch.zeros((3, n), dtype=torch.float64, device=dev)
    d_status = torch.zeros(1, dtype=torch.int32, device=dev)

    def one(formod):
        ctl = abi.ctl_t.from_buffer_copy(bytes(case.ctl))
        ctl.formod = formod
        model = lib.Model(ctl, tables, device=0)
        model.set_atm(case.atm)
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
        mean = float(d_rad.mean().item())
        model.close()
        if not ok:
            raise SystemExit("%s FORMOD %d: NLOS overflow or a non-finite radiance" % (workload, formod))
        return dict(res, mean_radiance=mean)

    series = {1: [], 2: []}
    for _ in range(rounds):
        for formod in (1, 2):
            series[formod].append(one(formod))
            print("%s FORMOD %d %s" % (workload, formod, json.dumps(series[formod][-1])), flush=True)
    out = {"rays": n, "channels": nd, "emitters": case.ctl.ng, "rounds": rounds}
    for formod, name in ((1, "formod1_cga"), (2, "formod2_ega")):
        ms = [r["ega_ms"] for r in series[formod]]
        out[name] = {"lookup_ms": ms, "lookup_ms_median": float(np.median(ms)), "lookup_ms_range": [min(ms), max(ms)],
                     "lookup_launches": series[formod][0]["ega_launches"], "pencil_launches": series[formod][0]["pencil_launches"],
                     "trace_ms_median": float(np.median([r["trace_ms"] for r in series[formod]])),
                     "combine_ms_median": float(np.median([r["combine_ms"] for r in series[formod]])),
                     "mean_radiance": series[formod][0]["mean_radiance"]}
    out["cga_over_ega_lookup_time"] = out["formod1_cga"]["lookup_ms_median"] / out["formod2_ega"]["lookup_ms_median"]
    return out


def bench_rounds(parent_so, rounds, parent_first=False):
    def child(so):
        env = dict(os.environ)
        if so:
            env["JURASSIC_HIP_SO"] = os.path.abspath(so)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1"], env=env,
                             capture_output=True, text=True, check=True, timeout=300).stdout   # (a failure ends the tool)
        doc = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
        return {"value": doc["value"], "unit": doc.get("unit")}
    this, parent = [], []
    for _ in range(rounds):
        if parent_first:
            parent.append(child(parent_so)["value"])
            this.append(child(None)["value"])
        else:
            this.append(child(None)["value"])
            parent.append(child(parent_so)["value"])
        print("bench.py round: this %.4g parent %.4g rays/s" % (this[-1], parent[-1]), flush=True)
    med = sorted(this)[len(this) // 2]
    return {"command": "python bench.py --gpus 1 --steps 5 --warmup 1", "unit": "rays/s",
            "first_in_every_round": "parent_commit" if parent_first else "this_commit", "this_commit": this, "parent_commit": parent,
            "this_commit_median": med, "parent_commit_median": sorted(parent)[len(parent) // 2],
            "parent_commit_spread": [min(parent), max(parent)],
            "median_of_this_commit_inside_the_parents_spread": bool(min(parent) <= med <= max(parent)),
            "median_of_this_commit_at_or_above_the_parents_minimum": bool(med >= min(parent))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-so", help="a libjurassic_hip.so built from the parent commit: bench.py alternates between the two")
    ap.add_argument("--resources", help="a file written by --resources-only (default: compile here)")
    ap.add_argument("--resources-only", action="store_true", help="write the kernels' resource usage and stop (needs no GPU)")
    ap.add_argument("--bench-only", action="store_true", help="only the bench.py rounds against --parent-so")
    ap.add_argument("--parent-first", action="store_true", help="the parent's library runs first in every bench.py round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cga.json"))
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
    doc = {"what": "Curtis-Godson look-up (FORMOD 1) beside the emissivity-growth look-up (FORMOD 2): event time of the look-up "
                   "kernel of one device-resident forward-model call on the same inputs, resource usage of the kernels, and "
                   "bench.py on this commit and on the parent (tools/bench_cga.py)",
           "timing": "HIP events around every launch of the call (jur_model_enable_timing); %d alternating rounds, each a fresh model "
                     "with one warm-up call; no target was set for any of these numbers" % args.rounds,
           "device": lib.device_info(0)["pci_bus_id"]}
    doc["resources"] = json.load(open(args.resources)) if args.resources else resources()
    # dynamic LDS of both kernels: 24 bytes per level slot and per curve of the largest pair (33 levels x 10 temperatures)
    doc["resources"]["dynamic_lds_bytes_per_workgroup"] = 24 * 40 + 24 * 330
    for workload in ("limb_1e6", "nadir_1e5"):
        doc[workload] = lookup(workload, args.rounds)
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
