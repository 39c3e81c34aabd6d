#!/usr/bin/env python3
"""Gain matrix and per-source error budget of every slice of a scene (Model.gain_scene, jur_gain_scene_host) on the two
workloads of the other scene benchmarks, against the route the library offered before: Model.diagnose_scene with S and
the blocks copied home, then per slice (S @ K.T) * omega and the row sums of G^2 var in numpy.  Writes
profiles/scene_gain.json; asserts no threshold -- nobody has measured these before.

  A  64 profiles, nadir example, T and CO2 retrieved on all levels, 1e5 nadir rays
  B  64 profiles, limb example: 64 scans of the example's 66 rays, T and O3 retrieved on all levels

Weight and the two variances (noise, forward model) come from lib.error_components on the measurements; both routes use
the same diagonal prior, 1e-2 of the mean diagonal of A_s on every element (tools/bench_scene_diagnose.py's).

  device_s           Model.gain_scene with two components, the gain left on the device (only sigma_comp and the
                     diagnostics' vectors come home)
  device_gain_s      the same with want_gain: the gain comes home too
  host_s             Model.diagnose_scene(want_S, want_k), then the products and the sums per slice in numpy
  host_linalg_s      the numpy part of host_s alone

Each time is the median of --steps calls after one warm-up call, a host clock around calls that end in a device
synchronise.  The new kernels' time comes from the model's event timing (jur_model_last_scene_ms) in calls of their own:
the scene kernels' time of a gain_scene call less that of a diagnose_scene call is the effective-weight, gain and budget
kernels (the passes of the two calls are cut alike where max_rays_per_pass is given; with 0 the retained blocks change
the cut, and the difference carries that too).

  baseline           Model.diagnose_scene and Model.retrieve_scene (workload B), and, with --parent-so, the same from a
                     library built from the parent commit: the two alternate in processes of their own, --rounds each

  python tools/bench_scene_gain.py [--steps 3] [--rays-a 100000] [--only A|B] [--rounds 5] [--parent-so path/to/libjurassic_hip.so]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
from jurassic_hip import lib
from bench_scene_jacobian import NPROF, median_s, workload
from bench_scene_step import scene_kernels_ms

ERR_NOISE, ERR_FORMOD = 1e-5, 1.0          # radiance units; per cent
KERNEL_RESOURCES = ("from the compiler's resource-usage remark for gfx950: jur_scene_gain_kernel 70 VGPRs, 17792 bytes of LDS, no "
                    "scratch, 7 waves/SIMD; jur_scene_budget_kernel 50 VGPRs, 9216 bytes of LDS, no scratch, 8 waves/SIMD; "
                    "jur_scene_weff_kernel 6 VGPRs, no LDS, no scratch")


def setup(name, nrays_a):
    case = workload(name, nrays_a)
    c, atm, geom = case.ctl, case.atm, case.geom
    model = lib.Model(c, case.lib_tables())
    model.set_atm(atm)
    rng = np.random.default_rng(5)
    y = model.formod_host(geom)["rad"] * (1.0 + 1e-3 * rng.standard_normal((len(geom), c.nd)))
    var, weight = error_inputs(y)
    first = model.normal_scene(atm, geom, y, weight)
    wptr, aptr = first["wptr"], first["aptr"]
    r = np.concatenate([np.full(int(wptr[s + 1] - wptr[s]), 1e-2 * np.diag(first["A"][aptr[s]:aptr[s + 1]].reshape(
        int(wptr[s + 1] - wptr[s]), -1)).mean()) for s in range(len(wptr) - 1)])
    return case, model, y, weight, var, r


def error_inputs(y):
    return lib.error_components(y, np.full(y.shape[1], ERR_NOISE), np.full(y.shape[1], ERR_FORMOD))


def host_gain(out, weight, var, nd):
    """sigma_comp of Model.gain_scene from S and the blocks, per slice, in numpy (the gain of every slice is formed)"""
    wptr, aptr, rp, sid = out["wptr"], out["aptr"], out["rowptr"], out["sid"]
    sig = np.zeros((var.shape[0], int(wptr[-1])))
    live = np.isfinite(out["rad"]) & (weight > 0)
    omega = np.where(live, weight, 0.0)
    for s in range(len(wptr) - 1):
        w = int(wptr[s + 1] - wptr[s])
        rays = np.flatnonzero(sid == s)
        S = out["S"][aptr[s]:aptr[s + 1]].reshape(w, w)
        K = np.concatenate([out["k"][rp[r] * nd:rp[r + 1] * nd].reshape(nd, w) for r in rays])
        G = (S @ K.T) * omega[rays].reshape(-1)
        sig[:, wptr[s]:wptr[s + 1]] = np.sqrt((var[:, rays].reshape(var.shape[0], -1) @ (G * G).T))
    return sig


def run(name, steps, nrays_a):
    case, model, y, weight, var, r = setup(name, nrays_a)
    c, atm, geom = case.ctl, case.atm, case.geom
    nd, nr = c.nd, len(geom)
    keep = {"linalg_s": []}

    def device():
        keep["dev"] = model.gain_scene(atm, geom, y, weight, var=var, prior_ivar=r)
    device_s, device_all = median_s(device, steps)

    def device_gain():
        keep["gain"] = model.gain_scene(atm, geom, y, weight, var=var, prior_ivar=r, want_gain=True)
    gain_s, gain_all = median_s(device_gain, steps)

    def host():
        out = model.diagnose_scene(atm, geom, y, weight, prior_ivar=r, want_S=True, want_k=True)
        t0 = time.perf_counter()
        keep["host"] = host_gain(out, weight, var, nd)
        keep["linalg_s"].append(time.perf_counter() - t0)
        keep["lay"] = {f: out[f] for f in ("wptr", "aptr", "rowptr")}
    host_s, host_all = median_s(host, steps)

    dev, lay = keep["dev"], keep["lay"]
    assert np.all(dev["status"] == 0)
    ns, n, na, nk = len(lay["wptr"]) - 1, int(lay["wptr"][-1]), int(lay["aptr"][-1]), int(lay["rowptr"][-1]) * nd
    gain_ms, gain_launches, timed_s = scene_kernels_ms(model, lambda: model.gain_scene(atm, geom, y, weight, var=var, prior_ivar=r))
    diag_ms, diag_launches, _ = scene_kernels_ms(model, lambda: model.diagnose_scene(atm, geom, y, weight, prior_ivar=r))
    model.close()
    forward_bytes = nr * (2 * nd * 8 + 3 * 8 + 4) + 2 * ns * 8               # rad, tau, tp, np; cost, nlive
    diag_bytes = 4 * n * 8 + ns * 8 + ns * 4                                 # the vectors, dofs, status
    host_sig = keep["host"]
    return {"rays": nr, "profiles": NPROF, "channels": nd, "slices": ns, "columns_per_slice": int(np.diff(lay["wptr"]).max()),
            "components": int(var.shape[0]), "err_noise": ERR_NOISE, "err_formod_per_cent": ERR_FORMOD,
            "device_s": device_s, "device_s_all": device_all, "device_gain_s": gain_s, "device_gain_s_all": gain_all,
            "host_s": host_s, "host_s_all": host_all, "host_linalg_s": float(np.median(keep["linalg_s"][1:])),
            "host_over_device": host_s / device_s, "host_over_device_with_the_gain_home": host_s / gain_s,
            "bytes_to_host_device_route": forward_bytes + diag_bytes + var.shape[0] * n * 8,
            "bytes_to_host_device_route_with_the_gain": forward_bytes + diag_bytes + var.shape[0] * n * 8 + nk * 8,
            "bytes_to_host_host_route": forward_bytes + diag_bytes + (na + nk) * 8,
            "blocks_bytes": nk * 8, "S_bytes": na * 8,
            "device_memory_of_the_retained_blocks_and_the_gain": 2 * nk * 8,
            "largest_relative_difference_of_the_two_routes": float(np.abs(dev["sigma_comp"] - host_sig).max() / np.abs(host_sig).max()),
            "event_timed_call": {"call_s": timed_s, "scene_kernels_ms_gain_scene": gain_ms, "scene_kernels_ms_diagnose_scene": diag_ms,
                                 "timed_intervals_added": gain_launches - diag_launches, "gain_kernels_ms": gain_ms - diag_ms,
                                 "gain_kernels_share_of_the_call": (gain_ms - diag_ms) * 1e-3 / timed_s}}


def baseline(steps):
    """diagnose_scene and retrieve_scene on workload B: entries the parent commit has too"""
    from bench_scene_retrieve import FAC, LAM0, LAM_MAX, LAM_MIN, MAX_ITER, TOL
    from bench_scene_recomp import setup as loop_setup, found_prior, retrieval
    case, model, lay, y, weight, x0, diagonal = loop_setup("B", 0)
    c, atm, geom = case.ctl, case.atm, case.geom
    prior, _ = found_prior(case, model, y, weight, diagonal)
    r = diagonal[0]

    def diagnose():
        model.set_atm(atm)
        model.diagnose_scene(atm, geom, y, weight, prior_ivar=r)
    out = {}
    for name, fn in (("diagnose_scene", diagnose), ("retrieve_scene", retrieval(case, model, y, weight, prior))):
        med, every = median_s(fn, steps)
        out[name + "_s"], out[name + "_s_all"] = med, every
    model.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rays-a", type=int, default=100000)
    ap.add_argument("--only", choices=["A", "B"])
    ap.add_argument("--rounds", type=int, default=5, help="alternating runs of this commit's and the parent's library")
    ap.add_argument("--parent-so", help="a libjurassic_hip.so built from the parent commit: its times are measured in processes of their own")
    ap.add_argument("--baseline-only", action="store_true", help="print the baseline times as one JSON line and stop")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_gain.json"))
    args = ap.parse_args()
    if args.baseline_only:
        print("BASELINE " + json.dumps(baseline(args.steps)), flush=True)
        return
    doc = {"what": "gain matrix and error budget of every slice of a scene: Model.gain_scene with two components (noise, forward "
                   "model), the gain left on the device or copied home, against Model.diagnose_scene(want_S, want_k) plus "
                   "(S @ K.T) * omega and the row sums per slice in numpy (tools/bench_scene_gain.py)",
           "timing": "median of %d calls after one warm-up, host clock around calls that end in a device synchronise; pageable host "
                     "arrays on both routes; no target was set for any of these numbers" % args.steps,
           "device": lib.device_info(0)["pci_bus_id"], "kernel_resources": KERNEL_RESOURCES}
    for name in ("A", "B"):
        if args.only in (None, name):
            doc[name] = run(name, args.steps, args.rays_a)
            print(name, json.dumps(doc[name]), flush=True)

    def child(so):
        env = dict(os.environ)
        if so:
            env["JURASSIC_HIP_SO"] = os.path.abspath(so)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-only", "--steps", str(args.steps)], env=env,
                             capture_output=True, text=True, check=True).stdout
        return json.loads([ln for ln in out.splitlines() if ln.startswith("BASELINE ")][-1][len("BASELINE "):])

    if args.parent_so:
        rounds = []
        for _ in range(args.rounds):
            rounds.append({"this_commit": child(None), "parent_commit": child(args.parent_so)})
            print("round " + json.dumps(rounds[-1]), flush=True)
        so = {"rounds": rounds}
        for f in ("diagnose_scene", "retrieve_scene"):
            this = [r_["this_commit"][f + "_s"] for r_ in rounds]
            parent = [r_["parent_commit"][f + "_s"] for r_ in rounds]
            so[f] = {"this_commit_medians_s": this, "parent_commit_medians_s": parent,
                     "this_commit_spread_s": [min(this), max(this)], "parent_commit_spread_s": [min(parent), max(parent)],
                     "median_of_this_commit_inside_the_parents_spread": bool(min(parent) <= sorted(this)[len(this) // 2] <= max(parent)),
                     "median_of_this_commit_at_or_below_the_parents_maximum": bool(sorted(this)[len(this) // 2] <= max(parent))}
        doc["existing_entries"] = so
    elif not args.no_baseline:
        doc["existing_entries"] = {"this_commit": baseline(args.steps)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
