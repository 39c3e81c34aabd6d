#!/usr/bin/env python3
"""Parameter errors of every slice of a scene (lib.param_error_scene: Model.gain_scene, Model.kernel_scene under the
parameters' windows on the same model, Model.param_slices) on the two workloads of the other scene benchmarks, against the
route the library offered before: Model.gain_scene with the gain copied home, a second model created with the
parameters' windows for K_b, then per slice G.T @ Kb over the live measurements and the quadratic forms in numpy.  Writes
profiles/scene_param.json; asserts no threshold -- nobody has measured these before.

  A  64 profiles, nadir example, CO2 retrieved on all levels, T the parameter on all levels, 1e5 nadir rays
  B  64 profiles, limb example: 64 scans of the example's 66 rays, O3 retrieved on all levels, T the parameter

Weight comes from lib.error_components on the measurements; both routes use the same diagonal prior, 1e-2 of the mean
diagonal of A_s on every element.  The parameter covariances: one diagonal component (1 K^2) and one full component,
sigma_i sigma_j exp(-|dz| / 5 km) with sigma = 1 K from Model-side prior_corr_slices.

  device_s           lib.param_error_scene: one model; the gain and K_b come home and go up again for param_slices (an entry
                     that keeps both on the device is the sequel)
  host_s             gain_scene(want_gain) on the first model, kernel_scene on the second, then numpy per slice
  host_linalg_s      the numpy part of host_s alone
  second_model_s     creating the second model (a second upload of the tables), not part of host_s
  param_slices_s     Model.param_slices alone on arrays the host holds: uploads, the two kernels, C and sigma_param home
  kernels_ms         jur_scene_cross_kernel and jur_scene_param_kernel together, from the model's event timing
                     (jur_model_last_scene_ms) of a param_slices call of their own

Each time is the median of --steps calls after one warm-up call, a host clock around calls that end in a device
synchronise.

  baseline           Model.diagnose_scene and Model.retrieve_scene (workload B) as tools/bench_scene_gain.py measures them,
                     and, with --parent-so, the same from a library built from the parent commit: the two alternate in
                     processes of their own, --rounds each

  python tools/bench_scene_param.py [--steps 3] [--rays-a 100000] [--only A|B] [--rounds 5] [--parent-so path/to/libjurassic_hip.so]"""
import argparse, ctypes, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
from jurassic_hip import abi, lib
from bench_scene_jacobian import NPROF, median_s, workload
from bench_scene_step import scene_kernels_ms
from bench_scene_gain import baseline, error_inputs

KERNEL_RESOURCES = ("from the compiler's resource-usage remark for gfx950: jur_scene_cross_kernel 68 VGPRs, 16384 bytes of LDS, no "
                    "scratch, 7 waves/SIMD; jur_scene_param_kernel 90 VGPRs, 29312 bytes of LDS, no scratch, 5 waves/SIMD")
CZ_KM = 5.0


def copy_ctl(c):
    out = abi.ctl_t()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(c), ctypes.sizeof(abi.ctl_t))
    return out


def setup(name, nrays_a):
    """the workload with the gas alone retrieved (ctl_x, the model's) and T alone as the parameter (ctl_b)"""
    case = workload(name, nrays_a)
    ctl_x, ctl_b = copy_ctl(case.ctl), copy_ctl(case.ctl)
    ctl_x.rett_zmin, ctl_x.rett_zmax = -999.0, -999.0
    for g in range(ctl_b.ng):
        ctl_b.retq_zmin[g], ctl_b.retq_zmax[g] = -999.0, -999.0
    atm, geom = case.atm, case.geom
    model = lib.Model(ctl_x, case.lib_tables())
    model.set_atm(atm)
    rng = np.random.default_rng(5)
    y = model.formod_host(geom)["rad"] * (1.0 + 1e-3 * rng.standard_normal((len(geom), ctl_x.nd)))
    _, weight = error_inputs(y)
    first = model.normal_scene(atm, geom, y, weight)
    wptr, aptr = first["wptr"], first["aptr"]
    r = np.concatenate([np.full(int(wptr[s + 1] - wptr[s]), 1e-2 * np.diag(first["A"][aptr[s]:aptr[s + 1]].reshape(
        int(wptr[s + 1] - wptr[s]), -1)).mean()) for s in range(len(wptr) - 1)])
    return case, ctl_x, ctl_b, model, y, weight, r, first


def covariances(model, ctl_b, atm, first):
    """(var_b (1, nbw), cov_b (1, nbb), bwptr) over the T elements of every slice"""
    iq, z = [], []
    for f, l in zip(first["sfirst"], first["slen"]):
        el = lib.scene_elements(ctl_b, atm, int(f), int(l))
        iq.append(el["iq"]); z.append([atm.z[i] for i in el["ip"]])
    bwptr = np.concatenate([[0], np.cumsum([len(q) for q in iq])]).astype(np.int64)
    iq, z = np.concatenate(iq), np.concatenate(z)
    cz = np.zeros(2 + ctl_b.ng + ctl_b.nw)
    cz[1] = CZ_KM
    pc = lib.prior_corr_slices(model, bwptr, iq, z, np.ones(len(iq)), cz, want_Sa=True)
    assert np.all(pc["status"] == 0)
    return np.ones((1, len(iq))), pc["Sa"][None, :], bwptr


def host_param(gs, kb, weight, var_b, cov_b, bwptr, nd):
    """C and sigma_param of lib.param_error_scene from the gain and the blocks of K_b, per slice, in numpy"""
    wptr, rp, rb, sid = gs["wptr"], gs["rowptr"], kb["rowptr"], gs["sid"]
    bbptr = np.concatenate([[0], np.cumsum(np.diff(bwptr) ** 2)])
    sig = np.zeros((2, int(wptr[-1])))
    Cs = []
    live = np.isfinite(gs["rad"]) & (weight > 0)
    for s in range(len(wptr) - 1):
        w, wb = int(wptr[s + 1] - wptr[s]), int(bwptr[s + 1] - bwptr[s])
        rays = np.flatnonzero(sid == s)
        lm = live[rays].reshape(-1)
        Gm = np.concatenate([gs["gain"][rp[r] * nd:rp[r + 1] * nd].reshape(nd, w) for r in rays])[lm]
        Km = np.concatenate([kb["k"][rb[r] * nd:rb[r + 1] * nd].reshape(nd, wb) for r in rays])[lm]
        C = Gm.T @ Km
        Sg = cov_b[0, bbptr[s]:bbptr[s + 1]].reshape(wb, wb)
        sig[0, wptr[s]:wptr[s + 1]] = np.sqrt((C * C) @ var_b[0, bwptr[s]:bwptr[s + 1]])
        sig[1, wptr[s]:wptr[s + 1]] = np.sqrt(np.maximum(((C @ Sg) * C).sum(axis=1), 0.0))
        Cs.append(C.ravel())
    return np.concatenate(Cs), sig


def run(name, steps, nrays_a):
    case, ctl_x, ctl_b, model, y, weight, r, first = setup(name, nrays_a)
    atm, geom = case.atm, case.geom
    nd, nr = ctl_x.nd, len(geom)
    var_b, cov_b, bwptr = covariances(model, ctl_b, atm, first)
    keep = {"linalg_s": []}

    def device():
        keep["dev"] = lib.param_error_scene(model, ctl_b, atm, geom, y, weight, var_b=var_b, cov_b=cov_b, prior_ivar=r)
    device_s, device_all = median_s(device, steps)

    t0 = time.perf_counter()
    second = lib.Model(ctl_b, case.lib_tables())
    second.set_atm(atm)
    second_model_s = time.perf_counter() - t0

    def host():
        gs = model.gain_scene(atm, geom, y, weight, prior_ivar=r, want_gain=True)
        kb = second.kernel_scene(atm, geom)
        t1 = time.perf_counter()
        keep["host"] = host_param(gs, kb, weight, var_b, cov_b, bwptr, nd)
        keep["linalg_s"].append(time.perf_counter() - t1)
        keep["kb"] = kb
    host_s, host_all = median_s(host, steps)
    second.close()

    dev, kb = keep["dev"], keep["kb"]
    assert np.all(dev["status"] == 0) and np.array_equal(dev["bwptr"], bwptr)

    def slices():
        keep["ps"] = model.param_slices(dev["wptr"], dev["rowptr"], kb["rowptr"], dev["sid"], dev["gain"], kb["k"], dev["weight_eff"],
                                        var=var_b, cov=cov_b)
    slices_s, slices_all = median_s(slices, steps)
    kernels_ms, launches, timed_s = scene_kernels_ms(model, slices)
    model.close()
    ns, n = len(dev["wptr"]) - 1, int(dev["wptr"][-1])
    nk, nkb, nc = int(dev["rowptr"][-1]) * nd, int(kb["rowptr"][-1]) * nd, int(dev["cptr"][-1])
    forward_bytes = nr * (2 * nd * 8 + 3 * 8 + 4) + 2 * ns * 8               # rad, tau, tp, np; cost, nlive
    diag_bytes = 4 * n * 8 + ns * 8 + ns * 4                                 # the vectors, dofs, status
    host_C, host_sig = keep["host"]
    return {"rays": nr, "profiles": NPROF, "channels": nd, "slices": ns, "columns_per_slice": int(np.diff(dev["wptr"]).max()),
            "parameters_per_slice": int(np.diff(bwptr).max()), "components": {"diagonal": 1, "full": 1, "cz_km": CZ_KM},
            "device_s": device_s, "device_s_all": device_all, "host_s": host_s, "host_s_all": host_all,
            "host_linalg_s": float(np.median(keep["linalg_s"][1:])), "second_model_s": second_model_s,
            "host_over_device": host_s / device_s,
            "param_slices_s": slices_s, "param_slices_s_all": slices_all,
            "bytes_to_host_device_route": 2 * forward_bytes + diag_bytes + (nk + nkb + nc + 2 * n) * 8,
            "bytes_to_device_device_route_for_param_slices": (nk + nkb + nr * nd) * 8 + (var_b.size + cov_b.size) * 8,
            "bytes_to_host_host_route": 2 * forward_bytes + diag_bytes + (nk + nkb) * 8,
            "gain_bytes": nk * 8, "kb_bytes": nkb * 8, "C_bytes": nc * 8,
            "largest_relative_difference_of_the_two_routes": {
                "C": float(np.abs(dev["C"] - host_C).max() / np.abs(host_C).max()),
                "sigma_param": float(np.abs(dev["sigma_param"] - host_sig).max() / np.abs(host_sig).max())},
            "event_timed_call": {"param_slices_call_s": timed_s, "kernels_ms": kernels_ms, "timed_intervals": launches,
                                 "kernels_share_of_param_slices": kernels_ms * 1e-3 / timed_s,
                                 "kernels_share_of_param_error_scene": kernels_ms * 1e-3 / device_s,
                                 "copies_and_host_work_of_param_slices_s": slices_s - kernels_ms * 1e-3}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rays-a", type=int, default=100000)
    ap.add_argument("--only", choices=["A", "B"])
    ap.add_argument("--rounds", type=int, default=5, help="alternating runs of this commit's and the parent's library")
    ap.add_argument("--parent-so", help="a libjurassic_hip.so built from the parent commit: its times are measured in processes of their own")
    ap.add_argument("--baseline-only", action="store_true", help="print the baseline times as one JSON line and stop")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_param.json"))
    args = ap.parse_args()
    if args.baseline_only:
        print("BASELINE " + json.dumps(baseline(args.steps)), flush=True)
        return
    doc = {"what": "parameter errors of every slice of a scene: lib.param_error_scene (one model: gain_scene, kernel_scene under the "
                   "parameters' windows, param_slices) with one diagonal and one full covariance of T, a single gas retrieved, against "
                   "gain_scene with the gain home, kernel_scene on a second model and G.T @ Kb plus the quadratic forms per slice in "
                   "numpy (tools/bench_scene_param.py)",
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
