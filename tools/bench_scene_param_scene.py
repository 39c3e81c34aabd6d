#!/usr/bin/env python3
"""Model.param_scene (jur_param_scene_host: the gain and K_b stay on the device) against lib.param_error_scene (gain_scene,
kernel_scene under the parameters' windows, param_slices: the gain and K_b come home and go up again) on the two workloads
and with the inputs of tools/bench_scene_param.py, on one model.  Writes profiles/scene_param_scene.json; asserts no
threshold.

  A  64 profiles, nadir example, CO2 retrieved on all levels, T the parameter on all levels, 1e5 nadir rays
  B  64 profiles, limb example: 64 scans of the example's 66 rays, O3 retrieved on all levels, T the parameter

  route_s / entry_s  one call each per round, the two alternating for --rounds rounds after a warm-up call of each; a host
                     clock around calls that end in a device synchronise; medians and [min, max]
  bytes              what each route copies to the host and to the device, counted from the shapes
  device_bytes       jur_model_workspace_bytes (the forward model's workspace) and jur_model_scene_bytes (the slab of the
                     scene entries and param_scene's buffer beside it) after one call of either route on a model of its own
  cross_pass_kernel  jur_scene_cross_pass_kernel in an event-timed call of param_scene: its total time, launches and share
  existing_entries   gain_scene, kernel_scene (A and B) and retrieve_scene (B; A where it goes through) with this commit's
                     library and, with --parent-so, one built from the parent commit: processes of their own, alternating

  python tools/bench_scene_param_scene.py [--rounds 5] [--steps 3] [--rays-a 100000] [--only A|B] [--parent-so path]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
from jurassic_hip import lib
from bench_scene_jacobian import median_s
from bench_scene_param import covariances, setup

KERNEL_RESOURCES = ("from the build's resource report for gfx950 (tools/kernel_regs.sh): jur_scene_cross_pass_kernel 74 VGPRs, 74 SGPRs, "
                    "16384 bytes of LDS, no scratch; jur_scene_cross_kernel 68 VGPRs, 16384 bytes of LDS, no scratch, as before")


def spread(t):
    return {"all_s": t, "median_s": statistics.median(t), "spread_s": [min(t), max(t)]}


def run(name, rounds, nrays_a):
    case, ctl_x, ctl_b, model, y, weight, r, first = setup(name, nrays_a)
    atm, geom = case.atm, case.geom
    nd, nr = ctl_x.nd, len(geom)
    var_b, cov_b, bwptr = covariances(model, ctl_b, atm, first)
    keep = {}

    def route(m=model):
        keep["route"] = lib.param_error_scene(m, ctl_b, atm, geom, y, weight, var_b=var_b, cov_b=cov_b, prior_ivar=r)

    def entry(m=model):
        keep["entry"] = m.param_scene(ctl_b, atm, geom, y, weight, var_b=var_b, cov_b=cov_b, prior_ivar=r)

    route(); entry()                                          # warm-up: workspace, slab, buffer and code objects
    t_route, t_entry = [], []
    for _ in range(rounds):
        for fn, t in ((route, t_route), (entry, t_entry)):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
    a, b = keep["route"], keep["entry"]
    same = all(np.array_equal(a[f], b[f], equal_nan=True) for f in ("C", "sigma_param", "sigma", "rad", "weight_eff", "sigma_comp"))
    model.enable_timing(True)
    t0 = time.perf_counter()
    entry()
    timed_s = time.perf_counter() - t0
    model.kernel_ms()
    sc, cr = model.scene_ms(), model.cross_ms()
    model.enable_timing(False)
    model.close()

    def device_bytes(fn):
        m = lib.Model(ctl_x, case.lib_tables())
        m.set_atm(atm)
        fn(m)
        out = {"workspace_bytes": m.workspace_bytes(), "scene_bytes": m.scene_bytes()}
        m.close()
        return out

    ns, n = len(a["wptr"]) - 1, int(a["wptr"][-1])
    nk, nkb, nc = int(a["rowptr"][-1]) * nd, int(a["rowptr_b"][-1]) * nd, int(a["cptr"][-1])
    forward = nr * (2 * nd * 8 + 3 * 8 + 4) + 2 * ns * 8               # rad, tau, tp, np; cost, nlive
    diag = 4 * n * 8 + ns * 8 + ns * 4                                 # the vectors, dofs, status
    inputs = nr * (7 + 3 * nd) * 8 + n * 8                             # geometry, mask, y, weight; prior_ivar (per forward pass)
    cov_bytes = (var_b.size + cov_b.size) * 8
    med_r, med_e = statistics.median(t_route), statistics.median(t_entry)
    return {"rays": nr, "channels": nd, "slices": ns, "columns_per_slice": int(np.diff(a["wptr"]).max()),
            "parameters_per_slice": int(np.diff(bwptr).max()), "rounds": rounds,
            "route_param_error_scene": spread(t_route), "entry_param_scene": spread(t_entry),
            "route_minus_entry_median_s": med_r - med_e, "route_over_entry": med_r / med_e,
            "entry_median_inside_the_routes_spread": bool(min(t_route) <= med_e <= max(t_route)),
            "the_two_routes_agree_bit_for_bit": bool(same),
            "bytes": {"route_to_host": 2 * forward + diag + (nk + nkb + nc + 2 * n) * 8,
                      "route_to_device": 2 * inputs - n * 8 + (nk + nkb + nr * nd) * 8 + cov_bytes,
                      "entry_to_host": forward + diag + (nc + 2 * n + nr * nd) * 8,
                      "entry_to_device": 2 * inputs - n * 8 + cov_bytes,
                      "gain_bytes": nk * 8, "kb_bytes": nkb * 8, "C_bytes": nc * 8},
            "device_bytes": {"route": device_bytes(route), "entry": device_bytes(entry)},
            "cross_pass_kernel": {"timed_call_s": timed_s, "cross_ms": cr["cross_ms"], "launches": cr["cross_launches"],
                                  "share_of_the_call": cr["cross_ms"] * 1e-3 / timed_s, "all_scene_kernels_ms": sc["scene_ms"]}}


def existing(steps, nrays_a):
    """gain_scene, kernel_scene and retrieve_scene: entries the parent commit has too"""
    from bench_scene_recomp import setup as loop_setup, found_prior, retrieval
    out = {}
    for name in ("A", "B"):
        case, ctl_x, ctl_b, model, y, weight, r, first = setup(name, nrays_a)
        atm, geom = case.atm, case.geom
        for what, fn in (("gain_scene", lambda: model.gain_scene(atm, geom, y, weight, prior_ivar=r, want_gain=True)),
                         ("kernel_scene", lambda: model.kernel_scene(atm, geom))):
            med, every = median_s(fn, steps)
            out["%s_%s_s" % (what, name)], out["%s_%s_s_all" % (what, name)] = med, every
        model.close()
        try:
            case, model, lay, y, weight, x0, diagonal = loop_setup(name, nrays_a)
            prior, _ = found_prior(case, model, y, weight, diagonal)
            med, every = median_s(retrieval(case, model, y, weight, prior), steps)
            out["retrieve_scene_%s_s" % name], out["retrieve_scene_%s_s_all" % name] = med, every
            model.close()
        except (lib.JurassicError, SystemExit) as e:
            out["retrieve_scene_%s_error" % name] = str(e)[:300]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rays-a", type=int, default=100000)
    ap.add_argument("--only", choices=["A", "B"])
    ap.add_argument("--parent-so", help="a libjurassic_hip.so built from the parent commit")
    ap.add_argument("--existing-only", action="store_true", help="print the existing entries' times as one JSON line and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_param_scene.json"))
    args = ap.parse_args()
    if args.existing_only:
        print("EXISTING " + json.dumps(existing(args.steps, args.rays_a)), flush=True)
        return
    doc = {"what": "Model.param_scene (jur_param_scene_host) against lib.param_error_scene on one model, one diagonal and one full "
                   "covariance of T, a single gas retrieved (tools/bench_scene_param_scene.py)",
           "timing": "one call of each route per round, alternating, after a warm-up call of each; host clock around calls that end in "
                     "a device synchronise; pageable host arrays; no target was set for any of these numbers",
           "device": lib.device_info(0)["pci_bus_id"], "kernel_resources": KERNEL_RESOURCES}
    for name in ("A", "B"):
        if args.only in (None, name):
            doc[name] = run(name, args.rounds, args.rays_a)
            print(name, json.dumps(doc[name]), flush=True)

    def child(so):
        env = dict(os.environ)
        if so:
            env["JURASSIC_HIP_SO"] = os.path.abspath(so)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--existing-only", "--steps", str(args.steps), "--rays-a",
                              str(args.rays_a)], env=env, capture_output=True, text=True, check=True).stdout
        return json.loads([ln for ln in out.splitlines() if ln.startswith("EXISTING ")][-1][len("EXISTING "):])

    if args.parent_so:
        rounds = []
        for _ in range(args.rounds):
            rounds.append({"this_commit": child(None), "parent_commit": child(args.parent_so)})
            print("round " + json.dumps(rounds[-1]), flush=True)
        so = {"rounds": rounds}
        for f in sorted(k for k in rounds[0]["this_commit"] if k.endswith("_s")):
            this = [r_["this_commit"][f] for r_ in rounds]
            parent = [r_["parent_commit"][f] for r_ in rounds if f in r_["parent_commit"]]
            if len(parent) != len(this):
                continue
            so[f[:-2]] = {"this_commit_medians_s": this, "parent_commit_medians_s": parent,
                          "this_commit_spread_s": [min(this), max(this)], "parent_commit_spread_s": [min(parent), max(parent)],
                          "median_of_this_commit_inside_the_parents_spread": bool(min(parent) <= statistics.median(this) <= max(parent)),
                          "median_of_this_commit_at_or_below_the_parents_maximum": bool(statistics.median(this) <= max(parent))}
        doc["existing_entries"] = so
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
