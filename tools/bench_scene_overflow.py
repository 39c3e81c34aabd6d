#!/usr/bin/env python3
"""Untraceable rays isolated in the scene retrieval (Model.set_scene_overflow) on the two workloads of
tools/bench_scene_retrieve.py.  Writes profiles/scene_overflow.json; asserts no threshold -- nobody has measured these
before.

  A  64 profiles, nadir example, T and CO2 retrieved on all levels, 1e5 nadir rays
  B  64 profiles, limb example: 64 scans of the example's 66 rays, T and O3 retrieved on all levels

Settings: max_iter = 4, tol = 0, fac = (0.1, 1, 10), lam0 = 1, Marquardt damping; the prior is found as
tools/bench_scene_retrieve.py finds it (none, or the diagonal one where the call without it ends with JUR_ENLOS) with the
switch off.

  switch_off   Model.step_scene and Model.retrieve_scene with the switch never touched: wall time and the launches of an
               event-timed call, and, with --parent-so, the same from a library built from the parent commit: the two
               alternate in processes of their own, --rounds each, --steps calls per round
  switch_on    the same retrieve_scene call under OVERFLOW_ISOLATE: wall time, the launches and the scene kernels' time of
               an event-timed call beside those of the switch-off call (the launches added are jur_scene_overflow_kernel
               once a pass and jur_scene_overflow_fold_kernel twice an iteration; they are not timed by themselves:
               added_scene_kernel_ms is the difference of the sums of ONE call each way, an upper bound within the
               scatter of such a call), the counters
  B_no_prior   workload B without a prior under OVERFLOW_ISOLATE, the call that ends with JUR_ENLOS while the switch is
               off: how it ends -- slices per final state, iterations, overflowing trials by iteration, wall time

Each time is the median of --steps calls after one warm-up call, a host clock around calls that end in a device
synchronise.

  python tools/bench_scene_overflow.py [--steps 3] [--rays-a 100000] [--rounds 5] [--parent-so path/to/libjurassic_hip.so]"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
from jurassic_hip import lib
from bench_scene_jacobian import median_s
from bench_scene_step import scene_kernels_ms
from bench_scene_retrieve import FAC, MAX_ITER
from bench_scene_recomp import found_prior, retrieval, setup

STATES = ("active", "converged", "stalled", "maxiter", "failed")


def baseline(steps, nrays_a):
    """step_scene and retrieve_scene on both workloads with the switch never touched (a parent library has no such entry)"""
    out = {}
    for name in ("A", "B"):
        case, model, lay, y, weight, x0, diagonal = setup(name, nrays_a)
        atm, geom = case.atm, case.geom
        prior, _ = found_prior(case, model, y, weight, diagonal)

        def step():
            model.set_atm(atm)
            kw = dict(prior_ivar=prior[0], prior_dx=np.zeros(len(x0))) if prior else {}
            model.step_scene(atm, geom, y, weight, np.array(FAC), **kw)
        res = {}
        for entry, fn in (("step_scene", step), ("retrieve_scene", retrieval(case, model, y, weight, prior))):
            med, every = median_s(fn, steps)
            ms, launches, _ = scene_kernels_ms(model, fn)
            res[entry + "_s"], res[entry + "_s_all"], res[entry + "_scene_launches"] = med, every, launches
        out[name] = res
        model.close()
    return out


def how_it_ended(model, ret):
    over = ret["h_status"] == lib.TRIAL_OVERFLOW
    return {"slices_per_final_state": dict(zip(STATES, (int(v) for v in np.bincount(ret["state"], minlength=5)))),
            "iterations_run": int(ret["iters"].max()), "iterations_per_slice_min_median_max": [int(ret["iters"].min()), float(np.median(ret["iters"])), int(ret["iters"].max())],
            "overflowing_trials_by_iteration": [int(o.sum()) for o in over],
            "slices_with_an_overflowing_trial_by_iteration": [int(o.any(axis=0).sum()) for o in over],
            "steps_accepted_by_iteration": [int((a == 1).sum()) for a in ret["h_accept"]],
            "counters_trial_cells_and_failed_slices": list(model.last_scene_overflow()),
            "rays_that_overflow_on_the_result": int(sum(lib.np_overflows(n) for n in ret["np"])),
            "sum_J_by_iteration_over_the_slices_that_did_not_fail": [float(v) for v in np.nansum(np.where(ret["state"] == lib.RET_FAILED, np.nan, ret["h_cost"] + ret["h_prior"]), axis=1)]}


def switch_on(name, steps, nrays_a):
    case, model, lay, y, weight, x0, diagonal = setup(name, nrays_a)
    prior, refused = found_prior(case, model, y, weight, diagonal)
    res = {"rays": len(case.geom), "slices": len(lay["sfirst"]), "diagonal_prior": prior is not None, "max_iter": MAX_ITER, "fac": list(FAC),
           "calls_that_ended_with_an_error_with_the_switch_off": refused}
    keep = {}
    for mode, label in ((lib.OVERFLOW_ERROR, "off"), (lib.OVERFLOW_ISOLATE, "on")):
        model.set_scene_overflow(mode)
        call = retrieval(case, model, y, weight, prior, keep)
        med, runs = median_s(call, steps)
        ms, launches, dt = scene_kernels_ms(model, call)
        res[label] = {"wall_s": med, "wall_s_all": runs, "event_timed_call": {"call_s": dt, "scene_kernels_ms": ms, "scene_launches": launches}}
        if mode == lib.OVERFLOW_ISOLATE:
            res[label]["how_it_ended"] = how_it_ended(model, keep["ret"])
    res["added_launches"] = res["on"]["event_timed_call"]["scene_launches"] - res["off"]["event_timed_call"]["scene_launches"]
    res["added_scene_kernel_ms"] = res["on"]["event_timed_call"]["scene_kernels_ms"] - res["off"]["event_timed_call"]["scene_kernels_ms"]
    res["added_scene_kernel_ms_as_a_share_of_the_call"] = res["added_scene_kernel_ms"] * 1e-3 / res["on"]["wall_s"]
    res["wall_on_relative_to_off"] = res["on"]["wall_s"] / res["off"]["wall_s"]
    if name == "B":                                 # the README's workload: no prior, the call that ends with JUR_ENLOS today
        model.set_scene_overflow(lib.OVERFLOW_ISOLATE)
        call = retrieval(case, model, y, weight, None, keep)
        med, runs = median_s(call, steps)
        res["no_prior_switch_on"] = dict(how_it_ended(model, keep["ret"]), wall_s=med, wall_s_all=runs)
    model.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rays-a", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=5, help="alternating runs of this commit's and the parent's library")
    ap.add_argument("--parent-so", help="a libjurassic_hip.so built from the parent commit: its switch-off times are measured in processes of their own")
    ap.add_argument("--baseline-only", action="store_true", help="print the switch-off times as one JSON line and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_overflow.json"))
    args = ap.parse_args()
    if args.baseline_only:
        print("BASELINE " + json.dumps(baseline(args.steps, args.rays_a)), flush=True)
        return
    doc = {"what": "untraceable rays isolated in Model.retrieve_scene (Model.set_scene_overflow) on 1e5 nadir rays (A) and 64 limb scans "
                   "(B): the switch-off times against the parent commit's, the switch-on call beside the switch-off call, and workload "
                   "B without a prior, which ends with JUR_ENLOS while the switch is off (tools/bench_scene_overflow.py)",
           "timing": "median of %d calls after one warm-up, host clock around calls that end in a device synchronise; pageable host "
                     "arrays; no target was set for any of these numbers and nobody had measured them before" % args.steps,
           "device": lib.device_info(0)["pci_bus_id"]}
    for name in ("A", "B"):
        doc[name] = switch_on(name, args.steps, args.rays_a)
        print(name, json.dumps(doc[name]), flush=True)

    def child(so):
        env = dict(os.environ)
        if so:
            env["JURASSIC_HIP_SO"] = os.path.abspath(so)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-only", "--steps", str(args.steps), "--rays-a", str(args.rays_a)],
                             env=env, capture_output=True, text=True, check=True).stdout
        return json.loads([ln for ln in out.splitlines() if ln.startswith("BASELINE ")][-1][len("BASELINE "):])

    if not args.parent_so:
        doc["switch_off"] = {"this_commit": baseline(args.steps, args.rays_a)}
    else:
        rounds = []
        for _ in range(args.rounds):
            rounds.append({"this_commit": child(None), "parent_commit": child(args.parent_so)})
            print("round " + json.dumps(rounds[-1]), flush=True)
        so = {"rounds": rounds}
        for name in ("A", "B"):
            for f in ("step_scene", "retrieve_scene"):
                this = [r_["this_commit"][name][f + "_s"] for r_ in rounds]
                parent = [r_["parent_commit"][name][f + "_s"] for r_ in rounds]
                so[name + "_" + f] = {"this_commit_medians_s": this, "parent_commit_medians_s": parent,
                                      "this_commit_spread_s": [min(this), max(this)], "parent_commit_spread_s": [min(parent), max(parent)],
                                      "median_of_this_commit_inside_the_parents_spread": bool(min(parent) <= sorted(this)[len(this) // 2] <= max(parent)),
                                      "median_of_this_commit_at_or_below_the_parents_maximum": bool(sorted(this)[len(this) // 2] <= max(parent)),
                                      "scene_launches_this_commit_and_parent": [rounds[0]["this_commit"][name][f + "_scene_launches"],
                                                                                rounds[0]["parent_commit"][name][f + "_scene_launches"]]}
        doc["switch_off"] = so
    print(json.dumps(doc["switch_off"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
