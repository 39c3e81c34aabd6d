#!/usr/bin/env python3
"""The scene Jacobian reused between the iterations of a retrieval (Model.set_kernel_recomp, upstream's KERNEL_RECOMP) on
the two workloads of tools/bench_scene_retrieve.py.  Writes profiles/scene_recomp.json; asserts no threshold -- nobody
has measured these before.

  A  64 profiles, nadir example, T and CO2 retrieved on all levels, 1e5 nadir rays
  B  64 profiles, limb example: 64 scans of the example's 66 rays, T and O3 retrieved on all levels

Settings: max_iter = 4, tol = 0, fac = (0.1, 1, 10), lam0 = 1, Marquardt damping; the prior is found as
tools/bench_scene_retrieve.py finds it (none, or the diagonal one where the call without it ends with JUR_ENLOS) with the
switch off and then kept for every setting of the switch.

  every = 1, 2, 4   one Model.retrieve_scene call each: wall time, h_work (rays traced for the Jacobian or the gradient
                    and for the trials, by iteration), the scene kernels' time and launches of an event-timed call
                    (jur_model_last_scene_ms), the bytes moved each way (from the shapes; the blocks never leave the
                    device) and the device memory the retained blocks take, and per slice the final cost + prior
                    relative to the every = 1 run: stale Jacobians trade iterations for time, and the user chooses
  gradient_scene    one Model.gradient_scene call on the blocks of Model.kernel_scene: wall time and the scene kernels of
                    the call (stacking, replication and mask, the gathering of the results, jur_scene_gradient_kernel):
                    the new kernel's time is at most that sum
  switch_off        Model.step_scene and Model.retrieve_scene with the switch never touched, and, with --parent-so, the
                    same from a library built from the parent commit: the two alternate in processes of their own,
                    --rounds each (workload B)

Each time is the median of --steps calls after one warm-up call, a host clock around calls that end in a device
synchronise.

  python tools/bench_scene_recomp.py [--steps 5] [--rays-a 100000] [--only A|B] [--rounds 5] [--parent-so path/to/libjurassic_hip.so]"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
from jurassic_hip import lib
from bench_scene_jacobian import NPROF, median_s, workload
from bench_scene_step import scene_kernels_ms
from bench_scene_retrieve import FAC, LAM0, LAM_MAX, LAM_MIN, MAX_ITER, TOL, rows_of

EVERY = (1, 2, 4)


def setup(name, nrays_a):
    case = workload(name, nrays_a)
    c, atm, geom = case.ctl, case.atm, case.geom
    model = lib.Model(c, case.lib_tables())
    model.set_atm(atm)
    lay = lib.scene_slices(c, atm, geom[:, 0])
    els = [lib.scene_elements(c, atm, lay["sfirst"][s], lay["slen"][s]) for s in range(len(lay["sfirst"]))]
    iq, ip = np.concatenate([e["iq"] for e in els]), np.concatenate([e["ip"] for e in els])
    rng = np.random.default_rng(5)
    y = model.formod_host(geom)["rad"] * (1.0 + 1e-3 * rng.standard_normal((len(geom), c.nd)))
    weight = 10.0 ** rng.uniform(0.0, 3.0, y.shape)
    rows0 = rows_of(c, atm)
    x0 = np.array([rows0[q][p] for q, p in zip(iq, ip)])
    sigma = np.where(iq == 1, 1.0, 0.1 * np.abs(x0) + 1e-12)
    return case, model, lay, y, weight, x0, (1.0 / sigma ** 2, x0)


def retrieval(case, model, y, weight, prior, keep=None):
    c, atm, geom = case.ctl, case.atm, case.geom

    def call():
        model.set_atm(atm)
        pk = dict(prior_ivar=prior[0], prior_xa=prior[1]) if prior else {}
        out = model.retrieve_scene(atm, geom, y, weight, MAX_ITER, FAC, lam0=LAM0, lam_min=LAM_MIN, lam_max=LAM_MAX, tol=TOL,
                                   history=True, **pk)
        if keep is not None:
            keep["ret"] = out
    return call


def found_prior(case, model, y, weight, diagonal):
    """none, or the diagonal one where the call without it ends with an error (the switch off)"""
    refused = []
    for prior in (None, diagonal):
        try:
            retrieval(case, model, y, weight, prior)()
            return prior, refused
        except lib.JurassicError as e:
            refused.append({"prior": prior is not None, "error": str(e)})
    raise SystemExit("neither route went through: %s" % refused)


def baseline(steps):
    """step_scene and retrieve_scene on workload B with the switch never touched (a parent library has no such entry)"""
    case, model, lay, y, weight, x0, diagonal = setup("B", 0)
    c, atm, geom = case.ctl, case.atm, case.geom
    prior, _ = found_prior(case, model, y, weight, diagonal)

    def step():
        model.set_atm(atm)
        kw = dict(prior_ivar=prior[0], prior_dx=np.zeros(len(x0))) if prior else {}
        model.step_scene(atm, geom, y, weight, np.array(FAC), **kw)
    out = {}
    for name, fn in (("step_scene", step), ("retrieve_scene", retrieval(case, model, y, weight, prior))):
        med, every = median_s(fn, steps)
        out[name + "_s"], out[name + "_s_all"] = med, every
    model.close()
    return out


def run(name, steps, nrays_a):
    case, model, lay, y, weight, x0, diagonal = setup(name, nrays_a)
    c, atm, geom = case.ctl, case.atm, case.geom
    nd, nr = c.nd, len(geom)
    prior, refused = found_prior(case, model, y, weight, diagonal)
    ns, n, nlam = len(lay["sfirst"]), int(lay["wptr"][-1]), len(FAC)
    rowptr = lib.scene_layout(c, atm, geom[:, 0])["rowptr"]
    nrow = 6 + c.ng + c.nw
    res = {"rays": nr, "profiles": NPROF, "channels": nd, "slices": ns, "columns_per_slice": int(np.diff(lay["wptr"]).max()),
           "max_iter": MAX_ITER, "tol": TOL, "fac": list(FAC), "lam0": LAM0, "diagonal_prior": prior is not None,
           "calls_that_ended_with_an_error": refused,
           "retained_blocks_bytes_on_the_device": int(rowptr[-1]) * nd * 8}
    keep, final = {}, {}
    for every in EVERY:
        model.set_kernel_recomp(every)
        call = retrieval(case, model, y, weight, prior, keep)
        med, runs = median_s(call, steps)
        ms, launches, dt = scene_kernels_ms(model, call)
        ret = keep["ret"]
        iters = int(ret["iters"].max())
        ray_in = nr * (7 * 8 + 3 * nd * 8 + 3 * 4 + 8)
        results = nr * (2 * nd * 8 + 3 * 8 + 4)
        scalars = ns * (3 * 8 + 8) + nlam * ns * (3 * 8 + 4)
        choices = ns * (4 + 4) + nlam * ns * 8
        offsets = sum(int(w[0] > 0) for w in ret["h_work"][:iters]) * nr * 8 if every > 1 else 0   # the per-ray block offsets, at most once an iteration
        final[every] = ret["cost"] + ret["prior"]
        rel = final[every] / final[1]
        res["every_%d" % every] = {
            "wall_s": med, "wall_s_all": runs, "wall_relative_to_every_1": med / res["every_1"]["wall_s"] if every > 1 else 1.0,
            "h_work_jacobian_or_gradient_and_trial_rays_by_iteration": ret["h_work"].tolist(),
            "iterations_run": iters, "states": [int(v) for v in np.bincount(ret["state"], minlength=4)],
            "steps_accepted_by_iteration": [int((a == 1).sum()) for a in ret["h_accept"]],
            "event_timed_call": {"call_s": dt, "scene_kernels_ms": ms, "scene_launches": launches},
            "bytes_to_device": ray_in + nrow * atm.np * 8 + nr * 4 * 3 + iters * choices + offsets,
            "bytes_to_host": results + n * 8 + iters * scalars,
            "sum_J_by_iteration": [float(v) for v in (ret["h_cost"] + ret["h_prior"]).sum(axis=1)] + [float(final[every].sum())],
            "final_J_relative_to_every_1": {"sum": float(final[every].sum() / final[1].sum()), "per_slice_min": float(rel.min()),
                                            "per_slice_median": float(np.median(rel)), "per_slice_max": float(rel.max()),
                                            "per_slice": [float(v) for v in rel]}}
        print(name, "every", every, json.dumps({k: v for k, v in res["every_%d" % every].items() if k != "final_J_relative_to_every_1"}), flush=True)
    model.set_kernel_recomp(1)

    model.set_atm(atm)
    k = model.kernel_scene(atm, geom)["k"]

    def gradient():
        model.set_atm(atm)
        model.gradient_scene(atm, geom, y, weight, k)
    med, runs = median_s(gradient, steps)
    ms, launches, dt = scene_kernels_ms(model, gradient)
    res["gradient_scene"] = {"wall_s": med, "wall_s_all": runs, "blocks_to_device_bytes": int(k.nbytes),
                             "event_timed_call": {"call_s": dt, "scene_kernels_ms_all_of_the_call": ms, "scene_launches": launches}}
    model.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rays-a", type=int, default=100000)
    ap.add_argument("--only", choices=["A", "B"])
    ap.add_argument("--rounds", type=int, default=5, help="alternating runs of this commit's and the parent's library")
    ap.add_argument("--parent-so", help="a libjurassic_hip.so built from the parent commit: its switch-off times are measured in processes of their own")
    ap.add_argument("--baseline-only", action="store_true", help="print the switch-off times as one JSON line and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_recomp.json"))
    args = ap.parse_args()
    if args.baseline_only:
        print("BASELINE " + json.dumps(baseline(args.steps)), flush=True)
        return
    doc = {"what": "the scene Jacobian reused between the iterations of Model.retrieve_scene (Model.set_kernel_recomp): every = 1, 2, 4 "
                   "on 1e5 nadir rays (A) and 64 limb scans (B), Model.gradient_scene alone, and the switch-off times against the "
                   "parent commit's (tools/bench_scene_recomp.py)",
           "timing": "median of %d calls after one warm-up, host clock around calls that end in a device synchronise; pageable host "
                     "arrays; no target was set for any of these numbers and nobody had measured them before" % args.steps,
           "expectation_from_ray_counts": "a reuse iteration traces one ray per ray where a Jacobian iteration traces width + 1: every = 4 "
                                          "should remove most of three of the four Jacobian passes",
           "device": lib.device_info(0)["pci_bus_id"],
           "kernel_resources": "jur_scene_gradient_kernel, from the compiler's report for gfx950: 34 VGPRs, 65 SGPRs, 3072 bytes of LDS, no scratch, no spills"}
    for name in ("A", "B"):
        if args.only in (None, name):
            doc[name] = run(name, args.steps, args.rays_a)

    def child(so):
        env = dict(os.environ)
        if so:
            env["JURASSIC_HIP_SO"] = os.path.abspath(so)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-only", "--steps", str(args.steps)], env=env,
                             capture_output=True, text=True, check=True).stdout
        return json.loads([ln for ln in out.splitlines() if ln.startswith("BASELINE ")][-1][len("BASELINE "):])

    if not args.parent_so:
        doc["switch_off"] = {"this_commit": baseline(args.steps)}
    else:
        rounds = []
        for _ in range(args.rounds):
            rounds.append({"this_commit": child(None), "parent_commit": child(args.parent_so)})
            print("round " + json.dumps(rounds[-1]), flush=True)
        so = {"rounds": rounds}
        for f in ("step_scene", "retrieve_scene"):
            this = [r_["this_commit"][f + "_s"] for r_ in rounds]
            parent = [r_["parent_commit"][f + "_s"] for r_ in rounds]
            so[f] = {"this_commit_medians_s": this, "parent_commit_medians_s": parent,
                     "this_commit_spread_s": [min(this), max(this)], "parent_commit_spread_s": [min(parent), max(parent)],
                     "median_of_this_commit_inside_the_parents_spread": bool(min(parent) <= sorted(this)[len(this) // 2] <= max(parent)),
                     "median_of_this_commit_at_or_below_the_parents_maximum": bool(sorted(this)[len(this) // 2] <= max(parent))}
        doc["switch_off"] = so
    print(json.dumps(doc["switch_off"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
