#!/usr/bin/env python3
"""The box on the state of the scene retrieval (Model.set_state_bounds) on workload B of tools/bench_scene_retrieve.py,
bench_scene_prior.py and bench_scene_hydro.py: 64 limb scans of the example's 66 rays, T and O3 retrieved on all levels,
the diagonal prior sigma = 1 K for T and 10 % for O3 around the first guess.  Writes profiles/scene_bounds.json; asserts
no threshold -- nobody has measured these before.

  on / off      Model.retrieve_scene with upstream's box (state_bounds_upstream) on and off, the overhead in percent, the
                scene kernels of an event-timed call each way, and how many elements the box holds at the end
                (state_on_bounds of the returned x)
  box_off       Model.step_scene and Model.retrieve_scene with no box set (never touched: a parent library has no such
                entry), and, with --parent-so, the same from a library built from the parent commit: the two alternate in
                processes of their own, --rounds each.  The claim to support is "inside the parent's spread".
  no_prior      the same workload WITHOUT a prior, which ends in JUR_ENLOS with no box: one call with upstream's box, in a
                process of its own under its own time limit.  Whether it completes is a finding that is written down, not
                asserted; if it does not, the iteration in which it ended is the number of iterations the slices counted
                before the error, and where that is iteration 0 its passes are named by the merged entries on the first
                guess (step_scene: the Jacobian pass; trial_scene on each of its steps: the trial pass).

Each time is the median of --steps calls after one warm-up call, a host clock around calls that end in a device
synchronise.

  python tools/bench_scene_bounds.py [--steps 3] [--rounds 5] [--parent-so path/to/libjurassic_hip.so]"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
from jurassic_hip import lib
from bench_scene_jacobian import NPROF, median_s, workload
from bench_scene_step import scene_kernels_ms
from bench_scene_retrieve import FAC, LAM0, LAM_MAX, LAM_MIN, MAX_ITER, TOL, rows_of

SIGMA_T, SIGMA_REL = 1.0, 0.1
NO_PRIOR_TIMEOUT_S = 240


def setup():
    case = workload("B", 0)
    c, atm, geom = case.ctl, case.atm, case.geom
    model = lib.Model(c, case.lib_tables())
    model.set_atm(atm)
    lay = lib.scene_slices(c, atm, geom[:, 0])
    rng = np.random.default_rng(5)
    y = model.formod_host(geom)["rad"] * (1.0 + 1e-3 * rng.standard_normal((len(geom), c.nd)))
    weight = 10.0 ** rng.uniform(0.0, 3.0, y.shape)
    els = [lib.scene_elements(c, atm, lay["sfirst"][s], lay["slen"][s]) for s in range(len(lay["sfirst"]))]
    iq, ip = np.concatenate([e["iq"] for e in els]), np.concatenate([e["ip"] for e in els])
    rows0 = rows_of(c, atm)
    x0 = np.array([rows0[q][p] for q, p in zip(iq, ip)])
    r = 1.0 / np.where(iq == 1, SIGMA_T, SIGMA_REL * np.abs(x0) + 1e-12) ** 2
    return case, model, lay, y, weight, iq, x0, r


def calls(case, model, y, weight, x0, r, keep=None):
    atm, geom = case.atm, case.geom

    def step():
        model.set_atm(atm)
        model.step_scene(atm, geom, y, weight, np.array(FAC), prior_ivar=r, prior_dx=np.zeros(len(x0)))

    def retrieve():
        model.set_atm(atm)
        out = model.retrieve_scene(atm, geom, y, weight, MAX_ITER, FAC, lam0=LAM0, lam_min=LAM_MIN, lam_max=LAM_MAX, tol=TOL,
                                   prior_ivar=r, prior_xa=x0)
        if keep is not None:
            keep["ret"] = out
    return step, retrieve


def baseline(steps):
    """step_scene and retrieve_scene with no box set"""
    case, model, lay, y, weight, iq, x0, r = setup()
    step, retrieve = calls(case, model, y, weight, x0, r)
    out = {}
    for name, fn in (("step_scene", step), ("retrieve_scene", retrieve)):
        out[name + "_s"], out[name + "_s_all"] = median_s(fn, steps)
    model.close()
    return out


def held(box, iq, x):
    side = lib.state_on_bounds(box[0], box[1], iq, x)["side"]
    return {"elements": len(x), "on_a_bound": int(np.count_nonzero(side)), "on_the_lower": int((side < 0).sum()), "on_the_upper": int((side > 0).sum()),
            "by_quantity": {str(int(q)): int(np.count_nonzero(side[iq == q])) for q in np.unique(iq)}}


def run(steps):
    case, model, lay, y, weight, iq, x0, r = setup()
    keep = {}
    _, retrieve = calls(case, model, y, weight, x0, r, keep)
    box = lib.state_bounds_upstream(case.ctl)
    res = {"rays": len(case.geom), "profiles": NPROF, "slices": len(lay["sfirst"]), "columns_per_slice": int(np.diff(lay["wptr"]).max()),
           "max_iter": MAX_ITER, "fac": list(FAC), "box": {"lo": [float(v) for v in box[0]], "hi": [float(v) for v in box[1]]}}
    for tag, b in (("off", None), ("on", box)):
        model.set_state_bounds(*(b or (None,)))
        res["retrieve_scene_%s_s" % tag], res["retrieve_scene_%s_s_all" % tag] = median_s(retrieve, steps)
        ms, launches, dt = scene_kernels_ms(model, retrieve)
        res["event_timed_call_" + tag] = {"scene_kernels_ms": ms, "scene_launches": launches, "call_s": dt}
        res["states_" + tag] = [int(v) for v in np.bincount(keep["ret"]["state"], minlength=4)]
        res["cost_plus_prior_" + tag] = float((keep["ret"]["cost"] + keep["ret"]["prior"]).sum())
        res["held_at_the_end_" + tag] = held(box, iq, keep["ret"]["x"])
        keep["x_" + tag] = keep["ret"]["x"]
    res["retrieve_scene_overhead_percent"] = 100.0 * (res["retrieve_scene_on_s"] / res["retrieve_scene_off_s"] - 1.0)
    res["launches_added"] = res["event_timed_call_on"]["scene_launches"] - res["event_timed_call_off"]["scene_launches"]
    res["elements_whose_result_differs"] = int(np.count_nonzero(keep["x_on"] != keep["x_off"]))
    model.close()
    return res


def no_prior():
    """one call without a prior under upstream's box; prints one line"""
    case, model, lay, y, weight, iq, x0, r = setup()
    box = lib.state_bounds_upstream(case.ctl)
    model.set_state_bounds(*box)
    model.set_atm(case.atm)
    out = {"box": "upstream's", "prior": None, "max_iter": MAX_ITER}
    try:
        ret = model.retrieve_scene(case.atm, case.geom, y, weight, MAX_ITER, FAC, lam0=LAM0, lam_min=LAM_MIN, lam_max=LAM_MAX, tol=TOL, history=True)
        out.update(completes=True, states=[int(v) for v in np.bincount(ret["state"], minlength=4)], cost=float(ret["cost"].sum()),
                   first_cost=float(ret["h_cost"][0].sum()), held_at_the_end=held(box, iq, ret["x"]),
                   iterations_run=int(np.count_nonzero(ret["h_work"][:, 0])))
    except lib.JurassicError as e:
        # one run.  The iterations that completed have counted themselves in the per-slice arrays (the wrapper hands them
        # on with the error): the call ended in the iteration after them.  Where that is iteration 0, its two passes are
        # the merged entries on the first guess: step_scene is the Jacobian pass, trial_scene on its steps the trial pass.
        out.update(completes=False, error=str(e))
        part = getattr(e, "partial", None)
        if part is not None:
            out["ended_in_iteration"] = int(part["iters"].max())
            if out["ended_in_iteration"] == 0:
                lam = LAM0 * np.array(FAC)
                try:
                    model.set_atm(case.atm)
                    step = model.step_scene(case.atm, case.geom, y, weight, lam)
                    out["pass"] = "trial"
                    out["step_status"] = [int(v) for v in np.bincount(step["status"].ravel(), minlength=2)]
                    out["trials"] = {}
                    for l in range(len(FAC)):
                        xb = lib.state_bound(x0 + step["dx"][l], box[0][iq], box[1][iq])
                        info = {"lam": float(lam[l]), "elements_clamped": int(np.count_nonzero(xb != x0 + step["dx"][l])),
                                "largest_T_step_K": float(np.abs(step["dx"][l][iq == 1]).max())}
                        try:
                            model.trial_scene(case.atm, case.geom, y, weight, step["dx"][l])
                            info["traces"] = True
                        except lib.JurassicError as e2:
                            info.update(traces=False, error=str(e2))
                        out["trials"][str(l)] = info
                except lib.JurassicError as e1:
                    out.update({"pass": "Jacobian", "jacobian_error": str(e1)})
    model.close()
    print("NO_PRIOR " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5, help="alternating runs of this commit's and the parent's library")
    ap.add_argument("--parent-so", help="a libjurassic_hip.so built from the parent commit: its times are measured in processes of their own")
    ap.add_argument("--baseline-only", action="store_true", help="print the times with no box set as one JSON line and stop")
    ap.add_argument("--no-prior-only", action="store_true", help="run the call without a prior under upstream's box, print one JSON line and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_bounds.json"))
    args = ap.parse_args()
    if args.baseline_only:
        print("BASELINE " + json.dumps(baseline(args.steps)), flush=True)
        return
    if args.no_prior_only:
        no_prior()
        return
    doc = {"what": "the box on the state of the scene retrieval on workload B (64 limb scans, T and O3 on all levels, diagonal prior): "
                   "Model.retrieve_scene with upstream's box on and off, the times with no box set against the parent commit's, and the "
                   "same workload without a prior under upstream's box (tools/bench_scene_bounds.py)",
           "timing": "median of %d calls after one warm-up, host clock around calls that end in a device synchronise; pageable host "
                     "arrays; no target was set for any of these numbers and nobody had measured them before" % args.steps,
           "device": lib.device_info(0)["pci_bus_id"],
           "kernel_resources": "from the compiler's report for gfx950, parent commit -> this commit: jur_scene_elements_kernel 20 -> 22 VGPRs, "
                               "49 -> 49 SGPRs; jur_scene_prior_kernel 24 -> 28 VGPRs, 38 -> 38 SGPRs; jur_scene_prior_diff_kernel 13 -> 13 "
                               "VGPRs, 33 -> 34 SGPRs; no LDS, no scratch, no spills in any of them, before or after"}
    doc["B"] = run(args.steps)
    print("B " + json.dumps(doc["B"]), flush=True)

    def child(so, flag):
        """one library in a process of its own (both libraries alike: same start, same work)"""
        env = dict(os.environ)
        if so:
            env["JURASSIC_HIP_SO"] = os.path.abspath(so)
        return subprocess.run([sys.executable, os.path.abspath(__file__), flag, "--steps", str(args.steps)], env=env, capture_output=True,
                              text=True, timeout=NO_PRIOR_TIMEOUT_S if flag == "--no-prior-only" else None)

    def tagged(proc, tag):
        return json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith(tag)][-1][len(tag):])

    if not args.parent_so:
        doc["box_off"] = {"this_commit": baseline(args.steps)}
    else:
        rounds = []
        for _ in range(args.rounds):
            this, parent = child(None, "--baseline-only"), child(args.parent_so, "--baseline-only")
            this.check_returncode(); parent.check_returncode()
            rounds.append({"this_commit": tagged(this, "BASELINE "), "parent_commit": tagged(parent, "BASELINE ")})
            print("round " + json.dumps(rounds[-1]), flush=True)
        so = {"rounds": rounds}
        for f in ("step_scene", "retrieve_scene"):
            this = [r_["this_commit"][f + "_s"] for r_ in rounds]
            parent = [r_["parent_commit"][f + "_s"] for r_ in rounds]
            so[f] = {"this_commit_medians_s": this, "parent_commit_medians_s": parent,
                     "this_commit_spread_s": [min(this), max(this)], "parent_commit_spread_s": [min(parent), max(parent)],
                     "median_of_this_commit_inside_the_parents_spread": bool(min(parent) <= sorted(this)[len(this) // 2] <= max(parent)),
                     "median_of_this_commit_at_or_below_the_parents_maximum": bool(sorted(this)[len(this) // 2] <= max(parent))}
        doc["box_off"] = so
    print("box_off " + json.dumps(doc["box_off"]), flush=True)
    try:                                              # one run, under its own time limit; an error code is a finding
        proc = child(None, "--no-prior-only")
        doc["no_prior"] = tagged(proc, "NO_PRIOR ") if proc.returncode == 0 else {"completes": False, "exit_status": proc.returncode, "stderr_tail": proc.stderr[-500:]}
    except subprocess.TimeoutExpired:
        doc["no_prior"] = {"completes": False, "timed_out_after_s": NO_PRIOR_TIMEOUT_S}
    print("no_prior " + json.dumps(doc["no_prior"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
