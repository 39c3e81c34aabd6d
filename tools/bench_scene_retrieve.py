#!/usr/bin/env python3
"""The retrieval loop of a scene on the device (Model.retrieve_scene, jur_retrieve_scene_host) on the two workloads of
tools/bench_scene_step.py, against the route the library offered before.  Writes profiles/scene_retrieve.json; asserts
no threshold.

  A  64 profiles, nadir example, T and CO2 retrieved on all levels, 1e5 nadir rays
  B  64 profiles, limb example: 64 scans of the example's 66 rays, T and O3 retrieved on all levels

Settings on both routes: max_iter = 4, tol = 0, fac = (0.1, 1, 10), lam0 = 1, Marquardt damping.  No prior -- unless the
call without one ends with JUR_ENLOS (every level of T and a gas is ill-posed: an accepted step can leave the range in
which a ray can be traced); then both routes run with a diagonal prior around the first guess, sigma 1 K for T and 10 %
for the gas, and the result says so.

  device_s  one Model.retrieve_scene call: everything on the device, scalars per slice and damping home per iteration
  host_s    per iteration Model.step_scene (three dampings), the three steps written back through scene_elements,
            Model.set_atm and Model.formod_host on each trial atmosphere, the cost of every slice in numpy,
            retrieve_decide, the accepted steps written back; one Model.formod_host on the result at the end

Each time is the median of --steps calls after one warm-up call, a host clock around calls that end in a device
synchronise.  The bytes are counted from the shapes, per call.  The kernels' times come from the model's event timing
(jur_model_last_scene_ms) in calls of their own: the scene kernels of one retrieve_scene call less those of max_iter
step_scene calls are the kernels this loop adds (trial stacking and element moves, trial replication, trial cost, the
gathering of the remaining rays, the accepted moves, the state's way home), given as one sum and as a share of the call.

  python tools/bench_scene_retrieve.py [--steps 3] [--rays-a 100000] [--only A|B]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import ctypes as C
import numpy as np
from jurassic_hip import abi, lib
from bench_scene_jacobian import NPROF, median_s, workload
from bench_scene_step import scene_kernels_ms

MAX_ITER, TOL, FAC, LAM0, LAM_MIN, LAM_MAX = 4, 0.0, (0.1, 1.0, 10.0), 1.0, 1e-6, 1e6


def copy_atm(a):
    out = abi.atm_t()
    C.memmove(C.byref(out), C.byref(a), C.sizeof(abi.atm_t))
    return out


def rows_of(c, atm):
    rows = [np.ctypeslib.as_array(atm.p), np.ctypeslib.as_array(atm.t)]
    return rows + list(np.ctypeslib.as_array(atm.q)[:c.ng]) + list(np.ctypeslib.as_array(atm.k)[:c.nw])


def host_route(model, c, atm0, geom, y, weight, lay, iq, ip, prior):
    """the loop as a caller writes it today; -> (final atm, cost per iteration)"""
    ns, wptr, sid = len(lay["sfirst"]), lay["wptr"], lay["sid"]
    fac = np.array(FAC)
    atm = copy_atm(atm0)
    lam, state = np.full(ns, LAM0), np.zeros(ns, dtype=np.int32)
    own = np.repeat(np.arange(ns), np.diff(wptr))                      # slice of every element
    history = []
    for it in range(MAX_ITER):
        if not np.any(state == lib.RET_ACTIVE):
            break
        lamt = np.minimum(np.maximum(lam[None, :] * fac[:, None], LAM_MIN), LAM_MAX)
        model.set_atm(atm)
        rows = rows_of(c, atm)
        x = np.array([rows[q][p] for q, p in zip(iq, ip)])
        kw = dict(prior_ivar=prior[0], prior_dx=prior[1] - x) if prior else {}
        step = model.step_scene(atm, geom, y, weight, lamt, **kw)
        term_of = lambda xx: np.bincount(own, weights=prior[0] * (prior[1] - xx) ** 2, minlength=ns) if prior else np.zeros(ns)
        tcost = np.zeros((len(FAC), ns))
        live = (weight > 0) & np.isfinite(y) & (sid >= 0)[:, None]
        for l in range(len(FAC)):
            trial = copy_atm(atm)
            rows = rows_of(c, trial)
            for q in np.unique(iq):
                m = iq == q
                rows[q][ip[m]] += step["dx"][l][m]
            model.set_atm(trial)
            d = y - model.formod_host(geom)["rad"]
            term = np.where(live, weight * d * d, 0.0).sum(axis=1)
            tcost[l] = np.bincount(sid[sid >= 0], weights=term[sid >= 0], minlength=ns) + term_of(x + step["dx"][l])
        dec = lib.retrieve_decide(step["cost"] + term_of(x), tcost, lamt, step["status"], lam, state, TOL, LAM_MAX, fac.max())
        lam, state = dec["lam"], dec["state"]
        rows = rows_of(c, atm)
        for l in range(len(FAC)):
            took = (dec["accept"][own] == 1) & (dec["best"][own] == l)
            for q in np.unique(iq[took]):
                m = took & (iq == q)
                rows[q][ip[m]] += step["dx"][l][m]
        history.append(float(step["cost"].sum()))
    model.set_atm(atm)
    model.formod_host(geom)
    return atm, history


def run(name, steps, nrays_a):
    case = workload(name, nrays_a)
    c, atm, geom = case.ctl, case.atm, case.geom
    nd, nr = c.nd, len(case.geom)
    model = lib.Model(c, case.lib_tables())
    model.set_atm(atm)
    lay = lib.scene_slices(c, atm, geom[:, 0])
    els = [lib.scene_elements(c, atm, lay["sfirst"][s], lay["slen"][s]) for s in range(len(lay["sfirst"]))]
    iq, ip = np.concatenate([e["iq"] for e in els]), np.concatenate([e["ip"] for e in els])
    rng = np.random.default_rng(5)
    y = model.formod_host(geom)["rad"] * (1.0 + 1e-3 * rng.standard_normal((nr, nd)))
    weight = 10.0 ** rng.uniform(0.0, 3.0, y.shape)

    keep = {"refused": []}
    def device():
        model.set_atm(atm)
        pk = dict(prior_ivar=keep["prior"][0], prior_xa=keep["prior"][1]) if keep["prior"] else {}
        keep["dev"] = model.retrieve_scene(atm, geom, y, weight, MAX_ITER, FAC, lam0=LAM0, lam_min=LAM_MIN, lam_max=LAM_MAX,
                                           tol=TOL, history=True, **pk)
    rows0 = rows_of(c, atm)
    x0 = np.array([rows0[q][p] for q, p in zip(iq, ip)])
    sigma = np.where(iq == 1, 1.0, 0.1 * np.abs(x0) + 1e-12)
    for prior in (None, (1.0 / sigma ** 2, x0)):
        keep["prior"] = prior
        try:
            device()
            break
        except lib.JurassicError as e:
            keep["refused"].append({"prior": prior is not None, "error": str(e)})
    else:
        raise SystemExit("neither route went through: %s" % keep["refused"])
    device_s, device_all = median_s(device, steps)

    def host():
        keep["host"] = host_route(model, c, atm, geom, y, weight, lay, iq, ip, keep["prior"])
    host_s, host_all = median_s(host, steps)

    dev = keep["dev"]
    rows_d, rows_h = rows_of(c, dev["atm"]), rows_of(c, keep["host"][0])
    x_d = np.array([rows_d[q][p] for q, p in zip(iq, ip)])
    x_h = np.array([rows_h[q][p] for q, p in zip(iq, ip)])
    rel = float(np.abs(x_d - x_h).max() / np.abs(x_h).max())

    model.set_atm(atm)
    loop_ms, loop_launches, timed_s = scene_kernels_ms(model, device)
    model.set_atm(atm)
    step_ms, step_launches, _ = scene_kernels_ms(model, lambda: model.step_scene(atm, geom, y, weight, np.array(FAC)))
    model.close()

    ns, n, nlam = len(lay["sfirst"]), int(lay["wptr"][-1]), len(FAC)
    iters = int(dev["iters"].max())
    nrow = 6 + c.ng + c.nw
    ray_in = nr * (7 * 8 + 3 * nd * 8 + 3 * 4 + 8)                                   # geometry, mask, y, weight; first, len, copy0; rowptr
    results = nr * (2 * nd * 8 + 3 * 8 + 4)                                         # rad, tau, tp, np
    scalars = ns * (3 * 8 + 8) + nlam * ns * (3 * 8 + 4)                            # cost, prior, nlive; pred, tcost, tprior, status
    choices = ns * (4 + 4) + nlam * ns * 8                                          # state, choice; dampings
    up_dev = ray_in + nrow * atm.np * 8 + nr * 4 * 3 + iters * choices              # + base rows, the plan's ray lists
    down_dev = results + n * 8 + iters * scalars
    per_it_up = ray_in + (1 + nlam) * (nrow * atm.np * 8 + nr * 7 * 8)              # step_scene's uploads; set_atm and geometry per trial
    per_it_down = results + ns * 16 + nlam * (n * 8 + ns * 12) + nlam * results
    return {"rays": nr, "profiles": NPROF, "channels": nd, "slices": ns, "columns_per_slice": int(np.diff(lay["wptr"]).max()),
            "max_iter": MAX_ITER, "tol": TOL, "fac": list(FAC), "lam0": LAM0, "diagonal_prior": keep["prior"] is not None, "calls_that_ended_with_an_error": keep["refused"],
            "iterations_run": iters,
            "states": [int(v) for v in np.bincount(dev["state"], minlength=4)],
            "device_s": device_s, "device_s_all": device_all, "host_s": host_s, "host_s_all": host_all,
            "host_over_device": host_s / device_s,
            "sum_J_by_iteration_device": [float(v) for v in (dev["h_cost"] + dev["h_prior"]).sum(axis=1)] + [float((dev["cost"] + dev["prior"]).sum())],
            "sum_cost_at_iteration_start_host": keep["host"][1],
            "largest_relative_difference_of_the_retrieved_states": rel,
            "replicated_rays_jacobian_and_trial_by_iteration": dev["h_work"].tolist(),
            "bytes_to_device_device_route": up_dev, "bytes_to_host_device_route": down_dev,
            "bytes_to_device_host_route": iters * per_it_up + nrow * atm.np * 8 + nr * 7 * 8,
            "bytes_to_host_host_route": iters * per_it_down + results,
            "event_timed_call": {"call_s": timed_s, "scene_kernels_ms_retrieve_scene": loop_ms, "scene_launches_retrieve_scene": loop_launches,
                                 "scene_kernels_ms_one_step_scene": step_ms, "scene_launches_one_step_scene": step_launches,
                                 "new_kernels_ms": loop_ms - iters * step_ms,
                                 "new_kernels_share_of_the_call": (loop_ms - iters * step_ms) * 1e-3 / timed_s}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rays-a", type=int, default=100000)
    ap.add_argument("--only", choices=["A", "B"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_retrieve.json"))
    args = ap.parse_args()
    doc = {"what": "retrieval loop of a scene: Model.retrieve_scene (Jacobians, normal equations, solves, trial passes and the "
                   "accepted moves on the device) against a host loop over Model.step_scene, write-back through scene_elements, "
                   "Model.set_atm and Model.formod_host per damping (tools/bench_scene_retrieve.py)",
           "timing": "median of %d calls after one warm-up, host clock around calls that end in a device synchronise; pageable "
                     "host arrays on both routes" % args.steps,
           "device": lib.device_info(0)["pci_bus_id"]}
    for name in ("A", "B"):
        if args.only in (None, name):
            doc[name] = run(name, args.steps, args.rays_a)
            print(name, json.dumps(doc[name]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
