#!/usr/bin/env python3
"""The Levenberg-Marquardt step of every slice of a scene (Model.step_scene, jur_step_scene_host) on the two workloads of
tools/bench_scene_normal.py, against the route the library offered before: Model.normal_scene, every matrix copied to
the host, and a Cholesky factorisation and two triangular solves per slice and damping there in numpy.  Three dampings
on both routes.  Writes profiles/scene_step.json; asserts no threshold.

  A  64 profiles, nadir example, T and CO2 retrieved on all levels, 1e5 nadir rays
  B  64 profiles, limb example: 64 scans of the example's 66 rays, T and O3 retrieved on all levels

  device_s   Model.step_scene, three dampings, nothing wanted home (no A, b, k, L), one call
  host_s     Model.normal_scene, then per slice and damping np.linalg.cholesky of the damped live part and two solves
  host_solve_s  the numpy part of host_s alone

Each time is the median of --steps calls after one warm-up call, a host clock around calls that end in a device
synchronise.  The new kernel's time comes from the model's event timing (jur_model_last_scene_ms) in calls of their own:
the scene kernels' time of a step_scene call less that of a normal_scene call (three launches, one per damping).  The
kernel's time for one 1120-wide system is the event time of one Model.solve_slices call on a seeded G^T G + I.

  python tools/bench_scene_step.py [--steps 3] [--rays-a 100000] [--only A|B]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
from jurassic_hip import lib
from bench_scene_jacobian import NPROF, median_s, workload

LAMS = (1e-2, 1.0, 1e2)


def host_steps(out):
    """dx (nlam, n) of Model.step_scene from the sums of Model.normal_scene, per slice and damping, in numpy"""
    wptr, aptr = out["wptr"], out["aptr"]
    dx = np.zeros((len(LAMS), int(wptr[-1])))
    for s in range(len(wptr) - 1):
        w = int(wptr[s + 1] - wptr[s])
        A, b = out["A"][aptr[s]:aptr[s + 1]].reshape(w, w), out["b"][wptr[s]:wptr[s + 1]]
        live = np.diag(A) > 0
        Al, bl = A[np.ix_(live, live)], b[live]
        for l, lam in enumerate(LAMS):
            L = np.linalg.cholesky(Al + lam * np.diag(np.diag(Al)))
            dx[l, wptr[s]:wptr[s + 1]][live] = np.linalg.solve(L.T, np.linalg.solve(L, bl))
    return dx


def scene_kernels_ms(model, call):
    model.enable_timing(True)
    t0 = time.perf_counter()
    call()
    dt = time.perf_counter() - t0
    model.kernel_ms()
    ms = model.scene_ms()
    model.enable_timing(False)
    return ms["scene_ms"], ms["scene_launches"], dt


def run(name, steps, nrays_a):
    case = workload(name, nrays_a)
    c, atm, geom = case.ctl, case.atm, case.geom
    nd = c.nd
    model = lib.Model(c, case.lib_tables())
    model.set_atm(atm)
    lay = lib.scene_slices(c, atm, geom[:, 0])
    rng = np.random.default_rng(5)
    y = model.formod_host(geom)["rad"] * (1.0 + 1e-3 * rng.standard_normal((len(geom), nd)))
    weight = 10.0 ** rng.uniform(0.0, 3.0, y.shape)

    keep = {"solve_s": []}
    def device():
        keep["dev"] = model.step_scene(atm, geom, y, weight, LAMS)
    device_s, device_all = median_s(device, steps)

    def host():
        out = model.normal_scene(atm, geom, y, weight)
        t0 = time.perf_counter()
        keep["host"] = host_steps(out)
        keep["solve_s"].append(time.perf_counter() - t0)
    host_s, host_all = median_s(host, steps)

    dev = keep["dev"]
    assert np.all(dev["status"] == 0)
    rel = float(np.abs(dev["dx"] - keep["host"]).max() / np.abs(keep["host"]).max())

    step_ms, step_launches, timed_s = scene_kernels_ms(model, lambda: model.step_scene(atm, geom, y, weight, LAMS))
    normal_ms, normal_launches, _ = scene_kernels_ms(model, lambda: model.normal_scene(atm, geom, y, weight))
    model.close()

    ns, n, na = len(lay["sfirst"]), int(lay["wptr"][-1]), int(lay["aptr"][-1])
    forward_bytes = len(geom) * (2 * nd * 8 + 3 * 8 + 4) + 2 * ns * 8               # rad, tau, tp, np; cost, nlive
    step_bytes = len(LAMS) * (n * 8 + ns * 8 + ns * 4)                              # dx, pred, status
    return {"rays": len(geom), "profiles": NPROF, "channels": nd, "slices": ns, "columns_per_slice": int(np.diff(lay["wptr"]).max()),
            "dampings": list(LAMS),
            "device_s": device_s, "device_s_all": device_all, "host_s": host_s, "host_s_all": host_all,
            "host_solve_s": float(np.median(keep["solve_s"][1:])), "host_over_device": host_s / device_s,
            "bytes_to_host_device_route": forward_bytes + step_bytes, "bytes_to_host_host_route": forward_bytes + (na + n) * 8,
            "step_bytes": step_bytes, "matrix_bytes": na * 8,
            "largest_relative_difference_of_the_two_routes": rel,
            "event_timed_call": {"call_s": timed_s, "scene_kernels_ms_step_scene": step_ms, "scene_kernels_ms_normal_scene": normal_ms,
                                 "solve_launches": step_launches - normal_launches, "solve_kernel_ms": step_ms - normal_ms,
                                 "solve_kernel_share_of_the_call": (step_ms - normal_ms) * 1e-3 / timed_s}}


def one_wide_system(w=1120):
    """the kernel's time for one system of w columns: a seeded G^T G + I, one damping, through Model.solve_slices"""
    import common
    case = common.limb_case()
    model = lib.Model(case.ctl, case.lib_tables())
    rng = np.random.default_rng(9)
    G = rng.standard_normal((w + 3, w))
    A, b = G.T @ G + np.eye(w), rng.standard_normal(w)
    call = lambda: model.solve_slices([0, w], A, b, 1.0)
    call()                                                                          # warm-up
    ms, launches, dt = scene_kernels_ms(model, call)
    res = model.solve_slices([0, w], A, b, 1.0)
    model.close()
    M = A + np.diag(np.diag(A))
    resid = float(np.abs(M @ res["dx"][0] - b).max() / np.abs(b).max())
    return {"columns": w, "status": int(res["status"][0, 0]), "solve_kernel_ms": ms, "launches": launches, "call_s": dt,
            "largest_residual_relative_to_b": resid}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rays-a", type=int, default=100000)
    ap.add_argument("--only", choices=["A", "B"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_step.json"))
    args = ap.parse_args()
    doc = {"what": "Levenberg-Marquardt step of every slice of a scene: Model.step_scene (normal equations and a batched Cholesky "
                   "solve on the device, three dampings, nothing but the steps copied out) against Model.normal_scene plus "
                   "np.linalg.cholesky and two solves per slice and damping on the host (tools/bench_scene_step.py)",
           "timing": "median of %d calls after one warm-up, host clock around calls that end in a device synchronise; pageable "
                     "host arrays on both routes" % args.steps,
           "device": lib.device_info(0)["pci_bus_id"]}
    for name in ("A", "B"):
        if args.only in (None, name):
            doc[name] = run(name, args.steps, args.rays_a)
            print(name, json.dumps(doc[name]), flush=True)
    doc["one_wide_system"] = one_wide_system()
    print("wide", json.dumps(doc["one_wide_system"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
