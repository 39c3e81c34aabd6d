#!/usr/bin/env python3
"""Posterior diagnostics of every slice of a scene (Model.diagnose_scene, jur_diagnose_scene_host) on the two workloads of
tools/bench_scene_step.py and on one 1120-wide system (Model.diagnose_slices), against the route the library offered
before: Model.normal_scene, every matrix copied to the host, and per slice in numpy np.linalg.cholesky of A + diag(r), the
inverse from two triangular solves, the product S A and the vectors.  Writes profiles/scene_diagnose.json; asserts no
threshold.

  A  64 profiles, nadir example, T and CO2 retrieved on all levels, 1e5 nadir rays
  B  64 profiles, limb example: 64 scans of the example's 66 rays, T and O3 retrieved on all levels
  one_wide_system  a seeded (G^T G + I) / 100 of 1120 columns with a seeded prior

Both routes use the same diagonal prior, 1e-2 of the mean diagonal of A_s on every element (without one the A_s of a
scene whose slices have more elements than measurements are singular).

  device_s   Model.diagnose_scene, nothing wanted home but the vectors, dofs and status; one call
  host_s     Model.normal_scene, then the linear algebra per slice in numpy
  host_linalg_s  the numpy part of host_s alone

Each time is the median of --steps calls after one warm-up call, a host clock around calls that end in a device
synchronise.  The new kernels' time comes from the model's event timing (jur_model_last_scene_ms) in calls of their own:
the scene kernels' time of a diagnose_scene call less that of a normal_scene call is the factorisation (the solve kernel
at lam = 0) plus the inverse, product and vector kernels.  For the wide system the factorisation's share is the event
time of one Model.solve_slices call on the same matrix.

  python tools/bench_scene_diagnose.py [--steps 3] [--rays-a 100000] [--only A|B|W]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
from jurassic_hip import lib
from bench_scene_jacobian import NPROF, median_s, workload
from bench_scene_step import scene_kernels_ms

VECTORS = ("sigma", "sigma_noise", "sigma_smooth", "avk_diag")


def host_diagnostics(wptr, aptr, A, r):
    """the vectors, dofs of Model.diagnose_slices from the matrices, per slice, in numpy"""
    n, ns = int(wptr[-1]), len(wptr) - 1
    out = {f: np.zeros(n) for f in VECTORS}
    out["dofs"] = np.zeros(ns)
    for s in range(ns):
        w = int(wptr[s + 1] - wptr[s])
        As, rs = A[aptr[s]:aptr[s + 1]].reshape(w, w), r[wptr[s]:wptr[s + 1]]
        live = (np.diag(As) + rs) > 0
        Al, rl = As[np.ix_(live, live)], rs[live]
        L = np.linalg.cholesky(Al + np.diag(rl))
        Y = np.linalg.solve(L, np.eye(len(rl)))
        S = np.linalg.solve(L.T, Y)
        K = S @ Al
        sl = np.arange(wptr[s], wptr[s + 1])[live]
        out["sigma"][sl] = np.sqrt(np.diag(S))
        out["sigma_noise"][sl] = np.sqrt(np.maximum((K * S.T).sum(axis=1), 0.0))
        out["sigma_smooth"][sl] = np.sqrt((S * S) @ rl)
        out["avk_diag"][sl] = np.diag(K)
        out["dofs"][s] = np.trace(K)
    return out


def largest_difference(dev, host):
    return {f: float(np.abs(dev[f] - host[f]).max() / np.abs(host[f]).max()) for f in VECTORS + ("dofs",)}


def run(name, steps, nrays_a):
    case = workload(name, nrays_a)
    c, atm, geom = case.ctl, case.atm, case.geom
    nd = c.nd
    model = lib.Model(c, case.lib_tables())
    model.set_atm(atm)
    rng = np.random.default_rng(5)
    y = model.formod_host(geom)["rad"] * (1.0 + 1e-3 * rng.standard_normal((len(geom), nd)))
    weight = 10.0 ** rng.uniform(0.0, 3.0, y.shape)
    first = model.normal_scene(atm, geom, y, weight)
    wptr, aptr = first["wptr"], first["aptr"]
    ns, n, na = len(wptr) - 1, int(wptr[-1]), int(aptr[-1])
    r = np.concatenate([np.full(int(wptr[s + 1] - wptr[s]), 1e-2 * np.diag(first["A"][aptr[s]:aptr[s + 1]].reshape(
        int(wptr[s + 1] - wptr[s]), -1)).mean()) for s in range(ns)])
    del first

    keep = {"linalg_s": []}
    def device():
        keep["dev"] = model.diagnose_scene(atm, geom, y, weight, prior_ivar=r)
    device_s, device_all = median_s(device, steps)

    def host():
        out = model.normal_scene(atm, geom, y, weight)
        t0 = time.perf_counter()
        keep["host"] = host_diagnostics(wptr, aptr, out["A"], r)
        keep["linalg_s"].append(time.perf_counter() - t0)
    host_s, host_all = median_s(host, steps)

    dev = keep["dev"]
    assert np.all(dev["status"] == 0)
    diag_ms, diag_launches, timed_s = scene_kernels_ms(model, lambda: model.diagnose_scene(atm, geom, y, weight, prior_ivar=r))
    normal_ms, normal_launches, _ = scene_kernels_ms(model, lambda: model.normal_scene(atm, geom, y, weight))
    model.close()

    forward_bytes = len(geom) * (2 * nd * 8 + 3 * 8 + 4) + 2 * ns * 8               # rad, tau, tp, np; cost, nlive
    diag_bytes = 4 * n * 8 + ns * 8 + ns * 4                                        # the vectors, dofs, status
    return {"rays": len(geom), "profiles": NPROF, "channels": nd, "slices": ns, "columns_per_slice": int(np.diff(wptr).max()),
            "dofs_min_max": [float(dev["dofs"].min()), float(dev["dofs"].max())],
            "device_s": device_s, "device_s_all": device_all, "host_s": host_s, "host_s_all": host_all,
            "host_linalg_s": float(np.median(keep["linalg_s"][1:])), "host_over_device": host_s / device_s,
            "bytes_to_host_device_route": forward_bytes + diag_bytes, "bytes_to_host_host_route": forward_bytes + (na + n) * 8,
            "diagnostics_bytes": diag_bytes, "matrix_bytes": na * 8,
            "largest_relative_difference_of_the_two_routes": largest_difference(dev, keep["host"]),
            "event_timed_call": {"call_s": timed_s, "scene_kernels_ms_diagnose_scene": diag_ms, "scene_kernels_ms_normal_scene": normal_ms,
                                 "timed_intervals_added": diag_launches - normal_launches, "diagnostics_kernels_ms": diag_ms - normal_ms,
                                 "diagnostics_kernels_share_of_the_call": (diag_ms - normal_ms) * 1e-3 / timed_s}}


def one_wide_system(steps, w=1120):
    """one system of w columns through Model.diagnose_slices against numpy on the host"""
    import common
    case = common.limb_case()
    model = lib.Model(case.ctl, case.lib_tables())
    rng = np.random.default_rng(9)
    G = rng.standard_normal((w + 3, w))
    A = (G.T @ G + np.eye(w)) / 100.0
    A = np.tril(A) + np.tril(A, -1).T
    r = 10.0 ** rng.uniform(-2.0, 1.0, w)
    wptr, aptr = np.array([0, w]), np.array([0, w * w])
    keep = {}
    def device():
        keep["dev"] = model.diagnose_slices(wptr, A, prior_ivar=r)
    device_s, device_all = median_s(device, steps)
    def device_all_home():
        keep["full"] = model.diagnose_slices(wptr, A, prior_ivar=r, want_S=True, want_avk=True)
    full_s, _ = median_s(device_all_home, steps)
    def host():
        keep["host"] = host_diagnostics(wptr, aptr, A.ravel(), r)
    host_s, host_all = median_s(host, steps)
    ms, launches, dt = scene_kernels_ms(model, device)
    solve_ms, _, _ = scene_kernels_ms(model, lambda: model.solve_slices(wptr, A, np.zeros(w), 0.0, prior_ivar=r, prior_dx=np.zeros(w)))
    model.close()
    return {"columns": w, "status": int(keep["dev"]["status"][0]), "dofs": float(keep["dev"]["dofs"][0]),
            "device_s": device_s, "device_s_all": device_all, "device_s_with_S_and_avk_home": full_s, "host_s": host_s, "host_s_all": host_all,
            "host_over_device": host_s / device_s,
            "bytes_to_host_device_route": 4 * w * 8 + 12, "bytes_to_host_with_S_and_avk": 4 * w * 8 + 12 + 2 * w * w * 8,
            "bytes_to_device": w * w * 8 + w * 8,
            "kernels_ms": ms, "factor_kernel_ms": solve_ms, "inverse_product_vectors_ms": ms - solve_ms, "call_s": dt,
            "largest_relative_difference_of_the_two_routes": largest_difference(keep["dev"], keep["host"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rays-a", type=int, default=100000)
    ap.add_argument("--only", choices=["A", "B", "W"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_diagnose.json"))
    args = ap.parse_args()
    doc = {"what": "posterior diagnostics of every slice of a scene: Model.diagnose_scene (normal equations, factor, inverse, "
                   "averaging kernel and the vectors on the device, nothing but the vectors copied out) against Model.normal_scene "
                   "plus np.linalg.cholesky, two solves and the products per slice on the host (tools/bench_scene_diagnose.py)",
           "timing": "median of %d calls after one warm-up, host clock around calls that end in a device synchronise; pageable "
                     "host arrays on both routes" % args.steps,
           "device": lib.device_info(0)["pci_bus_id"]}
    for name in ("A", "B"):
        if args.only in (None, name):
            doc[name] = run(name, args.steps, args.rays_a)
            print(name, json.dumps(doc[name]), flush=True)
    if args.only in (None, "W"):
        doc["one_wide_system"] = one_wide_system(args.steps)
        print("wide", json.dumps(doc["one_wide_system"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
