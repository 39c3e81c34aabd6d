#!/usr/bin/env python3
"""The normal equations of a scene per slice (Model.normal_scene, jur_normal_scene_host) on the two workloads of
tools/bench_scene_jacobian.py, against the only route the library offered before: Model.kernel_scene, every block
copied to the host, and the same sums there in numpy.  Writes profiles/scene_normal.json; asserts no threshold.

  A  64 profiles, nadir example, T and CO2 retrieved on all levels, 1e5 nadir rays
  B  64 profiles, limb example: 64 scans of the example's 66 rays, T and O3 retrieved on all levels

  device_s   Model.normal_scene without k, one call
  host_s     Model.kernel_scene, then per slice K^T (W K), K^T W (y - F), (y - F)^T W (y - F) with numpy (one matrix
             product per slice: the host's BLAS, not a term-by-term loop)
  host_sums_s  the numpy part of host_s alone

Each time is the median of --steps calls after one warm-up call, a host clock around calls that end in a device
synchronise.  The new kernel's share comes from the model's event timing (jur_model_last_scene_ms) in calls of their
own: the scene kernels' time of a normal_scene call less that of a kernel_scene call.

  python tools/bench_scene_normal.py [--steps 3] [--rays-a 100000] [--only A|B]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
from jurassic_hip import lib
from bench_scene_jacobian import NPROF, median_s, workload


def host_sums(out, lay, y, weight):
    """the sums of Model.normal_scene from the blocks of Model.kernel_scene, per slice, in numpy"""
    nd = y.shape[1]
    rp, k = out["rowptr"], out["k"]
    res = []
    for s in range(len(lay["sfirst"])):
        rays = np.flatnonzero(lay["sid"] == s)
        w = int(lay["wptr"][s + 1] - lay["wptr"][s])
        K = np.concatenate([k[rp[r] * nd:rp[r + 1] * nd] for r in rays]).reshape(len(rays) * nd, w)
        wt = weight[rays].reshape(-1)
        d = (y[rays] - out["rad"][rays]).reshape(-1)
        WK = K * wt[:, None]
        res.append((K.T @ WK, WK.T @ d, float(np.dot(wt * d, d)), len(d)))
    return res


def run(name, steps, nrays_a):
    case = workload(name, nrays_a)
    c, atm, geom = case.ctl, case.atm, case.geom
    nd = c.nd
    model = lib.Model(c, case.lib_tables())
    model.set_atm(atm)
    lay = lib.scene_layout(c, atm, geom[:, 0])
    lay.update(lib.scene_slices(c, atm, geom[:, 0]))
    rng = np.random.default_rng(5)
    y = model.formod_host(geom)["rad"] * (1.0 + 1e-3 * rng.standard_normal((len(geom), nd)))
    weight = 10.0 ** rng.uniform(0.0, 3.0, y.shape)

    keep = {}
    def device():
        keep["dev"] = model.normal_scene(atm, geom, y, weight)
    device_s, device_all = median_s(device, steps)

    def host():
        out = model.kernel_scene(atm, geom)
        t0 = time.perf_counter()
        keep["host"] = host_sums(out, lay, y, weight)
        keep["sums_s"].append(time.perf_counter() - t0)
    keep["sums_s"] = []
    host_s, host_all = median_s(host, steps)

    # the same numbers, to the rounding of sums in another order?  (largest difference relative to the largest entry)
    dev, rel = keep["dev"], 0.0
    for s, (A, b, cost, n) in enumerate(keep["host"]):
        w = len(b)
        Ad = dev["A"][dev["aptr"][s]:dev["aptr"][s + 1]].reshape(w, w)
        rel = max(rel, float(np.abs(Ad - A).max() / np.abs(A).max()), abs(dev["cost"][s] - cost) / cost)
        assert dev["nlive"][s] == n

    def scene_kernels_ms(call):
        model.enable_timing(True)
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        model.kernel_ms()
        ms = model.scene_ms()["scene_ms"]
        model.enable_timing(False)
        return ms, dt
    with_ms, timed_s = scene_kernels_ms(lambda: model.normal_scene(atm, geom, y, weight))
    without_ms, _ = scene_kernels_ms(lambda: model.kernel_scene(atm, geom))
    model.close()

    forward_bytes = len(geom) * (2 * nd * 8 + 3 * 8 + 4)
    sums_bytes = int(lay["aptr"][-1] + lay["wptr"][-1] + 2 * len(lay["sfirst"])) * 8
    block_bytes = int(lay["rowptr"][-1]) * nd * 8
    return {"rays": len(geom), "profiles": NPROF, "channels": nd, "slices": len(lay["sfirst"]),
            "columns_per_slice": int(np.diff(lay["wptr"]).max()), "block_elements": int(lay["rowptr"][-1]) * nd,
            "device_s": device_s, "device_s_all": device_all, "host_s": host_s, "host_s_all": host_all,
            "host_sums_s": float(np.median(keep["sums_s"][1:])), "host_over_device": host_s / device_s,
            "bytes_to_host_device_route": forward_bytes + sums_bytes, "bytes_to_host_host_route": forward_bytes + block_bytes,
            "largest_relative_difference_of_the_two_routes": rel,
            "event_timed_call": {"call_s": timed_s, "scene_kernels_ms_normal_scene": with_ms, "scene_kernels_ms_kernel_scene": without_ms,
                                 "normal_kernel_ms": with_ms - without_ms,
                                 "normal_kernel_share_of_the_call": (with_ms - without_ms) * 1e-3 / timed_s}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rays-a", type=int, default=100000)
    ap.add_argument("--only", choices=["A", "B"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_normal.json"))
    args = ap.parse_args()
    doc = {"what": "normal equations of a scene per slice: Model.normal_scene (sums on the device, no block copied out) against "
                   "Model.kernel_scene plus the same sums in numpy on the host (tools/bench_scene_normal.py)",
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
