#!/usr/bin/env python3
"""The field of view inside the scene entries (Model.set_fov) on the limb workload of tools/bench_scene_jacobian.py --
64 profiles, 64 scans of the limb example's 66 rays, T and O3 retrieved on all levels -- with a 21-point shape, against
the only route the library offered before.  Writes profiles/scene_fov.json; asserts no threshold.

  device_s   Model.normal_scene with the shape set, no block copied out, one call
  host_s     Model.normal_scene's predecessor on the host: Model.kernel_scene without a shape (every block copied home),
             lib.fov_apply on F and on every block column (a scan's columns as the channels of one call, half of them
             in the place of the transmittances so that nothing is convolved for nothing), then per slice K^T (W K),
             K^T W (y - G), (y - G)^T W (y - G) with numpy
  plain_s    Model.normal_scene without a shape (what the convolution adds to the call: device_s - plain_s)

The host route convolves the quotients where the device differences the convolved radiances; the convolution is linear,
so the two agree to rounding (largest_relative_difference_of_the_two_routes).  Each time is the median of --steps calls
after one warm-up call, a host clock around calls that end in a device synchronise.  The new kernel's time comes from
the model's event timing (jur_model_last_scene_ms) in calls of their own: the scene kernels' time of a normal_scene call
with the shape less that of one without.

  python tools/scene_fov_bench.py [--steps 3] [--out profiles/scene_fov.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
from jurassic_hip import lib
from bench_scene_jacobian import NPROF, median_s, workload
from bench_scene_normal import host_sums

NSHAPE = 21


def shape():
    dz = np.linspace(-2.0, 2.0, NSHAPE)
    return dz, np.exp(-0.5 * (dz / 0.8) ** 2)


def host_convolve(out, lay, geom, dz, w):
    """F and every block column of Model.kernel_scene's result convolved with lib.fov_apply, scan by scan, in place"""
    nd = out["rad"].shape[1]
    rp, k = out["rowptr"], out["k"]
    time_, vpz = geom[:, 0], geom[:, 4]
    lib.fov_apply(time_, vpz, out["rad"], out["tau"], dz, w)
    starts = np.flatnonzero(np.r_[True, time_[1:] != time_[:-1], True])
    for a, b in zip(starts[:-1], starts[1:]):
        width = int(rp[a + 1] - rp[a])
        if width == 0:
            continue
        cols = nd * width
        K = k[rp[a] * nd:rp[b] * nd].reshape(b - a, cols)
        half = cols // 2
        left, right = np.ascontiguousarray(K[:, :half]), np.ascontiguousarray(K[:, half:2 * half])
        lib.fov_apply(time_[a:b], vpz[a:b], left, right, dz, w)
        K[:, :half], K[:, half:2 * half] = left, right
        if cols > 2 * half:
            last = np.ascontiguousarray(K[:, 2 * half:])
            lib.fov_apply(time_[a:b], vpz[a:b], last, last.copy(), dz, w)
            K[:, 2 * half:] = last


def run(steps):
    case = workload("B", 0)
    c, atm, geom = case.ctl, case.atm, case.geom
    nd = c.nd
    dz, w = shape()
    model = lib.Model(c, case.lib_tables())
    model.set_atm(atm)
    lay = lib.scene_layout(c, atm, geom[:, 0])
    lay.update(lib.scene_slices(c, atm, geom[:, 0]))
    rng = np.random.default_rng(5)
    pencil = model.formod_host(geom)
    g, t = pencil["rad"].copy(), pencil["tau"].copy()
    lib.fov_apply(geom[:, 0], geom[:, 4], g, t, dz, w)
    y = g * (1.0 + 1e-3 * rng.standard_normal(g.shape))
    weight = 10.0 ** rng.uniform(0.0, 3.0, y.shape)

    keep = {"conv_s": [], "sums_s": []}
    model.set_fov(dz, w)
    def device():
        keep["dev"] = model.normal_scene(atm, geom, y, weight)
    device_s, device_all = median_s(device, steps)

    model.set_fov(None)
    def plain():
        keep["plain"] = model.normal_scene(atm, geom, y, weight)
    plain_s, plain_all = median_s(plain, steps)

    def host():
        out = model.kernel_scene(atm, geom)
        t0 = time.perf_counter()
        host_convolve(out, lay, geom, dz, w)
        t1 = time.perf_counter()
        keep["host"] = host_sums(out, lay, y, weight)
        keep["conv_s"].append(t1 - t0)
        keep["sums_s"].append(time.perf_counter() - t1)
        keep["host_rad"] = out["rad"]
    host_s, host_all = median_s(host, steps)

    dev, rel = keep["dev"], 0.0
    for s, (A, b, cost, n) in enumerate(keep["host"]):
        width = len(b)
        Ad = dev["A"][dev["aptr"][s]:dev["aptr"][s + 1]].reshape(width, width)
        rel = max(rel, float(np.abs(Ad - A).max() / np.abs(A).max()), abs(dev["cost"][s] - cost) / cost)
        assert dev["nlive"][s] == n
    same_g = bool(np.array_equal(dev["rad"].view(np.uint64), keep["host_rad"].view(np.uint64)))

    def scene_kernels_ms(call):
        model.enable_timing(True)
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        model.kernel_ms()
        ms = model.scene_ms()
        model.enable_timing(False)
        return ms["scene_ms"], ms["scene_launches"], dt
    without_ms, without_n, _ = scene_kernels_ms(lambda: model.normal_scene(atm, geom, y, weight))
    model.set_fov(dz, w)
    with_ms, with_n, timed_s = scene_kernels_ms(lambda: model.normal_scene(atm, geom, y, weight))
    model.close()

    forward_bytes = len(geom) * (2 * nd * 8 + 3 * 8 + 4)
    sums_bytes = int(lay["aptr"][-1] + lay["wptr"][-1] + 2 * len(lay["sfirst"])) * 8
    block_bytes = int(lay["rowptr"][-1]) * nd * 8
    return {"rays": len(geom), "profiles": NPROF, "rays_per_scan": len(geom) // NPROF, "channels": nd, "slices": len(lay["sfirst"]),
            "columns_per_slice": int(np.diff(lay["wptr"]).max()), "block_elements": int(lay["rowptr"][-1]) * nd,
            "shape_points": NSHAPE, "convolved_values_per_call": (int(lay["rowptr"][-1]) + len(geom)) * nd,
            "device_s": device_s, "device_s_all": device_all, "plain_s": plain_s, "plain_s_all": plain_all,
            "host_s": host_s, "host_s_all": host_all,
            "host_convolution_s": float(np.median(keep["conv_s"][1:])), "host_sums_s": float(np.median(keep["sums_s"][1:])),
            "host_over_device": host_s / device_s, "device_over_plain": device_s / plain_s,
            "bytes_to_host_device_route": forward_bytes + sums_bytes, "bytes_to_host_host_route": forward_bytes + block_bytes,
            "largest_relative_difference_of_the_two_routes": rel, "G_of_the_two_routes_bit_identical": same_g,
            "event_timed_call": {"call_s": timed_s, "scene_kernels_ms_with_the_shape": with_ms, "scene_kernels_ms_without": without_ms,
                                 "fov_kernel_launches": with_n - without_n, "fov_kernel_ms": with_ms - without_ms,
                                 "fov_kernel_share_of_the_call": (with_ms - without_ms) * 1e-3 / timed_s}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_fov.json"))
    args = ap.parse_args()
    doc = {"what": "field of view in the scene entries: Model.normal_scene with a shape set against Model.kernel_scene, "
                   "lib.fov_apply on F and every block column and the sums in numpy on the host (tools/scene_fov_bench.py)",
           "timing": "median of %d calls after one warm-up, host clock around calls that end in a device synchronise; pageable "
                     "host arrays on both routes" % args.steps,
           "device": lib.device_info(0)["pci_bus_id"]}
    doc["B"] = run(args.steps)
    print("B", json.dumps(doc["B"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
