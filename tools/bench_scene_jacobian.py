#!/usr/bin/env python3
"""The block Jacobian of a scene (Model.kernel_scene, jur_kernel_scene_host) on two workloads, against the only way
the dense entry offers for the same numbers and against the forward model's floor.  Writes
profiles/scene_jacobian.json; asserts no threshold.

  A  64 profiles (synth.stack_profiles, as bench.py), nadir example, T and CO2 retrieved on all levels, 1e5 nadir rays
  B  64 profiles, limb example: 64 scans of the example's 66 rays, T and O3 retrieved on all levels

  scene_s    Model.kernel_scene on the whole scene, one call
  loop_s     per profile: Model.kernel with that profile alone as the atmosphere, on its rays in packages of <= 1088
             (the dense entry on the whole atmosphere would compute 64 columns for every one that matters)
  floor_s    Model.formod_host on as many rays as kernel_scene replicates (the scene's rays tiled): the same forward
             work without stacking, replication and quotients

Each time is the median of --steps calls after one warm-up call, a host clock around calls that end in a device
synchronise.  The share of the new kernels comes from the model's event timing in a call of its own.

  python tools/bench_scene_jacobian.py [--steps 3] [--rays-a 100000] [--only A|B]"""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import common
from jurassic_hip import abi, lib, synth

NPROF, PKG = 64, 1088


def one_profile(atm, i, n):
    """profile i (n levels) of a stacked atmosphere as an atmosphere of its own"""
    a = abi.atm_t()
    a.np = n
    s = slice(i * n, (i + 1) * n)
    for f in ("time", "z", "lon", "lat", "p", "t"):
        np.ctypeslib.as_array(getattr(a, f))[:n] = np.ctypeslib.as_array(getattr(atm, f))[s]
    np.ctypeslib.as_array(a.q)[:, :n] = np.ctypeslib.as_array(atm.q)[:, s]
    np.ctypeslib.as_array(a.k)[:, :n] = np.ctypeslib.as_array(atm.k)[:, s]
    return a


def median_s(fn, steps):
    fn()                                         # warm-up: workspace, staging and code objects of this shape
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t), t


def workload(name, nrays_a):
    if name == "A":
        geom = synth.nadir_rays(np.arange(nrays_a), nprofiles=NPROF)
        case = common.nadir_case(geom=geom, nprofiles=NPROF)
        gas = 0                                  # CO2
    else:
        scan = common.golden_geometry("limb")
        geom = np.tile(scan, (NPROF, 1))
        geom[:, 0] = np.repeat(np.arange(NPROF), len(scan))
        case = common.limb_case(geom=geom, nprofiles=NPROF)
        gas = 2                                  # O3
    c = case.ctl
    c.rett_zmin, c.rett_zmax = 0.0, 1000.0
    c.retq_zmin[gas], c.retq_zmax[gas] = 0.0, 1000.0
    return case


def run(name, steps, nrays_a):
    case = workload(name, nrays_a)
    c, atm, geom = case.ctl, case.atm, case.geom
    nlev = atm.np // NPROF
    model = lib.Model(c, case.lib_tables())
    model.set_atm(atm)
    lay = lib.scene_layout(c, atm, geom[:, 0])
    slots = int(lay["rowptr"][-1]) + len(geom)

    keep = {}
    def scene():
        keep["out"] = model.kernel_scene(atm, geom)
    scene_s, scene_all = median_s(scene, steps)

    profiles = [one_profile(atm, i, nlev) for i in range(NPROF)]
    rays_of = [np.flatnonzero(geom[:, 0] == i) for i in range(NPROF)]
    def loop():
        blocks = []
        for i in range(NPROF):
            for a in range(0, len(rays_of[i]), PKG):
                obs = common.obs_from_geom(geom[rays_of[i][a:a + PKG]], c.nd)
                np.ctypeslib.as_array(obs.rad)[:] = 0.0
                blocks.append(model.kernel(profiles[i], obs))
        keep["loop"] = blocks
    loop_s, loop_all = median_s(loop, max(1, steps - 1))

    # the same numbers?  (bit for bit: both put the same values through the same forward model)
    out, nd = keep["out"], c.nd
    differing, j = 0, 0
    for i in range(NPROF):
        for a in range(0, len(rays_of[i]), PKG):
            k = keep["loop"][j]
            j += 1
            for row, r in enumerate(rays_of[i][a:a + PKG]):
                blk = out["k"][out["rowptr"][r] * nd:out["rowptr"][r + 1] * nd].reshape(nd, -1)
                differing += int(np.count_nonzero(blk.view(np.uint64) != k[row * nd:(row + 1) * nd].view(np.uint64)))
    model.set_atm(atm)

    big = np.tile(geom, (-(-slots // len(geom)), 1))[:slots]
    buf = model.host_buffers(slots, pinned=False)
    buf.set_geometry(big)
    def floor():
        buf.rad[...] = 0.0
        model.formod_host_buffers(buf)
    floor_s, floor_all = median_s(floor, steps)

    model.enable_timing(True)
    t0 = time.perf_counter()
    model.kernel_scene(atm, geom)
    timed_s = time.perf_counter() - t0
    kms = model.kernel_ms()
    sms = model.scene_ms()
    model.enable_timing(False)
    model.close()
    forward_ms = kms["trace_ms"] + kms["ega_ms"] + kms["combine_ms"] + kms["pencil_ms"]
    return {"rays": len(geom), "profiles": NPROF, "levels_per_profile": nlev, "channels": nd, "emitters": c.ng,
            "columns_per_ray": int(np.diff(lay["rowptr"]).max()), "state_size_of_the_scene": int(len(lib.scene_columns(c, atm, 0, atm.np))),
            "replicated_rays": slots, "block_elements": int(lay["rowptr"][-1]) * nd,
            "scene_s": scene_s, "scene_s_all": scene_all, "loop_s": loop_s, "loop_s_all": loop_all, "loop_calls": len(keep["loop"]),
            "floor_s": floor_s, "floor_s_all": floor_all,
            "scene_over_floor": scene_s / floor_s, "loop_over_scene": loop_s / scene_s,
            "entries_that_differ_from_the_loop": differing,
            "event_timed_call": {"call_s": timed_s, "scene_kernels_ms": sms["scene_ms"], "scene_kernel_brackets": sms["scene_launches"],
                                 "forward_model_kernels_ms": forward_ms,
                                 "scene_kernels_share_of_the_call": sms["scene_ms"] * 1e-3 / timed_s}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rays-a", type=int, default=100000)
    ap.add_argument("--only", choices=["A", "B"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_jacobian.json"))
    args = ap.parse_args()
    doc = {"what": "block Jacobian of a scene: Model.kernel_scene against the per-profile loop over Model.kernel and against "
                   "Model.formod_host on as many rays as it replicates (tools/bench_scene_jacobian.py)",
           "timing": "median of %d calls after one warm-up, host clock around calls that end in a device synchronise; pageable "
                     "host arrays on all three" % args.steps,
           "device": lib.device_info(0)["pci_bus_id"]}
    for name in ("A", "B"):
        if args.only in (None, name):
            doc[name] = run(name, args.steps, args.rays_a)
            print(name, json.dumps(doc[name]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {q: doc[k][q] for q in ("scene_s", "loop_s", "floor_s", "scene_over_floor", "loop_over_scene")}
                      for k in ("A", "B") if k in doc}))


if __name__ == "__main__":
    main()
