#!/usr/bin/env python3
"""The hydrostatic balance per slice in the scene entries (Model.set_scene_hydz) on workload B of
tools/bench_scene_retrieve.py: 64 limb scans of the example's 66 rays, here with T retrieved on all levels and p at the
reference level (hydz = 10 km, a level of the example's profile).  Writes profiles/scene_hydro.json; asserts no threshold
-- nobody has measured these before.

  on / off          Model.retrieve_scene and Model.normal_scene with the switch on and off, the overhead in percent, and
                    the new kernel's milliseconds: the scene kernels of an event-timed call with the switch on less those
                    with it off
  todays_route      the only way to a hydrostatic Jacobian before: Model.kernel profile by profile on a model whose
                    ctl->hydz is set, against Model.kernel_scene with the switch on
  switch_off        Model.step_scene and Model.retrieve_scene with the switch off, and, with --parent-so, the same from
                    a library built from the parent commit: the two alternate in processes of their own, --rounds each
  one_scan          one scan of 13 limb rays through one profile whose truth is hydrostatic (the first guess balanced,
                    then a 3 K bump in T, balanced again): T retrieved from the same first guess with and without the
                    constraint, the root mean square of T - truth over the levels the scan sees

Each time is the median of --steps calls after one warm-up call, a host clock around calls that end in a device
synchronise.

  python tools/bench_scene_hydro.py [--steps 3] [--rounds 5] [--parent-so path/to/libjurassic_hip.so]"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
import common
from jurassic_hip import abi, lib
from bench_scene_jacobian import NPROF, PKG, median_s, one_profile, workload
from bench_scene_step import scene_kernels_ms
from bench_scene_retrieve import FAC, LAM0, LAM_MAX, LAM_MIN, MAX_ITER, TOL, copy_atm, rows_of

HYDZ = 10.0


def windows(c):
    """T on all levels, p at the reference level alone, no gas"""
    for g in range(c.ng):
        c.retq_zmin[g], c.retq_zmax[g] = -999.0, -999.0
    c.rett_zmin, c.rett_zmax = 0.0, 1000.0
    c.retp_zmin, c.retp_zmax = HYDZ - 0.1, HYDZ + 0.1


def setup():
    case = workload("B", 0)
    windows(case.ctl)
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
    r = 1.0 / np.where(iq == 1, 1.0, 0.1 * np.abs(x0) + 1e-12) ** 2     # sigma = 1 K, 10 % of p
    return case, model, lay, y, weight, iq, x0, r


def calls(case, model, y, weight, x0, r, keep=None):
    c, atm, geom = case.ctl, case.atm, case.geom

    def step():
        model.set_atm(atm)
        model.step_scene(atm, geom, y, weight, np.array(FAC), prior_ivar=r, prior_dx=np.zeros(len(x0)))

    def retrieve():
        model.set_atm(atm)
        out = model.retrieve_scene(atm, geom, y, weight, MAX_ITER, FAC, lam0=LAM0, lam_min=LAM_MIN, lam_max=LAM_MAX, tol=TOL,
                                   prior_ivar=r, prior_xa=x0)
        if keep is not None:
            keep["ret"] = out

    def normal():
        model.set_atm(atm)
        model.normal_scene(atm, geom, y, weight)
    return step, retrieve, normal


def baseline(steps):
    """step_scene and retrieve_scene with the switch off (never touched: a parent library has no such entry)"""
    case, model, lay, y, weight, iq, x0, r = setup()
    step, retrieve, _ = calls(case, model, y, weight, x0, r)
    out = {}
    for name, fn in (("step_scene", step), ("retrieve_scene", retrieve)):
        med, every = median_s(fn, steps)
        out[name + "_s"], out[name + "_s_all"] = med, every
    model.close()
    return out


def todays_route(case, steps):
    """Model.kernel on every profile alone under ctl->hydz, on its rays in packages"""
    c, atm, geom = case.ctl, case.atm, case.geom
    ch = abi.ctl_t.from_buffer_copy(bytes(c))
    ch.hydz = HYDZ
    model = lib.Model(ch, case.lib_tables())
    nlev = atm.np // NPROF
    profiles = [one_profile(atm, i, nlev) for i in range(NPROF)]
    rays_of = [np.flatnonzero(geom[:, 0] == i) for i in range(NPROF)]

    def loop():
        for i in range(NPROF):
            model.set_atm(profiles[i])
            for a in range(0, len(rays_of[i]), PKG):
                obs = common.obs_from_geom(geom[rays_of[i][a:a + PKG]], c.nd)
                np.ctypeslib.as_array(obs.rad)[:] = 0.0
                model.kernel(profiles[i], obs)
    med, every = median_s(loop, max(1, steps - 1))
    model.close()
    return med, every


def one_scan():
    """-> dict: rms of T - truth [K] over the levels between the lowest and the highest tangent point, both ways"""
    scan = common.golden_geometry("limb")
    geom = scan[np.linspace(5, len(scan) - 15, 13).astype(int)].copy()
    case = common.limb_case(geom=geom)
    c = case.ctl
    for g in range(c.ng):
        c.retq_zmin[g], c.retq_zmax[g] = -999.0, -999.0
    lo, hi = float(geom[:, 4].min()), float(geom[:, 4].max())
    c.rett_zmin, c.rett_zmax = lo - 0.1, hi + 0.1
    model = lib.Model(c, case.lib_tables())
    model.set_scene_hydz(HYDZ)
    time = geom[:, 0]
    guess = model.scene_hydrostatic(case.atm, time)                     # the first guess: the example's profile, balanced
    truth = copy_atm(guess)
    n = truth.np
    z = np.ctypeslib.as_array(truth.z)[:n]
    inside = (z >= c.rett_zmin) & (z <= c.rett_zmax)
    np.ctypeslib.as_array(truth.t)[:n][inside] += 3.0 * np.sin(np.pi * (z[inside] - lo) / (hi - lo)) ** 2
    truth = model.scene_hydrostatic(truth, time)
    model.set_atm(truth)
    y = model.formod_host(geom)["rad"]
    weight = np.full(y.shape, 1.0 / (1e-3 * np.abs(y).mean()) ** 2)
    t_true = np.ctypeslib.as_array(truth.t)[:n][inside]
    out = {"rays": len(geom), "levels": int(inside.sum()), "tangent_heights_km": [lo, hi], "bump_K": 3.0,
           "first_guess_rms_K": float(np.sqrt(np.mean((np.ctypeslib.as_array(guess.t)[:n][inside] - t_true) ** 2)))}
    for name, hydz in (("with_the_constraint", HYDZ), ("without_the_constraint", None)):
        model.set_scene_hydz(hydz)
        model.set_atm(guess)
        ret = model.retrieve_scene(guess, geom, y, weight, 8, FAC, lam0=LAM0, lam_min=LAM_MIN, lam_max=LAM_MAX, tol=TOL)
        t = np.ctypeslib.as_array(ret["atm"].t)[:n][inside]
        out[name + "_rms_K"] = float(np.sqrt(np.mean((t - t_true) ** 2)))
        out[name + "_cost"] = float(ret["cost"].sum())
    model.close()
    return out


def run(steps):
    case, model, lay, y, weight, iq, x0, r = setup()
    c, atm, geom = case.ctl, case.atm, case.geom
    keep = {}
    step, retrieve, normal = calls(case, model, y, weight, x0, r, keep)
    res = {"rays": len(geom), "profiles": NPROF, "slices": len(lay["sfirst"]), "columns_per_slice": int(np.diff(lay["wptr"]).max()),
           "p_elements": int((iq == 0).sum()), "hydz_km": HYDZ, "max_iter": MAX_ITER, "fac": list(FAC)}
    ev = {}
    for tag, hydz in (("off", None), ("on", HYDZ)):
        model.set_scene_hydz(hydz)
        for name, fn in (("retrieve_scene", retrieve), ("normal_scene", normal)):
            res["%s_%s_s" % (name, tag)], res["%s_%s_s_all" % (name, tag)] = median_s(fn, steps)
            ms, launches, dt = scene_kernels_ms(model, fn)
            ev["%s_%s" % (name, tag)] = {"scene_kernels_ms": ms, "scene_launches": launches, "call_s": dt}
        res["states_" + tag] = [int(v) for v in np.bincount(keep["ret"]["state"], minlength=4)]
    for name in ("retrieve_scene", "normal_scene"):
        res[name + "_overhead_percent"] = 100.0 * (res[name + "_on_s"] / res[name + "_off_s"] - 1.0)
        on, off = ev[name + "_on"], ev[name + "_off"]
        ev[name + "_new_kernel_ms"] = on["scene_kernels_ms"] - off["scene_kernels_ms"]
        ev[name + "_new_kernel_launches"] = on["scene_launches"] - off["scene_launches"]
        ev[name + "_new_kernel_share_of_the_call"] = ev[name + "_new_kernel_ms"] * 1e-3 / on["call_s"]
    res["event_timed_calls"] = ev

    def scene():
        model.set_atm(atm)
        model.kernel_scene(atm, geom)
    res["kernel_scene_on_s"], res["kernel_scene_on_s_all"] = median_s(scene, steps)
    model.close()
    res["todays_route_s"], res["todays_route_s_all"] = todays_route(case, steps)
    res["todays_route_over_kernel_scene"] = res["todays_route_s"] / res["kernel_scene_on_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5, help="alternating runs of this commit's and the parent's library")
    ap.add_argument("--parent-so", help="a libjurassic_hip.so built from the parent commit: its switch-off times are measured in processes of their own")
    ap.add_argument("--baseline-only", action="store_true", help="print the switch-off times as one JSON line and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_hydro.json"))
    args = ap.parse_args()
    if args.baseline_only:
        print("BASELINE " + json.dumps(baseline(args.steps)), flush=True)
        return
    doc = {"what": "hydrostatic balance per slice in the scene entries on workload B (64 limb scans, T on all levels and p at the "
                   "reference level): Model.retrieve_scene and Model.normal_scene with Model.set_scene_hydz on and off, Model.kernel "
                   "profile by profile under ctl->hydz against Model.kernel_scene, the switch-off times against the parent commit's, "
                   "and the T error of one 13-ray scan with and without the constraint (tools/bench_scene_hydro.py)",
           "timing": "median of %d calls after one warm-up, host clock around calls that end in a device synchronise; pageable host "
                     "arrays; no target was set for any of these numbers and nobody had measured them before" % args.steps,
           "device": lib.device_info(0)["pci_bus_id"],
           "kernel_resources": "jur_scene_hydro_kernel, from the compiler's report for gfx950: 70 VGPRs, 62 SGPRs, 1024 bytes of LDS, no scratch, no spills"}
    doc["B"] = run(args.steps)
    print("B " + json.dumps(doc["B"]), flush=True)
    doc["one_scan"] = one_scan()
    print("one_scan " + json.dumps(doc["one_scan"]), flush=True)

    def child(so):
        """the switch-off times of one library in a process of its own (both libraries alike: same start, same work)"""
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
