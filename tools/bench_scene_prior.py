#!/usr/bin/env python3
"""The full a-priori precision of the slices (Model.set_prior_precision, prior_corr) on workload B of
tools/bench_scene_retrieve.py: 64 limb scans of the example's 66 rays, T and O3 retrieved on all levels, 182 columns a
slice.  The prior is prior_corr with sigma = 1 K for T and 10 % for O3 and cz = 5 km for both.  Writes
profiles/scene_prior.json; asserts no threshold -- nobody has measured these before.

  full_device_s     Model.retrieve_scene and Model.diagnose_scene with the precision set (prior_ivar all zeros)
  full_host_s       the route a caller had before: Model.normal_scene, A + P, np.linalg.cholesky and the solves and
                    products per slice and damping in numpy, Model.set_atm and Model.formod_host per trial; for the
                    diagnostics normal_scene and the inverse, the products and the sums per slice in numpy
  diagonal_device_s the same two device calls with the diagonal prior 1 / sigma^2 alone, and the extra cost of the full one
  new kernels       the scene kernels of the event-timed call with the precision set less those with the diagonal prior
  prior_corr_s      against Sa in numpy and np.linalg.inv per slice
  no_precision      Model.step_scene and Model.retrieve_scene with nothing set: three calls each after a warm-up, and,
                    with --parent-so, the same from a library built from the parent commit, in a process of its own

Each time is the median of --steps calls after one warm-up call, a host clock around calls that end in a device
synchronise.

  python tools/bench_scene_prior.py [--steps 3] [--parent-so path/to/libjurassic_hip.so]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
from jurassic_hip import lib
from bench_scene_jacobian import NPROF, median_s, workload
from bench_scene_step import scene_kernels_ms
from bench_scene_retrieve import FAC, LAM0, LAM_MAX, LAM_MIN, MAX_ITER, TOL, copy_atm, rows_of

CZ_KM, SIGMA_T, SIGMA_REL = 5.0, 1.0, 0.1


def setup():
    case = workload("B", 0)
    c, atm, geom = case.ctl, case.atm, case.geom
    model = lib.Model(c, case.lib_tables())
    model.set_atm(atm)
    lay = lib.scene_slices(c, atm, geom[:, 0])
    rng = np.random.default_rng(5)
    y = model.formod_host(geom)["rad"] * (1.0 + 1e-3 * rng.standard_normal((len(geom), c.nd)))
    weight = 10.0 ** rng.uniform(0.0, 3.0, y.shape)
    return case, model, lay, y, weight


def baseline(steps):
    """step_scene and retrieve_scene with no precision set and the diagonal prior of tools/bench_scene_retrieve.py"""
    case, model, lay, y, weight = setup()
    c, atm, geom = case.ctl, case.atm, case.geom
    els = [lib.scene_elements(c, atm, lay["sfirst"][s], lay["slen"][s]) for s in range(len(lay["sfirst"]))]
    iq, ip = np.concatenate([e["iq"] for e in els]), np.concatenate([e["ip"] for e in els])
    rows0 = rows_of(c, atm)
    x0 = np.array([rows0[q][p] for q, p in zip(iq, ip)])
    sigma = np.where(iq == 1, SIGMA_T, SIGMA_REL * np.abs(x0) + 1e-12)
    r = 1.0 / sigma ** 2

    def step():
        model.set_atm(atm)
        model.step_scene(atm, geom, y, weight, np.array(FAC), prior_ivar=r, prior_dx=np.zeros(len(x0)))

    def retrieve():
        model.set_atm(atm)
        model.retrieve_scene(atm, geom, y, weight, MAX_ITER, FAC, lam0=LAM0, lam_min=LAM_MIN, lam_max=LAM_MAX, tol=TOL,
                             prior_ivar=r, prior_xa=x0)
    out = {}
    for name, fn in (("step_scene", step), ("retrieve_scene", retrieve)):
        med, every = median_s(fn, steps)
        out[name + "_s"], out[name + "_s_all"] = med, every
    model.close()
    return out


def host_retrieve(model, c, atm0, geom, y, weight, lay, iq, ip, P, xa):
    """the loop with a full prior as a caller writes it without this feature; -> final atm"""
    ns, wptr, aptr, sid = len(lay["sfirst"]), lay["wptr"], lay["aptr"], lay["sid"]
    fac = np.array(FAC)
    atm = copy_atm(atm0)
    lam, state = np.full(ns, LAM0), np.zeros(ns, dtype=np.int32)
    own = np.repeat(np.arange(ns), np.diff(wptr))
    live = (weight > 0) & np.isfinite(y) & (sid >= 0)[:, None]

    def prior_of(xx):
        return np.array([(xa - xx)[wptr[s]:wptr[s + 1]] @ P[s] @ (xa - xx)[wptr[s]:wptr[s + 1]] for s in range(ns)])

    for it in range(MAX_ITER):
        if not np.any(state == lib.RET_ACTIVE):
            break
        lamt = np.minimum(np.maximum(lam[None, :] * fac[:, None], LAM_MIN), LAM_MAX)
        model.set_atm(atm)
        rows = rows_of(c, atm)
        x = np.array([rows[q][p] for q, p in zip(iq, ip)])
        nm = model.normal_scene(atm, geom, y, weight)
        dx, status = np.zeros((len(FAC), len(x))), np.zeros((len(FAC), ns), dtype=np.int32)
        for s in range(ns):
            sl = slice(wptr[s], wptr[s + 1])
            w = wptr[s + 1] - wptr[s]
            M0 = nm["A"][aptr[s]:aptr[s + 1]].reshape(w, w) + P[s]
            g = nm["b"][sl] + P[s] @ (xa - x)[sl]
            for l in range(len(FAC)):
                M = M0 + lamt[l, s] * np.diag(np.diag(M0))
                try:
                    L = np.linalg.cholesky(M)
                    dx[l, sl] = np.linalg.solve(L.T, np.linalg.solve(L, g))
                except np.linalg.LinAlgError:
                    status[l, s] = 1
        tcost = np.zeros((len(FAC), ns))
        for l in range(len(FAC)):
            trial = copy_atm(atm)
            rows = rows_of(c, trial)
            for q in np.unique(iq):
                m = iq == q
                rows[q][ip[m]] += dx[l][m]
            model.set_atm(trial)
            d = y - model.formod_host(geom)["rad"]
            term = np.where(live, weight * d * d, 0.0).sum(axis=1)
            tcost[l] = np.bincount(sid[sid >= 0], weights=term[sid >= 0], minlength=ns) + prior_of(x + dx[l])
        dec = lib.retrieve_decide(nm["cost"] + prior_of(x), tcost, lamt, status, lam, state, TOL, LAM_MAX, fac.max())
        lam, state = dec["lam"], dec["state"]
        rows = rows_of(c, atm)
        for l in range(len(FAC)):
            took = (dec["accept"][own] == 1) & (dec["best"][own] == l)
            for q in np.unique(iq[took]):
                m = took & (iq == q)
                rows[q][ip[m]] += dx[l][m]
    model.set_atm(atm)
    model.formod_host(geom)
    return atm


def host_diagnose(model, atm, geom, y, weight, lay, P):
    ns, wptr, aptr = len(lay["sfirst"]), lay["wptr"], lay["aptr"]
    model.set_atm(atm)
    nm = model.normal_scene(atm, geom, y, weight)
    out = dict(sigma=np.zeros(wptr[-1]), sigma_noise=np.zeros(wptr[-1]), sigma_smooth=np.zeros(wptr[-1]), dofs=np.zeros(ns))
    for s in range(ns):
        w = wptr[s + 1] - wptr[s]
        A = nm["A"][aptr[s]:aptr[s + 1]].reshape(w, w)
        S = np.linalg.inv(A + P[s])
        K = S @ A
        sl = slice(wptr[s], wptr[s + 1])
        out["sigma"][sl] = np.sqrt(np.diag(S))
        out["sigma_noise"][sl] = np.sqrt(np.maximum((K * S).sum(axis=1), 0))
        out["sigma_smooth"][sl] = np.sqrt(np.maximum(((S @ P[s]) * S).sum(axis=1), 0))
        out["dofs"][s] = np.trace(K)
    return out


def run(steps):
    case, model, lay, y, weight = setup()
    c, atm, geom = case.ctl, case.atm, case.geom
    ns, wptr, aptr = len(lay["sfirst"]), lay["wptr"], lay["aptr"]
    nq = 2 + c.ng + c.nw
    sigma_q = [1.0, SIGMA_T] + [lambda v: SIGMA_REL * abs(v) + 1e-12] * c.ng + [1.0] * c.nw
    cz_q = [0.0, CZ_KM] + [CZ_KM] * c.ng + [0.0] * c.nw
    keep = {}

    def corr():
        keep["pc"] = lib.prior_corr(model, c, atm, geom[:, 0], sigma_q, cz_q)
    corr_s, corr_all = median_s(corr, steps)
    pc = keep["pc"]
    iq, ip, sigma, z = pc["iq"], pc["ip"], pc["sigma"], pc["z"]

    def corr_host():
        Rs = []
        for s in range(ns):
            sl = slice(wptr[s], wptr[s + 1])
            same = (iq[sl][:, None] == iq[sl][None, :]) & (np.array(cz_q)[iq[sl]][:, None] > 0)
            cz = np.where(same, np.array(cz_q)[iq[sl]][:, None], 1.0)
            Sa = np.where(same, np.outer(sigma[sl], sigma[sl]) * np.exp(-np.abs(z[sl][:, None] - z[sl][None, :]) / cz), 0.0)
            Sa[np.diag_indices(len(Sa))] = sigma[sl] ** 2
            Rs.append(np.linalg.inv(Sa))
        keep["R_host"] = Rs
    corr_host_s, corr_host_all = median_s(corr_host, steps)
    rel_R = max(float(np.abs(pc["R"][aptr[s]:aptr[s + 1]].reshape(Rm.shape) - Rm).max() / np.abs(Rm).max()) for s, Rm in enumerate(keep["R_host"]))

    rows0 = rows_of(c, atm)
    x0 = np.array([rows0[q][p] for q, p in zip(iq, ip)])
    zeros = np.zeros(len(x0))
    P = [pc["R"][aptr[s]:aptr[s + 1]].reshape(wptr[s + 1] - wptr[s], -1) for s in range(ns)]

    def retrieve(**pk):
        model.set_atm(atm)
        keep["ret"] = model.retrieve_scene(atm, geom, y, weight, MAX_ITER, FAC, lam0=LAM0, lam_min=LAM_MIN, lam_max=LAM_MAX, tol=TOL,
                                           history=True, **pk)

    def diagnose(prior_ivar):
        keep["dg"] = model.diagnose_scene(keep["ret"]["atm"], geom, y, weight, prior_ivar=prior_ivar)

    res = {}
    model.set_prior_precision(wptr, pc["R"])
    res["full_device_retrieve_s"], res["full_device_retrieve_s_all"] = median_s(lambda: retrieve(prior_ivar=zeros, prior_xa=x0), steps)
    full = keep["ret"]
    res["full_device_diagnose_s"], res["full_device_diagnose_s_all"] = median_s(lambda: diagnose(zeros), steps)
    dg_full = keep["dg"]
    model.set_atm(atm)
    full_ms, full_launches, timed_s = scene_kernels_ms(model, lambda: retrieve(prior_ivar=zeros, prior_xa=x0))
    dgf_ms, dgf_launches, dg_timed_s = scene_kernels_ms(model, lambda: diagnose(zeros))
    model.set_prior_precision(None)

    def host():
        keep["host_atm"] = host_retrieve(model, c, atm, geom, y, weight, lay, iq, ip, P, x0)
    res["full_host_retrieve_s"], res["full_host_retrieve_s_all"] = median_s(host, max(1, steps - 1))

    def host_dg():
        keep["host_dg"] = host_diagnose(model, full["atm"], geom, y, weight, lay, P)
    res["full_host_diagnose_s"], res["full_host_diagnose_s_all"] = median_s(host_dg, max(1, steps - 1))
    rows_d, rows_h = rows_of(c, full["atm"]), rows_of(c, keep["host_atm"])
    x_d = np.array([rows_d[q][p] for q, p in zip(iq, ip)])
    x_h = np.array([rows_h[q][p] for q, p in zip(iq, ip)])

    r = 1.0 / sigma ** 2
    res["diagonal_device_retrieve_s"], res["diagonal_device_retrieve_s_all"] = median_s(lambda: retrieve(prior_ivar=r, prior_xa=x0), steps)
    res["diagonal_device_diagnose_s"], res["diagonal_device_diagnose_s_all"] = median_s(lambda: diagnose(r), steps)
    model.set_atm(atm)
    dia_ms, dia_launches, dia_timed_s = scene_kernels_ms(model, lambda: retrieve(prior_ivar=r, prior_xa=x0))
    dgd_ms, dgd_launches, _ = scene_kernels_ms(model, lambda: diagnose(r))
    model.close()

    res.update({
        "rays": len(geom), "profiles": NPROF, "slices": ns, "columns_per_slice": int(np.diff(wptr).max()),
        "sigma": "1 K (T), 10 % (O3)", "cz_km": CZ_KM, "max_iter": MAX_ITER, "fac": list(FAC), "damping": "Marquardt",
        "prior_corr_status_nonzero": int(np.count_nonzero(pc["status"])),
        "states_full": [int(v) for v in np.bincount(full["state"], minlength=4)],
        "states_diagonal": [int(v) for v in np.bincount(keep["ret"]["state"], minlength=4)],
        "host_over_device_retrieve": res["full_host_retrieve_s"] / res["full_device_retrieve_s"],
        "host_over_device_diagnose": res["full_host_diagnose_s"] / res["full_device_diagnose_s"],
        "extra_cost_of_the_full_prior_retrieve_percent": 100.0 * (res["full_device_retrieve_s"] / res["diagonal_device_retrieve_s"] - 1.0),
        "extra_cost_of_the_full_prior_diagnose_percent": 100.0 * (res["full_device_diagnose_s"] / res["diagonal_device_diagnose_s"] - 1.0),
        "largest_relative_difference_of_the_retrieved_states_device_host": float(np.abs(x_d - x_h).max() / np.abs(x_h).max()),
        "largest_relative_difference_of_sigma_device_host": float(np.max(np.abs(dg_full["sigma"] - keep["host_dg"]["sigma"]) / keep["host_dg"]["sigma"])),
        "dofs_per_slice_full_min_max": [float(dg_full["dofs"].min()), float(dg_full["dofs"].max())],
        "bytes_of_normal_matrices_the_host_route_brings_home_per_iteration": int(aptr[-1]) * 8,
        "prior_corr_s": corr_s, "prior_corr_s_all": corr_all, "prior_corr_numpy_s": corr_host_s, "prior_corr_numpy_s_all": corr_host_all,
        "largest_relative_difference_of_R_device_numpy": rel_R,
        "event_timed_calls": {"retrieve_call_s": timed_s, "scene_kernels_ms_retrieve_full": full_ms, "scene_launches_retrieve_full": full_launches,
                              "scene_kernels_ms_retrieve_diagonal": dia_ms, "scene_launches_retrieve_diagonal": dia_launches,
                              "new_kernels_ms_retrieve": full_ms - dia_ms, "new_kernels_share_of_the_retrieve_call": (full_ms - dia_ms) * 1e-3 / timed_s,
                              "diagnose_call_s": dg_timed_s, "scene_kernels_ms_diagnose_full": dgf_ms, "scene_kernels_ms_diagnose_diagonal": dgd_ms,
                              "new_kernels_ms_diagnose": dgf_ms - dgd_ms, "new_kernels_share_of_the_diagnose_call": (dgf_ms - dgd_ms) * 1e-3 / dg_timed_s}})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--parent-so", help="a libjurassic_hip.so built from the parent commit: its no-precision times are measured in a process of its own")
    ap.add_argument("--baseline-only", action="store_true", help="print the no-precision times as one JSON line and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_prior.json"))
    args = ap.parse_args()
    if args.baseline_only:
        print("BASELINE " + json.dumps(baseline(args.steps)), flush=True)
        return
    doc = {"what": "full a-priori precision of the slices on workload B (64 limb scans, 182 columns a slice): Model.retrieve_scene and "
                   "Model.diagnose_scene with Model.set_prior_precision against the host route over Model.normal_scene and numpy, "
                   "against the diagonal prior, and prior_corr against numpy (tools/bench_scene_prior.py)",
           "timing": "median of %d calls after one warm-up, host clock around calls that end in a device synchronise; pageable host "
                     "arrays; no target was set for any of these numbers and nobody had measured them before" % args.steps,
           "device": lib.device_info(0)["pci_bus_id"]}
    doc["B"] = run(args.steps)
    def child(so):
        """the no-precision times of one library in a process of its own (both libraries alike: same start, same work)"""
        env = dict(os.environ)
        if so:
            env["JURASSIC_HIP_SO"] = os.path.abspath(so)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-only", "--steps", str(args.steps)], env=env,
                             capture_output=True, text=True, check=True).stdout
        return json.loads([ln for ln in out.splitlines() if ln.startswith("BASELINE ")][-1][len("BASELINE "):])

    if not args.parent_so:
        doc["no_precision"] = {"this_commit": baseline(args.steps)}
    else:                                               # the two libraries alternate, twice: a round is one comparison
        doc["no_precision"] = {"rounds": []}
        for _ in range(2):
            this, parent = child(None), child(args.parent_so)
            rnd = {"this_commit": this, "parent_commit": parent}
            for f in ("step_scene", "retrieve_scene"):
                rnd[f + "_within_or_below_the_spread_of_the_parent"] = bool(this[f + "_s"] <= max(parent[f + "_s_all"]))
            doc["no_precision"]["rounds"].append(rnd)
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
