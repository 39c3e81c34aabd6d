"""The cases on which oracle and HIP path are held against the reference's own CPU forward model
(tests/test_reference_cpu.py live and against the stored results, tests/test_reference_gpu.py against the stored
results, tools/make_reference_goldens.py writes them), and what the three share: how a case's files are written,
the hash over its inputs, the stored results, and the predicate that names the rays on which the reference's result
is not defined.

Every program reads the SAME table and filter files (Case.write_files): the oracle fed the in-memory rows against
a reference reading their %.9g text differs by 2.7e-8 relative on radiances."""
import hashlib
import json
import os
import numpy as np
import common
from jurassic_hip import abi, synth

STORE = os.path.join(common.GOLD, "reference_runs")

# bounds of oracle against reference (tau, tangent point, finite mask: equal bits)
RAD_RTOL = 1e-14           # ~24x the 4.2e-16 measured: a few ulp for a compiler that contracts differently
JAC_RTOL = 1e-10           # of the column's largest entry: ~24x the 4.2e-12 measured (last-bit rad difference / h)

SWITCHES = {"no_co2": dict(ctm_co2=0), "no_h2o": dict(ctm_h2o=0), "no_n2_o2": dict(ctm_n2=0, ctm_o2=0),
            "no_continua": dict(ctm_co2=0, ctm_h2o=0, ctm_n2=0, ctm_o2=0), "no_refrac": dict(refrac=0),
            "coarse_steps": dict(rayds=20.0, raydz=1.0), "hydz10": dict(hydz=10.0)}

# test_table_shapes' cases.  The reference defines a result for all seven, so all seven are run through it: fewer than two
# levels / temperatures / column densities are its own "no table" branches (jr_common.h:240-246), descending levels
# send locate_id (jr_common.h:107-115) to an end bracket from which it extrapolates, and a missing file leaves the
# table's counters as get_tbl's malloc hands them out (jr_common.h:71) -- zero in a fresh process, which is one more
# reason why oracle/ref.py starts one per configuration.
TABLE_SHAPES = {"descending": dict(table_kw=dict(descending=True)),
                "one_level": dict(table_kw=dict(nlev=1)),
                "one_temperature": dict(table_kw=dict(ntemp=1)),
                "one_column_density": dict(table_kw=dict(umax_eps=-1.0)),
                "max_extents": dict(table_kw=dict(nlev=40, ntemp=30, ratio=1.08)),
                "duplicates": dict(table_kw=dict(dup_every=7)),
                "missing": dict(missing={(0, 1), (2, 0), (3, 0), (3, 1)})}


def scene_case(name, extinction=False):
    case = common.limb_case()
    if extinction:                                      # on the base profile: synth.scene regrids k from it
        common.extinction_profile(case.atm)
    case.atm, case.geom, _ = synth.scene(name, case.ctl, case.atm)
    return case


def _with_extinction(case):
    """The shipped profiles carry k = 0 and the random cases a constant: these carry common.extinction_profile."""
    common.extinction_profile(case.atm)
    return case


def _extinction_only():
    """No emitter, no continuum: the extinction alone, on the limb example's rays and 13 nadir rays."""
    geom = np.vstack([common.golden_geometry("limb"), synth.nadir_geometry(13, seed=4)])
    return _with_extinction(common.Case([], [792.0, 832.0], os.path.join(common.GOLD, "limb", "atm.tab"), geom,
                                        ctm_co2=0, ctm_h2o=0, ctm_n2=0, ctm_o2=0, ctm_auto=1))


def _nan_mask():
    case = common.limb_case()
    rad_in = np.zeros((len(case.geom), 2))
    rad_in[0, 0] = np.nan
    rad_in[65, 1] = -np.inf
    return case, rad_in


def _builders():
    b = {"limb": lambda: (common.limb_case(), None),
         "nadir": lambda: (common.nadir_case(), None),
         "limb_four_continua": lambda: (common.limb_case(nu=common.CTM4_NU), None)}
    for seed in range(24):
        b["random_%d" % (100 + seed)] = lambda seed=seed: (common.random_case(100 + seed), None)
    for name, sw in SWITCHES.items():
        b["switch_" + name] = lambda sw=sw: (common.limb_case(geom=synth.limb_geometry(300, seed=2), nu=common.CTM4_NU,
                                                              ctm_auto=1, **sw), None)
    for name, kw in TABLE_SHAPES.items():
        b["tables_" + name] = lambda kw=kw: (common.limb_case(geom=synth.limb_geometry(200, seed=9), **kw), None)
    b["nan_mask"] = _nan_mask
    for name in sorted(synth.SCENES):
        b["scene_" + name] = lambda name=name: (scene_case(name), None)
    b["extinction_limb"] = lambda: (_with_extinction(common.limb_case()), None)
    b["extinction_nadir"] = lambda: (_with_extinction(common.nadir_case()), None)
    b["extinction_only"] = lambda: (_extinction_only(), None)
    b["scene_ragged_extinction"] = lambda: (scene_case("ragged", extinction=True), None)
    return b


FORMOD = _builders()
SCENE_CASES = [n for n in FORMOD if n.startswith("scene_")]
# (extinction: the retk columns, 10 .. 20 km, perturb the non-zero values of common.extinction_profile)
# (nd3_bbt: three channels in brightness temperatures -- the epilogue's log1p inside every difference quotient)
JACOBIANS = {"jacobian": dict(), "jacobian_hydz10": dict(hydz=10.0), "jacobian_extinction": dict(extinction=True),
             "jacobian_nd3_bbt": dict(channels="nd3bbt")}


def jacobian_case(name):
    """-> (case, obs with one measurement masked) as test_jacobian_matches_reference_kernel."""
    kw = dict(JACOBIANS[name])
    extinction = kw.pop("extinction", False)
    kw.update(common.CHANNELS[kw.pop("channels")] if "channels" in kw else {})
    case = common.retrieval_case(**kw)
    if extinction:
        common.extinction_profile(case.atm)
    obs = common.obs_from_geom(case.geom, case.ctl.nd)
    obs.rad[5][1] = float("nan")
    return case, obs


def obs_of(case, rad_in=None):
    obs = common.obs_from_geom(case.geom, case.ctl.nd)
    if rad_in is not None:
        np.ctypeslib.as_array(obs.rad)[:len(case.geom), :case.ctl.nd] = rad_in
    return obs


# ---------------------------------------------------------------------------------------------------------------------
# hash over a case's inputs

_CTL_SCALARS = ("ng", "nd", "nw", "hydz", "ctm_co2", "ctm_h2o", "ctm_n2", "ctm_o2", "ip", "cz", "cx", "refrac", "rayds",
                "raydz", "retp_zmin", "retp_zmax", "rett_zmin", "rett_zmax", "write_bbt", "formod")


def input_hash(case, dirname, rad_in=None):
    """sha256 over the control fields in use, the atmosphere's arrays, the geometry, the incoming radiance mask and the
    bytes of the table and filter files written to dirname (by name, without the directory)."""
    h = hashlib.sha256()
    c = case.ctl
    doc = {k: getattr(c, k) for k in _CTL_SCALARS}
    doc["emitter"] = [c.emitter[g].value.decode() for g in range(c.ng)]
    doc["nu"] = [float(c.nu[d]).hex() for d in range(c.nd)]
    doc["window"] = [int(c.window[d]) for d in range(c.nd)]
    doc["retq"] = [(float(c.retq_zmin[g]).hex(), float(c.retq_zmax[g]).hex()) for g in range(c.ng)]
    doc["retk"] = [(float(c.retk_zmin[w]).hex(), float(c.retk_zmax[w]).hex()) for w in range(c.nw)]
    for k, v in doc.items():
        if isinstance(v, float):
            doc[k] = v.hex()
    h.update(json.dumps(doc, sort_keys=True).encode())
    n = case.atm.np
    for name in ("time", "z", "lon", "lat", "p", "t"):
        h.update(np.ctypeslib.as_array(getattr(case.atm, name))[:n].tobytes())
    h.update(np.ctypeslib.as_array(case.atm.q)[:c.ng, :n].tobytes())
    h.update(np.ctypeslib.as_array(case.atm.k)[:c.nw, :n].tobytes())
    h.update(np.ascontiguousarray(case.geom, dtype=np.float64).tobytes())
    if rad_in is not None:
        h.update(np.isfinite(rad_in).tobytes())
    for f in sorted(os.listdir(dirname)):
        if f.endswith(".tab") or f.endswith(".filt"):
            h.update(f.encode())
            with open(os.path.join(dirname, f), "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------------
# the three programs on one case's files

def oracle_tables(orc, case):
    tb = orc.Tables(case.ctl.ng, case.ctl.nd)
    tb.read_ascii(case.ctl)
    assert tb.planck_filt(case.ctl) == 0
    return tb


def run_oracle(orc, case, rad_in=None):
    """The oracle on the files case.write_files wrote -> dict(rad, tau, tp, np)."""
    return orc.formod_rays(case.ctl, case.atm, oracle_tables(orc, case), case.geom, rad_in=rad_in)


def run_reference(ref, case, rad_in=None):
    """The reference's formod() on the same files, in a fresh process -> dict(rad, tau, tp)."""
    return ref.arrays(ref.formod(case.ctl, case.atm, obs_of(case, rad_in)), case.ctl.nd)


# ---------------------------------------------------------------------------------------------------------------------
# stored reference results

def manifest():
    with open(os.path.join(STORE, "manifest.json")) as fh:
        return {e["case"]: e for e in json.load(fh)["cases"]}


def pack(res):
    """rad | tau | tp side by side: (nr, 2 nd + 3) float64."""
    return np.ascontiguousarray(np.hstack([res["rad"], res["tau"], res["tp"]]), dtype=np.float64)


def store(name, arr):
    """One .npy per case; a Jacobian (131 x 69 doubles = 72 KB, 197 x 69 = 109 KB with three channels) goes in two halves
    of its rows, each under 64 KB."""
    parts = {name: arr} if name not in JACOBIANS else {name + ".rows_a": arr[:len(arr) // 2], name + ".rows_b": arr[len(arr) // 2:]}
    for k, a in parts.items():
        np.save(os.path.join(STORE, k + ".npy"), np.ascontiguousarray(a, dtype=np.float64))
        assert os.path.getsize(os.path.join(STORE, k + ".npy")) < 64 * 1024, k
    return sorted(parts)


def stored(name):
    if name in JACOBIANS:
        return np.vstack([np.load(os.path.join(STORE, "%s.rows_%s.npy" % (name, h))) for h in "ab"])
    a = np.load(os.path.join(STORE, name + ".npy"))
    nd = (a.shape[1] - 3) // 2
    return dict(rad=a[:, :nd], tau=a[:, nd:2 * nd], tp=a[:, 2 * nd:])


# ---------------------------------------------------------------------------------------------------------------------
# rays on which the reference's result is not defined

def locate_atm(time, t):
    """The slice (first index, length) the reference's locate_atm (jr_common.h:127-154) gives a ray of time stamp t:
    two bisections over the profile time stamps as they are stored, sorted or not."""
    n = len(time)
    lo, hi = 0, n - 1
    while hi > lo + 1:
        i = (lo + hi) // 2
        if time[i] < t:
            lo = i
        else:
            hi = i
    lower = lo if lo == 0 else hi
    lo, hi = lower, n - 1
    while hi > lo + 1:
        i = (lo + hi) // 2
        if time[i] > t:
            hi = i
        else:
            lo = i
    upper = n if hi == n - 1 else hi
    return lower, upper - lower


def altitude_range(atm, idx, n):
    """altitude_range_nn (jr_common.h:410-419): the range of the slice's leading points that share the first one's place."""
    z, lon, lat = (np.ctypeslib.as_array(getattr(atm, k)) for k in ("z", "lon", "lat"))
    zmin = zmax = z[idx]
    for i in range(idx, idx + n):
        if lon[i] != lon[idx] or lat[i] != lat[idx]:
            break
        zmin, zmax = min(zmin, z[i]), max(zmax, z[i])
    return zmin, zmax


def departing(case):
    """Boolean per ray, from the inputs alone: the rays whose LOS the reference leaves at its FIRST point.

    A slice without vertical extent (zmin == zmax: one point, or a first point whose place the second does not share)
    that the ray passes both of traceray's early returns for (observer not below it, view point at least 1 m below
    it, jr_common.h:600-601): the entry search stops within 1 m below zmax, which is below zmin, so the escape branch
    runs with np == 0 and reads los[-1] (jr_common.h:640-646).  The oracle and the kernels do not enter such a
    slice (np = 0, no radiance, unit transmittance, the view point as tangent point)."""
    time = np.ctypeslib.as_array(case.atm.time)[:case.atm.np]
    out = np.zeros(len(case.geom), dtype=bool)
    for i, g in enumerate(case.geom):
        idx, n = locate_atm(time, g[0])
        zmin, zmax = altitude_range(case.atm, idx, n)
        out[i] = zmin == zmax and g[1] >= zmin and g[4] <= zmax - 0.001
    return out


# ---------------------------------------------------------------------------------------------------------------------
# child process of tests/test_reference_gpu.py: the drop-in formod() on every case, one after the other

def _dropin_child(outdir):
    """The drop-in entry keeps its tables for the life of the process, as the reference does; jur_dropin_finalize()
    between the cases lets the next formod() read the next case's files.  Ends at the first case that fails."""
    import tempfile
    from jurassic_hip import lib
    for name, build in FORMOD.items():
        case, rad_in = build()
        with tempfile.TemporaryDirectory() as d:
            case.write_files(d)
            case.ctl.useGPU = 1
            obs = obs_of(case, rad_in)
            lib.formod(case.ctl, case.atm, obs)
            lib.dropin_finalize()
        n, nd = obs.nr, case.ctl.nd
        res = {k: np.ctypeslib.as_array(getattr(obs, k))[:n, :nd] for k in ("rad", "tau")}
        res["tp"] = np.stack([np.ctypeslib.as_array(getattr(obs, k))[:n] for k in ("tpz", "tplon", "tplat")], axis=1)
        np.save(os.path.join(outdir, name + ".npy"), pack(res))
        print("DROPIN_DONE", name, flush=True)


if __name__ == "__main__":
    import sys
    _dropin_child(sys.argv[1])
