"""Inputs and yardstick of the LOS-record test (tests/test_kat_gpu.py::test_los_records_against_the_oracle, CPU twin in
tests/test_scenes_cpu.py): the configurations the batched ray tracer's per-point output is held to oracle.traceray on,
and the bound, which comes from the oracle alone.

Tracer and oracle run the same operations in the same order; they differ through the last bits of the device's
sin / cos / asin / atan2 / exp / log, amplified along up to 400 steps.  How far a one-ulp error moves a record is the
oracle's own conditioning: every ray is traced twice more on the CPU with all six geometry coordinates moved one ulp
up, then one ulp down, and Y_f is the largest movement of field f over all rays, each point's movement divided by that
ray's largest |value| of the field (per gas for the column densities) -- the worst point is always the clipped one
before the exit, whose plain relative error reaches 4e-9.  The device's deviation, scaled the same way, must stay within
FACTOR * max(Y_f, 2^-52) and within CAP whatever Y_f is.  FACTOR = 64: one-ulp errors injected in each of up to 400
steps add like a random walk (sqrt(400) = 20), each amplified like an input nudge, with a factor 3 of headroom."""
import os
import subprocess
import numpy as np
import common
from jurassic_hip import synth

FACTOR = 64.0
CAP = 1e-9
FIELDS = ("p", "t", "ds", "k", "q", "u")
EMITTERS8 = ["CO2", "H2O", "O3", "F11", "CCl4", "CH4", "N2O", "HNO3"]

# short paths on the 0 .. 90 km limb profile, with the oracle's LOS point counts: zenith views from just below the top,
# an observer 0.3 km above the ground looking straight down (ground hit), an observer on the ground (ds = 0)
SHORT_PATHS = np.array([[0, 89.2, 0, 0, 89.9, 0, 0], [0, 89.6, 0, 0, 89.9, 0, 0], [0, 0.3, 0, 0, 0.0, 0, 0],
                        [0, 0.0, 0, 0, 0.0, 0, 0]], dtype=np.float64)
SHORT_PATHS[3, 4] = -0.5
SHORT_NP = [3, 2, 2, 2]


def edge_rays():
    """The rays of test_edge_geometries (tests/test_parity_gpu.py)."""
    g = synth.limb_geometry(8, scan=True, zmin=-20.0, zmax=2.0)
    rest = np.array([[0, 30.0, 0, 0, 5.0, 0, 3.0], [0, 10.0, 0, 0, 60.0, 0, 2.0], [0, 20.0, 0, 0, 80.0, 0, 0.0],
                     [0, 780.0, 0, 0, 95.0, 0, 20.0], [0, -1.0, 0, 0, 10.0, 0, 1.0]])
    return np.vstack([g, rest])


def standard_rays(nprofiles=1):
    """A limb scan of 70 rays from -8 to 70 km tangent height (two tiles of 64 slots, the second ragged), 13 nadir
    rays, the edge rays, the short paths; 100 rays, dealt to the profiles in turn."""
    g = np.vstack([synth.limb_geometry(70, scan=True, zmin=-8.0, zmax=70.0), synth.nadir_geometry(13, seed=4), edge_rays(),
                   SHORT_PATHS])
    g[:, 0] = np.arange(len(g)) % nprofiles
    return g


def thin_slice_case():
    """The atmosphere of test_leaving_the_slice_at_the_first_point (tests/test_scenes_cpu.py): a slice 1 cm thick, whose
    two rays are the one point at which they enter (np = 1, ds = 0), and a 0 .. 60 km profile for the standard rays."""
    case = common.limb_case()
    common.extinction_profile(case.atm)
    spec = [dict(time=0.0, lon=0.0, lat=0.0, n=2, z0=10.0, z1=10.00001), dict(time=1.0, lon=0.0, lat=0.0, n=30, z0=0.0, z1=60.0)]
    case.atm = synth.ragged_atmosphere(case.ctl, spec, base=case.atm)
    rest = standard_rays()
    rest[:, 0] = 1.0
    case.geom = np.vstack([[[0.0, 700.0, 0.0, 0.0, 0.0, 0.0, 0.5], [0.0, 700.0, 0.0, 0.0, 9.9, 0.0, 0.0]], rest])
    return case


def generated_profiles(tmp_dir, emitters):
    """atm.tab of this tree's `climatology` tool for the emitters named (as test_eight_emitters_with_generated_profiles)."""
    text = "NG = %d\n" % len(emitters) + "".join("EMITTER[%d] = %s\n" % (i, e) for i, e in enumerate(emitters)) \
        + "ND = 2\nNU[0] = 792.0\nNU[1] = 832.0\n"
    with open(os.path.join(tmp_dir, "x.ctl"), "w") as fh:
        fh.write(text)
    exe = os.path.join(common.ROOT, "jurassic-gpu_amd", "climatology")
    assert subprocess.run([exe, "x.ctl", "atm.tab"], cwd=tmp_dir, capture_output=True, timeout=60).returncode == 0
    return os.path.join(tmp_dir, "atm.tab")


def _scene(name):
    case = common.limb_case()
    common.extinction_profile(case.atm)                     # on the base profile: synth.scene regrids k from it
    case.atm, case.geom, _ = synth.scene(name, case.ctl, case.atm)
    return case


def _limb(nprofiles=1, **kw):
    case = common.limb_case(geom=standard_rays(nprofiles), nprofiles=1, **kw)
    common.extinction_profile(case.atm)                     # before the profile is stacked: every copy carries it
    if nprofiles > 1:
        case.atm = synth.stack_profiles(case.atm, case.ctl, nprofiles, seed=7)
    return case


def _small(emitters, nu, atm_file, **kw):
    """The standard rays on a profile file, with the smallest tables that are looked up: the tracer reads none."""
    case = common.Case(emitters, nu, atm_file, standard_rays(), table_kw=dict(nlev=2, ntemp=2), **kw)
    common.extinction_profile(case.atm)
    return case


def _eight_without_h2o(tmp_dir):
    emitters = [e for e in EMITTERS8 if e != "H2O"]          # more gases than lanes in the quad; no q_H2O row
    return _small(emitters, [792.0, 832.0], generated_profiles(tmp_dir, emitters))


LIMB_ATM = os.path.join(common.GOLD, "limb", "atm.tab")
NADIR_ATM = os.path.join(common.GOLD, "nadir", "atm.tab")

# name -> builder(tmp_dir) of a case (ctl, atm, geom; tables unused), always with common.extinction_profile
CONFIGS = {
    "limb_x3": lambda d: _limb(3),                                         # three profiles, rays dealt to them in turn
    "ragged": lambda d: _scene("ragged"),                                  # descending slices, a 2-level profile
    "unsorted": lambda d: _scene("unsorted"),                              # atm_sorted = 0: plain lip, no hints
    "lone_up": lambda d: _scene("lone_up"),                                # one-point profiles join their neighbours
    "thin_slice": lambda d: thin_slice_case(),                             # np = 1
    "refrac0": lambda d: _limb(refrac=0),
    "coarse_steps": lambda d: _limb(rayds=20.0, raydz=1.0),
    "no_emitter": lambda d: _small([], [792.0, 832.0], LIMB_ATM),          # ng = 0
    "one_emitter_nadir": lambda d: _small(common.NADIR_EMITTERS, common.NADIR_NU, NADIR_ATM, write_bbt=1),   # ng = 1
    "eight_without_h2o": _eight_without_h2o,
}


def _nudged(geom7, direction):
    g = np.array(geom7, dtype=np.float64)
    g[1:] = np.nextafter(g[1:], direction * np.inf)
    return g


def h2o_index(ctl):
    """The emitter whose mixing ratio the tracer stores as q_H2O (only with the H2O continuum on), or -1."""
    names = [ctl.emitter[g].value.decode() for g in range(ctl.ng)]
    return names.index("H2O") if ctl.ctm_h2o and "H2O" in names else -1


def rows_of(ctl, rec):
    """The compared rows of one ray's record, oracle.traceray's or the hook's: field -> (rows, np) array."""
    ih = h2o_index(ctl)
    q = np.asarray(rec["q"])[ih:ih + 1] if ih >= 0 else np.zeros((0, len(rec["p"])))
    return {"p": np.asarray(rec["p"])[None], "t": np.asarray(rec["t"])[None], "ds": np.asarray(rec["ds"])[None],
            "k": np.asarray(rec["k"])[None], "q": q, "u": np.asarray(rec["u"])}


def hook_rows(ctl, out, i, n):
    """The same rows of ray i, first n points, from Model.kat_traceray's result."""
    q = out["qh2o"][i, :n][None] if h2o_index(ctl) >= 0 else np.zeros((0, n))
    return {"p": out["p"][i, :n][None], "t": out["t"][i, :n][None], "ds": out["ds"][i, :n][None], "k": out["k"][0, i, :n][None],
            "q": q, "u": out["u"][:, i, :n]}


def scaled_deviation(ref_rows, rows):
    """Per field the largest |rows - ref_rows| over the points, each row divided by its largest |ref value|; a row that
    is zero throughout in the reference must be zero throughout: inf otherwise."""
    out = {}
    for f in FIELDS:
        a, b = ref_rows[f], rows[f]
        worst = 0.0
        for x, y in zip(a, b):
            if len(x) == 0:
                continue
            s, d = np.abs(x).max(), np.abs(y - x).max()
            worst = max(worst, (d / s) if s > 0 else (0.0 if d == 0 else np.inf))
        out[f] = worst
    return out


def yardstick(orc, case):
    """-> (list of the oracle's records per ray, per-ray mask of the rays that are compared, {field: Y_f}).  A ray
    whose LOS point count changes under the nudge is left out of the comparison (its count is still asserted)."""
    base, use = [], np.ones(len(case.geom), dtype=bool)
    Y = {f: 0.0 for f in FIELDS}
    for i, g in enumerate(case.geom):
        tr = orc.traceray(case.ctl, case.atm, g)
        base.append(tr)
        near = [orc.traceray(case.ctl, case.atm, _nudged(g, s)) for s in (+1, -1)]
        if any(t["np"] != tr["np"] for t in near):
            use[i] = False
            continue
        r0 = rows_of(case.ctl, tr)
        for t in near:
            for f, v in scaled_deviation(r0, rows_of(case.ctl, t)).items():
                Y[f] = max(Y[f], v)
    return base, use, Y


def bound(Y_f):
    return min(FACTOR * max(Y_f, 2.0 ** -52), CAP)
