"""Shared builders for the parity tests: one `Case` = control block, atmosphere,
geometry and the same synthetic tables fed to both the oracle and the library."""
import os
import numpy as np
from jurassic_hip import abi, synth, textio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

LIMB_EMITTERS = ["CO2", "H2O", "O3", "F11", "CCl4"]
LIMB_NU = [792.0, 832.0]
NADIR_EMITTERS = ["CO2"]
NADIR_NU = [667.782, 668.541, 669.811]
CTM4_NU = [792.0, 832.0, 1450.0, 2150.0]     # keeps all four continua switched on
ND3_NU = [792.0, 832.0, 1450.0]
ND7_NU = [650.0, 792.0, 832.0, 1100.0, 1450.0, 2150.0, 2450.0]   # CO2 band, the two windows, O2 and N2 continua
# Channel configurations on the limb emitters, name -> keywords of limb_case: the smallest count (1), the smallest odd
# one (3: chunks of 8 / 64 / 256 measurements straddle rays), the same in brightness temperatures, a count coprime to
# every chunk size (7) and one that exceeds a chunk of 64 (65, on small tables so that a case stays quick)
CHANNELS = {"nd1": dict(nu=[792.0]),
            "nd3": dict(nu=ND3_NU),
            "nd3bbt": dict(nu=ND3_NU, write_bbt=1),
            "nd7": dict(nu=ND7_NU),
            "nd65": dict(nu=[650.0 + 28.125 * i for i in range(65)], table_kw=dict(nlev=5, ntemp=3))}


class Case:
    def __init__(self, emitters, nu, atm_file, geom, nprofiles=1, table_kw=None, missing=(), filt=None, **ctl_kw):
        self.ctl = abi.make_ctl(emitters, nu, **ctl_kw)
        base = textio.read_atm(atm_file, self.ctl)
        self.atm = synth.stack_profiles(base, self.ctl, nprofiles, seed=7) if nprofiles > 1 else base
        self.geom = np.asarray(geom, dtype=np.float64)
        self.rows = {}
        kw = table_kw or {}
        for g, em in enumerate(emitters):
            for d, v in enumerate(nu):
                if (g, d) in missing:
                    continue
                pkw = kw(g, d) if callable(kw) else kw          # per-pair table shapes when given a function
                self.rows[(g, d)] = synth.table_rows(em, v, id_=d, **pkw)
        self.filters = [filt(v) if filt else synth.boxcar_filter(v) for v in nu]

    def oracle_tables(self, orc, reference_layout=False):
        """reference_layout: channel stride ND as in the reference's tbl_t (jurassic.h:408-411: u/eps[...][ND], channel
        index fastest) instead of the number of channels in use -- same results, the reference's memory behaviour."""
        tb = orc.Tables(self.ctl.ng, abi.ND if reference_layout else self.ctl.nd)
        for (g, d), r in self.rows.items():
            tb.feed_rows(g, d, r)
        for d, (x, f) in enumerate(self.filters):
            tb.planck_shape(d, x, f)
        return tb

    def lib_tables(self):
        from jurassic_hip import lib
        tb = lib.Tables(self.ctl.ng, self.ctl.nd)
        for (g, d), r in self.rows.items():
            tb.feed_rows(g, d, r)
        for d, (x, f) in enumerate(self.filters):
            tb.set_filter(d, x, f)
        return tb

    def write_files(self, dirname, base="tbl"):
        """ASCII tables + filter files the way the reference expects them."""
        self.ctl.tblbase = os.path.join(dirname, base).encode()
        for (g, d), r in self.rows.items():
            name = "%s_%.4f_%s.tab" % (self.ctl.tblbase.decode(), self.ctl.nu[d], self.ctl.emitter[g].value.decode())
            synth.write_table_file(name, r)
        for d, (x, f) in enumerate(self.filters):
            synth.write_filter_file("%s_%.4f.filt" % (self.ctl.tblbase.decode(), self.ctl.nu[d]), x, f)


def golden_geometry(case):
    """(nr, 7) geometry of the reference example's rad.org rows."""
    nd = {"limb": 2, "nadir": 3}[case]
    return textio.read_obs_array(os.path.join(GOLD, case, "rad.org"), nd)[:, :7]


def limb_case(geom=None, **kw):
    g = golden_geometry("limb") if geom is None else geom
    return Case(LIMB_EMITTERS, kw.pop("nu", LIMB_NU), os.path.join(GOLD, "limb", "atm.tab"), g, **kw)


def nadir_case(geom=None, **kw):
    g = golden_geometry("nadir") if geom is None else geom
    kw.setdefault("write_bbt", 1)
    return Case(NADIR_EMITTERS, NADIR_NU, os.path.join(GOLD, "nadir", "atm.tab"), g, **kw)


def tau_atol(ref_tau):
    """Absolute allowance for a path transmittance next to the relative 1e-9.  The algorithm forms a segment's
    transmittance as (1 - eps) / tau: every look-up leaves ~1e-15 of ABSOLUTE rounding in eps, i.e. ~1e-15 / tau
    relative in the path transmittance, over some hundred segments -- and the last-bit differences between the device's
    and the host's libm in the ray tracer (exp, sin, cos, asin, atan2) enter every one of them.  So the allowance grows
    as tau falls: 1.5e-13 for tau of order one, 5e-14 / tau below, at most 5e-12 (tau <= 1e-2).  What set it: two of
    6 000 random configurations reach 1.2e-12 at tau ~ 1e-4, seed 62207 of tools/fuzz_parity.py 8.1e-12 at tau = 7.6e-3
    (1.06e-9 relative) -- each with every arrangement and every arithmetic of the kernels to the same bits, radiances
    within 1e-12 (profiles/r03_fuzz_failing_seeds_debug.log); the oracle's own transmittance of such rays moves by that
    much when the view latitude changes by 1e-13 degrees."""
    t = np.maximum(np.abs(np.asarray(ref_tau, dtype=np.float64)), 1e-300)
    return 1e-13 + np.minimum(5e-14 / t, 5e-12)


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    den = np.maximum(np.abs(b), 1e-300)
    return np.abs(a - b) / den


def oracle_goldens():
    """Committed oracle results for the reference examples with the seeded synthetic tables
    (tests/golden/oracle_examples.json, written by tools/make_oracle_goldens.py): name -> (case, dict of arrays)."""
    import json
    doc = json.load(open(os.path.join(GOLD, "oracle_examples.json")))
    cases = {"limb": limb_case(), "nadir": nadir_case(), "limb_four_continua": limb_case(nu=CTM4_NU)}
    out = {}
    for name, g in doc["cases"].items():
        arr = {k: np.array([[float.fromhex(v) for v in row] for row in g[k]]) for k in ("rad", "tau", "tp")}
        arr["np"] = np.array(g["np"], dtype=np.int32)
        out[name] = (cases[name], arr)
    return out


def random_case(seed):
    """Random small configuration: emitters, channels, table shapes (levels, temperatures, grid ratio,
    curve end), missing tables, perturbed atmosphere, mixed geometries, control switches."""
    rng = np.random.default_rng(seed)
    ng = int(rng.integers(1, 6))
    nd = int(rng.integers(1, 7))
    emitters = list(rng.permutation(LIMB_EMITTERS)[:ng])
    nu = sorted(float(x) for x in np.round(rng.uniform(650.0, 2600.0, nd), 4))
    missing = {(g, d) for g in range(ng) for d in range(nd) if rng.random() < 0.15}
    kw = dict(nlev=int(rng.integers(2, 9)), ntemp=int(rng.integers(2, 7)), ratio=float(rng.uniform(1.06, 2.2)),
              umax_eps=float(rng.choice([0.5, 0.9, 0.999, 0.99999])))
    nlimb, nnadir, nin = int(rng.integers(20, 120)), int(rng.integers(0, 60)), int(rng.integers(0, 20))
    geom = [synth.limb_geometry(nlimb, seed=seed, zmin=float(rng.uniform(-10, 10)), zmax=float(rng.uniform(20, 80)))]
    if nnadir:
        geom.append(synth.nadir_geometry(nnadir, seed=seed + 1, lat0=-40.0, lat1=40.0))
    for _ in range(nin):                               # observer inside the atmosphere, arbitrary view point
        geom.append(np.array([[0, rng.uniform(1, 80), rng.uniform(-5, 5), rng.uniform(-5, 5),
                               rng.uniform(0, 85), rng.uniform(-5, 5), rng.uniform(-5, 5)]]))
    switches = dict(refrac=int(rng.integers(0, 2)), write_bbt=int(rng.integers(0, 2)),
                    rayds=float(rng.choice([10.0, 20.0])), raydz=float(rng.choice([0.5, 1.0])),
                    ctm_co2=int(rng.integers(0, 2)), ctm_h2o=int(rng.integers(0, 2)), ctm_auto=1)
    if rng.random() < 0.3:
        switches["hydz"] = float(rng.uniform(5, 30))
    case = Case(emitters, nu, os.path.join(GOLD, "limb", "atm.tab"), np.vstack(geom),
                       nprofiles=int(rng.integers(1, 5)), table_kw=kw, missing=missing, **switches)
    n = case.atm.np                                    # reshuffle the gas columns of the shipped profile
    q = np.ctypeslib.as_array(case.atm.q)
    base = q[:5, :n].copy()
    for g, em in enumerate(emitters):
        q[g, :n] = base[LIMB_EMITTERS.index(em)] * rng.uniform(0.5, 2.0)
    np.ctypeslib.as_array(case.atm.k)[0, :n] = rng.uniform(0, 1e-4)
    case.geom[:, 0] = rng.integers(0, max(1, case.atm.np // 91), len(case.geom))   # random profile per ray
    return case


def extinction_profile(atm, k0=3e-4, h=6.0):
    """Writes an aerosol extinction that varies with altitude into window 0 of atm (in place; -> atm):
    k(z) = k0 exp(-z / h) (1 + 0.3 sin z) km^-1, z in km.  The shipped profiles carry k = 0 and every other builder a
    constant, which lip() returns from ANY bracket: only a profile like this one shows a wrong bracket, a wrong hint or
    a slip in the k row of the ray tracer.  For the scenes apply it to the base profile before synth.scene, which
    regrids k from the base."""
    n = atm.np
    z = np.ctypeslib.as_array(atm.z)[:n]
    np.ctypeslib.as_array(atm.k)[0, :n] = k0 * np.exp(-z / h) * (1.0 + 0.3 * np.sin(z))
    return atm


def obs_from_geom(geom, nd):
    obs = abi.obs_t()
    obs.nr = len(geom)
    for k, name in enumerate(("time", "obsz", "obslon", "obslat", "vpz", "vplon", "vplat")):
        np.ctypeslib.as_array(getattr(obs, name))[:len(geom)] = geom[:, k]
    np.ctypeslib.as_array(obs.rad)[:] = 7.0      # stale content the call must overwrite
    np.ctypeslib.as_array(obs.tau)[:] = 7.0
    return obs


def retrieval_case(**kw):
    case = limb_case(**kw)
    c = case.ctl
    c.retp_zmin, c.retp_zmax = 20.0, 25.0
    c.rett_zmin, c.rett_zmax = 10.0, 40.0
    for g in range(c.ng):
        c.retq_zmin[g], c.retq_zmax[g] = -999.0, -999.0
    c.retq_zmin[2], c.retq_zmax[2] = 15.0, 35.0          # O3
    c.retk_zmin[0], c.retk_zmax[0] = 10.0, 20.0
    return case
