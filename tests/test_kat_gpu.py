"""Function-level known-answer tests ON THE DEVICE (SURVEY.md section 4 "what the build must add", section 8c plan
item 2): the device functions of the hot path, evaluated one element per lane through the jur_kat_* hooks of the
C-ABI, against the oracle's restatement of the same reference function -- at the thresholds and range edges the
end-to-end parity tests only reach by chance:

  ega_eps            jr_common.h:237-268  tau around the 1e-9 gate, tau = 1, p and T below / on / above every axis
                                          end, u = 0 and u beyond both ends of a curve; all four search strategies
  continua_ctm*      jr_common.h:315-390  channels exactly on 2120 / 2605 / 1360 / 1805 / 820 / 960 / 4000 cm^-1
  src_planck_core    jr_common.h:220-224  T = 100 K, 399.99 K, grid points
  new_obs_core       jr_common.h:293-300  tau_gas around the 1e-50 gate
  add_surface_core / brightness_core      jr_common.h:187-190, 227-234
  traceray           jr_common.h:585-711  the LOS record of every point (p, T, ds, q_H2O, k, u) and tsurf, on limb scans,
                                          nadir and edge rays, paths of one to three points, ragged / unsorted scenes
                                          and every control switch of the tracer, always with an extinction that varies
                                          with altitude (tests/losrecords.py)

The look-up is plain IEEE arithmetic in the reference's operand order, so ega_eps must come back BIT-IDENTICAL in
modes 0 .. 2 (the reference's bisections; warm-started searches, descriptors from global memory / from LDS): these
are the known-answer reference on the device.  Mode 3 -- what the kernels run on strictly increasing tables since
round 3 -- replaces the reference's divisions by multiplications with stored slopes and reciprocal widths, NOT the
correctly rounded quotients (jur_kernels.hip, lip_slope / lip_mulr), and is held to the same oracle within FAST_ABS on the path transmittance, a factor 1e6 inside
the 1e-6 contract.  Functions that call exp / tanh / pow / log1p are held to a few ulp of the device math library.
"""
import os
import numpy as np
import pytest
import common
import losrecords as L
from jurassic_hip import abi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_doubles(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(bits(a)[~np.isnan(a)], bits(b)[~np.isnan(b)]) and np.array_equal(np.isnan(a), np.isnan(b))


FAST_ABS = 2e-13     # mode 3 against the oracle: |(1 - eps_t)_device - (1 - eps_t)_oracle|, both in [0, 1]


def fast_close(got, ref, tau):
    """ega_eps returns (1 - eps_t) / tau; mode 3 forms 1 - eps_t with divisions good to ~2^-46 of an interpolation
    increment.  Compared where the reference is finite, as the path transmittance it stands for."""
    got, ref, tau = (np.asarray(x, dtype=np.float64) for x in (got, ref, tau))
    fin = np.isfinite(ref)
    if not np.array_equal(fin, np.isfinite(got)):
        return False, np.inf
    err = np.abs((got[fin] - ref[fin]) * tau[fin])
    return bool(np.all(err <= FAST_ABS)), float(err.max()) if err.size else 0.0


def around(x, k=2):
    """x and its k neighbours in the doubles on either side."""
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


def ega_inputs(rows, seed, n_random=6000):
    """Edge values of every argument of ega_eps for one table, all combinations of a few of them plus random draws."""
    rng = np.random.default_rng(seed)
    plev = np.unique(rows[:, 0])
    tlev = np.unique(rows[:, 1])
    plev = np.concatenate([plev, np.repeat(plev[-1:], max(0, 6 - len(plev)))])      # tiny tables: indices below stay valid
    tlev = np.concatenate([tlev, np.repeat(tlev[-1:], max(0, 5 - len(tlev)))])
    ulo, uhi = rows[:, 2].min(), rows[:, 2].max()
    taus = around(1e-9) + [1.0, np.nextafter(1.0, 0), 1 - 1e-12, 0.999, 0.5, 1e-3, 1e-8, 3e-9, 0.0, 1e-10, 1e-300]
    ps = [plev[0] * 0.1, np.nextafter(plev[0], 0), plev[0], np.nextafter(plev[0], 1e9), plev[1], plev[len(plev) // 2],
          np.sqrt(plev[3] * plev[4]), np.nextafter(plev[-1], 0), plev[-1], np.nextafter(plev[-1], 1e9), plev[-1] * 1.2]
    ts = [100.0, tlev[0] - 1e-9, tlev[0], tlev[1], 0.5 * (tlev[2] + tlev[3]), tlev[len(tlev) // 2], tlev[-1], tlev[-1] + 1e-9,
          399.99]
    us = [0.0, ulo * 1e-6, ulo, np.sqrt(ulo * uhi), uhi, uhi * 1e6, 1e30]
    g = np.array(np.meshgrid(taus, ts, us, ps, indexing="ij")).reshape(4, -1)
    r = np.stack([10.0 ** rng.uniform(-9.3, 0, n_random), rng.uniform(150, 360, n_random),
                  10.0 ** rng.uniform(np.log10(ulo) - 3, np.log10(uhi) + 3, n_random),
                  10.0 ** rng.uniform(np.log10(plev[0]) - 1, np.log10(plev[-1]) + 0.3, n_random)])
    x = np.concatenate([g, r], axis=1)
    x = x[:, rng.permutation(x.shape[1])]        # a shuffled order: the chained evaluation jumps across the whole table
    return x[0], x[1], x[2], x[3]


def test_ega_eps_at_gates_and_axis_ends_is_bit_identical_in_every_mode(hip, oracle):
    case = common.limb_case()                                # 5 emitters x 2 channels, sorted strictly increasing tables
    m = hip.Model(case.ctl, case.lib_tables())
    ot = case.oracle_tables(oracle)
    for ig, id_ in ((0, 0), (2, 1), (4, 0)):
        tau, t, u, p = ega_inputs(case.rows[(ig, id_)], seed=10 * ig + id_)
        ref = oracle.ega_eps(ot, ig, id_, tau, t, u, p)
        assert np.all(ref[tau < 1e-9] == 0.0) and np.any(tau < 1e-9) and np.any(ref[tau >= 1e-9] > 0)     # the gate itself
        for mode in (0, 1, 2):
            got = m.kat_ega_eps(ig, id_, tau, t, u, p, mode=mode)
            bad = np.nonzero(bits(got) != bits(ref))[0]
            assert len(bad) == 0, (mode, ig, id_, len(bad), tau[bad[:3]], t[bad[:3]], u[bad[:3]], p[bad[:3]], got[bad[:3]], ref[bad[:3]])
        got3 = m.kat_ega_eps(ig, id_, tau, t, u, p, mode=3)
        ok, worst = fast_close(got3, ref, tau)
        print("mode 3 vs oracle, pair (%d, %d): worst |d(1 - eps_t)| = %.2e over %d inputs" % (ig, id_, worst, len(tau)))
        assert ok, (ig, id_, worst)
        assert np.array_equal(got3[tau < 1e-9], ref[tau < 1e-9])            # the gate answers 0 exactly in every mode
        # wavefronts whose 64 lanes all carry the same inputs fetch their bracket records through the scalar cache
        # (ld_rec2 / ld_rec_u in jur_kernels.hip), wavefronts of mixed inputs gather them: same doubles
        k = 512
        rep = [np.repeat(x[:k], 64) for x in (tau, t, u, p)]
        got_rep = m.kat_ega_eps(ig, id_, *rep, mode=3)
        assert same_doubles(got_rep.reshape(k, 64)[:, 0], got3[:k]), ("mode 3: uniform wavefront == mixed wavefront", ig, id_)
        assert same_doubles(got_rep, np.repeat(got_rep.reshape(k, 64)[:, 0], 64)), ("all lanes of a uniform wavefront agree", ig, id_)
        got_rep = m.kat_ega_eps(ig, id_, *rep, mode=3, chain=True)          # ... and resuming from the previous look-up's brackets
        assert same_doubles(got_rep.reshape(k, 64)[:, 0], got3[:k]), ("mode 3: chained uniform wavefront", ig, id_)
        # the searches resume from wherever the previous look-up ended: the result must not depend on that
        k = 4000
        for mode in (1, 2):
            got = m.kat_ega_eps(ig, id_, tau[:k], t[:k], u[:k], p[:k], mode=mode, chain=True)
            assert same_doubles(got, ref[:k]), (mode, ig, id_)
        got = m.kat_ega_eps(ig, id_, tau[:k], t[:k], u[:k], p[:k], mode=3, chain=True)
        assert same_doubles(got, got3[:k]), ("mode 3: chained == unchained, bit for bit", ig, id_)
    # NaN inputs come back as the reference's comparisons hand them through
    tau = np.array([0.5, np.nan, 0.5, 0.5, 0.5]); t = np.array([250.0, 250.0, np.nan, 250.0, 250.0])
    u = np.array([1e18, 1e18, 1e18, np.nan, 1e18]); p = np.array([100.0, 100.0, 100.0, 100.0, np.nan])
    ref = oracle.ega_eps(ot, 0, 0, tau, t, u, p)
    for mode in (0, 1, 2, 3):
        got = m.kat_ega_eps(0, 0, tau, t, u, p, mode=mode)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (mode, got, ref)
        assert got[0] == ref[0] if mode < 3 else abs(got[0] - ref[0]) * tau[0] <= FAST_ABS, (mode, got, ref)
    m.close()


@pytest.mark.parametrize("kw,modes", [(dict(table_kw=dict(dup_every=7)), (0, 1, 2)),        # sorted, not strictly: no reciprocal widths
                                      (dict(table_kw=dict(descending=True)), (0,)),          # unsorted pressure axis: bisections only
                                      (dict(table_kw=dict(nlev=2, ntemp=2)), (0, 1, 2, 3)),  # the smallest table that is looked up
                                      (dict(table_kw=dict(nlev=1)), (0, 1, 2, 3))])          # np < 2: transparent, after the tau gate
def test_ega_eps_other_table_shapes(hip, oracle, kw, modes):
    case = common.limb_case(**kw)
    m = hip.Model(case.ctl, case.lib_tables())
    ot = case.oracle_tables(oracle)
    tau, t, u, p = ega_inputs(case.rows[(1, 1)], seed=3, n_random=3000)
    ref = oracle.ega_eps(ot, 1, 1, tau, t, u, p)
    for mode in range(4):
        if mode in modes and mode < 3:
            assert same_doubles(m.kat_ega_eps(1, 1, tau, t, u, p, mode=mode), ref), mode
        elif mode in modes:
            ok, worst = fast_close(m.kat_ega_eps(1, 1, tau, t, u, p, mode=3), ref, tau)
            assert ok, (mode, worst)
        else:
            with pytest.raises(hip.JurassicError):
                m.kat_ega_eps(1, 1, tau, t, u, p, mode=mode)
    m.close()


EDGE_NU = [2120.0, 2605.0, 1360.0, 1805.0, 820.0, 960.0, 4000.0, np.nextafter(2120.0, 0), np.nextafter(2605.0, 1e9),
           np.nextafter(1360.0, 0), np.nextafter(1805.0, 1e9), np.nextafter(820.0, 1e9), np.nextafter(960.0, 0),
           np.nextafter(4000.0, 0), 1.0, 2362.5, 1582.5, 890.0, 667.782]


def test_continua_on_the_window_edges(hip, oracle):
    """Every continuum at channels exactly on / one ulp beside its window edges (jr_common.h:318, 345, 367, 381)."""
    n = 4096
    rng = np.random.default_rng(1)
    p = 10.0 ** rng.uniform(-2, 3.05, n)
    t = np.concatenate([[100.0, 399.99, 230.0, 260.0, 296.0, 273.0], rng.uniform(160, 330, n - 6)])
    q = np.concatenate([[0.0, 1.0], 10.0 ** rng.uniform(-7, -1.5, n - 2)])
    u_co2 = 10.0 ** rng.uniform(10, 24, n)
    u_h2o = 10.0 ** rng.uniform(10, 24, n)
    for lo in range(0, len(EDGE_NU), 4):                     # a few channels per model
        nus = EDGE_NU[lo:lo + 4]
        case = common.Case(["CO2", "H2O"], nus, os.path.join(common.GOLD, "limb", "atm.tab"), np.zeros((1, 7)),
                           table_kw=dict(nlev=2, ntemp=2))
        m = hip.Model(case.ctl, case.lib_tables())
        for d, nu in enumerate(nus):
            got = m.kat_continua(d, p, t, q, u_co2, u_h2o)
            ref = oracle.continua(nu, p, t, q, u_co2, u_h2o)
            inside = [0 <= nu < 4000, 0 <= nu < 20000, 2120 <= nu <= 2605, 1360 <= nu <= 1805]
            for k, name in enumerate(("co2", "h2o", "n2", "o2")):
                assert np.all(np.isfinite(got[k]))
                if not inside[k]:
                    assert np.all(got[k] == 0) and np.all(ref[k] == 0), (name, nu)
                    continue
                strictly = [0 < nu < 4000, 0 < nu < 20000, 2120 < nu < 2605, 1360 < nu < 1805]
                assert np.any(ref[k] != 0) or not strictly[k], (name, nu)    # (the N2 / O2 coefficients vanish at the edges)
                # co2 is arithmetic only (same doubles).  The others (round 3, jur_kernels.hip): exp through a 64-entry
                # table and a degree-5 polynomial (~1 ulp), the quotients by T through one shared reciprocal (~2 ulp),
                # tanh(x) as (1 - e) / (1 + e) with e = exp(-2x): relative error ~1e-16 / 2x, x = 0.7193876 nu / T --
                # 2e-15 for the infrared channels, more for the 1 cm^-1 channel this test includes on purpose
                tol = 0.0 if name == "co2" else 1e-14 if name in ("n2", "o2") else (5e-14 if nu >= 100 else 5e-13)
                err = np.abs(got[k] - ref[k]) / np.maximum(np.abs(ref[k]), 1e-300)
                assert err.max() <= tol, (name, nu, err.max())
        m.close()


def test_source_function_update_gate_surface_and_brightness(hip, oracle):
    case = common.nadir_case()                               # 3 channels, WRITE_BBT = 1
    m = hip.Model(case.ctl, case.lib_tables())
    ot = case.oracle_tables(oracle)
    rng = np.random.default_rng(2)
    gate = around(1e-50, 3) + [0.0, 1e-60, 1e-49, 1e-300, 1.0, 0.3]
    n = 3000
    # the table covers [100, 400) K; the reference's locate_st reads out of range beyond (jr_common.h:82-84): oracle
    # and device both clamp the index (end intervals extrapolate) -- held against each other just outside and far outside
    edge = [100.0, 100.25, 399.99, 399.75, 250.0, 250.125, np.nextafter(100.0, 0), 99.9, 50.0, 0.0, -10.0,
            400.0, np.nextafter(400.0, 500), 400.1, 450.0, 1000.0]
    t = np.concatenate([edge, rng.uniform(100.0, 399.99, n - len(edge))])
    tau_gas = np.concatenate([gate, 10.0 ** rng.uniform(-60, 0, n - len(gate))])
    beta = np.concatenate([[0.0, 700.0, 1e-300], 10.0 ** rng.uniform(-12, 2, n - 3)])
    rad0, tau0 = rng.uniform(0, 1e-3, n), rng.uniform(0, 1, n)
    for d in range(3):
        rad, tau, src = m.kat_update(d, 0, t, tau_gas, beta, rad0, tau0)
        rrad, rtau, rsrc = oracle.new_obs(ot, d, t, tau_gas, beta, rad0, tau0)
        assert same_doubles(src, rsrc)                                               # interpolation: same doubles
        closed = tau_gas <= 1e-50                                                    # gate shut: nothing changes
        assert np.any(closed) and np.array_equal(rad[closed], rad0[closed]) and np.array_equal(tau[closed], tau0[closed])
        assert np.array_equal(rrad[closed], rad0[closed]) and np.array_equal(rtau[closed], tau0[closed])
        # the device's exp (table + degree-5 polynomial) differs from libm's in the last place: eps = 1 - tau_gas exp(-beta)
        # moves by a few 1e-16
        assert np.all(np.abs(rad - rrad) <= 1e-15 * (np.abs(rrad) + np.abs(rsrc)))
        assert np.abs(tau - rtau).max() <= 1e-15
        # epilogue: surface term for tsurf > 0 (-999 = no ground hit), brightness temperature where asked
        tsurf = np.where(rng.uniform(size=n) < 0.5, t, -999.0)
        bbt = (rng.uniform(size=n) < 0.5).astype(np.float64)
        rad_e, _, _ = m.kat_update(d, 1, tsurf, bbt, np.zeros(n), rad0 + 1e-6, tau0)
        ref_e = oracle.epilogue(ot, d, case.ctl.nu[d], tsurf, bbt, rad0 + 1e-6, tau0)
        plain = bbt == 0
        assert same_doubles(rad_e[plain], ref_e[plain])                              # surface term: same doubles
        assert np.abs(rad_e[~plain] / ref_e[~plain] - 1).max() < 1e-14               # log1p of the device library
    m.close()


# ---------------------------------------------------------------------------------------------------------------------
# the ray tracer's LOS records, point by point

def _bit_equal_records(a, b, what):
    for key in ("p", "t", "ds", "qh2o", "k", "u", "tsurf", "tp"):
        assert same_doubles(a[key], b[key]), (what, key)
    assert np.array_equal(a["np"], b["np"]), what


@pytest.mark.parametrize("name", list(L.CONFIGS))
def test_los_records_against_the_oracle(hip, oracle, tmp_path, name):
    """What jur_trace_kernel / jur_trace_lanes_kernel write for every LOS point -- p, T, ds, q_H2O, k, u[ng] -- and
    tsurf per ray, read back through jur_kat_traceray and held to oracle.traceray, on the configurations of
    tests/losrecords.py (every one with an extinction that varies with altitude).

    Exactly: the point counts and the rays that hit the ground are the oracle's; tsurf of such a ray is the hook's own
    T of its last point, bit for bit; everything from np[ray] on is 0, and so is the q_H2O row of a model whose
    tracer never writes it; one lane per ray, a quad of lanes per ray and launches of 64 rays (two or more trace
    launches per call, the workspace slots reused) give the same doubles in every field of every point.
    Within the oracle's own conditioning (losrecords.yardstick, FACTOR, CAP): every field of every point of the rays
    whose point count a one-ulp nudge of the geometry does not change.  Y_f and the device's worst scaled deviation are
    printed per field; DESIGN.md section 2 records them.

    The fused kernel hands its LOS through LDS and cannot be read this way: it stays covered by the bit equality of its
    results with the batched kernels' (tests/test_pencil_gpu.py)."""
    case = L.CONFIGS[name](str(tmp_path))
    base, use, Y = L.yardstick(oracle, case)
    assert (~use).sum() <= 0.02 * len(use), ("rays whose point count a one-ulp nudge changes", np.nonzero(~use)[0])
    m = hip.Model(case.ctl, case.lib_tables())
    m.set_atm(case.atm)
    try:
        hip.tune_trace(1)
        one = m.kat_traceray(case.geom)
        hip.tune_trace(4)
        quad = m.kat_traceray(case.geom)
        # 64 rays per launch, and JUR_NLOS points set aside per ray (the compact layout would trace all rays in one launch)
        m.set_chunk_rays(64)
        m.set_compact_workspace(False)
        chunk4 = m.kat_traceray(case.geom)
        hip.tune_trace(1)
        chunk1 = m.kat_traceray(case.geom)
    finally:
        hip.tune_trace(0)
        m.close()
    _bit_equal_records(quad, one, "four lanes per ray == one lane per ray")
    _bit_equal_records(chunk4, one, "launches of 64 rays, four lanes == one launch")
    _bit_equal_records(chunk1, one, "launches of 64 rays, one lane == one launch")

    ctl, nr = case.ctl, len(case.geom)
    ref_np = np.array([tr["np"] for tr in base], dtype=np.int32)
    ref_tsurf = np.array([tr["tsurf"] for tr in base])
    assert one["status"] == 0 and np.array_equal(one["np"], ref_np), np.nonzero(one["np"] != ref_np)[0]
    assert np.array_equal(one["tsurf"] == -999, ref_tsurf == -999)
    assert (ref_tsurf != -999).any() and (ref_tsurf == -999).any()              # ground hits are among the rays
    worst = {f: (0.0, -1) for f in L.FIELDS}
    for i in range(nr):
        n = int(ref_np[i])
        for key in ("p", "t", "ds", "qh2o"):
            assert np.all(bits(one[key][i, n:]) == 0), (i, key, "beyond np")
        assert np.all(bits(one["k"][:, i, n:]) == 0) and np.all(bits(one["u"][:, i, n:]) == 0), (i, "beyond np")
        if L.h2o_index(ctl) < 0:
            assert np.all(bits(one["qh2o"][i]) == 0), (i, "q_H2O row of a tracer that never writes it")
        if ref_tsurf[i] != -999:
            assert bits(one["tsurf"][i:i + 1])[0] == bits(one["t"][i, n - 1:n])[0], (i, "tsurf is T of the last point")
        if n == 0:
            continue
        rows, ref_rows = L.hook_rows(ctl, one, i, n), L.rows_of(ctl, base[i])
        if not np.any(base[i]["ds"]):
            assert not np.any(rows["ds"]), (i, "a path without length")
        if use[i]:
            for f, v in L.scaled_deviation(ref_rows, rows).items():
                if v > worst[f][0]:
                    worst[f] = (v, i)
    print("LOS %s: %d rays (%d traced, %d left out), fields %s" % (name, nr, (ref_np > 0).sum(), (~use).sum(), " ".join(L.FIELDS)))
    print("LOS %s: Y_f      %s" % (name, " ".join("%.2e" % Y[f] for f in L.FIELDS)))
    print("LOS %s: device   %s" % (name, " ".join("%.2e" % worst[f][0] for f in L.FIELDS)))
    print("LOS %s: bound    %s" % (name, " ".join("%.2e" % L.bound(Y[f]) for f in L.FIELDS)))
    for f in L.FIELDS:
        v, i = worst[f]
        if v > L.bound(Y[f]):                                                  # a finding: say where
            a, b = L.rows_of(ctl, base[i])[f], L.hook_rows(ctl, one, i, int(ref_np[i]))[f]
            row, point = np.unravel_index(np.argmax(np.abs(b - a)), a.shape)
            raise AssertionError("field %s: scaled deviation %.3e above %.3e (Y = %.3e) at ray %d %s, row %d, point %d of %d: "
                                 "device %r, oracle %r" % (f, v, L.bound(Y[f]), Y[f], i, case.geom[i], row, point, ref_np[i],
                                                           b[row, point], a[row, point]))
    # the tangent point comes from the same bookkeeping: the suite's bounds (tests/test_parity_gpu.py)
    ref_tp = np.array([tr["tp"] for tr in base])
    assert np.abs(one["tp"] - ref_tp).max() < 1e-9


def test_los_records_of_a_ray_that_needs_nlos_points(hip):
    """The reported status the suite already exercises (test_nlos_overflow_is_reported, tests/sequences.py "overflow" on
    "tall"), through the hook only: the oracle ends the process on such a ray.  JUR_ENLOS, np clamped to NLOS - 1, the
    records the same doubles with one lane and with four lanes per ray."""
    case = common.limb_case(geom=synth.limb_geometry(1, scan=True, zmin=1.9, zmax=1.9))
    np.ctypeslib.as_array(case.atm.z)[:case.atm.np] *= 1.08                     # sequences.atmosphere(..., "tall")
    common.extinction_profile(case.atm)
    m = hip.Model(case.ctl, case.lib_tables())
    m.set_atm(case.atm)
    try:
        with pytest.raises(hip.JurassicError, match="Too many LOS points"):
            m.kat_traceray(case.geom)
        hip.tune_trace(1)
        one = m.kat_traceray(case.geom, overflow_ok=True)
        hip.tune_trace(4)
        quad = m.kat_traceray(case.geom, overflow_ok=True)
    finally:
        hip.tune_trace(0)
        m.close()
    assert one["status"] == quad["status"] == hip.ENLOS
    assert list(one["np"]) == [abi.NLOS - 1]
    _bit_equal_records(quad, one, "overflow: four lanes per ray == one lane per ray")
    n = abi.NLOS - 1
    assert np.all(one["p"][0, :n] > 0) and np.all(one["ds"][0, :n] > 0) and np.all(one["k"][0, 0, :n] > 0)
    assert np.all(bits(one["p"][0, n:]) == 0) and np.all(bits(one["u"][:, 0, n:]) == 0)
