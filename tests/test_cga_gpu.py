"""Curtis-Godson forward model (FORMOD 1) on the device: jur_cga_kernel behind every entry, against the CPU model of
tests/cga_model.py (whose look-up blocks tests/test_cga_cpu.py pins to the reference's ega_eps).

Bounds are the suite's own: radiances 1e-9 relative, transmittances 1e-9 relative plus common.tau_atol
(tests/test_parity_gpu.py), the strict-table arithmetic of the look-up FAST_ABS = 2e-13 on the path transmittance
(tests/test_kat_gpu.py: the bound the emissivity-growth look-up's mode 3, a superset of this arithmetic, is held to).
Every test here fails at model creation on a library that refuses FORMOD 1."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import common
import cga_model as M
import losrecords as L
from jurassic_hip import abi, synth
from test_cga_cpu import lookup_inputs, same_doubles, bits
from test_contrib_gpu import edited_atm

pytestmark = pytest.mark.gpu
RTOL = 1e-9
FAST_ABS = 2e-13
PAIRS = ((0, 0), (2, 1), (4, 0))


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def copy_atm(a):
    out = abi.atm_t()
    C.memmove(C.byref(out), C.byref(a), C.sizeof(abi.atm_t))
    return out


def model_of(hip, case, arith="fast", atm=None):
    m = hip.Model(case.ctl, case.lib_tables())
    m.set_arithmetic(hip.ARITH_EXACT if arith == "exact" else hip.ARITH_FAST)
    m.set_atm(case.atm if atm is None else atm)
    return m


def assert_parity(out, ref, what=""):
    assert np.array_equal(out["np"], ref["np"]), what
    fin = np.isfinite(ref["rad"])
    assert np.array_equal(fin, np.isfinite(out["rad"])), what
    rerr = common.rel_err(out["rad"][fin], ref["rad"][fin])
    terr = np.abs(out["tau"] - ref["tau"])
    allow = RTOL * np.abs(ref["tau"]) + common.tau_atol(ref["tau"])
    print("CGA %s: worst rel radiance error %.3e, worst |dtau| / allowance %.3e" % (what, rerr.max(), (terr / allow).max()))
    assert rerr.max() < RTOL, (what, rerr.max())
    k = np.unravel_index(np.argmax(terr - allow), terr.shape)
    assert np.all(terr <= allow), (what, k, out["tau"][k], ref["tau"][k])
    assert np.abs(out["tp"] - ref["tp"]).max() < 1e-9, what


# ---- 1. the hook ---------------------------------------------------------------------------------------------------------
def model_lookup(pair, tau, t, u, p):
    return np.array([M.cga_lookup(pair, *x) for x in zip(tau.tolist(), t.tolist(), u.tolist(), p.tolist())])


def fast_close(got, ref):
    if not np.array_equal(np.isnan(ref), np.isnan(got)):
        return False, np.inf
    fin = ~np.isnan(ref)
    err = np.abs(got[fin] - ref[fin])
    return bool(np.all(err <= FAST_ABS)), float(err.max()) if err.size else 0.0


def test_hook_at_gates_axis_ends_curve_ends_and_random_inputs(hip):
    case = common.limb_case(formod=1)
    m = hip.Model(case.ctl, case.lib_tables())
    try:
        for ig, id_ in PAIRS:
            pair = M.Pair(case.rows[(ig, id_)])
            tau, t, u, p = lookup_inputs(case.rows[(ig, id_)], seed=10 * ig + id_)
            perm = np.random.default_rng(ig).permutation(len(tau))     # the chained evaluation jumps across the whole table
            tau, t, u, p = tau[perm], t[perm], u[perm], p[perm]
            ref = model_lookup(pair, tau, t, u, p)
            gate = tau < 1e-9
            assert gate.any() and np.all(ref[gate] == 0) and np.any(u == 0) and np.any((ref > 0) & (ref < 1))
            for mode in (0, 1, 2):
                got = m.kat_cga_eps(ig, id_, tau, t, u, p, mode=mode)
                bad = np.nonzero(bits(got) != bits(ref))[0]
                assert len(bad) == 0, (mode, ig, id_, len(bad), tau[bad[:3]], t[bad[:3]], u[bad[:3]], p[bad[:3]], got[bad[:3]], ref[bad[:3]])
            got3 = m.kat_cga_eps(ig, id_, tau, t, u, p, mode=3)
            ok, worst = fast_close(got3, ref)
            print("CGA mode 3 vs CPU model, pair (%d, %d): worst |dtau| = %.2e over %d inputs" % (ig, id_, worst, len(tau)))
            assert ok, (ig, id_, worst)
            assert np.all(bits(got3[gate]) == 0)                        # the gate answers exactly 0 in every mode
            # uniform wavefronts read their records through the scalar cache, mixed ones gather: the same doubles
            k = 256
            rep = [np.repeat(x[:k], 64) for x in (tau, t, u, p)]
            got_rep = m.kat_cga_eps(ig, id_, *rep, mode=3)
            assert same_doubles(got_rep.reshape(k, 64)[:, 0], got3[:k]), ("uniform == mixed", ig, id_)
            assert same_doubles(got_rep, np.repeat(got_rep.reshape(k, 64)[:, 0], 64)), ("lanes of a uniform wavefront", ig, id_)
            # the searches resume where the previous look-up ended: the result must not depend on that
            k = 3000
            for mode in (1, 2):
                got = m.kat_cga_eps(ig, id_, tau[:k], t[:k], u[:k], p[:k], mode=mode, chain=True)
                assert same_doubles(got, ref[:k]), (mode, ig, id_)
            got = m.kat_cga_eps(ig, id_, tau[:k], t[:k], u[:k], p[:k], mode=3, chain=True)
            assert same_doubles(got, got3[:k]), ("mode 3: chained == unchained", ig, id_)
        # NaN inputs: tau is only the gate's operand (a NaN passes it and changes nothing), the others reach the result
        pair = M.Pair(case.rows[(0, 0)])
        tau = np.array([0.5, np.nan, 0.5, 0.5, 0.5]); t = np.array([250.0, 250.0, np.nan, 250.0, 250.0])
        u = np.array([1e18, 1e18, 1e18, np.nan, 1e18]); p = np.array([100.0, 100.0, 100.0, 100.0, np.nan])
        ref = model_lookup(pair, tau, t, u, p)
        assert list(np.isnan(ref)) == [False, False, True, True, True] and ref[0] == ref[1]
        for mode in (0, 1, 2, 3):
            got = m.kat_cga_eps(0, 0, tau, t, u, p, mode=mode)
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (mode, got, ref)
            assert same_doubles(got, ref) if mode < 3 else np.all(np.abs(got[:2] - ref[:2]) <= FAST_ABS), (mode, got, ref)
    finally:
        m.close()


@pytest.mark.parametrize("kw,modes", [(dict(table_kw=dict(dup_every=7)), (0, 1, 2)),
                                      (dict(table_kw=dict(descending=True)), (0,)),
                                      (dict(table_kw=dict(nlev=2, ntemp=2)), (0, 1, 2, 3)),
                                      (dict(table_kw=dict(nlev=1)), (0, 1, 2, 3))])
def test_hook_other_table_shapes(hip, kw, modes):
    case = common.limb_case(formod=1, **kw)
    m = hip.Model(case.ctl, case.lib_tables())
    try:
        tau, t, u, p = lookup_inputs(case.rows[(1, 1)], seed=3, n_random=1000)
        ref = model_lookup(M.Pair(case.rows[(1, 1)]), tau, t, u, p)
        if kw["table_kw"].get("nlev") == 1:                              # np < 2: transparent, after the gate
            assert np.array_equal(ref, np.where(tau < 1e-9, 0.0, tau))
        for mode in range(4):
            if mode in modes and mode < 3:
                assert same_doubles(m.kat_cga_eps(1, 1, tau, t, u, p, mode=mode), ref), mode
            elif mode in modes:
                ok, worst = fast_close(m.kat_cga_eps(1, 1, tau, t, u, p, mode=3), ref)
                assert ok, (mode, worst)
            else:
                with pytest.raises(hip.JurassicError):
                    m.kat_cga_eps(1, 1, tau, t, u, p, mode=mode)
    finally:
        m.close()


# ---- 2. the forward model against the CPU model --------------------------------------------------------------------------
def forward_case(name):
    if name == "limb":
        case = common.limb_case(formod=1, missing={(3, 0)})
        case.geom = case.geom[::6]
        common.extinction_profile(case.atm)
    elif name == "limb_ctm4":
        case = common.limb_case(formod=1, nu=common.CTM4_NU, missing={(3, 0)})
        case.geom = case.geom[::6]
        common.extinction_profile(case.atm)
    elif name == "nadir":
        case = common.nadir_case(formod=1)
        case.geom = case.geom[:12]
    else:
        case = common.limb_case(formod=1, geom=np.vstack([L.SHORT_PATHS, L.edge_rays()]))
        common.extinction_profile(case.atm)
    return case


_cpu = {}


def cpu_model(oracle, name):
    """(case, CPU model's result), computed once per configuration and shared by the arithmetics"""
    if name not in _cpu:
        case = forward_case(name)
        _cpu[name] = (case, M.formod(oracle, case, want_paths=True))
    return _cpu[name]


@pytest.mark.parametrize("arith", ["exact", "fast"])
@pytest.mark.parametrize("name", ["limb", "limb_ctm4", "nadir", "short_and_edge"])
def test_forward_model_against_the_cpu_model(hip, oracle, name, arith):
    case, ref = cpu_model(oracle, name)
    m = model_of(hip, case, arith)
    try:
        out = m.formod_host(case.geom)
    finally:
        m.close()
    if name == "short_and_edge":
        assert list(ref["np"][:4]) == L.SHORT_NP
    if name == "nadir":
        assert case.ctl.write_bbt == 1 and case.ctl.nd == 3
    assert np.any(ref["rad"] > 0)
    assert_parity(out, ref, "%s %s" % (name, arith))
    # the tracer is untouched: tangent points and point counts of an emissivity-growth model of the same case, bit for bit
    ega = hip.Model(M.ega_ctl(case.ctl), case.lib_tables())
    try:
        ega.set_atm(case.atm)
        ega.set_pencil(0)
        other = ega.formod_host(case.geom)
    finally:
        ega.close()
    assert np.array_equal(out["np"], other["np"]) and same_doubles(out["tp"], other["tp"])
    if name in ("limb", "limb_ctm4"):
        assert not same_doubles(out["rad"], other["rad"])               # ... and the band model is another one


# ---- 3. gates on whole rays -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_a_gas_that_goes_opaque_before_the_last_segment(hip, oracle, arith):
    g = 3                                                               # F11: no continuum goes with it
    case = common.limb_case(formod=1)
    case.geom = case.geom[[0, 2, 5, 9]]
    key = "opaque"
    if key not in _cpu:
        q = np.ctypeslib.as_array(case.atm.q)
        base = q[g].copy()
        for factor in 10.0 ** np.arange(2, 12):
            q[g] = base * factor
            ref = M.formod(oracle, case, want_paths=True)
            if all(any(x == 0.0 for x in ref["paths"][0][(g, d)][:-1]) for d in range(case.ctl.nd)):
                break
        _cpu[key] = (case, ref, factor)
    case, ref, factor = _cpu[key]
    hit = [ray[(g, d)].index(0.0) for ray in ref["paths"] for d in range(case.ctl.nd) if 0.0 in ray[(g, d)]]
    assert hit and all(ray[(g, 0)][-1] == 0.0 for ray in ref["paths"][:1])      # exactly 0, and it stays 0
    assert any(0.0 in ray[(g, d)][:-1] for ray in ref["paths"] for d in range(case.ctl.nd))
    rising = sum(int(np.sum(np.diff(ray[gd]) > 0)) for ray in ref["paths"] for gd in ray)
    total = sum(len(ray[gd]) for ray in ref["paths"] for gd in ray)
    print("CGA opaque gate: q[F11] x %g, first exact 0 after segment %d; %d of %d path transmittances rise" % (factor, min(hit), rising, total))
    m = model_of(hip, case, arith)
    try:
        out = m.formod_host(case.geom)
    finally:
        m.close()
    assert_parity(out, ref, "opaque %s" % arith)


@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_a_gas_without_any_column_is_a_gas_without_tables(hip, arith):
    g = 3
    with_tables = common.limb_case(formod=1)
    without = common.limb_case(formod=1, missing={(g, d) for d in range(2)})
    res = []
    for case in (with_tables, without):
        case.geom = case.geom[::5]
        np.ctypeslib.as_array(case.atm.q)[g] = 0.0
        m = model_of(hip, case, arith)
        try:
            res.append(m.formod_host(case.geom))
        finally:
            m.close()
    assert np.all(res[0]["rad"] > 0)
    for f in ("rad", "tau", "tp", "np"):
        assert same_doubles(res[0][f], res[1][f]), f


# ---- 4. invariance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_every_ray_has_the_same_bits_in_any_arrangement(hip, arith):
    case = common.limb_case(formod=1)
    limb = []
    for shift in (0.0, 0.13, -0.27, 0.31):
        g = case.geom.copy()
        g[:, 4] += shift
        limb.append(g)
    geom = np.vstack(limb + [synth.nadir_geometry(57, seed=5)])
    assert len(geom) == 321                                             # crosses a block of 256 slots, ends in a ragged wavefront
    perm = np.random.default_rng(8).permutation(len(geom))
    m = model_of(hip, case, arith)
    try:
        base = m.formod_host(geom)
        assert np.all(np.isfinite(base["rad"])) and np.all(base["np"] > 0)
        for chunk in (64, None):
            if chunk:
                m.set_chunk_rays(chunk)
            for sort in (True, False):
                m.set_sort_rays(sort)
                for order in (None, perm):
                    out = m.formod_host(geom if order is None else geom[order])
                    for f in ("rad", "tau", "tp", "np"):
                        want = base[f] if order is None else base[f][order]
                        assert same_doubles(out[f], want), (f, chunk, sort, order is not None)
            m.set_chunk_rays(1 << 21)
    finally:
        m.close()


# ---- 5. entries -------------------------------------------------------------------------------------------------------------
LIMB_CTL = """TBLBASE = ./boxcar
NG = 5
EMITTER[0] = CO2
EMITTER[1] = H2O
EMITTER[2] = O3
EMITTER[3] = F11
EMITTER[4] = CCl4
ND = 2
NU[0] = 792.0000
NU[1] = 832.0000
USEGPU = -1
WRITE_BINARY = 0
READ_BINARY = 0
"""


def test_drop_in_and_command_line_tool(hip, tmp_path):
    case = common.limb_case(formod=1)
    for d, nu in enumerate(common.LIMB_NU):
        case.filters[d] = tuple(np.loadtxt(os.path.join(common.GOLD, "limb", "boxcar_%.4f.filt" % nu), comments="#").T)
    case.write_files(str(tmp_path), base="boxcar")
    assert len(case.geom) == 66
    m = hip.Model(case.ctl)                                             # tables from the files
    try:
        m.set_pencil(10000, 4)                                          # accepted, without effect under FORMOD 1
        m.set_atm(case.atm)
        m.enable_timing(True)
        want = m.formod_host(case.geom)
        ms = m.kernel_ms()
    finally:
        m.close()
    assert ms["pencil_launches"] == 0 and ms["ega_launches"] >= 1 and ms["ega_ms"] > 0, ms
    hip.dropin_finalize()
    try:
        obs = common.obs_from_geom(case.geom, case.ctl.nd)
        hip.formod(case.ctl, case.atm, obs)
    finally:
        hip.dropin_finalize()
    n, nd = obs.nr, case.ctl.nd
    assert same_doubles(np.ctypeslib.as_array(obs.rad)[:n, :nd], want["rad"])
    assert same_doubles(np.ctypeslib.as_array(obs.tau)[:n, :nd], want["tau"])
    # the emissivity-growth answer is another one: the switch reached the kernels
    c2 = M.ega_ctl(case.ctl)
    ega = hip.Model(c2)
    try:
        ega.set_atm(case.atm)
        assert not same_doubles(ega.formod_host(case.geom)["rad"], want["rad"])
    finally:
        ega.close()
    (tmp_path / "limb.ctl").write_text(LIMB_CTL)
    exe = os.path.join(common.ROOT, "jurassic-gpu_amd", "formod")
    run = subprocess.run([exe, "limb.ctl", os.path.join(common.GOLD, "limb", "obs.tab"), os.path.join(common.GOLD, "limb", "atm.tab"),
                          "rad.tab", "FORMOD", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    got = [l.split() for l in open(tmp_path / "rad.tab") if l.strip() and not l.startswith("#")]
    assert len(got) == 66
    for row, rad, tau in zip(got, want["rad"], want["tau"]):
        assert row[10:14] == ["%g" % v for v in list(rad) + list(tau)], (row, rad, tau)


def test_contributions_are_the_cga_model_on_the_edited_atmospheres(hip):
    case = common.limb_case(formod=1)
    case.geom = case.geom[::3]
    common.extinction_profile(case.atm)
    m = model_of(hip, case)
    try:
        out = m.formod_contrib_host(case.geom)
        total = m.formod_host(case.geom)
        for f in ("rad", "tau", "tp", "np"):
            assert same_doubles(out[f], total[f]), f
        for v in range(case.ctl.ng):
            m.set_atm(edited_atm(case, v))
            ref = m.formod_host(case.geom)
            rerr = common.rel_err(out["rad_c"][v], ref["rad"])
            terr = np.abs(out["tau_c"][v] - ref["tau"])
            assert rerr.max() < RTOL, (v, rerr.max())
            assert np.all(terr <= RTOL * np.abs(ref["tau"]) + common.tau_atol(ref["tau"])), (v, terr.max())
            assert np.any(ref["tau"] < 0.999)
    finally:
        m.close()


def two_profile_scene():
    case = common.retrieval_case(formod=1)
    spec = [synth._spec(0.0, -60.0, 35.0, 25, 0.0, 70.0), synth._spec(1.0, 100.0, -20.0, 20, 0.0, 85.0, descending=True)]
    case.atm = synth.ragged_atmosphere(case.ctl, spec, seed=0, base=case.atm)
    case.geom = synth.global_geometry(spec, 12, seed=1)
    return case


def test_scene_blocks_equal_the_dense_jacobian(hip):
    case = two_profile_scene()
    nd = case.ctl.nd
    obs = common.obs_from_geom(case.geom, nd)
    np.ctypeslib.as_array(obs.rad)[:] = 0.0
    m = model_of(hip, case)
    try:
        k = m.kernel(case.atm, obs)
        out = m.kernel_scene(case.atm, case.geom)
    finally:
        m.close()
    assert k.shape[0] == len(case.geom) * nd
    dense = hip.scene_blocks_to_dense(case.ctl, case.atm, out, n=k.shape[1])
    inside = np.zeros(k.shape, dtype=bool)
    for r, (f, l) in enumerate(zip(out["first"], out["len"])):
        if out["rowptr"][r + 1] > out["rowptr"][r]:
            inside[r * nd:(r + 1) * nd, hip.scene_columns(case.ctl, case.atm, f, l)] = True
    assert inside.any() and not inside.all() and np.all(k[~inside] == 0)
    assert same_doubles(dense[inside], k[inside])
    assert (np.abs(k).max(axis=0) > 0).sum() >= 20
    n = obs.nr
    assert same_doubles(out["rad"], np.ctypeslib.as_array(obs.rad)[:n, :nd])
    assert same_doubles(out["tau"], np.ctypeslib.as_array(obs.tau)[:n, :nd])


def test_jacobian_columns_are_quotients_of_two_forward_models(hip):
    """T, one gas, extinction: jur_kernel's column against (F(x + h e) - F(x)) / h from two jur_formod_host calls with
    the step jur_kernel uses (jurassic.c:831-837); bound as tests/test_scene_jacobian_gpu.py: 1e-6 of the column's
    largest entry."""
    case = common.retrieval_case(formod=1)
    common.extinction_profile(case.atm)
    nd, natm = case.ctl.nd, case.atm.np
    obs = common.obs_from_geom(case.geom, nd)
    np.ctypeslib.as_array(obs.rad)[:] = 0.0
    m = model_of(hip, case)
    try:
        k = m.kernel(case.atm, obs)
        el = hip.scene_elements(case.ctl, case.atm, 0, natm)
        iq, ip = np.asarray(el["iq"]), np.asarray(el["ip"])
        assert k.shape == (len(case.geom) * nd, len(iq))
        m.set_atm(case.atm)
        y0 = m.formod_host(case.geom)["rad"]
        ng = case.ctl.ng
        for quantity in (1, 2 + 2, 2 + ng):                             # T, O3, extinction of window 0
            among = np.flatnonzero(iq == quantity)
            e = int(among[len(among) // 2])
            col = int(el["cols"][e])
            atm = copy_atm(case.atm)
            row = (np.ctypeslib.as_array(atm.t) if quantity == 1 else
                   np.ctypeslib.as_array(atm.q)[2] if quantity < 2 + ng else np.ctypeslib.as_array(atm.k)[0])
            x0 = float(row[ip[e]])
            h = 1.0 if quantity == 1 else max(abs(0.01 * x0), 1e-15) if quantity < 2 + ng else 1e-4
            row[ip[e]] = x0 + h
            m.set_atm(atm)
            y1 = m.formod_host(case.geom)["rad"]
            quot = ((y1 - y0) / h).ravel()
            scale = np.abs(quot).max()
            assert scale > 0, quantity
            worst = np.abs(k[:, col] - quot).max() / scale
            print("CGA Jacobian column %d (quantity %d): %.3e of the column's largest entry" % (col, quantity, worst))
            assert worst < 1e-6, (quantity, col, worst)
    finally:
        m.close()


def test_one_retrieval_of_the_smallest_case(hip):
    from test_scene_jacobian_gpu import scene_case, six_per_time_stamp
    from test_scene_normal_gpu import bumped
    case = scene_case("short_last")
    case.ctl.formod = 1
    geom = six_per_time_stamp(case.geom)
    m = model_of(hip, case, atm=bumped(case))
    try:
        y = m.formod_host(geom)["rad"]
        assert np.all(np.isfinite(y))
        weight = 10.0 ** np.random.default_rng(11).uniform(0.0, 3.0, y.shape)
        m.set_atm(case.atm)
        out = m.retrieve_scene(case.atm, geom, y, weight, 2, (0.1, 10.0), history=True)
    finally:
        m.close()
    start = out["h_cost"][0]
    print("CGA retrieval: cost per slice %s -> %s" % (start, out["cost"]))
    assert np.all(np.isfinite(out["cost"])) and np.all(out["cost"] <= start) and np.any(out["cost"] < start)
