"""The hydrostatic balance per slice in the scene entries (Model.set_scene_hydz): jur_scene_hydro_kernel against the host
rule, every entry against the merged entries on the atmosphere Model.scene_hydrostatic returns, the retrieval loop against
a replay on the host.

B(a) = model.scene_hydrostatic(a, time) below.  Apart from the first test (device against host arithmetic, a derived
bound) everything is bit identity: one kernel forms every balanced pressure on the device, so an entry with the switch on
must return what the merged entries return, switch off, on atmospheres balanced by the hook."""
import numpy as np
import pytest
import common
import sequences
from jurassic_hip import synth
from test_scene_jacobian_gpu import bits, formod_on, fresh_formod, scene_case, six_per_time_stamp
from test_scene_normal_gpu import bumped, copy_atm, interleaved, slice_of, sums_in_longdouble, U
from test_scene_retrieve_gpu import elements, prior_chain, rows_of, slice_mask, state_of, written_back

pytestmark = pytest.mark.gpu
HYDZ = 22.0
HYDZ_ALL = (10.0, 0.0, 35.5, 200.0)
LAMS = (1e-2, 1.0, 1e2)
SETTINGS = dict(max_iter=3, tol=0.0, lam0=1.0, fac=(0.01, 1.0, 100.0), lam_min=1e-6, lam_max=1e6)
PER_SLICE = ("lam", "cost", "prior", "nlive", "state", "iters")
HISTORY = ("h_cost", "h_prior", "h_lam", "h_tcost", "h_tprior", "h_status", "h_best", "h_accept", "h_work")
H2O, O3 = 1, 2


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def windows(c):
    """T over 10 - 40 km, p around the reference level of HYDZ alone (the 150-level profile has two more levels in it:
    elements the balance overwrites), H2O -- the gas the balance reads, ctm_h2o is on -- over 15 - 35 km, O3 over 20 - 30"""
    c.retp_zmin, c.retp_zmax = 21.3, 22.65
    c.rett_zmin, c.rett_zmax = 10.0, 40.0
    for g in range(c.ng):
        c.retq_zmin[g], c.retq_zmax[g] = -999.0, -999.0
    c.retq_zmin[H2O], c.retq_zmax[H2O] = 15.0, 35.0
    c.retq_zmin[O3], c.retq_zmax[O3] = 20.0, 30.0


def switched_on(hip, case, hydz=HYDZ):
    model = hip.Model(case.ctl, case.lib_tables())
    model.set_scene_hydz(hydz)
    model.set_atm(case.atm)
    return model


_scenes = {}


def scene(hip, name):
    """(case, geom, y, weight, lay, iq, ip), made once: six rays per time stamp, y the forward model on the balanced
    bumped atmosphere, seeded weights"""
    if name not in _scenes:
        case = scene_case(name, windows=windows)
        assert case.ctl.ctm_h2o == 1 and common.LIMB_EMITTERS[H2O] == "H2O" and common.LIMB_EMITTERS[O3] == "O3"
        geom = six_per_time_stamp(case.geom)
        on = switched_on(hip, case)
        try:
            y = fresh_formod(hip, case, on.scene_hydrostatic(bumped(case), geom[:, 0]), geom)["rad"]
        finally:
            on.close()
        assert np.all(np.isfinite(y))
        weight = 10.0 ** np.random.default_rng(11).uniform(0.0, 3.0, y.shape)
        lay = hip.scene_slices(case.ctl, case.atm, geom[:, 0])
        lay.update(hip.scene_layout(case.ctl, case.atm, geom[:, 0]))
        iq, ip = elements(hip, case, lay)
        for a in (geom, y, weight):
            a.setflags(write=False)
        _scenes[name] = (case, geom, y, weight, lay, iq, ip)
    return _scenes[name]


def p_of(atm):
    return np.ctypeslib.as_array(atm.p)[:atm.np]


def reference_points(hip, case, time, hydz=HYDZ):
    """point index of the reference parcel of every ray slice: the first minimum of |z - hydz|"""
    rs = hip.scene_ray_slices(case.ctl, case.atm, time)
    z = np.ctypeslib.as_array(case.atm.z)[:case.atm.np]
    return {int(f): int(f + np.argmin(np.abs(z[f:f + n] - hydz))) for f, n in zip(rs["sfirst"], rs["slen"])}


# ---- 1. the kernel against the host rule -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged", "short_last", "lone_up"])
def test_device_against_the_host_rule(hip, name):
    """Not the same bits: the device's exp and sin are not the libm's (1 ulp each at the most) and the host compiler may
    contract the 20-term mean (a few ulp, multiplied by an argument that sums to about 14 over a 95 km profile).  Over 150
    layers that is below about 4e2 ulp = 9e-14 relative in the linear worst case; 1e-12 leaves a factor 10."""
    case = scene_case(name, windows=windows)
    time = case.geom[:, 0]
    rs = hip.scene_ray_slices(case.ctl, case.atm, time)
    assert len(rs["sfirst"]) >= 3 and rs["slen"].max() <= 150 and (name != "ragged" or (rs["slen"].max() == 150 and rs["slen"].min() == 2))
    worst = 0.0
    for hydz in HYDZ_ALL:
        model = switched_on(hip, case, hydz)
        try:
            assert model.scene_hydz() == hydz
            dev = model.scene_hydrostatic(case.atm, time)
            again = model.scene_hydrostatic(dev, time)
        finally:
            model.close()
        host = hip.scene_hydrostatic(case.ctl, hydz, case.atm, rs["sfirst"], rs["slen"])
        n = case.atm.np
        for k in ("time", "z", "lon", "lat", "t", "q", "k"):
            bits(np.ctypeslib.as_array(getattr(dev, k))[..., :n], np.ctypeslib.as_array(getattr(case.atm, k))[..., :n], k)
        err = float(np.abs(p_of(dev) / p_of(host) - 1).max())
        worst = max(worst, err)
        print("HYDRO gpu %s hydz = %g: largest relative pressure difference device / host %.3g" % (name, hydz, err))
        assert err < 1e-12
        for f, ipref in reference_points(hip, case, time, hydz).items():
            assert p_of(dev)[ipref] == p_of(case.atm)[ipref]          # the parcel (a tie: the lower index) keeps its pressure
        moved = p_of(dev) != p_of(case.atm)
        assert moved.sum() == rs["slen"].sum() - len(rs["slen"])        # every other point of a ray slice moves, nothing else
        bits(p_of(again), p_of(dev), "balancing twice on the device")
    print("HYDRO gpu %s: maximum over hydz %.3g" % (name, worst))


# ---- 2. every entry is the merged entries on the hook's atmosphere ----------------------------------------------------------
def raised(case, atm, q, p):
    """(a copy of atm with element (q, p) raised, h): the stack kernel's rule on the value as it stands"""
    out = copy_atm(atm)
    rows = rows_of(case, out)
    x = rows[q][p]
    h = max(abs(0.01 * x), 1e-7) if q == 0 else 1.0 if q == 1 else max(abs(0.01 * x), 1e-15) if q < 2 + case.ctl.ng else 1e-4
    rows[q][p] = x + h
    return out, h


_jac = {}


def jacobian(hip, name="ragged"):
    if name not in _jac:
        case, geom, y, weight, lay, iq, ip = scene(hip, name)
        on = switched_on(hip, case)
        try:
            ks = on.kernel_scene(case.atm, geom)
            nm = on.normal_scene(case.atm, geom, y, weight, want_k=True)
            after = formod_on(on, case.geom)
            B = on.scene_hydrostatic(case.atm, geom[:, 0])
        finally:
            on.close()
        _jac[name] = (ks, nm, after, B)
    return _jac[name]


def test_forward_results_and_blocks(hip):
    case, geom, y, weight, lay, iq, ip = scene(hip, "ragged")
    ks, nm, after, B = jacobian(hip)
    nd, time = case.ctl.nd, geom[:, 0]
    ref = reference_points(hip, case, time)
    on, off = switched_on(hip, case), hip.Model(case.ctl, case.lib_tables())
    try:
        off.set_atm(B)
        base = off.formod_host(geom)
        for f in ("rad", "tau", "tp", "np"):
            bits(ks[f], base[f], "%s against formod_host on B(atm)" % f)
        sequences.same_bits(after, fresh_formod(hip, case, case.atm, case.geom), "the model holds atm, unbalanced, afterwards")
        dead, e0 = 0, 0
        for s in range(len(lay["sfirst"])):
            rays = np.flatnonzero(lay["sid"] == s)
            w = int(lay["wptr"][s + 1] - lay["wptr"][s])
            for e in range(w):
                q, p = int(iq[e0 + e]), int(ip[e0 + e])
                up, h = raised(case, B, q, p)
                off.set_atm(on.scene_hydrostatic(up, time))
                y1 = off.formod_host(geom[rays])["rad"]
                for j, r in enumerate(rays):
                    col = ks["k"][ks["rowptr"][r] * nd:ks["rowptr"][r + 1] * nd].reshape(nd, w)[:, e]
                    bits(col, (y1[j] - base["rad"][r]) / h, "slice %d element %d (quantity %d, point %d), ray %d" % (s, e, q, p, r))
                    if q == 0 and p != ref[int(lay["sfirst"][s])]:
                        assert np.all(col.view(np.uint64) == 0), "the column of a p element away from the reference parcel is +0.0"
                        dead += j == 0
            e0 += w
        assert dead >= 2 and (iq == 0).sum() > dead and (iq == 2 + H2O).any() and (iq == 2 + O3).any()
    finally:
        on.close()
        off.close()


def test_normal_equations_are_the_sums_over_those_blocks(hip):
    case, geom, y, weight, lay, iq, ip = scene(hip, "ragged")
    ks, out, _, _ = jacobian(hip)
    for f in ("k", "rad", "tau", "tp", "np", "rowptr"):
        bits(out[f], ks[f], f)
    ref = sums_in_longdouble(out, out["k"], y, weight, np.ones(y.shape, bool))
    for s in range(len(out["sfirst"])):
        A, b = slice_of(out, s)
        n = ref[s]["n"]
        assert out["nlive"][s] == n > 0
        gamma = (n + 4) * U / (1 - (n + 4) * U)                         # (the bound of test_scene_normal_gpu.py::test_against_the_blocks)
        for got, want, mag in ((A, ref[s]["A"], ref[s]["Aabs"]), (b, ref[s]["b"], ref[s]["babs"]), (out["cost"][s], ref[s]["cost"], ref[s]["cost"])):
            assert np.all(np.abs(np.asarray(got, np.longdouble) - want) <= 2 * gamma * np.asarray(mag)), s


def test_trial_step_and_diagnostics(hip):
    case, geom, y, weight, lay, iq, ip = scene(hip, "ragged")
    _, nm, _, B = jacobian(hip)
    ns, n = len(lay["sfirst"]), len(iq)
    r = 10.0 ** np.random.default_rng(3).uniform(-3.0, -1.0, n) * np.repeat([np.diag(slice_of(nm, s)[0]).mean() for s in range(ns)], np.diff(lay["wptr"]))
    on = switched_on(hip, case)
    try:
        step = on.step_scene(case.atm, geom, y, weight, LAMS, want_normal=True)
        for f in ("A", "b", "cost", "nlive", "rad"):
            bits(step[f], nm[f], "%s of step_scene against normal_scene" % f)
        half = on.solve_slices(nm["wptr"], nm["A"], nm["b"], LAMS)
        for f in ("dx", "pred", "status"):
            bits(step[f], half[f], "%s against solve_slices" % f)
        assert np.all(step["status"] == 0) and np.any(step["dx"] != 0)
        full = on.diagnose_scene(case.atm, geom, y, weight, prior_ivar=r, want_S=True, want_avk=True)
        dh = on.diagnose_slices(nm["wptr"], nm["A"], prior_ivar=r, want_S=True, want_avk=True)
        for f in ("sigma", "sigma_noise", "sigma_smooth", "avk_diag", "dofs", "status", "S", "avk"):
            bits(full[f], dh[f], "%s against diagnose_slices" % f)
        bits(full["cost"], nm["cost"], "cost of diagnose_scene")
        trial = on.trial_scene(case.atm, geom, y, weight, step["dx"])
        sequences.same_bits(formod_on(on, case.geom), fresh_formod(hip, case, case.atm, case.geom), "the model holds atm afterwards")
        for t in range(len(LAMS)):
            back = on.scene_hydrostatic(written_back(case, B, iq, ip, step["dx"][t]), geom[:, 0])
            bits(trial["cost"][t], on.normal_scene(back, geom, y, weight)["cost"], "trial %d against normal_scene on B(written back)" % t)
    finally:
        on.close()


# ---- 3. the loop -------------------------------------------------------------------------------------------------------
def replay(hip, on, name, prior):
    """test_scene_retrieve_gpu.py's replay with the balance: the state is B(atm), step_scene and normal_scene run with the
    switch on, and what is written back is balanced before it becomes the state"""
    case, geom, y, weight, lay, iq, ip = scene(hip, name)
    s_ = SETTINGS
    ns, fac = len(lay["sfirst"]), np.array(s_["fac"])
    nlam, mi, wptr, sid, time = len(fac), s_["max_iter"], lay["wptr"], lay["sid"], geom[:, 0]
    r, xa = prior
    atm = on.scene_hydrostatic(case.atm, time)
    lam, state, iters = np.full(ns, s_["lam0"]), np.zeros(ns, dtype=np.int32), np.zeros(ns, dtype=np.int32)
    cost, pri, nlive = np.zeros(ns), np.zeros(ns), np.zeros(ns, dtype=np.int64)
    h = dict(h_cost=np.zeros((mi, ns)), h_prior=np.zeros((mi, ns)), h_lam=np.full((mi, nlam, ns), np.nan),
             h_tcost=np.full((mi, nlam, ns), np.nan), h_tprior=np.full((mi, nlam, ns), np.nan),
             h_status=np.full((mi, nlam, ns), -1, dtype=np.int32), h_best=np.full((mi, ns), -1, dtype=np.int32),
             h_accept=np.full((mi, ns), -1, dtype=np.int32), h_work=np.zeros((mi, 2), dtype=np.int64))
    for it in range(mi):
        active = state == hip.RET_ACTIVE
        if not active.any():
            h["h_cost"][it], h["h_prior"][it] = cost, pri
            continue
        rays = (sid >= 0) & active[np.maximum(sid, 0)]
        sub = hip.scene_slices(case.ctl, atm, geom[rays][:, 0])
        full_of = [int(np.flatnonzero((lay["sfirst"] == f) & (lay["slen"] == l))[0]) for f, l in zip(sub["sfirst"], sub["slen"])]
        els = np.concatenate([np.arange(wptr[s], wptr[s + 1]) for s in full_of])
        x = state_of(case, atm, iq, ip)
        lamt = np.minimum(np.maximum(lam[None, :] * fac[:, None], s_["lam_min"]), s_["lam_max"])
        step = on.step_scene(atm, geom[rays], y[rays], weight[rays], lamt[:, full_of], prior_ivar=r[els], prior_dx=(xa - x)[els])
        dx = np.zeros((nlam, len(x)))
        dx[:, els] = step["dx"]
        tcost, tpri, status = np.zeros((nlam, ns)), np.zeros((nlam, ns)), np.zeros((nlam, ns), dtype=np.int32)
        status[:, full_of] = step["status"]
        for l in range(nlam):
            trial = on.scene_hydrostatic(written_back(case, atm, iq, ip, dx[l]), time)
            tcost[l, full_of] = on.normal_scene(trial, geom[rays], y[rays], weight[rays])["cost"]
        for j, s in enumerate(full_of):
            sl = slice(wptr[s], wptr[s + 1])
            cost[s], nlive[s], iters[s] = step["cost"][j], step["nlive"][j], iters[s] + 1
            pri[s] = prior_chain(r[sl], xa[sl], x[sl])
            for l in range(nlam):
                tpri[l, s] = prior_chain(r[sl], xa[sl], x[sl], dx[l][sl])
        h["h_cost"][it], h["h_prior"][it] = cost, pri
        for f, v in (("h_lam", lamt), ("h_tcost", tcost), ("h_tprior", tpri), ("h_status", status)):
            h[f][it][:, active] = v[:, active]
        h["h_work"][it] = (np.diff(lay["rowptr"])[rays] + 1).sum(), nlam * rays.sum()
        d = hip.retrieve_decide(cost + pri, tcost + tpri, lamt, status, lam, state, s_["tol"], s_["lam_max"], fac.max())
        lam, state = d["lam"], d["state"]
        h["h_best"][it], h["h_accept"][it] = d["best"], d["accept"]
        for s in np.flatnonzero(d["accept"] == 1):
            b = d["best"][s]
            atm = written_back(case, atm, iq, ip, dx[b], only=slice_mask(lay, s))
            cost[s], pri[s] = tcost[b, s], tpri[b, s]
        atm = on.scene_hydrostatic(atm, time)
    state[state == hip.RET_ACTIVE] = hip.RET_MAXITER
    return dict(h, x=state_of(case, atm, iq, ip), atm=atm, lam=lam, cost=cost.copy(), prior=pri.copy(), nlive=nlive, state=state, iters=iters)


def diagonal_prior(hip, name):
    case, geom, y, weight, lay, iq, ip = scene(hip, name)
    on = switched_on(hip, case)
    try:
        nm = on.normal_scene(case.atm, geom, y, weight)
        x0 = state_of(case, on.scene_hydrostatic(case.atm, geom[:, 0]), iq, ip)
    finally:
        on.close()
    rng = np.random.default_rng(3)
    r = np.concatenate([10.0 ** rng.uniform(-3.0, -1.0, len(b)) * np.diag(A).mean() for A, b in (slice_of(nm, s) for s in range(len(lay["sfirst"])))])
    return r, x0 + 1e-3 * np.random.default_rng(5).standard_normal(len(x0))


def retrieve(model, hip, name, prior, **kw):
    case, geom, y, weight, lay, iq, ip = scene(hip, name)
    s = dict(SETTINGS)
    g = kw.pop("geom", geom)
    return model.retrieve_scene(case.atm, g, kw.pop("y", y), kw.pop("weight", weight), s.pop("max_iter"), s.pop("fac"), mode=kw.pop("mode", 0),
                                history=True, prior_ivar=prior[0], prior_xa=prior[1], **s, **kw)


@pytest.mark.parametrize("name", ["ragged", "short_last"])
def test_the_loop_against_a_replay_on_the_host(hip, name):
    case, geom, y, weight, lay, iq, ip = scene(hip, name)
    prior = diagonal_prior(hip, name)
    on = switched_on(hip, case)
    try:
        got = retrieve(on, hip, name, prior)
        after = formod_on(on, geom)
        again = retrieve(on, hip, name, prior, max_rays_per_pass=257)
        want = replay(hip, on, name, prior)
        if name == "ragged":                                            # the rays of two slices alone: the other profiles lie in no ray slice
            rays, n2 = (lay["sid"] == 0) | (lay["sid"] == 1), int(lay["wptr"][2])
            part = on.retrieve_scene(case.atm, geom[rays], y[rays], weight[rays], 1, SETTINGS["fac"], prior_ivar=prior[0][:n2], prior_xa=prior[1][:n2])
            away = np.ones(case.atm.np, dtype=bool)
            for s in (0, 1):
                away[lay["sfirst"][s]:lay["sfirst"][s] + lay["slen"][s]] = False
            assert away.any() and np.any(p_of(part["atm"])[~away] != p_of(case.atm)[~away])
            bits(p_of(part["atm"])[away], p_of(case.atm)[away], "atm_ret.p at the points in no ray slice")
    finally:
        on.close()
    for f in HISTORY + ("x",) + PER_SLICE:
        bits(got[f], want[f], f)
        bits(again[f], got[f], "%s with passes of 257" % f)
    assert np.all(got["h_status"][0] == 0) and np.any(got["h_accept"] == 1)
    bits(state_of(case, got["atm"], iq, ip), got["x"], "atm_ret holds x")
    bits(p_of(got["atm"]), p_of(want["atm"]), "atm_ret.p is B of the written-back state")
    inside = np.zeros(case.atm.np, dtype=bool)
    rs = hip.scene_ray_slices(case.ctl, case.atm, geom[:, 0])
    for f, l in zip(rs["sfirst"], rs["slen"]):
        inside[f:f + l] = True
    bits(p_of(got["atm"])[~inside], p_of(case.atm)[~inside], "atm_ret.p outside the ray slices")
    assert np.any(p_of(got["atm"])[inside] != p_of(case.atm)[inside])
    for f in ("rad", "tau", "tp", "np"):
        bits(got[f], after[f], "%s against formod_host on the model afterwards" % f)
    fresh = fresh_formod(hip, case, got["atm"], geom)
    for f in ("rad", "tau", "tp", "np"):
        bits(got[f], fresh[f], "%s against a fresh model on atm_ret" % f)


# ---- 4. independence and the off-state -------------------------------------------------------------------------------------
def test_passes_and_ray_order(hip):
    case, geom, y, weight, lay, iq, ip = scene(hip, "ragged")
    ks, nm, _, _ = jacobian(hip)
    assert 257 < ks["rowptr"][-1] + len(geom)
    on = switched_on(hip, case)
    try:
        other = on.normal_scene(case.atm, geom, y, weight, max_rays_per_pass=257, want_k=True)
        for f in ("A", "b", "cost", "nlive", "k", "rad", "tau", "tp", "np"):
            bits(other[f], nm[f], "%s with passes of 257" % f)
        perm = interleaved(nm["sid"])
        assert not np.array_equal(perm, np.arange(len(perm)))
        other = on.normal_scene(case.atm, geom[perm], y[perm], weight[perm], max_rays_per_pass=257)
        for f in ("rad", "tau", "tp", "np"):
            bits(other[f], nm[f][perm], "%s interleaved" % f)
        where = {(int(a), int(b)): s for s, (a, b) in enumerate(zip(other["sfirst"], other["slen"]))}
        for s, key in enumerate(zip(nm["sfirst"], nm["slen"])):
            p = where[(int(key[0]), int(key[1]))]
            for got, want, f in zip(slice_of(other, p), slice_of(nm, s), ("A", "b")):
                bits(got, want, "%s of slice %d interleaved" % (f, s))
            bits(other["cost"][p:p + 1], nm["cost"][s:s + 1], "cost interleaved")
    finally:
        on.close()


def test_beside_a_field_of_view(hip):
    import test_scene_fov_gpu as F
    case = scene_case("ragged", windows=windows)
    geom = F.scan_geometry(case)
    on, off = switched_on(hip, case), hip.Model(case.ctl, case.lib_tables())
    try:
        B = on.scene_hydrostatic(case.atm, geom[:, 0])
        on.set_fov(F.DZ, F.W)
        out = on.kernel_scene(case.atm, geom)
        base = F.convolved(hip, case, B, geom, model=off)
        bits(out["rad"], base["rad"], "rad against formod_host on B(atm) + fov_apply")
        bits(out["tau"], base["tau"], "tau against formod_host on B(atm) + fov_apply")
        lay = hip.scene_slices(case.ctl, case.atm, geom[:, 0])
        iq, ip = elements(hip, case, lay)
        e = int(np.flatnonzero(iq == 1)[3])                            # one T element of the first slice, raised and balanced again
        assert e < lay["wptr"][1]
        up, h = raised(case, B, 1, int(ip[e]))
        y1 = F.convolved(hip, case, on.scene_hydrostatic(up, geom[:, 0]), geom, model=off)["rad"]
        nd, w = case.ctl.nd, int(lay["wptr"][1])
        for r in np.flatnonzero(lay["sid"] == 0):
            col = out["k"][out["rowptr"][r] * nd:out["rowptr"][r + 1] * nd].reshape(nd, w)[:, e]
            bits(col, (y1[r] - base["rad"][r]) / h, "the quotient of convolved radiances, ray %d" % r)
        other = on.kernel_scene(case.atm, geom, max_rays_per_pass=257)
        for f in ("k", "rad", "tau"):
            bits(other[f], out[f], "%s with passes of 257" % f)
    finally:
        on.close()
        off.close()


def test_beside_a_full_prior_precision(hip):
    case, geom, y, weight, lay, iq, ip = scene(hip, "short_last")
    _, nm, _, _ = jacobian(hip, "short_last")
    rng = np.random.default_rng(9)
    R = []
    for s in range(len(lay["sfirst"])):
        w = int(lay["wptr"][s + 1] - lay["wptr"][s])
        G = rng.standard_normal((w, w))
        R.append((G @ G.T / w * np.diag(slice_of(nm, s)[0]).mean() * 1e-2).ravel())
    R = np.concatenate(R)
    n = len(iq)
    on = switched_on(hip, case)
    try:
        on.set_prior_precision(lay["wptr"], R)
        step = on.step_scene(case.atm, geom, y, weight, LAMS, prior_ivar=np.zeros(n), prior_dx=np.full(n, 1e-3), want_normal=True)
        for f in ("A", "b", "cost"):
            bits(step[f], nm[f], f)
        half = on.solve_slices(nm["wptr"], nm["A"], nm["b"], LAMS, prior_ivar=np.zeros(n), prior_dx=np.full(n, 1e-3))
        for f in ("dx", "pred", "status"):
            bits(step[f], half[f], "%s against solve_slices under the full prior" % f)
        assert np.all(step["status"] == 0)
        on.set_prior_precision(None)
        plain = on.step_scene(case.atm, geom, y, weight, LAMS)
        assert not np.array_equal(plain["dx"], step["dx"])
    finally:
        on.close()


def six_entries(hip, model, name, prior):
    case, geom, y, weight, lay, iq, ip = scene(hip, name)
    n = len(iq)
    out = [model.kernel_scene(case.atm, geom), model.normal_scene(case.atm, geom, y, weight),
           model.step_scene(case.atm, geom, y, weight, LAMS, want_normal=True)]
    out.append(model.trial_scene(case.atm, geom, y, weight, out[2]["dx"]))
    out.append({k: v for k, v in retrieve(model, hip, name, prior).items() if k != "atm"})
    out.append(model.diagnose_scene(case.atm, geom, y, weight, prior_ivar=prior[0]))
    out.append(formod_on(model, case.geom))
    assert len(out[2]["dx"][0]) == n
    return out


def test_switched_off_again_is_a_fresh_model(hip):
    name = "short_last"
    case, geom, y, weight, lay, iq, ip = scene(hip, name)
    prior = diagonal_prior(hip, name)
    fresh = hip.Model(case.ctl, case.lib_tables())
    try:
        fresh.set_atm(case.atm)
        assert fresh.scene_hydz() is None
        want = six_entries(hip, fresh, name, prior)
    finally:
        fresh.close()
    model = switched_on(hip, case)
    try:
        lit = six_entries(hip, model, name, prior)
        assert not np.array_equal(lit[0]["rad"], want[0]["rad"]) and not np.array_equal(lit[4]["x"], want[4]["x"])
        model.set_scene_hydz(None)
        assert model.scene_hydz() is None
        got = six_entries(hip, model, name, prior)
        for i, (a, b) in enumerate(zip(got, want)):
            assert a.keys() == b.keys()
            for f in a:
                if f != "rc":
                    bits(a[f], b[f], "entry %d, %s, after the switch went off" % (i, f))
        # set_atm between the settings: what was uploaded under one is uploaded again under the other
        ref = fresh_formod(hip, case, case.atm, case.geom)
        for hydz in (HYDZ, None, 10.0, -3.0):
            model.set_atm(case.atm)
            model.set_scene_hydz(hydz)
            model.set_atm(case.atm)
            sequences.same_bits(formod_on(model, case.geom), ref, "set_atm after set_scene_hydz(%r)" % hydz)
    finally:
        model.close()


# ---- 5. it matters ---------------------------------------------------------------------------------------------------------
def test_the_temperature_block_of_a_limb_ray_changes(hip):
    """a sanity floor, not a tolerance: a raised T now moves the pressures above and below it"""
    case = scene_case("ragged", windows=windows)
    spec = synth.SCENES["ragged"][0][0]
    import test_scene_fov_gpu as F
    geom = F.limb_scan(spec["time"], spec["lon"], spec["lat"], [18.0, 24.0, 30.0], 0.4)
    on = switched_on(hip, case)
    off = hip.Model(case.ctl, case.lib_tables())
    try:
        B = on.scene_hydrostatic(case.atm, geom[:, 0])
        lit = on.kernel_scene(case.atm, geom)
        off.set_atm(B)
        dark = off.kernel_scene(B, geom)                                # the same balanced atmosphere, the copies not balanced again
    finally:
        on.close()
        off.close()
    bits(lit["rad"], dark["rad"], "the same forward model")
    lay = hip.scene_slices(case.ctl, case.atm, geom[:, 0])
    iq, _ = elements(hip, case, lay)
    nd, w = case.ctl.nd, len(iq)
    T = iq == 1
    a = np.array([lit["k"][lit["rowptr"][r] * nd:lit["rowptr"][r + 1] * nd].reshape(nd, w)[:, T] for r in range(len(geom))])
    b = np.array([dark["k"][dark["rowptr"][r] * nd:dark["rowptr"][r + 1] * nd].reshape(nd, w)[:, T] for r in range(len(geom))])
    rel = float(np.abs(a - b).max() / np.abs(b).max())
    print("HYDRO T block of a limb scan: largest difference / largest entry %.3g" % rel)
    assert rel > 1e-3


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    import refcases as R
    case, geom, y, weight, lay, iq, ip = scene(hip, "short_last")
    einval = r"error %d: " % hip.EINVAL
    for name in ("ragged", "lone_ends", "lone_up", "short_last"):       # no named scene has ray slices that overlap: the
        c = scene_case(name, windows=windows)                           # refusal itself is tests/test_scene_hydro_cpu.py's
        rs = hip.scene_ray_slices(c.ctl, c.atm, c.geom[:, 0])
        owner = np.zeros(c.atm.np, dtype=int)
        for f, l in zip(rs["sfirst"], rs["slen"]):
            owner[f:f + l] += 1
        assert owner.max() == 1
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        with pytest.raises(hip.JurassicError, match=einval + r"jur_scene_hydrostatic_host: .*switched off"):
            model.scene_hydrostatic(case.atm, geom[:, 0])
        for bad in (float("nan"), float("inf"), float("-inf")):
            with pytest.raises(hip.JurassicError, match=einval + r"jur_model_set_scene_hydz: hydz is .*not finite"):
                model.set_scene_hydz(bad)
        assert model.scene_hydz() is None
        model.set_scene_hydz(HYDZ)
        with pytest.raises(hip.JurassicError, match=einval + r"jur_model_set_scene_hydz"):
            model.set_scene_hydz(float("nan"))
        assert model.scene_hydz() == HYDZ                               # what was set stays set
        sequences.same_bits(formod_on(model, case.geom), fresh_formod(hip, case, case.atm, case.geom), "after the refusals")
    finally:
        model.close()
    hcase, _ = R.jacobian_case("jacobian_hydz10")                       # ctl->hydz >= 0 is refused as before, switch on or off
    model = hip.Model(hcase.ctl, hcase.lib_tables())
    try:
        model.set_atm(hcase.atm)
        model.set_scene_hydz(HYDZ)
        with pytest.raises(hip.JurassicError, match=einval + r".*hydz = 10 >= 0"):
            model.kernel_scene(hcase.atm, hcase.geom)
    finally:
        model.close()
