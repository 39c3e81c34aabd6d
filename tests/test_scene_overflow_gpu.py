"""Model.set_scene_overflow(OVERFLOW_ISOLATE): a ray that needs NLOS points or more makes its trial's cost NaN (a rejected
step) or ends its own slice as RET_FAILED; it no longer ends trial_scene or retrieve_scene for every slice.

The scene is `ragged` cut down: three slices (time stamps 0.5, 2.75 and 1.25 -- the 150-level profile), a scan of four
limb rays each, T retrieved on the levels up to 12 km (17 elements in the widest slice), two channels (once three).  In
the 150-level profile the oracle's tracer, run in child processes on the CPU since it ends the process on such a ray,
counts for a limb ray with tangent height h, on the first guess | with T * 0.6 on the retrieved levels:
  5.0 km: 400 or more | 400 or more;   6.33 km: 395 | 400 or more;   8 km: 388 | 394;   10 km: 378 | 383;   12 km: 369 | 374
(T * 0.8 leaves the 6.33 km ray at 398, T * 1.01 and the +2 K bump of the measurements at 395; the rays of the other two
profiles need 239 .. 348).  The tests assert the counts they rely on through kat_traceray on the device's own tracer.
Everything is compared bit for bit."""
import numpy as np
import pytest
import sequences
from jurassic_hip import abi
from test_scene_fov_gpu import DZ, W, limb_scan
from test_scene_jacobian_gpu import bits, formod_on, fresh_formod, scene_case
from test_scene_normal_gpu import bumped, copy_atm, inputs
from test_scene_retrieve_gpu import REPLAY, elements, layout, prior_chain, same_atm, seeded_prior, slice_mask, state_of, written_back
from test_scene_retrieve_gpu import SCENES as RETRIEVE_SCENES
from test_scene_solve_gpu import STEP_LAMS

pytestmark = pytest.mark.gpu
EDGE, LONG = 6.33, 5.0
FAC = (0.1, 1.0, 10.0)
SETTINGS = dict(max_iter=3, tol=0.0, lam0=1.0, fac=FAC, lam_min=1e-6, lam_max=1e6)
PER_SLICE = ("lam", "cost", "prior", "nlive", "state", "iters")
HISTORY = ("h_cost", "h_prior", "h_lam", "h_tcost", "h_tprior", "h_status", "h_best", "h_accept")
TOO_MANY = r"error %d: Too many LOS points"


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def windows(c):
    """T alone, on the levels up to 12 km"""
    c.retp_zmin, c.retp_zmax = -999.0, -999.0
    c.rett_zmin, c.rett_zmax = 0.0, 12.0
    for g in range(c.ng):
        c.retq_zmin[g], c.retq_zmax[g] = -999.0, -999.0
    for w in range(c.nw):
        c.retk_zmin[w], c.retk_zmax[w] = -999.0, -999.0


def scans(lowest):
    """two slices that never overflow, then the scan through the 150-level profile whose lowest ray is `lowest`"""
    return np.vstack([limb_scan(0.5, 10.0, 45.0, [4.0, 6.0, 8.0, 10.0], 0.3),
                      limb_scan(2.75, 45.0, 89.99, [4.0, 6.0, 8.0, 10.0], 0.3),
                      limb_scan(1.25, -180.0, -30.0, [lowest, 8.0, 10.0, 12.0], 0.7)])


_scenes = {}


def scene(hip, lowest, name="ragged"):
    """(case, geom, y, weight, lay, iq, ip, x0): y the forward model on the bumped atmosphere for the rays that can be
    traced there, the first guess's own radiance (never read: the slice fails first) for the one that cannot"""
    key = (lowest, name)
    if key not in _scenes:
        case = scene_case(name, windows=windows)
        geom = scans(lowest)
        lay = hip.scene_slices(case.ctl, case.atm, geom[:, 0])
        lay.update(hip.scene_layout(case.ctl, case.atm, geom[:, 0]))
        assert len(lay["sfirst"]) == 3 and list(lay["sid"]) == [0] * 4 + [1] * 4 + [2] * 4
        assert 4 <= np.diff(lay["wptr"]).min() and np.diff(lay["wptr"]).max() <= 20
        iq, ip = elements(hip, case, lay)
        fits = np.ones(len(geom), dtype=bool)
        fits[8] = lowest != LONG
        y = np.ones((len(geom), case.ctl.nd))
        y[fits] = fresh_formod(hip, case, bumped(case), geom[fits])["rad"]
        assert np.all(np.isfinite(y))
        weight = 10.0 ** np.random.default_rng(11).uniform(0.0, 3.0, y.shape)
        for a in (geom, y, weight):
            a.setflags(write=False)
        _scenes[key] = (case, geom, y, weight, lay, iq, ip, state_of(case, case.atm, iq, ip))
    return _scenes[key]


def counts(hip, model, atm, geom):
    """LOS points of the rays on atm by the device's tracer; the model is left holding atm"""
    model.set_atm(atm)
    return model.kat_traceray(geom, overflow_ok=True)["np"]


def overflows(hip, npts):
    return np.array([hip.np_overflows(n) for n in npts])


def trial_steps(lay, x0):
    """three trials: +0.5 K, the large one (T * 0.6 in slice 2, -0.5 K elsewhere), -0.5 K"""
    big = slice_mask(lay, 2)
    dx = np.vstack([np.full(len(x0), 0.5), np.where(big, -0.4 * x0, -0.5), np.full(len(x0), -0.5)])
    zeroed = dx.copy()
    zeroed[1, big] = 0.0
    return dx, zeroed, big


# ---- 1. a trial that overflows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged", "ragged@nd3"])
def test_a_trial_that_overflows_costs_nan_and_nothing_else_moves(hip, name):
    case, geom, y, weight, lay, iq, ip, x0 = scene(hip, EDGE, name)
    dx, zeroed, big = trial_steps(lay, x0)
    r = np.full(len(x0), 1e-2)
    xa = x0 + 0.25
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        # the preconditions, on the device's tracer: first guess and small trials fit, the large one does not, in slice 2 alone
        assert not overflows(hip, counts(hip, model, case.atm, geom)).any()
        for t in range(3):
            over = overflows(hip, counts(hip, model, written_back(case, case.atm, iq, ip, dx[t]), geom))
            assert list(np.flatnonzero(over)) == ([8] if t == 1 else []), (t, over)
        model.set_atm(case.atm)
        assert model.scene_overflow() == hip.OVERFLOW_ERROR
        with pytest.raises(hip.JurassicError, match=TOO_MANY % hip.ENLOS):
            model.trial_scene(case.atm, geom, y, weight, dx, prior_ivar=r, prior_xa=xa)
        assert model.last_scene_overflow() == (0, 0)
        want = model.trial_scene(case.atm, geom, y, weight, zeroed, prior_ivar=r, prior_xa=xa)
        assert np.all(np.isfinite(want["cost"])) and model.last_scene_overflow() == (0, 0)
        model.set_scene_overflow(hip.OVERFLOW_ISOLATE)
        for cap in (0, 1, 5):
            got = model.trial_scene(case.atm, geom, y, weight, dx, prior_ivar=r, prior_xa=xa, max_rays_per_pass=cap)
            assert model.last_scene_overflow() == (1, 0)
            cell = np.zeros((3, 3), dtype=bool)
            cell[1, 2] = True
            assert np.array_equal(np.isnan(got["cost"]), cell), "exactly that one cost is NaN"
            bits(got["cost"][~cell], want["cost"][~cell], "every other cost, passes of %d" % cap)
            bits(got["prior"][~cell], want["prior"][~cell], "every other prior term")
            bits(got["prior"][1, 2], prior_chain(r[big], xa[big], x0[big], dx[1][big]), "the prior term of the trial that overflowed")
        sequences.same_bits(formod_on(model, geom), fresh_formod(hip, case, case.atm, geom), "the model holds atm, its status word is clean")
    finally:
        model.close()


# ---- 2. a first guess that cannot be traced --------------------------------------------------------------------------------
def retrieve(hip, model, sc, rays=slice(None), **kw):
    case, geom, y, weight = sc[:4]
    s = dict(SETTINGS)
    return model.retrieve_scene(case.atm, geom[rays], y[rays], weight[rays], s.pop("max_iter"), s.pop("fac"), history=True, **s, **kw)


def others_match(got, ref, lay, what):
    """the slices 0 and 1 of a call on all three against the call on their rays alone"""
    n = int(lay["wptr"][2])
    for f in PER_SLICE:
        bits(got[f][:2], ref[f], "%s: %s" % (what, f))
    for f in HISTORY:
        bits(got[f][..., :2], ref[f], "%s: %s" % (what, f))
    bits(got["x"][:n], ref["x"], what + ": x")
    for f in ("rad", "tau", "tp", "np"):
        bits(got[f][:8], ref[f], "%s: %s" % (what, f))
    bits(got["h_work"][1:], ref["h_work"][1:], what + ": the work of the iterations after the failure")


def failed_at_once(hip, got, lay, x0, what):
    s2 = slice(int(lay["wptr"][2]), int(lay["wptr"][3]))
    assert got["state"][2] == hip.RET_FAILED and got["iters"][2] == 0 and got["nlive"][2] == 0, what
    assert np.isnan(got["cost"][2]) and np.isnan(got["prior"][2]), what
    bits(got["x"][s2], x0[s2], what + ": x stays the first guess")
    assert np.all(np.isnan(got["h_lam"][..., 2])) and np.all(np.isnan(got["h_tcost"][..., 2])) and np.all(np.isnan(got["h_tprior"][..., 2]))
    assert np.all(got["h_status"][..., 2] == -1) and np.all(got["h_best"][:, 2] == -1) and np.all(got["h_accept"][:, 2] == -1)
    assert np.all(np.isnan(got["h_cost"][:, 2])) and np.all(np.isnan(got["h_prior"][:, 2]))
    assert got["np"][8] == abi.NLOS - 1 and not overflows(hip, np.delete(got["np"], 8)).any()


def test_a_first_guess_that_cannot_be_traced_fails_its_slice_alone(hip):
    sc = scene(hip, LONG)
    case, geom, y, weight, lay, iq, ip, x0 = sc
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        over = overflows(hip, counts(hip, model, case.atm, geom))
        assert list(np.flatnonzero(over)) == [8]
        model.set_atm(case.atm)
        with pytest.raises(hip.JurassicError, match=TOO_MANY % hip.ENLOS):
            retrieve(hip, model, sc)
        sequences.same_bits(formod_on(model, geom[:8]), fresh_formod(hip, case, case.atm, geom[:8]), "after the error the model holds atm0")
        ref = retrieve(hip, model, sc, rays=slice(0, 8))
        assert np.any(ref["h_accept"] == 1) and model.last_scene_overflow() == (0, 0)
        model.set_atm(case.atm)
        model.set_scene_overflow(hip.OVERFLOW_ISOLATE)
        got = retrieve(hip, model, sc)
        assert model.last_scene_overflow() == (0, 1)
        failed_at_once(hip, got, lay, x0, "switch on")
        others_match(got, ref, lay, "switch on")
        bits(state_of(case, got["atm"], iq, ip), got["x"], "atm_ret holds x")
        # the model holds atm_ret and its status word is clean: the rays that fit come back as from a fresh model
        sequences.same_bits(formod_on(model, geom[:8]), fresh_formod(hip, case, got["atm"], geom[:8]), "the model holds atm_ret")
        with pytest.raises(hip.JurassicError, match=TOO_MANY % hip.ENLOS):
            model.formod_host(geom)                                      # (formod_host keeps JUR_ENLOS)
        assert model.scene_overflow() == hip.OVERFLOW_ISOLATE
    finally:
        model.close()


# ---- 3. the loop recovers ------------------------------------------------------------------------------------------------------
RECOVER = dict(max_iter=6, tol=0.0, lam0=1e-2, fac=(1.0, 10.0), lam_min=1e-9, lam_max=1e6)


def recovering(hip):
    """The scene of test 1 with the measurements of slice 2 taken on T * 0.9 on its retrieved levels (the lowest ray needs
    396 points there), unit weights, no prior, little damping: the steps of slice 2 run into states its lowest ray cannot
    be traced through."""
    case, geom, y, weight, lay, iq, ip, x0 = scene(hip, EDGE)
    assert np.all(iq == 1)
    truth = copy_atm(case.atm)
    np.ctypeslib.as_array(truth.t)[ip[slice_mask(lay, 2)]] *= 0.9
    y2 = y.copy()
    y2[8:] = fresh_formod(hip, case, truth, geom[8:])["rad"]
    return y2, np.ones_like(weight)


def replay(hip, model, sc, y, weight, settings, prior=None):
    """The loop over the merged entries, slice by slice (a slice's doubles depend on its own rays alone): step_scene, which
    keeps JUR_ENLOS -- the slice fails --, trial_scene under the switch, the device's tracer on every trial atmosphere whose
    cost is NaN, the prior term of the state as a chain of float64 scalars, retrieve_decide."""
    case, geom = sc[:2]
    r, xa = prior if prior else (None, None)
    lay, iq, ip, x0 = sc[4:]
    ns, fac = 3, np.array(settings["fac"])
    nlam, mi = len(fac), settings["max_iter"]
    wptr, sid, widths = lay["wptr"], lay["sid"], np.diff(lay["rowptr"])
    atm = copy_atm(case.atm)
    lam, state, iters = np.full(ns, settings["lam0"]), np.zeros(ns, dtype=np.int32), np.zeros(ns, dtype=np.int32)
    cost, pri, nlive = np.zeros(ns), np.zeros(ns), np.zeros(ns, dtype=np.int64)
    nan = np.nan
    h = dict(h_cost=np.zeros((mi, ns)), h_prior=np.zeros((mi, ns)), h_lam=np.full((mi, nlam, ns), nan),
             h_tcost=np.full((mi, nlam, ns), nan), h_tprior=np.full((mi, nlam, ns), nan),
             h_status=np.full((mi, nlam, ns), -1, dtype=np.int32), h_best=np.full((mi, ns), -1, dtype=np.int32),
             h_accept=np.full((mi, ns), -1, dtype=np.int32), h_work=np.zeros((mi, 2), dtype=np.int64))
    cells = flagged = 0
    for it in range(mi):
        active = state == hip.RET_ACTIVE
        if active.any():
            rays_all = active[sid]
            h["h_work"][it] = (widths[rays_all] + 1).sum(), nlam * rays_all.sum()
        lamt = np.minimum(np.maximum(lam[None, :] * fac[:, None], settings["lam_min"]), settings["lam_max"])
        dx = np.zeros((nlam, len(x0)))
        tcost, tpri, hstat = np.zeros((nlam, ns)), np.zeros((nlam, ns)), np.zeros((nlam, ns), dtype=np.int32)
        x = state_of(case, atm, iq, ip)
        for s in np.flatnonzero(active):
            rays, els = sid == s, slice(wptr[s], wptr[s + 1])
            model.set_atm(atm)
            try:
                kw = dict(prior_ivar=r[els], prior_dx=(xa - x)[els]) if prior else {}
                step = model.step_scene(atm, geom[rays], y[rays], weight[rays], lamt[:, s:s + 1], **kw)
            except hip.JurassicError as e:
                assert "Too many LOS points" in str(e)
                state[s] = hip.RET_FAILED
                if iters[s] == 0:
                    cost[s], pri[s] = nan, nan
                continue
            assert np.all(step["status"] == 0)
            dx[:, els] = step["dx"]
            kw = dict(prior_ivar=r[els], prior_xa=xa[els]) if prior else {}
            trial = model.trial_scene(atm, geom[rays], y[rays], weight[rays], step["dx"], **kw)
            cells += model.last_scene_overflow()[0]
            tcost[:, s], tpri[:, s] = trial["cost"][:, 0], trial["prior"][:, 0]
            if prior:
                pri[s] = prior_chain(r[els], xa[els], x[els])
                for l in range(nlam):
                    bits(tpri[l, s], prior_chain(r[els], xa[els], x[els], dx[l][els]), "the prior term of a trial, overflowing or not")
            for l in np.flatnonzero(np.isnan(tcost[:, s])):
                moved = written_back(case, atm, iq, ip, dx[l], only=slice_mask(lay, s))
                if overflows(hip, counts(hip, model, moved, geom[rays])).any():   # (a radiance that is not finite costs NaN too)
                    hstat[l, s] = hip.TRIAL_OVERFLOW
                    flagged += 1
            cost[s], nlive[s], iters[s] = step["cost"][0], step["nlive"][0], iters[s] + 1
        h["h_cost"][it], h["h_prior"][it] = cost, pri
        took = state == hip.RET_ACTIVE
        took &= active
        for f, v in (("h_lam", lamt), ("h_tcost", tcost), ("h_tprior", tpri), ("h_status", hstat)):
            h[f][it][:, took] = v[:, took]
        d = hip.retrieve_decide(np.where(took, cost + pri, 0.0), tcost + tpri, lamt, np.maximum(hstat, 0), lam, state, settings["tol"],
                                settings["lam_max"], fac.max())
        lam, state = d["lam"], d["state"]
        h["h_best"][it], h["h_accept"][it] = d["best"], d["accept"]
        for s in np.flatnonzero(d["accept"] == 1):
            atm = written_back(case, atm, iq, ip, dx[d["best"][s]], only=slice_mask(lay, s))
            cost[s], pri[s] = tcost[d["best"][s], s], tpri[d["best"][s], s]
    state[state == hip.RET_ACTIVE] = hip.RET_MAXITER
    assert cells == flagged, "trial_scene counts the cells the tracer finds"
    return dict(h, x=state_of(case, atm, iq, ip), atm=atm, lam=lam, cost=cost, prior=pri, nlive=nlive, state=state, iters=iters,
                counters=(cells, int((state == hip.RET_FAILED).sum())))


@pytest.mark.parametrize("with_prior", [False, True])
def test_the_loop_recovers_from_trials_that_overflow(hip, with_prior):
    """with_prior: the diagonal prior with prior_ivar = 0 (every r_i >= 0 is accepted) around the first guess: D, M and g keep
    their bits, so the case is the same, and the loop's prior path runs -- prior_dx and the prior terms formed on the device
    every iteration, h_tprior = +0.0 beside NaN trial costs, Jt = NaN + prior no candidate.  (Any r > 0 damps the barely
    seen levels whose steps make the overflows: with 1e-12 and with 1e-30 alike every step is accepted and nothing
    overflows, so no case with a positive prior was found at this shape.)  Found on an MI355X at this shape: slice 2 accepts its first step, has every trial rejected in iterations 1 - 3 (one of
    them an overflow in iteration 3), overflows in the less damped trial of iteration 4 and accepts the more damped one,
    and in iteration 5 cannot trace the accepted state: RET_FAILED with iters == 5.  The preconditions are asserted, the
    rest is the replay's."""
    sc = scene(hip, EDGE)
    case, geom = sc[:2]
    y, weight = recovering(hip)
    s = dict(RECOVER)
    prior = (np.zeros(len(sc[7])), sc[7].copy()) if with_prior else None
    pk = dict(prior_ivar=prior[0], prior_xa=prior[1]) if prior else {}
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        model.set_scene_overflow(hip.OVERFLOW_ISOLATE)
        got = model.retrieve_scene(case.atm, geom, y, weight, s.pop("max_iter"), s.pop("fac"), history=True, **s, **pk)
        counters = model.last_scene_overflow()
        after = formod_on(model, geom[:8])
        want = replay(hip, model, sc, y, weight, RECOVER, prior)
    finally:
        model.close()
    # the preconditions: a trial of slice 2 overflowed and a later step of that slice was accepted
    its, _ = np.nonzero(got["h_status"][:, :, 2] == hip.TRIAL_OVERFLOW)
    assert len(its) > 0 and np.any(got["h_accept"][its.min():, 2] == 1), (got["h_status"][:, :, 2], got["h_accept"][:, 2])
    assert np.all(np.isnan(got["h_tcost"][:, :, 2][got["h_status"][:, :, 2] == hip.TRIAL_OVERFLOW]))
    if with_prior:
        assert np.all(got["h_tprior"][:, :, 2][got["h_status"][:, :, 2] == hip.TRIAL_OVERFLOW].view(np.uint64) == 0), "the prior term beside the NaN cost"
    for f in HISTORY + ("h_work", "x") + PER_SLICE:
        bits(got[f], want[f], f)
    same_atm(hip, got["atm"], want["atm"])
    assert counters == want["counters"] and counters[0] >= 1
    sequences.same_bits(after, fresh_formod(hip, case, got["atm"], geom[:8]), "the model holds atm_ret")


# ---- 4. invariance with the switch on ----------------------------------------------------------------------------------------
def box(hip, case):
    lo, hi = hip.state_bounds_upstream(case.ctl)
    lo[1], hi[1] = 215.0, 290.0                                          # (T: a box the retrieval of the other slices meets or not)
    return lo, hi


@pytest.mark.parametrize("setting", ["passes", "recomp", "fov", "box", "prior"])
def test_the_isolation_holds_under_every_setting(hip, setting):
    """The failed slice changes nothing for the others whatever else is set: against the switch-off call on their rays
    alone under the same setting; for the passes also against the call with the model's own passes."""
    sc = scene(hip, LONG)
    case, geom, y, weight, lay, iq, ip, x0 = sc
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        if setting == "recomp":
            model.set_kernel_recomp(2)
        if setting == "fov":
            model.set_fov(DZ, W)
        if setting == "box":
            model.set_state_bounds(*box(hip, case))
        kw, kw8 = {}, {}
        if setting == "prior":                                           # JUR_DAMP_PRIOR: 1e-2 of the mean diagonal of A_s, around the first guess
            n8 = int(lay["wptr"][2])
            nrm = model.normal_scene(case.atm, geom[:8], y[:8], weight[:8])
            scale = [np.diag(nrm["A"][nrm["aptr"][q]:nrm["aptr"][q + 1]].reshape(w, w)).mean() for q, w in enumerate(np.diff(lay["wptr"][:3]))]
            r = 1e-2 * np.repeat(scale + [scale[1]], np.diff(lay["wptr"]))
            assert np.all(r > 0)
            kw, kw8 = dict(mode=hip.DAMP_PRIOR, prior_ivar=r, prior_xa=x0), dict(mode=hip.DAMP_PRIOR, prior_ivar=r[:n8], prior_xa=x0[:n8])
            model.set_atm(case.atm)
        ref = retrieve(hip, model, sc, rays=slice(0, 8), **kw8)
        assert np.any(ref["h_accept"] == 1)
        model.set_atm(case.atm)
        model.set_scene_overflow(hip.OVERFLOW_ISOLATE)
        base = None
        for cap in ((0, 1, 7) if setting == "passes" else (0,)):
            got = retrieve(hip, model, sc, max_rays_per_pass=cap, **kw)
            assert model.last_scene_overflow() == (0, 1)
            failed_at_once(hip, got, lay, x0, "%s, cap %d" % (setting, cap))
            others_match(got, ref, lay, "%s, cap %d" % (setting, cap))
            if base is None:
                base = got
            for f in PER_SLICE + HISTORY + ("x", "rad", "tau", "tp", "np"):
                bits(got[f], base[f], "%s: cap %d against the model's own passes" % (f, cap))
            same_atm(hip, got["atm"], base["atm"])
    finally:
        model.close()


# ---- 5. where nothing overflows ------------------------------------------------------------------------------------------------
def test_where_nothing_overflows_the_switch_changes_no_bit(hip):
    sc = scene(hip, EDGE)
    case, geom, y, weight, lay, iq, ip, x0 = sc
    dx = np.vstack([np.full(len(x0), 0.5), np.full(len(x0), -0.5)])
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        off = retrieve(hip, model, sc)
        model.set_atm(case.atm)
        toff = model.trial_scene(case.atm, geom, y, weight, dx)
        model.set_scene_overflow(hip.OVERFLOW_ISOLATE)
        on = retrieve(hip, model, sc)
        assert model.last_scene_overflow() == (0, 0)
        model.set_atm(case.atm)
        ton = model.trial_scene(case.atm, geom, y, weight, dx)
        assert model.last_scene_overflow() == (0, 0)
    finally:
        model.close()
    assert np.all(off["state"] != hip.RET_FAILED) and np.all(off["h_status"][0] == 0) and np.any(off["h_accept"] == 1)
    for f in PER_SLICE + HISTORY + ("h_work", "x", "rad", "tau", "tp", "np"):
        bits(on[f], off[f], f)
    same_atm(hip, on["atm"], off["atm"])
    for f in ("cost", "prior"):
        bits(ton[f], toff[f], "trial_scene: " + f)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", RETRIEVE_SCENES)
def test_the_existing_retrieval_cases_return_the_same_bits_on_and_off(hip, name, mode):
    """tests/test_scene_retrieve_gpu.py's cases -- `ragged` and `short_last` under REPLAY, Marquardt damping without a prior
    and JUR_DAMP_PRIOR with the seeded diagonal prior -- through retrieve_scene and trial_scene (with the prior pair)."""
    case, geom, y, weight = inputs(hip, name)
    lay, iq, ip, x0 = layout(hip, name)
    prior = seeded_prior(hip, name, lay, x0) if mode == hip.DAMP_PRIOR else None
    pk = dict(prior_ivar=prior[0], prior_xa=prior[1]) if prior else {}
    r, xa = seeded_prior(hip, name, lay, x0)
    xa = xa + 1e-3 * np.random.default_rng(5).standard_normal(len(x0))
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        out, tri = {}, {}
        for label, switch in (("off", hip.OVERFLOW_ERROR), ("on", hip.OVERFLOW_ISOLATE)):
            model.set_scene_overflow(switch)
            model.set_atm(case.atm)
            s = dict(REPLAY)
            out[label] = model.retrieve_scene(case.atm, geom, y, weight, s.pop("max_iter"), s.pop("fac"), mode=mode, history=True, **s, **pk)
            assert model.last_scene_overflow() == (0, 0)
            model.set_atm(case.atm)
            dx = model.step_scene(case.atm, geom, y, weight, STEP_LAMS)["dx"]
            tri[label] = model.trial_scene(case.atm, geom, y, weight, dx, prior_ivar=r, prior_xa=xa)
            assert model.last_scene_overflow() == (0, 0)
    finally:
        model.close()
    off, on = out["off"], out["on"]
    assert np.all(off["state"] != hip.RET_FAILED) and np.any(off["h_accept"] == 1) and np.all(off["h_status"] != hip.TRIAL_OVERFLOW)
    for f in PER_SLICE + HISTORY + ("h_work", "x", "rad", "tau", "tp", "np"):
        bits(on[f], off[f], f)
    same_atm(hip, on["atm"], off["atm"])
    for f in ("cost", "prior"):
        bits(tri["on"][f], tri["off"][f], "trial_scene: " + f)
    assert np.all(tri["off"]["prior"] > 0)


# ---- 6. state -------------------------------------------------------------------------------------------------------------------
def test_the_switch_is_the_models_and_refusals_keep_their_words(hip):
    sc = scene(hip, LONG)
    case, geom, y, weight, lay, iq, ip, x0 = sc
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        assert model.scene_overflow() == hip.OVERFLOW_ERROR and model.last_scene_overflow() == (0, 0)
        for bad in (-1, 2, 7):
            with pytest.raises(hip.JurassicError, match=r"error %d: jur_model_set_scene_overflow: unknown mode %d: JUR_OVERFLOW_ERROR \(0\) or "
                                                        r"JUR_OVERFLOW_ISOLATE \(1\)" % (hip.EINVAL, bad)):
                model.set_scene_overflow(bad)
            assert model.scene_overflow() == hip.OVERFLOW_ERROR
        model.set_scene_overflow(hip.OVERFLOW_ISOLATE)
        model.set_atm(case.atm)
        model.set_kernel_recomp(2)
        model.set_fov(DZ, W)
        model.set_fov(None)
        model.set_state_bounds(*box(hip, case))
        model.set_state_bounds(None)
        model.set_scene_hydz(None)
        model.set_kernel_recomp(1)
        assert model.scene_overflow() == hip.OVERFLOW_ISOLATE
        got = retrieve(hip, model, sc)
        assert model.last_scene_overflow() == (0, 1)
        # after a call with failures the forward model sees a clean status word ...
        sequences.same_bits(formod_on(model, geom[:8]), fresh_formod(hip, case, got["atm"], geom[:8]), "formod_host after failures")
        # ... the entries that do not honour the switch keep JUR_ENLOS ...
        model.set_atm(case.atm)
        with pytest.raises(hip.JurassicError, match=TOO_MANY % hip.ENLOS):
            model.step_scene(case.atm, geom, y, weight, FAC)
        # ... a refused call counts nothing and the next good one counts anew
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_retrieve_scene_host: max_iter = 0" % hip.EINVAL):
            model.retrieve_scene(case.atm, geom, y, weight, 0, FAC)
        assert model.last_scene_overflow() == (0, 0)
        model.set_scene_overflow(hip.OVERFLOW_ERROR)
        with pytest.raises(hip.JurassicError, match=TOO_MANY % hip.ENLOS):
            retrieve(hip, model, sc)
        assert model.last_scene_overflow() == (0, 0)
    finally:
        model.close()
