"""The box on the state of the scene retrieval (Model.set_state_bounds, jur_model_set_state_bounds): trial_scene and
retrieve_scene form state_bound(x + dx) wherever they formed x + dx.

The reference has no retrieval program, so the yardstick is the project's own merged entries, none of which reads the box,
replayed on the host as tests/test_scene_retrieve_gpu.py and tests/test_scene_recomp_gpu.py replay them, with the clamp
in the write-back: normal_scene on the atmosphere with state_bound(x_e + dx_e) written at every element for a trial cost,
the prior chain in float64 scalars on that bounded state, step_scene (or gradient_scene + solve_slices in a reuse
iteration) for the steps, retrieve_decide for the policy.  Everything is compared bit for bit: no tolerance.

The boxes come from the inputs alone: per quantity the range of the first guess over the state elements of that quantity
(lo_q = min, hi_q = max; a quantity without elements is left open), so the first guess lies inside and every step that
carries an element past the extremes of its quantity is clamped."""
import numpy as np
import pytest
import sequences
from test_scene_jacobian_gpu import bits, formod_on, fresh_formod
from test_scene_normal_gpu import copy_atm, inputs, interleaved
from test_scene_solve_gpu import STEP_LAMS
from test_scene_retrieve_gpu import (HISTORY, PER_SLICE, REPLAY, SCENES, elements, layout, prior_chain, rows_of, same_atm, seeded_prior,
                                     slice_mask, state_of)
import test_scene_fov_gpu as F
import test_scene_hydro_gpu as H
import test_prior_full_gpu as P

pytestmark = pytest.mark.gpu
COMPARED = HISTORY + ("h_work", "x") + PER_SLICE
INF = np.inf


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def range_box(case, iq, x):
    """per quantity the range of x over its elements; a quantity without elements is left open"""
    nq = 2 + case.ctl.ng + case.ctl.nw
    lo, hi = np.full(nq, -INF), np.full(nq, INF)
    for q in np.unique(iq):
        lo[q], hi[q] = x[iq == q].min(), x[iq == q].max()
    return lo, hi


def bounded(hip, box, iq, v):
    return hip.state_bound(v, box[0][iq], box[1][iq])


def bounded_written_back(hip, case, atm, iq, ip, dx, box, only=None):
    """a copy of atm with state_bound(x_e + dx_e) at every element (of the slices in `only`: a mask over elements)"""
    out = copy_atm(atm)
    rows = rows_of(case, out)
    v = bounded(hip, box, iq, state_of(case, atm, iq, ip) + dx)
    for e in range(len(dx)):
        if only is None or only[e]:
            rows[iq[e]][ip[e]] = v[e]
    return out


def scene_T(hip, name):
    case, geom, y, weight = inputs(hip, name)
    lay, iq, ip, x0 = layout(hip, name)
    return case, geom, y, weight, lay, iq, ip


def scene_of(hip, case, geom, y, weight):
    """the tuple of a scene for rays in another order"""
    lay = hip.scene_slices(case.ctl, case.atm, geom[:, 0])
    lay.update(hip.scene_layout(case.ctl, case.atm, geom[:, 0]))
    iq, ip = elements(hip, case, lay)
    return case, geom, y, weight, lay, iq, ip


# ---- 1. the trial entry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_trial_costs_are_normal_scene_on_the_bounded_written_back_atmosphere(hip, name):
    case, geom, y, weight = inputs(hip, name)
    lay, iq, ip, x0 = layout(hip, name)
    ns, n, wptr = len(lay["sfirst"]), len(x0), lay["wptr"]
    assert set(np.unique(iq)) >= {0, 1, 2 + case.ctl.ng}, "p, T and an extinction window are in the state"
    box = range_box(case, iq, x0)
    r, xa = seeded_prior(hip, name, lay, x0)
    xa = xa + 1e-3 * np.random.default_rng(5).standard_normal(n)
    pc, rf, xaf = P.scene_prior(hip, name)
    slices = [slice(wptr[s], wptr[s + 1]) for s in range(ns)]
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        step = model.step_scene(case.atm, geom, y, weight, STEP_LAMS)
        assert np.all(step["status"] == 0)
        out_of_it = (box[1][iq] - box[0][iq] + 1.0) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        dx = np.vstack([step["dx"], out_of_it])
        nt = len(dx)
        xb = np.array([bounded(hip, box, iq, x0 + dx[t]) for t in range(nt)])
        clamped = np.array([(xb[t] != x0 + dx[t]).sum() for t in range(nt)])
        print("BOUNDS trial %s: elements clamped per trial %s of %d" % (name, clamped.tolist(), n))
        assert clamped[-1] == n and clamped[:-1].sum() > 0
        want, open_ = np.zeros((nt, ns)), np.zeros((nt, ns))
        full_want = np.zeros((nt, ns))
        for t in range(nt):
            atm = bounded_written_back(hip, case, case.atm, iq, ip, dx[t], box)
            bits(state_of(case, atm, iq, ip), xb[t], "the written-back state")
            model.set_atm(atm)
            want[t] = model.normal_scene(atm, geom, y, weight)["cost"]
        chain = np.array([[prior_chain(r[sl], xa[sl], xb[t][sl]) for sl in slices] for t in range(nt)])
        # the full prior precision: the merged trial entry with no box, on the bounded written-back atmosphere with dx = 0
        # (xb + 0.0 is xb: no element of these states is -0.0)
        assert not np.any((xb == 0) & np.signbit(xb))
        model.set_prior_precision(wptr, pc["R"])
        for t in range(nt):
            atm = bounded_written_back(hip, case, case.atm, iq, ip, dx[t], box)
            model.set_atm(atm)
            full_want[t] = model.trial_scene(atm, geom, y, weight, np.zeros(n), prior_ivar=rf, prior_xa=xaf)["prior"][0]
        model.set_prior_precision(None)
        model.set_atm(case.atm)
        open_ = model.trial_scene(case.atm, geom, y, weight, dx)["cost"]
        assert np.all(open_[-1].view(np.uint64) != want[-1].view(np.uint64)), "bounded and unbounded costs of the constructed row differ"

        model.set_state_bounds(*box)
        bare = model.trial_scene(case.atm, geom, y, weight, dx)
        bits(bare["cost"], want, "cost against normal_scene on the bounded write-back")
        assert np.all(bare["prior"].view(np.uint64) == 0)
        sequences.same_bits(formod_on(model, case.geom), fresh_formod(hip, case, case.atm, case.geom), "the model holds atm afterwards")
        for cap in (0, 1, 257):
            got = model.trial_scene(case.atm, geom, y, weight, dx, prior_ivar=r, prior_xa=xa, max_rays_per_pass=cap)
            bits(got["cost"], want, "cost, passes of %d" % cap)
            bits(got["prior"], chain, "prior against the chain on the bounded state, passes of %d" % cap)
        for t in range(nt):
            one = model.trial_scene(case.atm, geom, y, weight, dx[t], prior_ivar=r, prior_xa=xa)
            bits(one["cost"][0], want[t], "trial %d alone" % t)
            bits(one["prior"][0], chain[t], "prior of trial %d alone" % t)
        for s in range(ns):
            rays = lay["sid"] == s
            alone = model.trial_scene(case.atm, geom[rays], y[rays], weight[rays], dx[:, slices[s]], prior_ivar=r[slices[s]], prior_xa=xa[slices[s]])
            bits(alone["cost"][:, 0], want[:, s], "slice %d's rays alone" % s)
            bits(alone["prior"][:, 0], chain[:, s], "prior, slice %d's rays alone" % s)
        model.set_prior_precision(wptr, pc["R"])
        for cap in (0, 1, 257):
            full = model.trial_scene(case.atm, geom, y, weight, dx, prior_ivar=rf, prior_xa=xaf, max_rays_per_pass=cap)
            bits(full["cost"], want, "cost with a full prior precision, passes of %d" % cap)
            bits(full["prior"], full_want, "prior with a full prior precision, passes of %d" % cap)
    finally:
        model.close()


# ---- 2. a box that cannot bite -----------------------------------------------------------------------------------------
def run(model, sc, settings, mode=0, prior=None, **kw):
    case, geom, y, weight = sc[:4]
    s = dict(settings)
    pk = dict(prior_ivar=prior[0], prior_xa=prior[1]) if prior else {}
    return model.retrieve_scene(case.atm, kw.pop("geom", geom), kw.pop("y", y), kw.pop("weight", weight), s.pop("max_iter"), s.pop("fac"),
                                mode=mode, history=True, **s, **pk, **kw)


def test_an_open_box_is_no_box(hip):
    name = "ragged"
    sc = scene_T(hip, name)
    case, geom, y, weight, lay, iq, ip = sc
    x0 = layout(hip, name)[3]
    prior = seeded_prior(hip, name, lay, x0)
    nq = 2 + case.ctl.ng + case.ctl.nw
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        assert model.state_bounds() is None
        dx = model.step_scene(case.atm, geom, y, weight, STEP_LAMS)["dx"]
        off = model.trial_scene(case.atm, geom, y, weight, dx, prior_ivar=prior[0], prior_xa=prior[1]), run(model, sc, REPLAY, 1, prior)
        model.set_state_bounds(np.full(nq, -INF), np.full(nq, INF))
        assert model.state_bounds() is not None
        on = model.trial_scene(case.atm, geom, y, weight, dx, prior_ivar=prior[0], prior_xa=prior[1]), run(model, sc, REPLAY, 1, prior)
    finally:
        model.close()
    for f in ("cost", "prior"):
        bits(on[0][f], off[0][f], "trial %s" % f)
    for f in COMPARED + ("rad", "tau", "tp", "np"):
        bits(on[1][f], off[1][f], f)
    same_atm(hip, on[1]["atm"], off[1]["atm"])
    assert np.any(off[1]["h_accept"] == 1)


# ---- 3. the loop against a replay on the host, with the clamp in the write-back ----------------------------------------------
def replay(hip, model, sc, settings, box, every=1, mode=0, prior=None, balance=None):
    """The loop of jur_retrieve_scene_host over the merged entries of `model` (none reads the box; its other switches set by
    the caller), as tests/test_scene_recomp_gpu.py replays it, with state_bound in every write-back: the trial
    atmospheres, the prior chains and the accepted steps.  balance: what makes a written-back atmosphere the state (the
    hydrostatic balance, after the bound), or None.  clamped: the elements of accepted steps with bound(x + dx) != x + dx;
    reuse_accepts: reuse iterations in which a slice accepted a step."""
    case, geom, y, weight, lay, iq, ip = sc
    ns, nd = len(lay["sfirst"]), y.shape[1]
    fac = np.array(settings["fac"])
    nlam, mi = len(fac), settings["max_iter"]
    wptr, sid = lay["wptr"], lay["sid"]
    widths = np.diff(lay["rowptr"])
    r, xa = prior if prior else (None, None)
    atm = copy_atm(case.atm)
    if balance:
        atm = balance(atm)
    lam, state, iters = np.full(ns, settings["lam0"]), np.zeros(ns, dtype=np.int32), np.zeros(ns, dtype=np.int32)
    cost, pri, nlive = np.zeros(ns), np.zeros(ns), np.zeros(ns, dtype=np.int64)
    nan = np.nan
    h = dict(h_cost=np.zeros((mi, ns)), h_prior=np.zeros((mi, ns)), h_lam=np.full((mi, nlam, ns), nan),
             h_tcost=np.full((mi, nlam, ns), nan), h_tprior=np.full((mi, nlam, ns), nan),
             h_status=np.full((mi, nlam, ns), -1, dtype=np.int32), h_best=np.full((mi, ns), -1, dtype=np.int32),
             h_accept=np.full((mi, ns), -1, dtype=np.int32), h_work=np.zeros((mi, 2), dtype=np.int64))
    kept_A, kept_k = {}, {}
    clamped = reuse_accepts = 0
    for it in range(mi):
        active = state == hip.RET_ACTIVE
        if not active.any():
            h["h_cost"][it], h["h_prior"][it] = cost, pri
            continue
        rays = (sid >= 0) & active[np.maximum(sid, 0)]
        ridx = np.flatnonzero(rays)
        sub = hip.scene_slices(case.ctl, atm, geom[rays][:, 0])
        full_of = [int(np.flatnonzero((lay["sfirst"] == f) & (lay["slen"] == l))[0]) for f, l in zip(sub["sfirst"], sub["slen"])]
        assert sorted(full_of) == list(np.flatnonzero(active))
        els = np.concatenate([np.arange(wptr[s], wptr[s + 1]) for s in full_of])
        x = state_of(case, atm, iq, ip)
        lamt = np.minimum(np.maximum(lam[None, :] * fac[:, None], settings["lam_min"]), settings["lam_max"])
        kw = dict(prior_ivar=r[els], prior_dx=(xa - x)[els]) if prior else {}
        model.set_atm(atm)
        if it % every == 0:
            step = model.step_scene(atm, geom[rays], y[rays], weight[rays], lamt[:, full_of], mode=mode, want_normal=True, want_k=every > 1, **kw)
            if every > 1:
                for j, s in enumerate(full_of):
                    kept_A[s] = step["A"][sub["aptr"][j]:sub["aptr"][j + 1]].copy()
                for j, ray in enumerate(ridx):
                    kept_k[ray] = step["k"][step["rowptr"][j] * nd:step["rowptr"][j + 1] * nd].copy()
            sdx, sstatus, scost, snlive = step["dx"], step["status"], step["cost"], step["nlive"]
            work = (widths[rays] + 1).sum()
        else:
            grad = model.gradient_scene(atm, geom[rays], y[rays], weight[rays], np.concatenate([kept_k[ray] for ray in ridx]))
            sol = model.solve_slices(sub["wptr"], np.concatenate([kept_A[s] for s in full_of]), grad["b"], lamt[:, full_of], mode=mode, **kw)
            sdx, sstatus, scost, snlive = sol["dx"], sol["status"], grad["cost"], grad["nlive"]
            work = rays.sum()
        dx = np.zeros((nlam, len(x)))
        dx[:, els] = sdx
        xb = np.array([bounded(hip, box, iq, x + dx[l]) for l in range(nlam)])
        tcost, tpri, status = np.zeros((nlam, ns)), np.zeros((nlam, ns)), np.zeros((nlam, ns), dtype=np.int32)
        status[:, full_of] = sstatus
        for l in range(nlam):
            trial = bounded_written_back(hip, case, atm, iq, ip, dx[l], box)
            model.set_atm(trial)
            tcost[l, full_of] = model.normal_scene(trial, geom[rays], y[rays], weight[rays])["cost"]
        for j, s in enumerate(full_of):
            sl = slice(wptr[s], wptr[s + 1])
            cost[s], nlive[s], iters[s] = scost[j], snlive[j], iters[s] + 1
            pri[s] = prior_chain(r[sl], xa[sl], x[sl]) if prior else 0.0
            for l in range(nlam):
                tpri[l, s] = prior_chain(r[sl], xa[sl], xb[l][sl]) if prior else 0.0
        h["h_cost"][it], h["h_prior"][it] = cost, pri
        for f, v in (("h_lam", lamt), ("h_tcost", tcost), ("h_tprior", tpri), ("h_status", status)):
            h[f][it][:, active] = v[:, active]
        h["h_work"][it] = work, nlam * rays.sum()
        d = hip.retrieve_decide(cost + pri, tcost + tpri, lamt, status, lam, state, settings["tol"], settings["lam_max"], fac.max())
        lam, state = d["lam"], d["state"]
        h["h_best"][it], h["h_accept"][it] = d["best"], d["accept"]
        for s in np.flatnonzero(d["accept"] == 1):
            b = d["best"][s]
            mask = slice_mask(lay, s)
            clamped += int((xb[b][mask] != (x + dx[b])[mask]).sum())
            atm = bounded_written_back(hip, case, atm, iq, ip, dx[b], box, only=mask)
            cost[s], pri[s] = tcost[b, s], tpri[b, s]
        reuse_accepts += int(it % every != 0 and np.any(d["accept"] == 1))
        if balance:
            atm = balance(atm)
    state[state == hip.RET_ACTIVE] = hip.RET_MAXITER
    return dict(h, x=state_of(case, atm, iq, ip), atm=atm, lam=lam, cost=cost.copy(), prior=pri.copy(), nlive=nlive, state=state, iters=iters,
                clamped=clamped, reuse_accepts=reuse_accepts)


def check_loop(hip, sc, box, got, want, open_, after=None, final=None, balanced=None):
    """got against its replay, bit for bit; the box held elements of accepted steps and changed the result"""
    case, geom, iq, ip = sc[0], sc[1], sc[5], sc[6]
    for f in COMPARED:
        bits(got[f], want[f], f)
    same_atm(hip, got["atm"], want["atm"])
    bits(state_of(case, got["atm"], iq, ip), got["x"], "atm_ret holds x")
    if final is None:
        fresh = fresh_formod(hip, case, got["atm"], geom)
        final = {f: fresh[f] for f in ("rad", "tau", "tp", "np")}
    for f in final:
        bits(got[f], final[f], "%s against the forward model on atm_ret" % f)
    if after is not None:
        sequences.same_bits(after, fresh_formod(hip, case, got["atm"], case.geom), "the model holds atm_ret")
    assert want["clamped"] > 0, "no element of an accepted step was clamped"
    assert np.any(got["x"] != open_["x"]), "the box did not change the result"
    side = hip.state_on_bounds(box[0], box[1], iq, got["x"])
    mine = np.where(got["x"] == box[0][iq], -1, np.where(got["x"] == box[1][iq], 1, 0))
    assert np.array_equal(side["side"], mine) and side["count"] == np.count_nonzero(mine) and side["count"] > 0
    if balanced is None:                                                # (a balance after the bound moves p elements on its own)
        inside = (got["x"] >= box[0][iq]) & (got["x"] <= box[1][iq])
        moved = got["x"] != state_of(case, case.atm, iq, ip)
        assert np.all(inside | ~moved), "an element that moved lies in its interval"
    return want["clamped"], side["count"]


@pytest.mark.parametrize("mode,with_prior", [(0, False), (0, True), (1, True)])
@pytest.mark.parametrize("name", SCENES)
def test_the_loop_against_its_replay(hip, name, mode, with_prior):
    """The box is the first-guess range box on both scenes: accepted steps are clamped on each (the counts are printed)."""
    sc = scene_T(hip, name)
    case, lay, iq = sc[0], sc[4], sc[5]
    x0 = layout(hip, name)[3]
    box = range_box(case, iq, x0)
    prior = seeded_prior(hip, name, lay, x0) if with_prior else None
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        open_ = run(model, sc, REPLAY, mode, prior)
        model.set_state_bounds(*box)
        got = run(model, sc, REPLAY, mode, prior)
        after = formod_on(model, case.geom)
        want = replay(hip, model, sc, REPLAY, box, 1, mode, prior)
    finally:
        model.close()
    n = check_loop(hip, sc, box, got, want, open_, after)
    assert np.all(got["h_status"][0] == 0) and np.any(got["h_accept"] == 1)
    print("BOUNDS loop %s mode %d prior %d: %d elements of accepted steps clamped, %d of %d on a bound at the end" % (name, mode, with_prior, n[0], n[1], len(x0)))


# ---- 4. beside the model's other switches ------------------------------------------------------------------------------------
def test_beside_the_hydrostatic_balance(hip):
    """the scene, the reference level and the settings of tests/test_scene_hydro_gpu.py: bound first, then the balance"""
    name = "ragged"
    sc = H.scene(hip, name)
    case, geom, y, weight, lay, iq, ip = sc
    prior = H.diagonal_prior(hip, name)
    box = range_box(case, iq, state_of(case, case.atm, iq, ip))
    on = H.switched_on(hip, case)
    try:
        balance = lambda a: on.scene_hydrostatic(a, geom[:, 0])
        open_ = run(on, sc, H.SETTINGS, 0, prior)
        on.set_state_bounds(*box)
        got = run(on, sc, H.SETTINGS, 0, prior)
        want = replay(hip, on, sc, H.SETTINGS, box, 1, 0, prior, balance=balance)
        # one trial pass: the bounded write-back, balanced by the entry that reads it
        dx = on.step_scene(case.atm, geom, y, weight, H.LAMS)["dx"]
        x = state_of(case, balance(case.atm), iq, ip)
        trial = on.trial_scene(case.atm, geom, y, weight, dx, prior_ivar=prior[0], prior_xa=prior[1])
        for t in range(len(dx)):
            atm = bounded_written_back(hip, case, balance(case.atm), iq, ip, dx[t], box)
            on.set_atm(atm)
            bits(trial["cost"][t], on.normal_scene(atm, geom, y, weight)["cost"], "trial %d under the balance" % t)
        on.set_atm(case.atm)
    finally:
        on.close()
    n = check_loop(hip, sc, box, got, want, open_, balanced=True)
    bits(H.p_of(got["atm"]), H.p_of(want["atm"]), "atm_ret.p is the balance of the bounded write-back")
    assert np.any(got["h_accept"] == 1)
    print("BOUNDS hydrostatic: %d elements of accepted steps clamped, %d on a bound at the end" % n)


def test_beside_kernel_recomp(hip):
    name = "ragged"
    sc = scene_T(hip, name)
    case, lay, iq = sc[0], sc[4], sc[5]
    x0 = layout(hip, name)[3]
    box = range_box(case, iq, x0)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        model.set_kernel_recomp(2)
        open_ = run(model, sc, REPLAY)
        model.set_state_bounds(*box)
        got = run(model, sc, REPLAY)
        after = formod_on(model, case.geom)
        want = replay(hip, model, sc, REPLAY, box, 2)
    finally:
        model.close()
    check_loop(hip, sc, box, got, want, open_, after)
    assert want["reuse_accepts"] >= 1 and np.any(got["h_accept"][1::2] == 1), "a reuse iteration accepted a step"
    assert got["h_work"][1, 0] < got["h_work"][0, 0]


def test_beside_a_field_of_view(hip):
    """the scene, the shape and the settings of tests/test_scene_fov_gpu.py"""
    case, geom, y, weight, lay, iq, ip, x0 = F.scene(hip)
    sc = (case, geom, y, weight, lay, iq, ip)
    prior = F.seeded_prior(hip)
    box = range_box(case, iq, x0)
    model = F.with_shape(hip, case)
    try:
        open_ = run(model, sc, F.SETTINGS, 0, prior)
        model.set_state_bounds(*box)
        got = run(model, sc, F.SETTINGS, 0, prior)
        want = replay(hip, model, sc, F.SETTINGS, box, 1, 0, prior)
    finally:
        model.close()
    final = F.convolved(hip, case, got["atm"], geom)
    check_loop(hip, sc, box, got, want, open_, final={f: final[f] for f in ("rad", "tau")})
    assert np.any(got["h_accept"] == 1)


def test_interleaved_rays_and_small_passes(hip):
    name = "ragged"
    sc = scene_T(hip, name)
    case, geom, y, weight, lay, iq, ip = sc
    x0 = layout(hip, name)[3]
    box = range_box(case, iq, x0)
    perm = interleaved(lay["sid"])
    assert not np.array_equal(perm, np.arange(len(perm)))
    dealt = scene_of(hip, case, geom[perm], y[perm], weight[perm])
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        open_ = run(model, sc, REPLAY), run(model, dealt, REPLAY)
        model.set_state_bounds(*box)
        capped = run(model, sc, REPLAY, max_rays_per_pass=257)
        after = formod_on(model, case.geom)
        mixed = run(model, dealt, REPLAY)
        want = replay(hip, model, sc, REPLAY, box), replay(hip, model, dealt, REPLAY, box)
    finally:
        model.close()
    check_loop(hip, sc, box, capped, want[0], open_[0], after)
    check_loop(hip, dealt, box, mixed, want[1], open_[1])
    order = [int(np.flatnonzero((lay["sfirst"] == f) & (lay["slen"] == l))[0]) for f, l in zip(dealt[4]["sfirst"], dealt[4]["slen"])]
    for j, q in enumerate(order):
        bits(mixed["x"][dealt[4]["wptr"][j]:dealt[4]["wptr"][j + 1]], capped["x"][lay["wptr"][q]:lay["wptr"][q + 1]], "x of slice %d, interleaved" % q)
        for f in PER_SLICE + HISTORY:
            bits(mixed[f][..., j], capped[f][..., q], "%s of slice %d, interleaved" % (f, q))
    bits(mixed["rad"], capped["rad"][perm], "rad, interleaved")


# ---- 5. switching ------------------------------------------------------------------------------------------------------------
def test_switched_off_again_is_a_fresh_model(hip):
    name = "short_last"
    case, geom, y, weight, lay, iq, ip = H.scene(hip, name)
    prior = H.diagonal_prior(hip, name)
    box = range_box(case, iq, state_of(case, case.atm, iq, ip))
    fresh = hip.Model(case.ctl, case.lib_tables())
    try:
        fresh.set_atm(case.atm)
        want = H.six_entries(hip, fresh, name, prior)
    finally:
        fresh.close()
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        model.set_state_bounds(*box)
        lit = H.six_entries(hip, model, name, prior)
        assert not np.array_equal(lit[4]["x"], want[4]["x"]) and not np.array_equal(lit[3]["cost"], want[3]["cost"])
        for i in (0, 1, 2, 5, 6):                                       # kernel_scene, normal_scene, step_scene, diagnose_scene, the forward model
            for f in lit[i]:
                if f != "rc":
                    bits(lit[i][f], want[i][f], "entry %d, %s, with the box on" % (i, f))
        model.set_state_bounds(None)
        assert model.state_bounds() is None
        got = H.six_entries(hip, model, name, prior)
        for i, (a, b) in enumerate(zip(got, want)):
            assert a.keys() == b.keys()
            for f in a:
                if f != "rc":
                    bits(a[f], b[f], "entry %d, %s, after the box went off" % (i, f))
    finally:
        model.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_by_message(hip):
    case, geom, y, weight = inputs(hip, "ragged")
    ng, nw = case.ctl.ng, case.ctl.nw
    nq = 2 + ng + nw
    lo, hi = hip.state_bounds_upstream(case.ctl)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        assert model.state_bounds() is None
        model.set_state_bounds(lo, hi)
        held = model.state_bounds()
        bits(held[0], lo, "lo round-trips")
        bits(held[1], hi, "hi round-trips")
        head = r"error %d: jur_model_set_state_bounds: " % hip.EINVAL
        with pytest.raises(hip.JurassicError, match=head + r"nq = %d, the model has %d quantities" % (nq - 1, nq)):
            model.set_state_bounds(lo[:-1], hi[:-1])
        bad = lo.copy()
        bad[3] = np.nan
        with pytest.raises(hip.JurassicError, match=head + r"the lower bound of quantity 3 \(q\[1\]\) is NaN"):
            model.set_state_bounds(bad, hi)
        bad = hi.copy()
        bad[1] = np.nan
        with pytest.raises(hip.JurassicError, match=head + r"the upper bound of quantity 1 \(T\) is NaN"):
            model.set_state_bounds(lo, bad)
        bad = hi.copy()
        bad[nq - 1] = -1.0
        with pytest.raises(hip.JurassicError, match=head + r"quantity %d \(k\[0\]\): lo = 0 > hi = -1" % (nq - 1)):
            model.set_state_bounds(lo, bad)
        bad = lo.copy()
        bad[0] = 1e5
        with pytest.raises(hip.JurassicError, match=head + r"quantity 0 \(p\): lo = 100000 > hi = 50000"):
            model.set_state_bounds(bad, hi)
        held = model.state_bounds()
        bits(held[0], lo, "lo survives the refusals")
        bits(held[1], hi, "hi survives the refusals")
        fixed = np.full(nq, 7.0)
        model.set_state_bounds(fixed, fixed)                            # lo == hi is a box
        bits(model.state_bounds()[0], fixed, "lo == hi")
        model.set_state_bounds(None)
        assert model.state_bounds() is None
    finally:
        model.close()
