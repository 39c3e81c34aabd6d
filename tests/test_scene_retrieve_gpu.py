"""Model.trial_scene (jur_trial_scene_host) and Model.retrieve_scene (jur_retrieve_scene_host): trial steps and the
iterated Levenberg-Marquardt loop of a scene on the device.

The reference has no retrieval program, so the yardstick is the project's own merged entries replayed on the host: per
iteration step_scene on the rays of the active slices, the steps written back through scene_elements, normal_scene on
every trial atmosphere for its cost, the prior term as a chain of float64 scalars, retrieve_decide for the policy.
Everything is compared bit for bit; the one bound (a cost against its sum in np.longdouble, where no Jacobian entry can
serve as the yardstick) is derived where it stands."""
import ctypes as C
import numpy as np
import pytest
import common
import refcases as R
import sequences
from jurassic_hip import synth
from test_scene_jacobian_gpu import bits, formod_on, fresh_formod
from test_scene_normal_gpu import copy_atm, inputs, interleaved
from test_scene_solve_gpu import STEP_LAMS

pytestmark = pytest.mark.gpu
SCENES = ("ragged", "short_last")
REPLAY = dict(max_iter=4, tol=0.0, lam0=1.0, fac=(0.01, 1.0, 100.0), lam_min=1e-6, lam_max=1e6)
PER_SLICE = ("lam", "cost", "prior", "nlive", "state", "iters")
HISTORY = ("h_cost", "h_prior", "h_lam", "h_tcost", "h_tprior", "h_status", "h_best", "h_accept")


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def rows_of(case, atm):
    """the arrays of an atm_t by quantity index (0 p, 1 T, 2 + g q, 2 + ng + w k), as views"""
    rows = [np.ctypeslib.as_array(atm.p), np.ctypeslib.as_array(atm.t)]
    return rows + list(np.ctypeslib.as_array(atm.q)[:case.ctl.ng]) + list(np.ctypeslib.as_array(atm.k)[:case.ctl.nw])


def elements(hip, case, lay):
    """(iq, ip) of every state element in the layout's order"""
    el = [hip.scene_elements(case.ctl, case.atm, lay["sfirst"][s], lay["slen"][s]) for s in range(len(lay["sfirst"]))]
    return np.concatenate([e["iq"] for e in el]), np.concatenate([e["ip"] for e in el])


def state_of(case, atm, iq, ip):
    rows = rows_of(case, atm)
    return np.array([rows[q][p] for q, p in zip(iq, ip)])


def written_back(case, atm, iq, ip, dx, only=None):
    """a copy of atm with x_e + dx_e (one IEEE addition) at every element (of the slices in `only`: a mask over elements)"""
    out = copy_atm(atm)
    rows = rows_of(case, out)
    for e in range(len(dx)):
        if only is None or only[e]:
            rows[iq[e]][ip[e]] = rows[iq[e]][ip[e]] + dx[e]
    return out


def prior_chain(r, xa, x, dx=None):
    """the prior term of one slice: separately rounded float64 operations, ascending"""
    acc = np.float64(0.0)
    for i in range(len(r)):
        xi = np.float64(x[i]) if dx is None else np.float64(x[i]) + np.float64(dx[i])
        d = np.float64(xa[i]) - xi
        t = np.float64(r[i]) * d
        t = t * d
        acc = acc + t
    return acc


def seeded_prior(hip, name, lay, x0):
    """prior_ivar as test_scene_solve_gpu.py::test_priors makes it (1e-3 .. 1e-1 of the mean diagonal of A_s, seeded);
    prior_xa the first guess"""
    case, geom, y, weight = inputs(hip, name)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        out = model.normal_scene(case.atm, geom, y, weight)
    finally:
        model.close()
    rng = np.random.default_rng(3)
    r = []
    for s in range(len(lay["sfirst"])):
        w = int(lay["wptr"][s + 1] - lay["wptr"][s])
        As = out["A"][lay["aptr"][s]:lay["aptr"][s + 1]].reshape(w, w)
        r.append(10.0 ** rng.uniform(-3.0, -1.0, w) * np.diag(As).mean())
    return np.concatenate(r), x0.copy()


_layouts = {}


def layout(hip, name):
    if name not in _layouts:
        case, geom, _, _ = inputs(hip, name)
        lay = hip.scene_slices(case.ctl, case.atm, geom[:, 0])
        lay.update(hip.scene_layout(case.ctl, case.atm, geom[:, 0]))
        iq, ip = elements(hip, case, lay)
        _layouts[name] = (lay, iq, ip, state_of(case, case.atm, iq, ip))
    return _layouts[name]


def slice_mask(lay, s):
    """mask over the elements: those of slice s"""
    m = np.zeros(int(lay["wptr"][-1]), dtype=bool)
    m[lay["wptr"][s]:lay["wptr"][s + 1]] = True
    return m


# ---- 1. the trial entry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_trial_costs_are_normal_scene_on_the_written_back_atmosphere(hip, name):
    case, geom, y, weight = inputs(hip, name)
    lay, iq, ip, x0 = layout(hip, name)
    ns, n = len(lay["sfirst"]), len(x0)
    r, xa = seeded_prior(hip, name, lay, x0)
    xa = xa + 1e-3 * np.random.default_rng(5).standard_normal(n)        # (a prior term that is not zero at dx = 0)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        step = model.step_scene(case.atm, geom, y, weight, STEP_LAMS, want_normal=True)
        assert np.all(step["status"] == 0)
        dx = step["dx"]
        want = np.zeros((len(STEP_LAMS), ns))
        for t in range(len(STEP_LAMS)):
            atm = written_back(case, case.atm, iq, ip, dx[t])
            model.set_atm(atm)
            want[t] = model.normal_scene(atm, geom, y, weight)["cost"]
        model.set_atm(case.atm)
        bare = model.trial_scene(case.atm, geom, y, weight, dx)
        bits(bare["cost"], want, "cost against normal_scene")
        assert np.all(bare["prior"].view(np.uint64) == 0), "the prior term without a prior is +0.0"
        sequences.same_bits(formod_on(model, case.geom), fresh_formod(hip, case, case.atm, case.geom), "the model holds atm afterwards")
        full = model.trial_scene(case.atm, geom, y, weight, dx, prior_ivar=r, prior_xa=xa)
        bits(full["cost"], want, "cost with a prior")
        chain = np.array([[prior_chain(r[sl], xa[sl], x0[sl], dx[t][sl]) for sl in (slice(lay["wptr"][s], lay["wptr"][s + 1]) for s in range(ns))]
                          for t in range(len(STEP_LAMS))])
        bits(full["prior"], chain, "the prior term against the chain in float64 scalars")
        assert np.all(chain > 0)
        for cap in (1, 257):
            got = model.trial_scene(case.atm, geom, y, weight, dx, prior_ivar=r, prior_xa=xa, max_rays_per_pass=cap)
            bits(got["cost"], want, "cost, passes of %d" % cap)
            bits(got["prior"], chain, "prior, passes of %d" % cap)
        for t in range(len(STEP_LAMS)):
            one = model.trial_scene(case.atm, geom, y, weight, dx[t])
            bits(one["cost"][0], want[t], "trial %d alone" % t)
        for s in range(ns):
            rays = lay["sid"] == s
            alone = model.trial_scene(case.atm, geom[rays], y[rays], weight[rays], dx[:, lay["wptr"][s]:lay["wptr"][s + 1]])
            assert alone["cost"].shape == (len(STEP_LAMS), 1)
            bits(alone["cost"][:, 0], want[:, s], "slice %d's rays alone" % s)
        still = model.trial_scene(case.atm, geom, y, weight, np.zeros(n))
        bits(still["cost"][0], step["cost"], "a trial dx = 0 against the cost of the base")
        back = model.trial_scene(case.atm, geom, y, weight, -1e-3 * dx[1])
        moved = np.array([np.any(step["b"][lay["wptr"][s]:lay["wptr"][s + 1]] != 0) for s in range(ns)])
        assert moved.any() and np.all(back["cost"][0][moved] > step["cost"][moved]), "a step against the descent direction costs more"
    finally:
        model.close()


# ---- 2. the loop against a replay on the host --------------------------------------------------------------------------
def replay(hip, model, name, mode, prior, settings, y=None):
    """The loop of jur_retrieve_scene_host over the merged entries; returns what retrieve_scene returns (without the
    forward results), the state after every iteration in xs."""
    case, geom, y0, weight = inputs(hip, name)
    y = y0 if y is None else y
    lay, iq, ip, x0 = layout(hip, name)
    ns, nd = len(lay["sfirst"]), y.shape[1]
    fac = np.array(settings["fac"])
    nlam, mi = len(fac), settings["max_iter"]
    wptr, sid = lay["wptr"], lay["sid"]
    widths = np.diff(lay["rowptr"])
    r, xa = prior if prior else (None, None)
    atm = copy_atm(case.atm)
    lam, state, iters = np.full(ns, settings["lam0"]), np.zeros(ns, dtype=np.int32), np.zeros(ns, dtype=np.int32)
    cost, pri, nlive = np.zeros(ns), np.zeros(ns), np.zeros(ns, dtype=np.int64)
    nan = np.nan
    h = dict(h_cost=np.zeros((mi, ns)), h_prior=np.zeros((mi, ns)), h_lam=np.full((mi, nlam, ns), nan),
             h_tcost=np.full((mi, nlam, ns), nan), h_tprior=np.full((mi, nlam, ns), nan),
             h_status=np.full((mi, nlam, ns), -1, dtype=np.int32), h_best=np.full((mi, ns), -1, dtype=np.int32),
             h_accept=np.full((mi, ns), -1, dtype=np.int32), h_work=np.zeros((mi, 2), dtype=np.int64))
    xs = []
    for it in range(mi):
        active = state == hip.RET_ACTIVE
        if not active.any():
            h["h_cost"][it], h["h_prior"][it] = cost, pri
            xs.append(state_of(case, atm, iq, ip))
            continue
        rays = (sid >= 0) & active[np.maximum(sid, 0)]
        sub = hip.scene_slices(case.ctl, atm, geom[rays][:, 0])
        full_of = [int(np.flatnonzero((lay["sfirst"] == f) & (lay["slen"] == l))[0]) for f, l in zip(sub["sfirst"], sub["slen"])]
        assert sorted(full_of) == list(np.flatnonzero(active))
        els = np.concatenate([np.arange(wptr[s], wptr[s + 1]) for s in full_of])          # the sub-call's elements in the full layout
        x = state_of(case, atm, iq, ip)
        lamt = np.minimum(np.maximum(lam[None, :] * fac[:, None], settings["lam_min"]), settings["lam_max"])
        kw = dict(prior_ivar=r[els], prior_dx=(xa - x)[els]) if prior else {}
        model.set_atm(atm)
        step = model.step_scene(atm, geom[rays], y[rays], weight[rays], lamt[:, full_of], mode=mode, **kw)
        dx = np.zeros((nlam, len(x)))
        dx[:, els] = step["dx"]
        tcost, tpri, status = np.zeros((nlam, ns)), np.zeros((nlam, ns)), np.zeros((nlam, ns), dtype=np.int32)
        status[:, full_of] = step["status"]
        for l in range(nlam):
            trial = written_back(case, atm, iq, ip, dx[l])
            model.set_atm(trial)
            tcost[l, full_of] = model.normal_scene(trial, geom[rays], y[rays], weight[rays])["cost"]
        for j, s in enumerate(full_of):
            sl = slice(wptr[s], wptr[s + 1])
            cost[s], nlive[s], iters[s] = step["cost"][j], step["nlive"][j], iters[s] + 1
            pri[s] = prior_chain(r[sl], xa[sl], x[sl]) if prior else 0.0
            for l in range(nlam):
                tpri[l, s] = prior_chain(r[sl], xa[sl], x[sl], dx[l][sl]) if prior else 0.0
        h["h_cost"][it], h["h_prior"][it] = cost, pri
        for f, v in (("h_lam", lamt), ("h_tcost", tcost), ("h_tprior", tpri), ("h_status", status)):
            h[f][it][:, active] = v[:, active]
        h["h_work"][it] = (widths[rays] + 1).sum(), nlam * rays.sum()
        d = hip.retrieve_decide(cost + pri, tcost + tpri, lamt, status, lam, state, settings["tol"], settings["lam_max"], fac.max())
        lam, state = d["lam"], d["state"]
        h["h_best"][it], h["h_accept"][it] = d["best"], d["accept"]
        for s in np.flatnonzero(d["accept"] == 1):
            b = d["best"][s]
            atm = written_back(case, atm, iq, ip, dx[b], only=slice_mask(lay, s))
            cost[s], pri[s] = tcost[b, s], tpri[b, s]
        xs.append(state_of(case, atm, iq, ip))
    state[state == hip.RET_ACTIVE] = hip.RET_MAXITER
    return dict(h, x=xs[-1], xs=xs, atm=atm, lam=lam, cost=cost.copy(), prior=pri.copy(), nlive=nlive, state=state, iters=iters)


_runs = {}


def retrieved(hip, name, mode, settings=None, **kw):
    """Model.retrieve_scene on a scene with full history, on a model of its own (made once per scene and mode for REPLAY)"""
    key = (name, mode)
    shared = settings is None and not kw
    if shared and key in _runs:
        return _runs[key]
    case, geom, y, weight = inputs(hip, name)
    lay, iq, ip, x0 = layout(hip, name)
    prior = seeded_prior(hip, name, lay, x0) if mode == hip.DAMP_PRIOR else None
    pk = dict(prior_ivar=prior[0], prior_xa=prior[1]) if prior else {}
    s = dict(settings or REPLAY)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        out = model.retrieve_scene(case.atm, kw.pop("geom", geom), kw.pop("y", y), kw.pop("weight", weight), s.pop("max_iter"),
                                   s.pop("fac"), mode=mode, history=True, **s, **pk, **kw)
        out["after"] = formod_on(model, case.geom)
    finally:
        model.close()
    if shared:
        _runs[key] = out
    return out


def same_atm(hip, a, b):
    assert bytes(C.string_at(C.byref(a), C.sizeof(a))) == bytes(C.string_at(C.byref(b), C.sizeof(b)))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", SCENES)
def test_replay_on_the_host(hip, name, mode):
    case, geom, y, weight = inputs(hip, name)
    lay, iq, ip, x0 = layout(hip, name)
    got = retrieved(hip, name, mode)
    prior = seeded_prior(hip, name, lay, x0) if mode == hip.DAMP_PRIOR else None
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        want = replay(hip, model, name, mode, prior, REPLAY)
        # x after every iteration: runs that stop earlier end in the state the replay passed through
        for it in range(1, REPLAY["max_iter"]):
            short = dict(REPLAY, max_iter=it)
            pk = dict(prior_ivar=prior[0], prior_xa=prior[1]) if prior else {}
            s = dict(short)
            part = model.retrieve_scene(case.atm, geom, y, weight, s.pop("max_iter"), s.pop("fac"), mode=mode, **s, **pk)
            bits(part["x"], want["xs"][it - 1], "x after iteration %d" % (it - 1))
    finally:
        model.close()
    for f in HISTORY + ("h_work", "x") + PER_SLICE:
        bits(got[f], want[f], f)
    assert np.all(got["h_status"][0] == 0) and np.any(got["h_accept"] == 1)
    same_atm(hip, got["atm"], want["atm"])
    bits(state_of(case, got["atm"], iq, ip), got["x"], "atm_ret holds x")
    for it in range(REPLAY["max_iter"]):                                # the reported choices are the policy's on the reported numbers
        took_part = ~np.isnan(got["h_lam"][it][0])
        state = np.where(took_part, 0, 1).astype(np.int32)
        J = got["h_cost"][it] + got["h_prior"][it]
        Jt = np.where(took_part, got["h_tcost"][it] + got["h_tprior"][it], 0.0)
        lamt = np.where(took_part, got["h_lam"][it], 1.0)
        d = hip.retrieve_decide(J, Jt, lamt, np.maximum(got["h_status"][it], 0), np.ones(len(J)), state, REPLAY["tol"], REPLAY["lam_max"], 100.0)
        bits(d["best"], got["h_best"][it], "h_best of iteration %d" % it)
        bits(d["accept"], got["h_accept"][it], "h_accept of iteration %d" % it)
    fresh = fresh_formod(hip, case, got["atm"], geom)
    for f in ("rad", "tau", "tp", "np"):
        bits(got[f], fresh[f], "%s against a fresh model on atm_ret" % f)
    sequences.same_bits(got["after"], fresh_formod(hip, case, got["atm"], case.geom), "the model holds atm_ret")


# ---- 3. descent ----------------------------------------------------------------------------------------------------------
def test_descent(hip):
    got = retrieved(hip, "ragged", hip.DAMP_MARQUARDT)
    J = got["h_cost"] + got["h_prior"]
    final = got["cost"] + got["prior"]
    assert np.all(np.diff(np.vstack([J, final[None, :]]), axis=0) <= 0), "J never rises for any slice"
    trial = (got["h_tcost"][0] + got["h_tprior"][0]).sum(axis=1)
    after0 = J[1].sum()
    assert after0 <= trial.min()                                        # every slice takes its own best damping or stays
    assert after0 < J[0].sum()
    print("RETRIEVE descent: sum J after / before %.4e, after iteration 0 %.4e" % (final.sum() / J[0].sum(), after0 / J[0].sum()))


# ---- 4. control flow without a bad state ---------------------------------------------------------------------------------
FLOW = dict(max_iter=4, tol=0.0, lam0=1.0, fac=(0.1, 1.0, 10.0), lam_min=1e-6, lam_max=100.0)


def test_a_slice_that_cannot_move_stalls(hip):
    """y of slice 1's rays is the forward model on the first guess: b = 0, dx = +0.0, every trial cost equals the cost,
    nothing is accepted, lam grows 1 -> 10 -> 100 and the third rejection, at lam_max, ends the slice.  The other slices
    are independent problems: they match the run with the same settings on the scene's own y bit for bit."""
    case, geom, y, weight = inputs(hip, "ragged")
    lay, iq, ip, x0 = layout(hip, "ragged")
    s0 = 1
    rays = lay["sid"] == s0
    y2 = y.copy()
    y2[rays] = fresh_formod(hip, case, case.atm, geom[rays])["rad"]
    plain = retrieved(hip, "ragged", 0, settings=FLOW)
    got = retrieved(hip, "ragged", 0, settings=FLOW, y=y2)
    assert got["state"][s0] == hip.RET_STALLED and got["iters"][s0] == 3 and got["lam"][s0] == 100.0
    sl = slice(lay["wptr"][s0], lay["wptr"][s0 + 1])
    assert np.array_equal(got["x"][sl].view(np.uint64), x0[sl].view(np.uint64)), "x unchanged by bit pattern"
    assert np.all(got["h_accept"][:3, s0] == 0) and got["h_accept"][3, s0] == -1
    bits(got["h_tcost"][:3, :, s0], np.broadcast_to(got["h_cost"][:3, None, s0], (3, 3)).copy(), "trial cost equals cost")
    others = np.arange(len(lay["sfirst"])) != s0
    for f in PER_SLICE + HISTORY:
        bits(got[f][..., others], plain[f][..., others], "%s of the other slices" % f)
    for f in ("x",):
        keep = ~slice_mask(lay, s0)
        bits(got[f][keep], plain[f][keep], "x of the other slices")
    share = int((np.diff(lay["rowptr"])[rays] + 1).sum()), 3 * int(rays.sum())
    assert np.all(plain["state"] == hip.RET_MAXITER)
    assert np.array_equal(got["h_work"][:3], plain["h_work"][:3])
    assert tuple(plain["h_work"][3] - got["h_work"][3]) == share, "h_work drops by exactly that slice's share"


def test_convergence_ends_a_slice(hip):
    """With tol = 0.5 a slice ends at the first accepted step that lowers J by no more than half; eight iterations leave
    room for that (the first steps lower J by orders of magnitude, those near the minimum hardly at all)."""
    tol, mi = 0.5, 8
    lay = layout(hip, "ragged")[0]
    got = retrieved(hip, "ragged", 0, settings=dict(FLOW, tol=tol, max_iter=mi))
    J, Jt = got["h_cost"] + got["h_prior"], got["h_tcost"] + got["h_tprior"]
    seen = 0
    for s in range(len(got["state"])):
        ended = None
        for it in range(mi):
            if ended is not None:
                assert got["h_best"][it, s] == -1 and got["h_accept"][it, s] == -1 and np.all(np.isnan(got["h_lam"][it, :, s]))
                continue
            assert got["h_accept"][it, s] >= 0
            b = got["h_best"][it, s]
            if got["h_accept"][it, s] == 1 and J[it, s] - Jt[it, b, s] <= tol * J[it, s]:
                ended = it
        if ended is not None:
            seen += 1
            assert got["state"][s] == hip.RET_CONVERGED and got["iters"][s] == ended + 1
        else:
            assert got["state"][s] != hip.RET_CONVERGED
    assert seen > 0
    widths = np.diff(lay["rowptr"])
    for it in range(mi):                                                # the passes hold the rays of the slices that took part, no others
        took_part = got["h_accept"][it] >= 0
        rays = (lay["sid"] >= 0) & took_part[np.maximum(lay["sid"], 0)]
        assert tuple(got["h_work"][it]) == (int((widths[rays] + 1).sum()), 3 * int(rays.sum())), it
    assert got["h_work"][-1, 0] < got["h_work"][0, 0], "no slice ended before the last iteration"


# ---- 5. independence -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_independence(hip, mode):
    name = "ragged"
    case, geom, y, weight = inputs(hip, name)
    lay, iq, ip, x0 = layout(hip, name)
    ns = len(lay["sfirst"])
    batch = retrieved(hip, name, mode)
    prior = seeded_prior(hip, name, lay, x0) if mode == hip.DAMP_PRIOR else None
    s = dict(REPLAY)
    mi, fac = s.pop("max_iter"), s.pop("fac")
    model = hip.Model(case.ctl, case.lib_tables())

    def run(rays_kw, els, **kw):
        pk = dict(prior_ivar=prior[0][els], prior_xa=prior[1][els]) if prior else {}
        return model.retrieve_scene(case.atm, *rays_kw, mi, fac, mode=mode, history=True, **s, **pk, **kw)

    try:
        model.set_atm(case.atm)
        for cap in (1, 257):
            got = run((geom, y, weight), slice(None), max_rays_per_pass=cap)
            for f in HISTORY + ("x", "rad", "tau") + PER_SLICE:
                bits(got[f], batch[f], "%s, passes of %d" % (f, cap))
        for q in range(ns):
            rays = lay["sid"] == q
            sl = slice(lay["wptr"][q], lay["wptr"][q + 1])
            got = run((geom[rays], y[rays], weight[rays]), sl)
            bits(got["x"], batch["x"][sl], "x of slice %d alone" % q)
            for f in PER_SLICE + HISTORY:
                bits(got[f][..., 0], batch[f][..., q], "%s of slice %d alone" % (f, q))
        perm = interleaved(lay["sid"])
        assert not np.array_equal(perm, np.arange(len(perm)))
        dealt = hip.scene_slices(case.ctl, case.atm, geom[perm][:, 0])   # the slices in the order the dealt rays meet them
        order = [int(np.flatnonzero((lay["sfirst"] == f) & (lay["slen"] == l))[0]) for f, l in zip(dealt["sfirst"], dealt["slen"])]
        got = run((geom[perm], y[perm], weight[perm]), np.concatenate([np.arange(lay["wptr"][q], lay["wptr"][q + 1]) for q in order]))
        for j, q in enumerate(order):
            bits(got["x"][got["wptr"][j]:got["wptr"][j + 1]], batch["x"][lay["wptr"][q]:lay["wptr"][q + 1]], "x of slice %d, interleaved" % q)
            for f in PER_SLICE + HISTORY:
                bits(got[f][..., j], batch[f][..., q], "%s of slice %d, interleaved" % (f, q))
        bits(got["rad"], batch["rad"][perm], "rad, interleaved")
    finally:
        model.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_and_state(hip):
    name = "ragged"
    case, geom, y, weight = inputs(hip, name)
    lay, iq, ip, x0 = layout(hip, name)
    n = len(x0)
    want = fresh_formod(hip, case, case.atm, case.geom)
    ones = np.ones(n)
    ok = dict(max_iter=2, fac=(0.1, 1.0, 10.0))
    refused = [
        (dict(max_iter=0), r"max_iter = 0"),
        (dict(fac=()), r"nlam = 0"),
        (dict(fac=(2.0,) * 9), r"nlam = 9"),
        (dict(fac=(0.1, -1.0, 10.0)), r"fac\[1\] is -1"),
        (dict(fac=(0.0, 10.0)), r"fac\[0\] is 0"),
        (dict(fac=(np.inf, 10.0)), r"fac\[0\] is inf"),
        (dict(fac=(np.nan, 10.0)), r"fac\[0\] is nan"),
        (dict(fac=(0.1, 1.0)), r"no fac above 1"),
        (dict(lam_min=0.0), r"need 0 < lam_min <= lam0 <= lam_max"),
        (dict(lam0=1e-7), r"lam_min = 1e-06, lam0 = 1e-07"),
        (dict(lam0=1e7), r"need 0 < lam_min <= lam0 <= lam_max"),
        (dict(lam_max=np.inf), r"need 0 < lam_min <= lam0 <= lam_max"),
        (dict(tol=-1.0), r"tol is -1"),
        (dict(tol=np.nan), r"tol is nan"),
        (dict(prior_ivar=ones), r"prior_ivar without prior_xa"),
        (dict(prior_xa=x0), r"prior_xa without prior_ivar"),
        (dict(mode=hip.DAMP_PRIOR), r"JUR_DAMP_PRIOR without a prior"),
        (dict(mode=7), r"unknown mode 7"),
        (dict(history=("h_cost", "h_work")), r"2 of the 9 history arrays"),
    ]
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        for kw, message in refused:
            ret = copy_atm(case.atm)
            np.ctypeslib.as_array(ret.t)[:3] = -7.0                     # (a mark: atm_ret is written only on success)
            mark = copy_atm(ret)
            with pytest.raises(hip.JurassicError, match=r"error %d: jur_retrieve_scene_host: .*%s" % (hip.EINVAL, message)):
                model.retrieve_scene(case.atm, geom, y, weight, **dict(ok, **kw), atm_ret=ret)
            same_atm(hip, ret, mark)
            sequences.same_bits(formod_on(model, case.geom), want, "after the refusal '%s'" % message)
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_trial_scene_host: .*ntrial = 65" % hip.EINVAL):
            model.trial_scene(case.atm, geom, y, weight, np.zeros((65, n)))
        bad = np.zeros((2, n))
        bad[1, lay["wptr"][1] + 2] = np.inf
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_trial_scene_host: dx of trial 1, slice 1, element 2 is inf" % hip.EINVAL):
            model.trial_scene(case.atm, geom, y, weight, bad)
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_trial_scene_host: prior_xa without prior_ivar" % hip.EINVAL):
            model.trial_scene(case.atm, geom, y, weight, np.zeros(n), prior_xa=x0)
        sequences.same_bits(formod_on(model, case.geom), want, "after the trial refusals")
        in_place = copy_atm(case.atm)                                   # atm_ret may be atm0 itself
        got = model.retrieve_scene(in_place, geom, y, weight, **ok, atm_ret=in_place)
        bits(state_of(case, in_place, iq, ip), got["x"], "retrieved in place")
        assert np.any(got["x"] != x0)
    finally:
        model.close()

    hyd, _ = R.jacobian_case("jacobian_hydz10")
    want = fresh_formod(hip, hyd, hyd.atm, hyd.geom)
    model = hip.Model(hyd.ctl, hyd.lib_tables())
    try:
        model.set_atm(hyd.atm)
        shape = (len(hyd.geom), hyd.ctl.nd)
        ret = copy_atm(hyd.atm)
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_retrieve_scene_host: hydz" % hip.EINVAL):
            model.retrieve_scene(hyd.atm, hyd.geom, np.zeros(shape), np.ones(shape), **ok, atm_ret=ret)
        same_atm(hip, ret, hyd.atm)
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_trial_scene_host: hydz" % hip.EINVAL):
            model.trial_scene(hyd.atm, hyd.geom, np.zeros(shape), np.ones(shape),
                              np.zeros(int(hip.scene_slices(hyd.ctl, hyd.atm, hyd.geom[:, 0])["wptr"][-1])))
        sequences.same_bits(formod_on(model, hyd.geom), want, "after the hydz refusals")
    finally:
        model.close()


def test_trial_copies_beyond_the_budget_are_refused(hip):
    """The construction of test_scene_solve_gpu.py::test_solver_scratch_beyond_the_budget_is_refused.  There the loop is
    refused as the step is (its iteration is that entry's body).  The trial entry alone stacks ntrial copies of a slice,
    not one per element: with a profile of 9000 levels, 64 trials need 64 x 9000 points of 6 + ng + nw rows and the
    pressure slopes, more than half of the smallest budget (32 MiB of 64), one trial does not: the first is refused with
    JUR_ENOMEM before anything is launched, the second runs, and the model answers as a fresh one."""
    case = common.limb_case()
    c = case.ctl
    spec = [synth._spec(0.0, 10.0, 45.0, 140, 0.0, 90.0), synth._spec(1.0, 20.0, 30.0, 20, 0.0, 60.0)]
    small = synth.ragged_atmosphere(c, spec, seed=0, base=case.atm, order=None)
    c.retp_zmin, c.retp_zmax, c.rett_zmin, c.rett_zmax = -10.0, 100.0, -10.0, 100.0
    for g in range(c.ng):
        c.retq_zmin[g], c.retq_zmax[g] = -10.0, 100.0
    c.retk_zmin[0], c.retk_zmax[0] = -10.0, 100.0
    geom = case.geom[:2].copy()
    geom[:, 0] = 0.0
    y, weight = np.zeros((2, c.nd)), np.ones((2, c.nd))
    want = fresh_formod(hip, case, small, geom)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_workspace_budget(64 << 20)
        model.set_atm(small)
        ret = copy_atm(small)
        with pytest.raises(hip.JurassicError, match=r"error -3: jur_retrieve_scene_host: .*solver scratch"):
            model.retrieve_scene(small, geom, y, weight, 2, (0.1, 10.0), atm_ret=ret)
        same_atm(hip, ret, small)
        sequences.same_bits(formod_on(model, geom), want, "after the loop's refusal")
    finally:
        model.close()

    c.retp_zmin, c.retp_zmax, c.rett_zmin, c.rett_zmax = 20.0, 20.5, 20.0, 20.5     # a narrow state: dx stays small
    for g in range(c.ng):
        c.retq_zmin[g], c.retq_zmax[g] = -999.0, -999.0
    c.retk_zmin[0], c.retk_zmax[0] = -999.0, -999.0
    spec = [synth._spec(0.0, 10.0, 45.0, 9000, 0.0, 90.0), synth._spec(1.0, 20.0, 30.0, 20, 0.0, 60.0)]
    tall = synth.ragged_atmosphere(c, spec, seed=0, base=case.atm, order=None)
    want = fresh_formod(hip, case, tall, geom)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_workspace_budget(64 << 20)
        model.set_atm(tall)
        lay = hip.scene_slices(c, tall, geom[:, 0])
        n = int(lay["wptr"][-1])
        assert len(lay["slen"]) == 1 and lay["slen"][0] == 9000 and 0 < n < 400
        point = 8 * (7 + c.ng + c.nw)
        half = (64 << 20) // 2
        assert point * (tall.np + 9000) + (1 << 20) < half < point * (tall.np + 64 * 9000)
        with pytest.raises(hip.JurassicError, match=r"error -3: jur_trial_scene_host: the trial copies \(585020 points"):
            model.trial_scene(tall, geom, y, weight, np.zeros((64, n)))
        sequences.same_bits(formod_on(model, geom), want, "after the trial refusal")
        one = model.trial_scene(tall, geom, y, weight, np.zeros((1, n)))
        two = model.trial_scene(tall, geom, y, weight, np.zeros((2, n)), max_rays_per_pass=1)
    finally:
        model.close()
    bits(two["cost"], np.vstack([one["cost"], one["cost"]]), "the tall profile: two trials in passes of one ray against one trial")
    # y = 0 and weight = 1: the cost is the sum of the m = 2 nd squared radiances.  All terms are positive, so a sum of
    # them in any order, each term rounded at most twice, is within gamma_{m+2} of the exact one (Higham, section 4.2);
    # twice that is allowed against the sum in np.longdouble
    m = 2 * c.nd
    exact = float((want["rad"].astype(np.longdouble) ** 2).sum())
    assert exact > 0 and abs(one["cost"][0, 0] - exact) <= 2 * (m + 2) * 2.0 ** -53 * exact
