"""The scene Jacobian reused between the iterations of Model.retrieve_scene (Model.set_kernel_recomp, upstream's
KERNEL_RECOMP) and the entry a reuse iteration is made of, Model.gradient_scene (jur_gradient_scene_host,
jur_scene_gradient_kernel).

The yardstick is the project's own merged entries.  The gradient is held to Model.normal_scene bit for bit where the
blocks are that atmosphere's own, and to the float64 chain of include/jurassic_hip.h written out here where they are
another's.  The loop is held to a replay on the host: Jacobian iterations are step_scene (A and the blocks are kept),
reuse iterations are gradient_scene on the kept blocks of the rays that remain followed by solve_slices on the kept A;
trial costs, the prior chain, retrieve_decide and the write-back are those of tests/test_scene_retrieve_gpu.py."""
from fractions import Fraction
import math
import numpy as np
import pytest
import common
import sequences
from jurassic_hip import synth
from test_scene_jacobian_gpu import bits, formod_on, fresh_formod, scene_case, six_per_time_stamp
from test_scene_normal_gpu import bumped, copy_atm, inputs, interleaved
from test_scene_retrieve_gpu import (FLOW, HISTORY, PER_SLICE, REPLAY, SCENES, layout, prior_chain, retrieved, same_atm, seeded_prior,
                                     slice_mask, state_of, written_back)
import test_scene_retrieve_gpu as T
import test_scene_fov_gpu as F
import test_scene_hydro_gpu as H
import test_prior_full_gpu as P
from test_scene_recut_gpu import grown, recuts, searched_cap, stalled_inputs

pytestmark = pytest.mark.gpu
COMPARED = HISTORY + ("h_work", "x") + PER_SLICE
STALL = dict(FLOW, lam0=10.0)           # lam 10 -> 100 = lam_max: a slice that cannot move ends in iteration 1 (test_scene_fov_gpu.py's settings)


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def fma(a, b, c):
    """a * b + c rounded once.  Without math.fma (Python < 3.13) the sum is formed exactly in rationals; float() of a
    Fraction is an integer true division, which CPython rounds correctly (to nearest, ties to even): the same double."""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def blocks_of(k, rowptr, nd, rays):
    """the flat blocks of the rays `rays` (indices) out of the flat blocks of a call laid out by rowptr"""
    parts = [k[rowptr[r] * nd:rowptr[r + 1] * nd] for r in rays]
    return np.concatenate(parts) if parts else np.zeros(0)


# ---- 1. the gradient against the normal equations ------------------------------------------------------------------------
def masked(hip, name):
    """the scene's inputs with some input radiances and some y NaN and some weights 0, each in every slice"""
    case, geom, y, weight = inputs(hip, name)
    rng = np.random.default_rng(17)
    rad_in, y2, w2 = np.zeros(y.shape), y.copy(), weight.copy()
    rad_in[rng.random(y.shape) < 0.05] = np.nan
    y2[rng.random(y.shape) < 0.05] = np.nan
    w2[rng.random(y.shape) < 0.05] = 0.0
    assert np.isnan(rad_in).any() and np.isnan(y2).any() and (w2 == 0).any()
    return case, geom, y2, w2, rad_in


@pytest.mark.parametrize("name", SCENES)
def test_gradient_against_the_normal_equations(hip, name):
    case, geom, y, weight, rad_in = masked(hip, name)
    lay = layout(hip, name)[0]
    nd, ns = y.shape[1], len(lay["sfirst"])
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        nm = model.normal_scene(case.atm, geom, y, weight, rad_in=rad_in)
        k = model.kernel_scene(case.atm, geom, rad_in=rad_in)["k"]
        assert np.isnan(k).any(), "masked channels hold NaN in the blocks"
        got = model.gradient_scene(case.atm, geom, y, weight, k, rad_in=rad_in)
        assert "A" not in got and np.all(nm["nlive"] > 0) and np.any(nm["b"] != 0)
        for f in ("b", "cost", "nlive", "rad", "tau", "tp", "np"):
            bits(got[f], nm[f], f)
        sequences.same_bits(formod_on(model, case.geom), fresh_formod(hip, case, case.atm, case.geom), "the model holds atm afterwards")
        for cap in (1, 257):
            capped = model.gradient_scene(case.atm, geom, y, weight, k, rad_in=rad_in, max_rays_per_pass=cap)
            for f in ("b", "cost", "nlive", "rad", "tau", "tp", "np"):
                bits(capped[f], nm[f], "%s, passes of %d rays" % (f, cap))
        for s in range(ns):
            rays = np.flatnonzero(lay["sid"] == s)
            alone = model.gradient_scene(case.atm, geom[rays], y[rays], weight[rays], blocks_of(k, lay["rowptr"], nd, rays), rad_in=rad_in[rays])
            bits(alone["b"], nm["b"][lay["wptr"][s]:lay["wptr"][s + 1]], "b of slice %d's rays alone" % s)
            bits(alone["cost"][0], nm["cost"][s], "cost of slice %d's rays alone" % s)
            assert alone["nlive"][0] == nm["nlive"][s]
        # blocks of another atmosphere: nothing but the chain the header states can be the yardstick
        model.set_atm(bumped(case))
        other = model.kernel_scene(bumped(case), geom, rad_in=rad_in)["k"]
        model.set_atm(case.atm)
        assert np.any(other[~np.isnan(other)] != k[~np.isnan(k)])
        got = model.gradient_scene(case.atm, geom, y, weight, other, rad_in=rad_in)
        for f in ("cost", "nlive", "rad", "tau", "tp", "np"):
            bits(got[f], nm[f], "%s with the blocks of another atmosphere" % f)
    finally:
        model.close()
    want = np.zeros(len(got["b"]))
    F_, live = got["rad"], np.isfinite(rad_in) & np.isfinite(got["rad"]) & np.isfinite(y) & (weight > 0)
    for s in range(ns):
        w0, w = int(lay["wptr"][s]), int(lay["wptr"][s + 1] - lay["wptr"][s])
        acc = [0.0] * w
        for r in np.flatnonzero(lay["sid"] == s):
            K = other[lay["rowptr"][r] * nd:lay["rowptr"][r + 1] * nd].reshape(nd, w)
            for i_d in range(nd):
                if not live[r, i_d]:
                    continue
                d = float(y[r, i_d]) - float(F_[r, i_d])
                wd = float(weight[r, i_d]) * d
                row = K[i_d]
                for i in range(w):
                    acc[i] = fma(float(row[i]), wd, acc[i])
        want[w0:w0 + w] = acc
    bits(got["b"], want, "b against the chain in float64")
    assert np.any(want != nm["b"])


def all_levels(c):
    """p and T on every level: a slice of 150 levels has 300 elements, more than the 256 lanes of a workgroup"""
    c.retp_zmin, c.retp_zmax, c.rett_zmin, c.rett_zmax = -10.0, 1000.0, -10.0, 1000.0
    for g in range(c.ng):
        c.retq_zmin[g], c.retq_zmax[g] = -999.0, -999.0
    c.retk_zmin[0], c.retk_zmax[0] = -999.0, -999.0


def test_slices_wider_than_a_workgroup(hip):
    """jur_scene_gradient_kernel gives a slice one workgroup per 256 elements: widths below 256, of 257 to 511 (a second,
    partly filled workgroup; the first alone carries cost and nlive) and the slice of two levels, in one call and in
    passes of one ray"""
    case = scene_case("ragged", windows=all_levels)
    geom = six_per_time_stamp(case.geom)
    y = fresh_formod(hip, case, bumped(case), geom)["rad"]
    weight = 10.0 ** np.random.default_rng(11).uniform(0.0, 3.0, y.shape)
    lay = hip.scene_slices(case.ctl, case.atm, geom[:, 0])
    widths = np.diff(lay["wptr"])
    assert 256 < widths.max() < 512 and widths.min() < 256 and (widths > 256).sum() >= 1
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        nm = model.normal_scene(case.atm, geom, y, weight, want_k=True)
        assert np.all(nm["nlive"] > 0) and all(np.any(nm["b"][a:b] != 0) for a, b in zip(lay["wptr"][:-1], lay["wptr"][1:]))
        for cap in (0, 1):
            got = model.gradient_scene(case.atm, geom, y, weight, nm["k"], max_rays_per_pass=cap)
            for f in ("b", "cost", "nlive", "rad", "tau", "tp", "np"):
                bits(got[f], nm[f], "%s, cap %d" % (f, cap))
    finally:
        model.close()


# ---- 2. the loop against a replay on the host ----------------------------------------------------------------------------
def scene_T(hip, name):
    case, geom, y, weight = inputs(hip, name)
    lay, iq, ip, _ = layout(hip, name)
    return case, geom, y, weight, lay, iq, ip


def replay(hip, model, sc, settings, every, mode=0, prior=None, balance=None, via_trial=False):
    """The loop of jur_retrieve_scene_host with the Jacobian recomputed every `every`-th iteration, over the merged
    entries of `model` (its switches set by the caller).  balance: what makes a written-back atmosphere the state (the
    hydrostatic balance), or None.  via_trial: the trial costs and the prior terms from trial_scene (as the replays of the
    field of view and of the full prior precision take them) instead of normal_scene on every written-back atmosphere
    and the chain in float64 scalars."""
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
    kept_A, kept_k, regathered_reuse = {}, {}, 0
    last_active = None
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
            step = model.step_scene(atm, geom[rays], y[rays], weight[rays], lamt[:, full_of], mode=mode, want_normal=True, want_k=True, **kw)
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
            regathered_reuse += last_active is not None and not np.array_equal(active, last_active)
        if it % every == 0:
            last_active = active.copy()
        dx = np.zeros((nlam, len(x)))
        dx[:, els] = sdx
        tcost, tpri, status = np.zeros((nlam, ns)), np.zeros((nlam, ns)), np.zeros((nlam, ns), dtype=np.int32)
        status[:, full_of] = sstatus
        if via_trial:
            tk = dict(prior_ivar=r[els], prior_xa=xa[els]) if prior else {}
            trial = model.trial_scene(atm, geom[rays], y[rays], weight[rays], sdx, **tk)
            base = model.trial_scene(atm, geom[rays], y[rays], weight[rays], np.zeros(len(els)), **tk)
            tcost[:, full_of], tpri[:, full_of] = trial["cost"], trial["prior"]
        else:
            for l in range(nlam):
                trial = written_back(case, atm, iq, ip, dx[l])
                model.set_atm(trial)
                tcost[l, full_of] = model.normal_scene(trial, geom[rays], y[rays], weight[rays])["cost"]
        for j, s in enumerate(full_of):
            sl = slice(wptr[s], wptr[s + 1])
            cost[s], nlive[s], iters[s] = scost[j], snlive[j], iters[s] + 1
            if via_trial:
                pri[s] = base["prior"][0, j]
            else:
                pri[s] = prior_chain(r[sl], xa[sl], x[sl]) if prior else 0.0
                for l in range(nlam):
                    tpri[l, s] = prior_chain(r[sl], xa[sl], x[sl], dx[l][sl]) if prior else 0.0
        h["h_cost"][it], h["h_prior"][it] = cost, pri
        for f, v in (("h_lam", lamt), ("h_tcost", tcost), ("h_tprior", tpri), ("h_status", status)):
            h[f][it][:, active] = v[:, active]
        h["h_work"][it] = work, nlam * rays.sum()
        d = hip.retrieve_decide(cost + pri, tcost + tpri, lamt, status, lam, state, settings["tol"], settings["lam_max"], fac.max())
        lam, state = d["lam"], d["state"]
        h["h_best"][it], h["h_accept"][it] = d["best"], d["accept"]
        for s in np.flatnonzero(d["accept"] == 1):
            b = d["best"][s]
            atm = written_back(case, atm, iq, ip, dx[b], only=slice_mask(lay, s))
            cost[s], pri[s] = tcost[b, s], tpri[b, s]
        if balance:
            atm = balance(atm)
    state[state == hip.RET_ACTIVE] = hip.RET_MAXITER
    return dict(h, x=state_of(case, atm, iq, ip), atm=atm, lam=lam, cost=cost.copy(), prior=pri.copy(), nlive=nlive, state=state, iters=iters,
                regathered_reuse=regathered_reuse)


def run(model, sc, settings, every, mode=0, prior=None, **kw):
    """retrieve_scene with full history under set_kernel_recomp(every)"""
    case, geom, y, weight = sc[:4]
    s = dict(settings)
    pk = dict(prior_ivar=prior[0], prior_xa=prior[1]) if prior else {}
    model.set_kernel_recomp(every)
    assert model.kernel_recomp() == every
    return model.retrieve_scene(case.atm, kw.pop("geom", geom), kw.pop("y", y), kw.pop("weight", weight), s.pop("max_iter"), s.pop("fac"),
                                mode=mode, history=True, **s, **pk, **kw)


def check_loop(hip, sc, got, want, after):
    case, geom, iq, ip = sc[0], sc[1], sc[5], sc[6]
    for f in COMPARED:
        bits(got[f], want[f], f)
    same_atm(hip, got["atm"], want["atm"])
    bits(state_of(case, got["atm"], iq, ip), got["x"], "atm_ret holds x")
    fresh = fresh_formod(hip, case, got["atm"], geom)
    for f in ("rad", "tau", "tp", "np"):
        bits(got[f], fresh[f], "%s against a fresh model on atm_ret" % f)
    sequences.same_bits(after, fresh_formod(hip, case, got["atm"], case.geom), "the model holds atm_ret")


@pytest.mark.parametrize("every", [2, 3, 4])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", SCENES)
def test_replay_on_the_host(hip, name, mode, every):
    sc = scene_T(hip, name)
    case, lay = sc[0], sc[4]
    prior = seeded_prior(hip, name, lay, layout(hip, name)[3]) if mode == hip.DAMP_PRIOR else None
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        got = run(model, sc, REPLAY, every, mode, prior)
        after = formod_on(model, case.geom)
        want = replay(hip, model, sc, REPLAY, every, mode, prior)
    finally:
        model.close()
    check_loop(hip, sc, got, want, after)
    assert np.all(got["h_status"][0] == 0) and np.any(got["h_accept"] == 1)


@pytest.mark.parametrize("every", [2, 3, 4])
def test_replay_with_a_slice_that_ends_before_a_reuse_iteration(hip, every):
    """Slice 1 cannot move (its y is the forward model on the first guess): under STALL it ends in iteration 1.  With
    every = 3 and 4 iteration 2 (and 3) is a reuse iteration on rays gathered anew: they find their blocks where iteration
    0 left them, among those of the slice that has gone.  With every = 2 iteration 2 recomputes the Jacobian on the rays
    that remain and iteration 3 reuses blocks written in that order."""
    case, geom, y2, weight, _ = stalled_inputs(hip)
    lay, iq, ip, _ = layout(hip, "ragged")
    sc = (case, geom, y2, weight, lay, iq, ip)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        got = run(model, sc, STALL, every)
        after = formod_on(model, case.geom)
        want = replay(hip, model, sc, STALL, every)
    finally:
        model.close()
    check_loop(hip, sc, got, want, after)
    assert got["state"][1] == hip.RET_STALLED and got["iters"][1] == 2, "the slice ended in iteration 1"
    assert 0 < np.flatnonzero(lay["sid"] == 1)[0] and np.flatnonzero(lay["sid"] == 1)[-1] < len(geom) - 1, "rays before and after those that left"
    assert (want["regathered_reuse"] >= 1) == (every > 2), "a reuse iteration ran on fewer slices than the Jacobian iteration before it"


# ---- 3. switched off it is today's loop ----------------------------------------------------------------------------------
def test_switched_off_is_the_loop_as_it_was(hip):
    name = "ragged"
    sc = scene_T(hip, name)
    case = sc[0]
    batch = retrieved(hip, name, 0)                                     # a fresh model that was never told
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        assert model.kernel_recomp() == 1
        model.set_atm(case.atm)
        model.formod_host(case.geom)
        before = model.workspace_bytes()
        model.set_kernel_recomp(3)
        assert model.workspace_bytes() == before, "the switch alone allocates nothing"
        model.set_kernel_recomp(1)
        first = run(model, sc, REPLAY, 1)                               # set to 1 on a used model
        other = run(model, sc, REPLAY, 3)
        again = run(model, sc, REPLAY, 1)                               # and back to 1 after a run with 3
    finally:
        model.close()
    for f in COMPARED + ("rad", "tau", "tp", "np"):
        bits(first[f], batch[f], "%s, set to 1" % f)
        bits(again[f], batch[f], "%s, back to 1" % f)
    assert np.array_equal(other["h_work"][0], batch["h_work"][0]) and other["h_work"][1, 0] < batch["h_work"][1, 0]


# ---- 4. independence -------------------------------------------------------------------------------------------------------
def test_independence(hip):
    """every = 2 with a slice that ends in iteration 1 (STALL): no result of a slice depends on max_rays_per_pass -- the
    caps are 1, 257 and the one tests/test_scene_recut_gpu.py searches for, under which a re-cut pass exceeds the first
    cut --, on the order of the rays or on the presence of the other slices."""
    case, geom, y2, weight, _ = stalled_inputs(hip)
    lay, iq, ip, _ = layout(hip, "ragged")
    sc = (case, geom, y2, weight, lay, iq, ip)
    ns, nlam = len(lay["sfirst"]), len(STALL["fac"])
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        batch = run(model, sc, STALL, 2)
        assert batch["state"][1] == hip.RET_STALLED and len(recuts(batch)) >= 1
        cap = searched_cap(hip, batch, nlam)
        assert cap is not None and grown(hip, batch, nlam, cap) >= 1, "no cap makes a re-cut pass exceed the first cut"
        for c in (1, 257, cap):
            got = run(model, sc, STALL, 2, max_rays_per_pass=c)
            for f in COMPARED + ("rad", "tau", "tp", "np"):
                bits(got[f], batch[f], "%s, passes of %d" % (f, c))
        for q in range(ns):
            rays = lay["sid"] == q
            sl = slice(lay["wptr"][q], lay["wptr"][q + 1])
            got = run(model, sc, STALL, 2, geom=geom[rays], y=y2[rays], weight=weight[rays])
            bits(got["x"], batch["x"][sl], "x of slice %d alone" % q)
            for f in PER_SLICE + HISTORY:
                bits(got[f][..., 0], batch[f][..., q], "%s of slice %d alone" % (f, q))
        perm = interleaved(lay["sid"])
        assert not np.array_equal(perm, np.arange(len(perm)))
        dealt = hip.scene_slices(case.ctl, case.atm, geom[perm][:, 0])
        order = [int(np.flatnonzero((lay["sfirst"] == f) & (lay["slen"] == l))[0]) for f, l in zip(dealt["sfirst"], dealt["slen"])]
        got = run(model, sc, STALL, 2, geom=geom[perm], y=y2[perm], weight=weight[perm])
        for j, q in enumerate(order):
            bits(got["x"][got["wptr"][j]:got["wptr"][j + 1]], batch["x"][lay["wptr"][q]:lay["wptr"][q + 1]], "x of slice %d, interleaved" % q)
            for f in PER_SLICE + HISTORY:
                bits(got[f][..., j], batch[f][..., q], "%s of slice %d, interleaved" % (f, q))
        bits(got["rad"], batch["rad"][perm], "rad, interleaved")
    finally:
        model.close()


# ---- 5. beside the model's other switches ----------------------------------------------------------------------------------
def test_beside_a_field_of_view(hip):
    """the scene, the shape and the settings of tests/test_scene_fov_gpu.py (slice 1 stalls in iteration 1, a reuse
    iteration); the retained blocks are the convolved ones"""
    case, geom, y, weight, lay, iq, ip, x0 = F.scene(hip)
    prior = F.seeded_prior(hip)
    y2 = y.copy()
    y2[lay["sid"] == 1] = F.convolved(hip, case, case.atm, geom)["rad"][lay["sid"] == 1]
    sc = (case, geom, y2, weight, lay, iq, ip)
    model = F.with_shape(hip, case)
    try:
        got = run(model, sc, F.SETTINGS, 2, prior=prior)
        small = run(model, sc, F.SETTINGS, 2, prior=prior, max_rays_per_pass=1)
        want = replay(hip, model, sc, F.SETTINGS, 2, prior=prior, via_trial=True)
    finally:
        model.close()
    for f in COMPARED:
        bits(got[f], want[f], f)
        bits(small[f], got[f], "%s, a scan per pass" % f)
    assert got["state"][1] == hip.RET_STALLED and np.any(got["h_accept"] == 1)
    final = F.convolved(hip, case, got["atm"], geom)
    for f in ("rad", "tau"):
        bits(got[f], final[f], "%s against formod_host + fov_apply on atm_ret" % f)


def test_beside_the_hydrostatic_balance(hip):
    """the scene, the reference level and the settings of tests/test_scene_hydro_gpu.py"""
    name = "ragged"
    case, geom, y, weight, lay, iq, ip = H.scene(hip, name)
    prior = H.diagonal_prior(hip, name)
    sc = (case, geom, y, weight, lay, iq, ip)
    on = H.switched_on(hip, case)
    try:
        got = run(on, sc, H.SETTINGS, 2, prior=prior)
        want = replay(hip, on, sc, H.SETTINGS, 2, prior=prior, balance=lambda a: on.scene_hydrostatic(a, geom[:, 0]), via_trial=True)
    finally:
        on.close()
    for f in COMPARED:
        bits(got[f], want[f], f)
    assert np.any(got["h_accept"] == 1)
    bits(H.p_of(got["atm"]), H.p_of(want["atm"]), "atm_ret.p is B of the written-back state")
    fresh = fresh_formod(hip, case, got["atm"], geom)
    for f in ("rad", "tau", "tp", "np"):
        bits(got[f], fresh[f], "%s against a fresh model on atm_ret" % f)


@pytest.mark.parametrize("mode", [0, 1])
def test_beside_a_full_prior_precision(hip, mode):
    """the scene and the precision of tests/test_prior_full_gpu.py; no slice ends, so solve_slices of the replay presents
    the precision as it is set"""
    name = "ragged"
    sc = scene_T(hip, name)
    case, lay = sc[0], sc[4]
    pc, r, xa = P.scene_prior(hip, name)
    settings = dict(REPLAY, max_iter=3)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        model.set_prior_precision(lay["wptr"], pc["R"])
        got = run(model, sc, settings, 2, mode, (r, xa))
        want = replay(hip, model, sc, settings, 2, mode, (r, xa), via_trial=True)
    finally:
        model.close()
    assert np.all(got["state"] == hip.RET_MAXITER) and np.all(got["iters"] == 3), "no slice ended"
    for f in COMPARED:
        bits(got[f], want[f], f)
    same_atm(hip, got["atm"], want["atm"])
    assert np.any(got["h_accept"][1] == 1) and np.all(got["prior"] > 0)


# ---- 6. work and descent ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [2, 4])
def test_work_and_descent(hip, every):
    """the scene and the settings of tests/test_scene_retrieve_gpu.py::test_descent"""
    sc = scene_T(hip, "ragged")
    case, lay = sc[0], sc[4]
    widths = np.diff(lay["rowptr"])
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        got = run(model, sc, REPLAY, every)
    finally:
        model.close()
    nlam = len(REPLAY["fac"])
    reuse_accepts = 0
    for it in range(REPLAY["max_iter"]):
        part = got["h_accept"][it] >= 0
        rays = (lay["sid"] >= 0) & part[np.maximum(lay["sid"], 0)]
        traced = int(rays.sum()) if it % every else int((widths[rays] + 1).sum())
        assert tuple(got["h_work"][it]) == (traced, nlam * int(rays.sum())), it
        if it % every:
            reuse_accepts += int((got["h_accept"][it] == 1).sum())
    J = got["h_cost"] + got["h_prior"]
    final = got["cost"] + got["prior"]
    assert np.all(np.diff(np.vstack([J, final[None, :]]), axis=0) <= 0), "J never rises for any slice"
    assert reuse_accepts > 0, "no reuse iteration accepted a step"
    print("RECOMP every %d: sum J after / before %.4e, %d steps accepted in reuse iterations, rays traced %s"
          % (every, final.sum() / J[0].sum(), reuse_accepts, got["h_work"][:, 0].tolist()))


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_and_state(hip):
    sc = scene_T(hip, "ragged")
    case, geom, y, weight = sc[:4]
    want = fresh_formod(hip, case, case.atm, case.geom)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        model.set_kernel_recomp(2)
        for bad in (0, -1):
            with pytest.raises(hip.JurassicError, match=r"error %d: jur_model_set_kernel_recomp: every is %d" % (hip.EINVAL, bad)):
                model.set_kernel_recomp(bad)
            assert model.kernel_recomp() == 2                           # what was set stays set
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_gradient_scene_host: null argument \(k\)" % hip.EINVAL):
            model.gradient_scene(case.atm, geom, y, weight, None)
        sequences.same_bits(formod_on(model, case.geom), want, "after the refusals")
        wrong = layout(hip, "ragged")[0]["rowptr"].copy()
        k0 = np.zeros(int(wrong[-1]) * y.shape[1])
        wrong[len(wrong) // 2:] += 1
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_gradient_scene_host: rowptr" % hip.EINVAL):
            model.gradient_scene(case.atm, geom, y, weight, k0, rowptr=wrong)
        w2 = weight.copy()
        w2[3, 0] = -1.0
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_gradient_scene_host: the weight of ray 3, channel 0 is -1" % hip.EINVAL):
            model.gradient_scene(case.atm, geom, y, w2, k0)
        sequences.same_bits(formod_on(model, case.geom), want, "after the refusals of normal_scene")
    finally:
        model.close()


def test_blocks_beyond_the_budget_are_refused(hip):
    """One profile of 140 levels with every quantity retrieved on all of them (the construction of
    tests/test_scene_retrieve_gpu.py::test_trial_copies_beyond_the_budget_are_refused) and as many rays as make the blocks
    of all rays, rowptr[nr] * nd doubles, larger than half of the smallest budget (32 MiB of 64) by themselves: the
    gradient entry, and the loop with the switch on, are refused with JUR_ENOMEM before anything is launched, and the
    model answers as a fresh one."""
    case = common.limb_case()
    c = case.ctl
    spec = [synth._spec(0.0, 10.0, 45.0, 140, 0.0, 90.0), synth._spec(1.0, 20.0, 30.0, 20, 0.0, 60.0)]
    c.retp_zmin, c.retp_zmax, c.rett_zmin, c.rett_zmax = -10.0, 100.0, -10.0, 100.0
    for g in range(c.ng):
        c.retq_zmin[g], c.retq_zmax[g] = -999.0, -999.0
    c.retk_zmin[0], c.retk_zmax[0] = -999.0, -999.0
    small = synth.ragged_atmosphere(c, spec, seed=0, base=case.atm, order=None)
    one = case.geom[:1].copy()
    one[:, 0] = 0.0
    w = int(hip.scene_layout(c, small, one[:, 0])["rowptr"][-1])
    half = (64 << 20) // 2
    nr = half // (8 * w * c.nd) + 1
    assert w >= 200 and 8 * nr * w * c.nd > half and nr < 20000
    geom = np.repeat(one, nr, axis=0)
    y, weight = np.zeros((nr, c.nd)), np.ones((nr, c.nd))
    probe = case.geom[:2].copy()
    probe[:, 0] = 0.0
    want = fresh_formod(hip, case, small, probe)
    model = hip.Model(c, case.lib_tables())
    try:
        model.set_workspace_budget(64 << 20)
        model.set_atm(small)
        with pytest.raises(hip.JurassicError, match=r"error -3: jur_gradient_scene_host: the blocks of all rays \(%d columns" % (nr * w)):
            model.gradient_scene(small, geom, y, weight, np.zeros(nr * w * c.nd))
        sequences.same_bits(formod_on(model, probe), want, "after the gradient's refusal")
        model.set_kernel_recomp(2)
        ret = copy_atm(small)
        with pytest.raises(hip.JurassicError, match=r"error -3: jur_retrieve_scene_host: the blocks of all rays \(%d columns" % (nr * w)):
            model.retrieve_scene(small, geom, y, weight, 2, (0.1, 10.0), atm_ret=ret)
        same_atm(hip, ret, small)
        sequences.same_bits(formod_on(model, probe), want, "after the loop's refusal")
    finally:
        model.close()
