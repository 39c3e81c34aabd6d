"""The full a-priori precision of the slices on the device: Model.set_prior_precision (jur_model_set_prior_precision),
prior_corr (jur_prior_corr_host) and what solve_slices, step_scene, trial_scene, retrieve_scene, diagnose_slices and
diagnose_scene compute while a precision is set: the prior is P = R + diag(prior_ivar) in place of diag(prior_ivar).

The error bounds are derived, not measured: those of tests/test_scene_solve_gpu.py and tests/test_scene_diagnose_gpu.py
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.; u = 2^-53, gamma_m = m u / (1 - m u)), widened by the
roundings the full prior adds.  With M = A + P + lam Z, g = b + P d and Z = diag(D) or P formed in np.longdouble:
  E_M = gamma_3 (|A| + |P| + lam |Z|) entrywise: P_ii = R_ii + r_i, A_ij + P_ij and the fma with lam, one rounding each
        (in place of the gamma_2 diag(M) of the diagonal prior);
  E_g = gamma_{w+2} (|b| + |P| |d|): a chain of w terms for (R d)_i in whatever order, fma(r_i, d_i, b_i), one addition;
  factor:   |M - L L^T| <= gamma_{n+1} |L| |L^T| + E_M
  solution: |g - M dx|  <= gamma_{3n+1} |L| |L^T| |dx| + E_M |dx| + E_g
  pred:     |pred - dx^T (g + lam Z dx)| <= gamma_{2n+6} (|dx|^T |g| + lam |dx|^T |Z| |dx|) + |dx|^T E_g: the sum of n
            terms of at most four roundings each, a chain of n terms for Z dx with the product by lam and the last sum.
  diagnostics: the bounds of test_scene_diagnose_gpu.py with E_M |S*| in place of gamma_2 diag(M) |S*| in the residual;
            T = S P is a product like AVK (E_T = gamma_n |S*| |P| + E_S |P|) and sigma_smooth^2 = sum_j T_ij S_ij a sum like
            sigma_noise^2.
  d^T P d (trial_scene's prior): d is formed in float64 as the device forms it; |got - d^T P d| <= gamma_{2w+8} |d|^T |P| |d|.
  Sa of prior_corr: (6 + 2 |dz| / cz) u relative: 3 ulp for exp (the OpenCL full-profile limit the device library is
            built to), the two roundings of its argument amplified by the argument, two products, one spare.
Twice each bound is allowed; the worst ratios are printed.  Everything else is bit identity.

A NaN cannot reach P: jur_model_set_prior_precision refuses an R that is not finite where it is read, and the entries
refuse a prior_ivar that is not finite.  The dead-element test therefore puts the NaN into A's dead row and 1e300 into
R's."""
import numpy as np
import pytest
import common
import sequences
from jurassic_hip import synth
from test_prior_full_cpu import exp_prior, exp_prior_inverse
from test_scene_jacobian_gpu import bits, formod_on, fresh_formod
from test_scene_normal_gpu import copy_atm, inputs, slice_of
from test_scene_solve_gpu import gamma, is_plus_zero, pack, spd, system
from test_scene_diagnose_gpu import VECTORS, check_system as check_diag, cholesky_ld, inverse_lower_ld, merged, report
from test_scene_diagnose_gpu import system as diag_system
import test_scene_retrieve_gpu as T

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
LD = np.longdouble
WIDTHS = (1, 2, 15, 16, 17, 63, 64, 65, 182, 300)
LAMS = (0.0, 1e-3, 10.0)
SCENES = ("ragged", "lone_ends")
DIAG_OUTS = VECTORS + ("dofs", "status", "S", "avk")


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


@pytest.fixture()
def model(hip):
    case = common.limb_case()
    m = hip.Model(case.ctl, case.lib_tables())
    yield m
    m.close()


def sym(a):
    """the symmetric matrix that is read: the diagonal and the lower triangle"""
    low = np.tril(a)
    return low + np.tril(low, -1).T


def seeded_R(rng, w):
    """H^T H of a seeded (w + 3) x w matrix times 10^U(-2, 1), its two triangles bit-identical"""
    H = rng.standard_normal((w + 3, w))
    return sym(H.T @ H * 10.0 ** rng.uniform(-2.0, 1.0))


def flat(mats):
    return np.concatenate([m.ravel() for m in mats]) if mats else np.zeros(0)


_batch = {}


def batch():
    if not _batch:
        rng = np.random.default_rng(2025)
        mats = [spd(rng, w) for w in WIDTHS]
        vecs = [rng.standard_normal(w) for w in WIDTHS]
        Rs = [seeded_R(rng, w) for w in WIDTHS]
        wptr, aptr, A, b = pack(mats, vecs)
        r = 10.0 ** rng.uniform(-2.0, 1.0, len(b))
        d = rng.standard_normal(len(b))
        _batch["v"] = (mats, vecs, Rs, wptr, aptr, A, b, r, d)
    return _batch["v"]


def check_solve(A, b, lam, mode, Rm, r, d, dx, pred, status, L):
    """the three bounds of the module docstring on the live elements, the exact properties on the dead ones; returns the
    worst error / allowed ratio"""
    w = len(b)
    with np.errstate(invalid="ignore"):
        live = (np.diag(A) + (np.diag(Rm) + r)) > 0
    n = int(live.sum())
    assert status == 0
    assert np.all(np.triu(L, 1) == 0) and np.all(np.diag(L) > 0)
    dead = np.flatnonzero(~live)
    assert is_plus_zero(dx[dead]) and np.all(np.diag(L)[dead] == 1)
    for i in dead:
        assert np.all(np.delete(L[i], i) == 0) and np.all(np.delete(L[:, i], i) == 0)
    if n == 0:
        assert pred == 0
        return 0.0
    ix = np.ix_(live, live)
    Al = sym(A).astype(LD)[ix]
    Pl = (sym(Rm).astype(LD) + np.diag(r.astype(LD)))[ix]
    dl, bl = d[live].astype(LD), b[live].astype(LD)
    Z = Pl if mode == 1 else np.diag(np.diag(Al) + np.diag(Pl))
    M = Al + Pl + LD(lam) * Z
    g = bl + Pl @ dl
    EM = gamma(3) * (np.abs(Al) + np.abs(Pl) + LD(lam) * np.abs(Z))
    Eg = gamma(w + 2) * (np.abs(bl) + np.abs(Pl) @ np.abs(dl))
    Ll, x = L[ix].astype(LD), dx[live].astype(LD)
    LLa = np.abs(Ll) @ np.abs(Ll).T
    ax = np.abs(x)
    worst = 0.0
    tiny = np.finfo(LD).tiny

    def within(err, bound, what):
        nonlocal worst
        worst = max(worst, float(np.max(err / np.maximum(2 * bound, tiny))))
        assert np.all(err <= 2 * bound), (what, w, lam, mode, float(np.max(err)), float(np.max(bound)))

    within(np.abs(M - Ll @ Ll.T), gamma(n + 1) * LLa + EM, "factor")
    within(np.abs(g - M @ x), gamma(3 * n + 1) * (LLa @ ax) + EM @ ax + Eg, "solution")
    want = x @ (g + LD(lam) * (Z @ x))
    within(np.abs(LD(pred) - want), gamma(2 * n + 6) * (ax @ np.abs(g) + LD(lam) * (ax @ (np.abs(Z) @ ax))) + ax @ Eg, "pred")
    return worst


# ---- 1. constructed systems ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_constructed_systems(hip, model, mode):
    mats, vecs, Rs, wptr, aptr, A, b, r, d = batch()
    bare = model.solve_slices(wptr, A, b, LAMS, mode=mode, prior_ivar=r, prior_dx=d, want_factor=True)
    model.set_prior_precision(wptr, flat(Rs))
    res = model.solve_slices(wptr, A, b, LAMS, mode=mode, prior_ivar=r, prior_dx=d, want_factor=True)
    assert np.all(res["status"] == 0)
    assert not np.array_equal(res["dx"], bare["dx"]), "the precision changes the step"
    worst = 0.0
    for l, lam in enumerate(LAMS):
        for s in range(len(WIDTHS)):
            sl = slice(wptr[s], wptr[s + 1])
            worst = max(worst, check_solve(mats[s], vecs[s], lam, mode, Rs[s], r[sl], d[sl], *system(res, wptr, aptr, l, s)))
    print("PRIOR solve constructed, mode %d: worst error / allowed %.3f" % (mode, worst))
    # a build that treated R's diagonal alone would miss the bounds: the off-diagonals of P carry most of |P|
    # R = 0 set explicitly: the bits of the call with nothing set
    model.set_prior_precision(wptr, np.zeros(int(aptr[-1])))
    zero = model.solve_slices(wptr, A, b, LAMS, mode=mode, prior_ivar=r, prior_dx=d, want_factor=True)
    for f in ("dx", "pred", "status", "L"):
        bits(zero[f], bare[f], "%s with R = 0 against no precision" % f)
    model.set_prior_precision(None)
    again = model.solve_slices(wptr, A, b, LAMS, mode=mode, prior_ivar=r, prior_dx=d, want_factor=True)
    for f in ("dx", "pred", "status", "L"):
        bits(again[f], bare[f], "%s after set_prior_precision(None)" % f)


# ---- 2. exact properties -------------------------------------------------------------------------------------------------
def test_dead_elements_and_breakdown(hip, model):
    rng = np.random.default_rng(6)
    w = 40
    A, Rm = spd(rng, w), seeded_R(rng, w)
    deads = (0, 16, 39)
    clean_A, clean_R = A.copy(), Rm.copy()
    for i in deads:
        for M, fill in ((A, np.nan), (Rm, 1e300), (clean_A, 0.0), (clean_R, 0.0)):
            M[i, :] = fill
            M[:, i] = fill
            M[i, i] = 0.0
    b, r, d = rng.standard_normal(w), 10.0 ** rng.uniform(-2, 1, w), rng.standard_normal(w)
    r[list(deads)] = 0.0
    for mode in (0, 1):
        model.set_prior_precision([0, w], Rm)
        got = model.solve_slices([0, w], A, b, LAMS, mode=mode, prior_ivar=r, prior_dx=d, want_factor=True)
        model.set_prior_precision([0, w], clean_R)
        want = model.solve_slices([0, w], clean_A, b, LAMS, mode=mode, prior_ivar=r, prior_dx=d, want_factor=True)
        assert np.all(got["status"] == 0)
        for f in ("dx", "pred", "L"):
            bits(got[f], want[f], "%s: a dead element's row and column never reach a live one (mode %d)" % (f, mode))
        for l, lam in enumerate(LAMS):
            check_solve(clean_A, b, lam, mode, clean_R, r, d, *system(got, np.array([0, w]), np.array([0, w * w]), l, 0))

    # an indefinite P between two good systems: status 2, zeros, and the neighbours as in their solo calls
    good = [(spd(rng, k), seeded_R(rng, k), rng.standard_normal(k)) for k in (17, 33)]
    mats = [good[0][0], np.zeros((2, 2)), good[1][0]]
    Rs = [good[0][1], np.array([[1.0, 2.0], [2.0, 1.0]]), good[1][1]]
    vecs = [good[0][2], np.ones(2), good[1][2]]
    wptr, aptr, Af, bf = pack(mats, vecs)
    zeros = np.zeros(len(bf))
    for mode in (0, 1):
        model.set_prior_precision(wptr, flat(Rs))
        res = model.solve_slices(wptr, Af, bf, LAMS, mode=mode, prior_ivar=zeros, prior_dx=zeros, want_factor=True)
        # (JUR_DAMP_MARQUARDT adds lam D to the diagonal alone: (1 + lam)^2 > 4 makes this matrix definite, so lam = 10 solves it)
        broken = [l for l, lam in enumerate(LAMS) if mode == 1 or (1 + lam) ** 2 < 4]
        assert len(broken) >= 2 and np.all(res["status"][broken, 1] == 2) and np.all(res["status"][:, [0, 2]] == 0)
        for l in broken:
            dx, pred, _, L = system(res, wptr, aptr, l, 1)
            assert is_plus_zero(dx) and is_plus_zero(pred) and is_plus_zero(L)
        for s in (0, 2):
            k = len(vecs[s])
            model.set_prior_precision([0, k], Rs[s])
            solo = model.solve_slices([0, k], mats[s], vecs[s], LAMS, mode=mode, prior_ivar=np.zeros(k), prior_dx=np.zeros(k), want_factor=True)
            for l in range(len(LAMS)):
                for a, c, what in zip(system(res, wptr, aptr, l, s), system(solo, np.array([0, k]), np.array([0, k * k]), l, 0), ("dx", "pred", "status", "L")):
                    bits(np.asarray(a), np.asarray(c), "%s of system %d beside a breakdown" % (what, s))


@pytest.mark.parametrize("mode", [0, 1])
def test_independence(hip, model, mode):
    mats, vecs, Rs, wptr, aptr, A, b, r, d = batch()
    model.set_prior_precision(wptr, flat(Rs))
    res = model.solve_slices(wptr, A, b, LAMS, mode=mode, prior_ivar=r, prior_dx=d, want_factor=True)
    # garbage above the diagonal of R: only the lower triangle is read
    rng = np.random.default_rng(9)
    dirty = []
    for Rm in Rs:
        G = Rm.copy()
        up = np.triu_indices(len(G), 1)
        G[up] = rng.standard_normal(len(up[0])) * 1e6
        if len(up[0]):
            G[up[0][0], up[1][0]] = np.nan
        dirty.append(G)
    model.set_prior_precision(wptr, flat(dirty))
    got = model.solve_slices(wptr, A, b, LAMS, mode=mode, prior_ivar=r, prior_dx=d, want_factor=True)
    for f in ("dx", "pred", "status", "L"):
        bits(got[f], res[f], "%s with garbage above the diagonal of R" % f)
    # another order, one damping, solo calls
    order = list(rng.permutation(len(WIDTHS)))
    w2, a2, A2, b2 = pack([mats[s] for s in order], [vecs[s] for s in order])
    els = np.concatenate([np.arange(wptr[s], wptr[s + 1]) for s in order])
    model.set_prior_precision(w2, flat([Rs[s] for s in order]))
    perm = model.solve_slices(w2, A2, b2, LAMS[1:2], mode=mode, prior_ivar=r[els], prior_dx=d[els], want_factor=True)
    for j, s in enumerate(order):
        for a, c, what in zip(system(perm, w2, a2, 0, j), system(res, wptr, aptr, 1, s), ("dx", "pred", "status", "L")):
            bits(np.asarray(a), np.asarray(c), "%s of system %d in another order, one damping" % (what, s))
    for s in (0, 4, 8):
        k = WIDTHS[s]
        sl = slice(wptr[s], wptr[s + 1])
        model.set_prior_precision([0, k], Rs[s])
        solo = model.solve_slices([0, k], mats[s], vecs[s], LAMS, mode=mode, prior_ivar=r[sl], prior_dx=d[sl], want_factor=True)
        for l in range(len(LAMS)):
            for a, c, what in zip(system(solo, np.array([0, k]), np.array([0, k * k]), l, 0), system(res, wptr, aptr, l, s), ("dx", "pred", "status", "L")):
                bits(np.asarray(a), np.asarray(c), "%s of system %d alone" % (what, s))


# ---- 3. the scene entries ------------------------------------------------------------------------------------------------
def scene_sigma(case):
    """1 % of p, 1 K, 10 % of a gas, 1e-4 / km of the extinction"""
    ng, nw = case.ctl.ng, case.ctl.nw
    return [lambda v: 0.01 * abs(v), 1.0] + [lambda v: 0.1 * abs(v)] * ng + [1e-4] * nw


_priors = {}


def scene_prior(hip, name):
    """(pc, r, xa) of a scene: prior_corr with cz = 5 km for every quantity, a small seeded diagonal part, xa near x0"""
    if name not in _priors:
        case, geom, y, weight = inputs(hip, name)
        lay, iq, ip, x0 = T.layout(hip, name)
        m = hip.Model(case.ctl, case.lib_tables())
        try:
            pc = hip.prior_corr(m, case.ctl, case.atm, geom[:, 0], scene_sigma(case), [5.0] * (2 + case.ctl.ng + case.ctl.nw))
        finally:
            m.close()
        assert np.all(pc["status"] == 0) and np.array_equal(pc["wptr"], lay["wptr"]) and np.array_equal(pc["aptr"], lay["aptr"])
        rng = np.random.default_rng(4)
        r = 1e-3 / pc["sigma"] ** 2 * 10.0 ** rng.uniform(-1.0, 1.0, len(x0))
        xa = x0 + 0.3 * pc["sigma"] * rng.standard_normal(len(x0))
        _priors[name] = (pc, r, xa)
    return _priors[name]


def form_bound(P, d):
    """d^T P d in longdouble and its bound"""
    P, d = P.astype(LD), d.astype(LD)
    return d @ (P @ d), gamma(2 * len(d) + 8) * (np.abs(d) @ (np.abs(P) @ np.abs(d)))


@pytest.mark.parametrize("name", SCENES)
def test_step_trial_and_diagnose_scene(hip, name):
    case, geom, y, weight = inputs(hip, name)
    lay, iq, ip, x0 = T.layout(hip, name)
    pc, r, xa = scene_prior(hip, name)
    wptr, aptr, ns, n = lay["wptr"], lay["aptr"], len(lay["sfirst"]), len(x0)
    want = fresh_formod(hip, case, case.atm, case.geom)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        model.set_prior_precision(wptr, pc["R"])
        got = model.prior_precision()
        bits(got["R"], pc["R"], "prior_precision returns what was set")
        assert np.array_equal(got["wptr"], wptr) and np.array_equal(got["aptr"], aptr)
        for mode in (0, 1):
            step = model.step_scene(case.atm, geom, y, weight, LAMS[1:], mode=mode, prior_ivar=r, prior_dx=xa - x0, want_normal=True,
                                    want_factor=True)
            sequences.same_bits(formod_on(model, case.geom), want, "after step_scene")
            half = model.solve_slices(wptr, step["A"], step["b"], LAMS[1:], mode=mode, prior_ivar=r, prior_dx=xa - x0, want_factor=True)
            assert np.all(step["status"] == 0)
            for f in ("dx", "pred", "status", "L"):
                bits(step[f], half[f], "%s of step_scene against normal_scene + solve_slices, mode %d" % (f, mode))
        dx = step["dx"]
        # the trial pass: the prior against the longdouble form, and bit-identical across ntrial and the passes
        trial = model.trial_scene(case.atm, geom, y, weight, dx, prior_ivar=r, prior_xa=xa)
        sequences.same_bits(formod_on(model, case.geom), want, "after trial_scene")
        worst = 0.0
        for t in range(len(dx)):
            for s in range(ns):
                sl = slice(wptr[s], wptr[s + 1])
                w = int(wptr[s + 1] - wptr[s])
                d = xa[sl] - (x0[sl] + dx[t][sl])
                P = pc["R"][aptr[s]:aptr[s + 1]].reshape(w, w) + np.diag(r[sl])
                form, bound = form_bound(sym(P), d)
                err = abs(LD(trial["prior"][t, s]) - form)
                worst = max(worst, float(err / (2 * bound)))
                assert err <= 2 * bound and form > 0, (t, s, float(err), float(bound))
        print("PRIOR trial_scene %s: worst error / allowed %.3f" % (name, worst))
        for cap in (1, 257):
            again = model.trial_scene(case.atm, geom, y, weight, dx, prior_ivar=r, prior_xa=xa, max_rays_per_pass=cap)
            for f in ("cost", "prior"):
                bits(again[f], trial[f], "%s, passes of %d" % (f, cap))
        one = model.trial_scene(case.atm, geom, y, weight, dx[1], prior_ivar=r, prior_xa=xa)
        for f in ("cost", "prior"):
            bits(one[f][0], trial[f][1], "%s of one trial alone" % f)
        model.set_prior_precision(None)
        bare = model.trial_scene(case.atm, geom, y, weight, dx, prior_ivar=r, prior_xa=xa)
        bits(bare["cost"], trial["cost"], "the cost does not depend on the prior")
        assert np.all(trial["prior"] > bare["prior"])
        # the diagnostics: the scene entry against its halves
        model.set_prior_precision(wptr, pc["R"])
        full = model.diagnose_scene(case.atm, geom, y, weight, prior_ivar=r, want_S=True, want_avk=True, want_normal=True)
        sequences.same_bits(formod_on(model, case.geom), want, "after diagnose_scene")
        bits(full["A"], step["A"], "A of diagnose_scene")
        half = model.diagnose_slices(wptr, full["A"], prior_ivar=r, want_S=True, want_avk=True)
        for f in DIAG_OUTS:
            bits(full[f], half[f], "%s of diagnose_scene against diagnose_slices" % f)
        assert np.all(full["status"] == 0)
        worst = {}
        for s in range(ns):
            sl = slice(wptr[s], wptr[s + 1])
            w = int(wptr[s + 1] - wptr[s])
            As, _ = slice_of(full, s)
            Rm = pc["R"][aptr[s]:aptr[s + 1]].reshape(w, w)
            ref = reference_full(As, Rm, r[sl])
            worst = merged(worst, check_diag(As, r[sl], diag_system(full, wptr, aptr, s), ref))
            # what a correlated prior promises: the measurement adds information, and never more than there is to know
            assert 0 < full["dofs"][s] < ref["n"]
            live = ref["live"]
            Sa = pc["Sa"][aptr[s]:aptr[s + 1]].reshape(w, w)
            prior_var = np.diag(Sa)[live].astype(LD)
            assert np.all(full["sigma"][sl][live].astype(LD) ** 2 <= prior_var + 2 * (np.diag(ref["ES"]) + gamma(2) * prior_var))
        report("PRIOR scene %s" % name, worst)
    finally:
        model.close()


def reference_full(A, Rm, r):
    """test_scene_diagnose_gpu.reference with M = A + P: S*, AVK* = S* A, Q* = diag(S* P S*) and their bounds"""
    with np.errstate(invalid="ignore"):
        live = (np.diag(A) + (np.diag(Rm) + r)) > 0
    n = int(live.sum())
    ref = dict(live=live, n=n)
    if n == 0:
        return ref
    ix = np.ix_(live, live)
    Al = sym(A).astype(LD)[ix]
    Pl = (sym(Rm).astype(LD) + np.diag(np.asarray(r).astype(LD)))[ix]
    M = Al + Pl
    L = cholesky_ld(M)
    Y = inverse_lower_ld(L)
    S = Y.T @ Y
    K, Tm = S @ Al, S @ Pl
    aS, aA, aK, aP, aT = np.abs(S), np.abs(Al), np.abs(K), np.abs(Pl), np.abs(Tm)
    EM = gamma(3) * (aA + aP)
    Bres = gamma(3 * n + 1) * ((np.abs(L) @ np.abs(L).T) @ aS) + EM @ aS
    ES = aS @ Bres
    EK = gamma(n) * (aS @ aA) + ES @ aA
    ET = gamma(n) * (aS @ aP) + ES @ aP
    g2 = gamma(n + 2)
    ref.update(S=S, K=K, ES=ES, EK=EK, dofs=np.trace(K), Bdofs=g2 * np.abs(np.diag(K)).sum() + np.diag(EK).sum(),
               N=(K * S).sum(axis=1), BN=g2 * (aK * aS).sum(axis=1) + (aK * ES + EK * aS + EK * ES).sum(axis=1),
               Q=(Tm * S).sum(axis=1), BQ=g2 * (aT * aS).sum(axis=1) + (aT * ES + ET * aS + ET * ES).sum(axis=1))
    return ref


def replay(hip, model, name, mode, pc, r, xa, settings):
    """test_scene_retrieve_gpu.replay with the full prior: the loop of jur_retrieve_scene_host over step_scene,
    trial_scene and retrieve_decide, the precision set anew for the slices that remain"""
    case, geom, y, weight = inputs(hip, name)
    lay, iq, ip, x0 = T.layout(hip, name)
    ns = len(lay["sfirst"])
    fac = np.array(settings["fac"])
    nlam, mi = len(fac), settings["max_iter"]
    wptr, aptr, sid = lay["wptr"], lay["aptr"], lay["sid"]
    atm = copy_atm(case.atm)
    lam, state, iters = np.full(ns, settings["lam0"]), np.zeros(ns, dtype=np.int32), np.zeros(ns, dtype=np.int32)
    cost, pri, nlive = np.zeros(ns), np.zeros(ns), np.zeros(ns, dtype=np.int64)
    nan = np.nan
    h = dict(h_cost=np.zeros((mi, ns)), h_prior=np.zeros((mi, ns)), h_lam=np.full((mi, nlam, ns), nan),
             h_tcost=np.full((mi, nlam, ns), nan), h_tprior=np.full((mi, nlam, ns), nan),
             h_status=np.full((mi, nlam, ns), -1, dtype=np.int32), h_best=np.full((mi, ns), -1, dtype=np.int32),
             h_accept=np.full((mi, ns), -1, dtype=np.int32))
    for it in range(mi):
        active = state == hip.RET_ACTIVE
        if not active.any():
            h["h_cost"][it], h["h_prior"][it] = cost, pri
            continue
        rays = (sid >= 0) & active[np.maximum(sid, 0)]
        sub = hip.scene_slices(case.ctl, atm, geom[rays][:, 0])
        full_of = [int(np.flatnonzero((lay["sfirst"] == f) & (lay["slen"] == l))[0]) for f, l in zip(sub["sfirst"], sub["slen"])]
        els = np.concatenate([np.arange(wptr[s], wptr[s + 1]) for s in full_of])
        model.set_prior_precision(sub["wptr"], np.concatenate([pc["R"][aptr[s]:aptr[s + 1]] for s in full_of]))
        x = T.state_of(case, atm, iq, ip)
        lamt = np.minimum(np.maximum(lam[None, :] * fac[:, None], settings["lam_min"]), settings["lam_max"])
        model.set_atm(atm)
        step = model.step_scene(atm, geom[rays], y[rays], weight[rays], lamt[:, full_of], mode=mode, prior_ivar=r[els], prior_dx=(xa - x)[els])
        trial = model.trial_scene(atm, geom[rays], y[rays], weight[rays], step["dx"], prior_ivar=r[els], prior_xa=xa[els])
        base = model.trial_scene(atm, geom[rays], y[rays], weight[rays], np.zeros(len(els)), prior_ivar=r[els], prior_xa=xa[els])
        dx = np.zeros((nlam, len(x)))
        dx[:, els] = step["dx"]
        tcost, tpri, status = np.zeros((nlam, ns)), np.zeros((nlam, ns)), np.zeros((nlam, ns), dtype=np.int32)
        status[:, full_of], tcost[:, full_of], tpri[:, full_of] = step["status"], trial["cost"], trial["prior"]
        for j, s in enumerate(full_of):
            cost[s], nlive[s], iters[s], pri[s] = step["cost"][j], step["nlive"][j], iters[s] + 1, base["prior"][0, j]
        h["h_cost"][it], h["h_prior"][it] = cost, pri
        for f, v in (("h_lam", lamt), ("h_tcost", tcost), ("h_tprior", tpri), ("h_status", status)):
            h[f][it][:, active] = v[:, active]
        d = hip.retrieve_decide(cost + pri, tcost + tpri, lamt, status, lam, state, settings["tol"], settings["lam_max"], fac.max())
        lam, state = d["lam"], d["state"]
        h["h_best"][it], h["h_accept"][it] = d["best"], d["accept"]
        for s in np.flatnonzero(d["accept"] == 1):
            bst = d["best"][s]
            atm = T.written_back(case, atm, iq, ip, dx[bst], only=T.slice_mask(lay, s))
            cost[s], pri[s] = tcost[bst, s], tpri[bst, s]
    state[state == hip.RET_ACTIVE] = hip.RET_MAXITER
    return dict(h, x=T.state_of(case, atm, iq, ip), atm=atm, lam=lam, cost=cost.copy(), prior=pri.copy(), nlive=nlive, state=state, iters=iters)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", SCENES)
def test_retrieve_scene_is_its_replay(hip, name, mode):
    """the replay of tests/test_scene_retrieve_gpu.py with the precision set, one slice made to stall: the measurements of
    its rays are the forward model on the first guess and its prior_xa is the first guess, so b = 0 and g = 0"""
    case, geom, y, weight = inputs(hip, name)
    lay, iq, ip, x0 = T.layout(hip, name)
    pc, r, xa = scene_prior(hip, name)
    s0 = 1
    rays = lay["sid"] == s0
    y2 = y.copy()
    y2[rays] = fresh_formod(hip, case, case.atm, geom[rays])["rad"]
    xa2 = xa.copy()
    xa2[T.slice_mask(lay, s0)] = x0[T.slice_mask(lay, s0)]
    settings = dict(T.FLOW)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        model.set_prior_precision(lay["wptr"], pc["R"])
        s = dict(settings)
        got = model.retrieve_scene(case.atm, geom, y2, weight, s.pop("max_iter"), s.pop("fac"), mode=mode, history=True,
                                   prior_ivar=r, prior_xa=xa2, **s)
        after = formod_on(model, case.geom)
        for cap in (1,):
            s = dict(settings)
            capped = model.retrieve_scene(case.atm, geom, y2, weight, s.pop("max_iter"), s.pop("fac"), mode=mode, history=True,
                                          prior_ivar=r, prior_xa=xa2, max_rays_per_pass=cap, **s)
            for f in T.HISTORY + ("x",) + T.PER_SLICE:
                bits(capped[f], got[f], "%s, passes of %d" % (f, cap))
        saved = _inputs_with(hip, name, y2)
        try:
            want = replay(hip, model, name, mode, pc, r, xa2, settings)
        finally:
            _inputs_restore(hip, name, saved)
    finally:
        model.close()
    for f in T.HISTORY + ("x",) + T.PER_SLICE:
        bits(got[f], want[f], f)
    assert got["state"][s0] == hip.RET_STALLED and np.any(got["h_accept"] == 1)
    assert np.all(got["prior"][np.arange(len(got["prior"])) != s0] > 0)
    T.same_atm(hip, got["atm"], want["atm"])
    fresh = fresh_formod(hip, case, got["atm"], geom)
    for f in ("rad", "tau", "tp", "np"):
        bits(got[f], fresh[f], "%s against a fresh model on atm_ret" % f)
    sequences.same_bits(after, fresh_formod(hip, case, got["atm"], case.geom), "the model holds atm_ret")


def _inputs_with(hip, name, y):
    """the replay reads the scene's inputs through test_scene_normal_gpu.inputs: hand it these measurements"""
    import test_scene_normal_gpu as N
    inputs(hip, name)
    saved = N._inputs[name]
    N._inputs[name] = (saved[0], saved[1], y, saved[3])
    return saved


def _inputs_restore(hip, name, saved):
    import test_scene_normal_gpu as N
    N._inputs[name] = saved


# ---- 4. diagnostics on constructed systems -------------------------------------------------------------------------------
def test_diagnostics_constructed(hip, model):
    mats, vecs, Rs, wptr, aptr, A, b, r, d = batch()
    model.set_prior_precision(wptr, flat(Rs))
    res = model.diagnose_slices(wptr, A, prior_ivar=r, want_S=True, want_avk=True)
    worst = {}
    for s in range(len(WIDTHS)):
        sl = slice(wptr[s], wptr[s + 1])
        ref = reference_full(mats[s], Rs[s], r[sl])
        worst = merged(worst, check_diag(mats[s], r[sl], diag_system(res, wptr, aptr, s), ref))
    report("PRIOR constructed", worst)
    # the limit R -> 0, r = 1e30: the results of the diagonal prior come back to their bound
    tiny = [Rm * 1e-30 for Rm in Rs]
    big = np.full(len(b), 1e30)
    model.set_prior_precision(wptr, flat(tiny))
    lim = model.diagnose_slices(wptr, A, prior_ivar=big, want_S=True, want_avk=True)
    model.set_prior_precision(None)
    dia = model.diagnose_slices(wptr, A, prior_ivar=big, want_S=True, want_avk=True)
    for s in range(len(WIDTHS)):
        sl = slice(wptr[s], wptr[s + 1])
        ref = reference_full(mats[s], tiny[s], big[sl])
        check_diag(mats[s], big[sl], diag_system(lim, wptr, aptr, s), ref)
        check_diag(mats[s], big[sl], diag_system(dia, wptr, aptr, s))
        check_diag(mats[s], big[sl], diag_system(lim, wptr, aptr, s))      # (against the reference of the diagonal prior)
    # a dead element and a breakdown
    rng = np.random.default_rng(8)
    w = 20
    A1, R1 = spd(rng, w), seeded_R(rng, w)
    for M in (A1, R1):
        M[5, :] = 0.0
        M[:, 5] = 0.0
    r1 = np.ones(w)
    r1[5] = 0.0
    wp, ap, Af, _ = pack([A1, np.zeros((2, 2))], [np.zeros(w), np.zeros(2)])
    model.set_prior_precision(wp, flat([R1, np.array([[1.0, 2.0], [2.0, 1.0]])]))
    res = model.diagnose_slices(wp, Af, prior_ivar=np.concatenate([r1, np.zeros(2)]), want_S=True, want_avk=True)
    assert list(res["status"]) == [0, 2]
    check_diag(A1, r1, diag_system(res, wp, ap, 0), reference_full(A1, R1, r1))
    for x in diag_system(res, wp, ap, 1)[:5] + diag_system(res, wp, ap, 1)[6:]:
        assert is_plus_zero(x)


# ---- 5. prior_corr ---------------------------------------------------------------------------------------------------------
def test_prior_corr(hip, model):
    rng = np.random.default_rng(12)
    n1, n2 = 65, 40
    z1 = np.sort(rng.uniform(0.0, 60.0, n1))
    z2 = np.sort(rng.uniform(5.0, 45.0, n2))
    # slice 0: quantity 0 on z1 then quantity 2 on z2 (cz 5 and 0.5 km); slice 1: quantity 1, uncorrelated; slice 2: two
    # equal altitudes (first, with sigma = 1: the second pivot is fma(-1, 1, 1) = 0 exactly; elsewhere the pivot of a
    # singular Sa is a rounding error of either sign); slice 3: one quantity alone, 17 levels, cz 20 km
    z3 = np.sort(rng.uniform(0.0, 30.0, 17))
    iq = np.concatenate([np.zeros(n1), np.full(n2, 2), np.ones(9), np.zeros(3), np.full(17, 3)]).astype(np.int32)
    z = np.concatenate([z1, z2, np.linspace(1.0, 9.0, 9), [4.0, 4.0, 3.0], z3])
    sigma = np.concatenate([10.0 ** rng.uniform(-1, 1, n1 + n2 + 9), np.ones(3), 10.0 ** rng.uniform(-1, 1, 17)])
    cz = np.array([5.0, 0.0, 0.5, 20.0])
    wptr = np.array([0, n1 + n2, n1 + n2 + 9, n1 + n2 + 12, n1 + n2 + 29])
    out = hip.prior_corr_slices(model, wptr, iq, z, sigma, cz)
    aptr = out["aptr"]
    assert list(out["status"][[0, 1, 3]]) == [0, 0, 0] and out["status"][2] != 0, "equal altitudes break down there and nowhere else"
    assert is_plus_zero(out["R"][aptr[2]:aptr[3]])
    worst_sa = worst_r = 0.0
    for s in (0, 1, 3):
        sl = slice(wptr[s], wptr[s + 1])
        w = int(wptr[s + 1] - wptr[s])
        Sa, Rm = (out[f][aptr[s]:aptr[s + 1]].reshape(w, w) for f in ("Sa", "R"))
        q, zz, sg = iq[sl], z[sl].astype(LD), sigma[sl].astype(LD)
        same = (q[:, None] == q[None, :]) & (cz[q][:, None] > 0)
        arg = np.where(same, np.abs(zz[:, None] - zz[None, :]) / np.where(same, cz[q][:, None], 1.0).astype(LD), 0)
        want = np.where(same, np.outer(sg, sg) * np.exp(-arg), 0)
        want[np.diag_indices(w)] = sg * sg
        bound = (6 + 2 * arg) * U * np.abs(want)
        err = np.abs(Sa.astype(LD) - want)
        assert np.all(err <= bound), (s, float(np.max(err / np.maximum(bound, np.finfo(LD).tiny))))
        worst_sa = max(worst_sa, float(np.max(err[want != 0] / bound[want != 0])))
        assert np.array_equal(Sa.view(np.uint64), Sa.T.copy().view(np.uint64)) and np.array_equal(Rm.view(np.uint64), Rm.T.copy().view(np.uint64))
        # R against the longdouble inverse of the Sa that was formed, within the inverse bound of the diagnose tests
        M = Sa.astype(LD)
        L = cholesky_ld(M)
        Y = inverse_lower_ld(L)
        S = Y.T @ Y
        aS = np.abs(S)
        Bres = gamma(3 * w + 1) * ((np.abs(L) @ np.abs(L).T) @ aS) + gamma(2) * np.diag(M)[:, None] * aS
        ES = aS @ Bres
        errR = np.abs(Rm.astype(LD) - S)
        assert np.all(errR <= 2 * ES), (s, float(np.max(errR / np.maximum(ES, np.finfo(LD).tiny))))
        worst_r = max(worst_r, float(np.max(errR / np.maximum(2 * ES, np.finfo(LD).tiny))))
        cross = q[:, None] != q[None, :]
        assert np.all(Rm[cross] == 0), "the blocks between different quantities are exact zeros"
        if s == 1:
            off = ~np.eye(w, dtype=bool)
            assert np.all(Rm[off] == 0) and np.all(np.abs(np.diag(Rm).astype(LD) * sg * sg - 1) <= 3 * U)
        # within a quantity on ascending z: tridiagonal to the bound, and the closed form on the three diagonals
        # (the closed form is that of the exact Sa: what the rounding of Sa moves R by is bounded the same way, through
        # |R| |dSa| |R| with |dSa| <= the bound on Sa above)
        for qq in np.unique(q):
            if cz[qq] == 0:
                continue
            k = np.flatnonzero(q == qq)
            blk = np.ix_(k, k)
            closed = exp_prior_inverse(z[sl][k], sigma[sl][k], cz[qq])
            moved = np.abs(closed) @ bound[blk] @ np.abs(closed)
            allowed = 2 * (ES[blk] + moved) + 2e-14 * np.sqrt(np.outer(np.diag(closed), np.diag(closed)))
            diff = np.abs(Rm[blk].astype(LD) - closed)
            assert np.all(diff <= allowed), (s, qq, float(np.max(diff / allowed)))
    print("PRIOR prior_corr: worst Sa error / bound %.3f, worst R error / allowed %.3f" % (worst_sa, worst_r))


# ---- 6. what the feature buys ----------------------------------------------------------------------------------------------
def test_a_correlated_prior_on_one_limb_scan(hip):
    """One limb scan of 13 rays, T and O3 retrieved on all levels from two channels: ill-posed without a prior.  With the
    correlated prior (cz = 5 km) at the same sigma the run ends CONVERGED or MAXITER without JUR_ENLOS, and its retrieved
    minus truth profile, in units of sigma, has the smaller second-difference norm for both quantities.  Confirmed
    beforehand on the CPU oracle for the exact solution of the linearised problem (its kernel() at the first guess, numpy's
    solve of (K^T W K + (1 + lam) R) dx = K^T W (y - F)): 2.90 (T) and 3.43 (O3) with the diagonal prior against 0.125 and
    0.113 with the correlated one at lam = 0, 2.50 and 2.89 against 0.124 and 0.109 at lam = 1."""
    case = common.limb_case()
    c = case.ctl
    c.retp_zmin, c.retp_zmax, c.rett_zmin, c.rett_zmax = -999.0, -999.0, -10.0, 200.0
    for g in range(c.ng):
        c.retq_zmin[g], c.retq_zmax[g] = -999.0, -999.0
    c.retq_zmin[2], c.retq_zmax[2] = -10.0, 200.0
    for w in range(c.nw):
        c.retk_zmin[w], c.retk_zmax[w] = -999.0, -999.0
    limb = case.geom[(case.geom[:, 1] > 700.0) & (case.geom[:, 4] > 5.0) & (case.geom[:, 4] < 60.0)]
    geom = limb[np.linspace(0, len(limb) - 1, 13).astype(int)].copy()
    geom[:, 0] = case.atm.time[0]
    n = case.atm.np
    z = np.ctypeslib.as_array(case.atm.z)[:n].copy()
    truth = copy_atm(case.atm)
    bump = np.sin(np.pi * np.clip((z - 10.0) / 40.0, 0.0, 1.0)) ** 2
    np.ctypeslib.as_array(truth.t)[:n] += 2.0 * bump
    np.ctypeslib.as_array(truth.q)[2, :n] *= 1.0 + 0.1 * bump
    y = fresh_formod(hip, case, truth, geom)["rad"]
    weight = np.broadcast_to(1.0 / (0.005 * np.abs(y).max(axis=0)) ** 2, y.shape).copy()
    sigma_q = [1.0, 1.0] + [lambda v: 0.1 * abs(v)] * c.ng + [1.0] * c.nw
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        runs = {}
        for what, czq in (("diagonal", 0.0), ("correlated", 5.0)):
            pc = hip.prior_corr(model, case.ctl, case.atm, geom[:, 0], sigma_q, [czq] * (2 + c.ng + c.nw))
            assert np.all(pc["status"] == 0) and len(pc["status"]) == 1
            iq, ip = pc["iq"], pc["ip"]
            x0 = T.state_of(case, case.atm, iq, ip)
            model.set_prior_precision(pc["wptr"], pc["R"])
            out = model.retrieve_scene(case.atm, geom, y, weight, 4, (0.1, 1.0, 10.0), mode=hip.DAMP_PRIOR,
                                       prior_ivar=np.zeros(len(x0)), prior_xa=x0)
            model.set_prior_precision(None)
            err = out["x"] - T.state_of(case, truth, iq, ip)
            runs[what] = {int(q): float(np.linalg.norm(np.diff(err[iq == q] / pc["sigma"][iq == q], 2))) for q in np.unique(iq)}
            if what == "correlated":
                assert out["state"][0] in (hip.RET_CONVERGED, hip.RET_MAXITER)
            print("PRIOR limb scan, %s prior: state %d, cost %.4e, prior %.4e, second-difference norm of (x - truth) / sigma by quantity %s"
                  % (what, out["state"][0], out["cost"][0], out["prior"][0], runs[what]))
        assert sorted(runs["correlated"]) == [1, 4]
        for q in runs["correlated"]:
            assert runs["correlated"][q] < runs["diagonal"][q], (q, runs)
    finally:
        model.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_and_state(hip):
    name = "ragged"
    case, geom, y, weight = inputs(hip, name)
    lay, iq, ip, x0 = T.layout(hip, name)
    pc, r, xa = scene_prior(hip, name)
    wptr, aptr, ns, n = lay["wptr"], lay["aptr"], len(lay["sfirst"]), len(x0)
    want = fresh_formod(hip, case, case.atm, case.geom)
    EINVAL = hip.EINVAL

    def changed(a, at, v):
        a = a.copy()
        a[at] = v
        return a

    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        model.set_prior_precision(wptr, pc["R"])
        good = model.step_scene(case.atm, geom, y, weight, LAMS[1:], mode=1, prior_ivar=r, prior_dx=xa - x0)
        w1 = int(wptr[2] - wptr[1])
        at = int(aptr[1]) + 2 * w1 + 1                                  # element (2, 1) of slice 1: in the read triangle
        for v, message in ((np.nan, r"R of slice 1, element \(2, 1\) is nan: not finite"), (np.inf, r"R of slice 1, element \(2, 1\) is inf")):
            with pytest.raises(hip.JurassicError, match=r"error %d: jur_model_set_prior_precision: %s" % (EINVAL, message)):
                model.set_prior_precision(wptr, changed(pc["R"], at, v))
        model.set_prior_precision(wptr, changed(pc["R"], int(aptr[1]) + 1 * w1 + 2, np.nan))   # (1, 2): above the diagonal, not read
        model.set_prior_precision(wptr, pc["R"])
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_model_set_prior_precision: R of slice 1, element \(2, 2\) is -1.*negative diagonal" % EINVAL):
            model.set_prior_precision(wptr, changed(pc["R"], int(aptr[1]) + 2 * w1 + 2, -1.0))
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_model_set_prior_precision: wptr is not an ascending.*slice 1" % EINVAL):
            model.set_prior_precision([0, 3, 2], np.zeros(10))
        bits(model.prior_precision()["R"], pc["R"], "a refused set call leaves what was set")
        # a layout that is not the one set, both counts named
        first = lay["sid"] == 0
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_step_scene_host: the call has 1 slices, the prior precision of the model was set for %d" % (EINVAL, ns)):
            model.step_scene(case.atm, geom[first], y[first], weight[first], 1.0, prior_ivar=r[:wptr[1]], prior_dx=np.zeros(wptr[1]))
        sequences.same_bits(formod_on(model, case.geom), want, "after the layout refusal")
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_solve_slices_host: slice 0 of the call has 3 elements, the prior precision of the model was set for %d" % (EINVAL, wptr[1])):
            model.solve_slices(np.concatenate([[0, 3], wptr[2:] - wptr[1] + 3]), np.zeros(9 + int(aptr[-1] - aptr[1])),
                               np.zeros(3 + n - int(wptr[1])), 1.0, prior_ivar=np.zeros(3 + n - int(wptr[1])), prior_dx=np.zeros(3 + n - int(wptr[1])))
        # prior_ivar missing while R is set: every entry that takes a prior
        calls = [("jur_step_scene_host", lambda: model.step_scene(case.atm, geom, y, weight, 1.0)),
                 ("jur_trial_scene_host", lambda: model.trial_scene(case.atm, geom, y, weight, np.zeros(n))),
                 ("jur_retrieve_scene_host", lambda: model.retrieve_scene(case.atm, geom, y, weight, 2, (0.1, 10.0))),
                 ("jur_diagnose_scene_host", lambda: model.diagnose_scene(case.atm, geom, y, weight)),
                 ("jur_solve_slices_host", lambda: model.solve_slices(wptr, np.zeros(int(aptr[-1])), np.zeros(n), 1.0)),
                 ("jur_diagnose_slices_host", lambda: model.diagnose_slices(wptr, np.zeros(int(aptr[-1]))))]
        for who, call in calls:
            with pytest.raises(hip.JurassicError, match=r"error %d: %s: a prior precision is set in the model: prior_ivar" % (EINVAL, who)):
                call()
            sequences.same_bits(formod_on(model, case.geom), want, "after %s without prior_ivar" % who)
        # the entries without a prior are unaffected
        plain = model.normal_scene(case.atm, geom, y, weight)
        model.set_prior_precision(None)
        bare = model.normal_scene(case.atm, geom, y, weight)
        for f in ("A", "b", "cost", "nlive", "rad"):
            bits(plain[f], bare[f], "%s of normal_scene with and without a precision" % f)
        model.set_prior_precision(wptr, pc["R"])
        again = model.step_scene(case.atm, geom, y, weight, LAMS[1:], mode=1, prior_ivar=r, prior_dx=xa - x0)
        for f in ("dx", "pred", "status", "cost"):
            bits(again[f], good[f], "%s in the call after the refusals" % f)
        # prior_corr's refusals
        el = dict(wptr=[0, 3], iq=[0, 0, 1], z=[1.0, 2.0, 3.0], sigma=[1.0, 1.0, 1.0], cz=[5.0, 0.0])
        for key, at_, v, message in (("sigma", 1, 0.0, r"sigma of slice 0, element 1 is 0"), ("sigma", 2, np.inf, r"sigma of slice 0, element 2 is inf"),
                                     ("sigma", 0, np.nan, r"sigma of slice 0, element 0 is nan"), ("cz", 1, -1.0, r"cz of quantity 1 is -1"),
                                     ("cz", 0, np.nan, r"cz of quantity 0 is nan"), ("iq", 2, 2, r"iq of slice 0, element 2 is 2: outside 0..1"),
                                     ("iq", 0, -1, r"iq of slice 0, element 0 is -1")):
            bad = dict(el)
            bad[key] = changed(np.array(el[key]), at_, v)
            with pytest.raises(hip.JurassicError, match=r"error %d: jur_prior_corr_host: %s" % (EINVAL, message)):
                hip.prior_corr_slices(model, bad["wptr"], bad["iq"], bad["z"], bad["sigma"], bad["cz"])
        ok = hip.prior_corr_slices(model, el["wptr"], el["iq"], el["z"], el["sigma"], el["cz"])
        assert list(ok["status"]) == [0]
        sequences.same_bits(formod_on(model, case.geom), want, "after prior_corr and its refusals")
        fresh = hip.Model(case.ctl, case.lib_tables())
        try:
            fresh.set_atm(case.atm)
            assert fresh.prior_precision() is None
            model.set_prior_precision(None)
            assert model.prior_precision() is None
            a, b2 = (m.step_scene(case.atm, geom, y, weight, LAMS[1:], mode=1, prior_ivar=r, prior_dx=xa - x0) for m in (model, fresh))
            for f in ("dx", "pred", "status", "cost", "rad"):
                bits(a[f], b2[f], "%s after set_prior_precision(None) against a fresh model" % f)
        finally:
            fresh.close()
    finally:
        model.close()


def test_scratch_beyond_the_budget_is_refused(hip):
    """The construction of tests/test_scene_solve_gpu.py::test_solver_scratch_beyond_the_budget_is_refused: one slice of
    1120 columns under the smallest workspace budget; with a precision set the solver scratch holds one more copy of the
    matrix and g: JUR_ENOMEM before anything is launched, the model answers as a fresh one and R is still set."""
    case = common.limb_case()
    spec = [synth._spec(0.0, 10.0, 45.0, 140, 0.0, 90.0), synth._spec(1.0, 20.0, 30.0, 20, 0.0, 60.0)]
    case.atm = synth.ragged_atmosphere(case.ctl, spec, seed=0, base=case.atm, order=None)
    c = case.ctl
    c.retp_zmin, c.retp_zmax, c.rett_zmin, c.rett_zmax = -10.0, 100.0, -10.0, 100.0
    for g in range(c.ng):
        c.retq_zmin[g], c.retq_zmax[g] = -10.0, 100.0
    c.retk_zmin[0], c.retk_zmax[0] = -10.0, 100.0
    geom = case.geom[:2].copy()
    geom[:, 0] = 0.0
    want = fresh_formod(hip, case, case.atm, geom)
    y, weight = np.zeros((2, c.nd)), np.ones((2, c.nd))
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_workspace_budget(64 << 20)
        model.set_atm(case.atm)
        lay = hip.scene_slices(case.ctl, case.atm, geom[:, 0])
        assert list(np.diff(lay["wptr"])) == [1120]
        model.set_prior_precision(lay["wptr"], np.eye(1120))
        with pytest.raises(hip.JurassicError, match=r"error -3: jur_step_scene_host: .*the solver scratch"):
            model.step_scene(case.atm, geom, y, weight, 1.0, prior_ivar=np.zeros(1120), prior_dx=np.zeros(1120))
        sequences.same_bits(formod_on(model, geom), want, "after the refusal")
        assert model.prior_precision()["R"].shape == (1120 * 1120,)
    finally:
        model.close()
