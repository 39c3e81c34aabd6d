"""Model.diagnose_slices (jur_diagnose_slices_host) and Model.diagnose_scene (jur_diagnose_scene_host): the posterior
covariance S = (A + diag r)^-1, the averaging kernel AVK = S A, their diagonals, the degrees of freedom and the noise and
smoothing errors of every slice, on the device.

The error bounds are derived, not measured (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.).  With
u = 2^-53, gamma_m = m u / (1 - m u), n live elements, M = A + diag(r) on them, and S*, AVK* = S* A formed in np.longdouble
from a longdouble Cholesky factor L of M (its own error, of the order n cond(M) 2^-64, is 2^-11 of what follows):
  column residuals (Thms 8.5, 10.4, exact right-hand sides e_j):
      |I - M S^| <= Bres = gamma_{3n+1} |L| |L^T| |S*| + gamma_2 diag(M) |S*|
  inverse, from S* - S^ = S* (I - M S^):        |S^ - S*| <= E_S = |S*| Bres            (entrywise: either triangle)
  product, any summation order:                  |AVK^ - AVK*| <= E_K = gamma_n |S*| |A| + E_S |A|
  sums of n terms with one extra rounding inside a term, any order: gamma_{n+2} sum |terms|, plus what the terms inherit:
      dofs = sum AVK_ii:             gamma_{n+2} sum |AVK*_ii| + sum E_K,ii
      N_i = sum_j AVK_ij S_ij:       gamma_{n+2} sum |AVK*_ij| |S*_ij| + sum (|AVK*_ij| E_S,ij + E_K,ij |S*_ij| + E_K,ij E_S,ij)
      Q_i = sum_j S_ij^2 r_j:        gamma_{n+2} Q*_i + sum (2 |S*_ij| E_S,ij + E_S,ij^2) r_j
  a correctly rounded square root: the squares of sigma, sigma_noise, sigma_smooth are held to S*_ii, N*_i, Q*_i within the
      bound B of the radicand plus gamma_2 times the value.
Twice each bound is allowed, as in tests/test_scene_solve_gpu.py.  The kernels divide by the diagonal of L (true
divisions), form every inner product as a chain of fused multiply-adds and use no MFMA.  Everything else is bit identity.

A NaN on the diagonal is no breakdown.  By the liveness rule -- the solve kernel's, D_i = A_ii + r_i > 0, "anything else,
NaN included, is dead" (include/jurassic_hip.h) -- such an element is dead and the system is solved without it, so the
diagnostics describe the system the step was taken in.  test_dead_elements_and_breakdown holds a NaN on the diagonal to
the dead-element rules, and takes the NaN breakdown from an entry below the diagonal between live elements, as
test_scene_solve_gpu.py does."""
import ctypes as C
import numpy as np
import pytest
import common
import refcases as R
import sequences
from jurassic_hip import synth
from test_scene_jacobian_gpu import bits, formod_on, fresh_formod, scene_case
from test_scene_normal_gpu import SUMS, blocks_and_sums, inputs, slice_of
from test_scene_solve_gpu import gamma, is_plus_zero, pack, spd

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
LD = np.longdouble
WIDTHS = (1, 2, 15, 16, 17, 63, 64, 65, 100, 182)
VECTORS = ("sigma", "sigma_noise", "sigma_smooth", "avk_diag")
OUTS = VECTORS + ("dofs", "status", "S", "avk")


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


@pytest.fixture(scope="module")
def model(hip):
    case = common.limb_case()
    m = hip.Model(case.ctl, case.lib_tables())
    yield m
    m.close()


def system(res, wptr, aptr, s):
    """the outputs of system s of a result, in the order of OUTS (S, avk as (w, w) or None)"""
    w = int(wptr[s + 1] - wptr[s])
    sl = slice(wptr[s], wptr[s + 1])
    mats = [res[f][aptr[s]:aptr[s + 1]].reshape(w, w) if f in res else None for f in ("S", "avk")]
    return [res[f][sl] for f in VECTORS] + [res["dofs"][s], int(res["status"][s])] + mats


def cholesky_ld(M):
    n = len(M)
    L = np.zeros((n, n), LD)
    for j in range(n):
        d = M[j, j] - L[j, :j] @ L[j, :j]
        assert d > 0
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def inverse_lower_ld(L):
    n = len(L)
    Y = np.zeros((n, n), LD)
    for i in range(n):
        rhs = -(L[i, :i] @ Y[:i])
        rhs[i] += 1
        Y[i] = rhs / L[i, i]
    return Y


def reference(A, r):
    """S*, AVK* and the bounds of the module docstring on the live elements of one system, in np.longdouble"""
    w = len(A)
    r = np.zeros(w) if r is None else np.asarray(r)
    with np.errstate(invalid="ignore"):
        live = (np.diag(A) + r) > 0
    n = int(live.sum())
    ref = dict(live=live, n=n)
    if n == 0:
        return ref
    ix = np.ix_(live, live)
    low = np.tril(A)
    Al = (low + np.tril(low, -1).T).astype(LD)[ix]                  # (only the diagonal and the lower triangle are read)
    rl = r[live].astype(LD)
    M = Al + np.diag(rl)
    L = cholesky_ld(M)
    Y = inverse_lower_ld(L)
    S = Y.T @ Y
    K = S @ Al
    aS, aA, aK = np.abs(S), np.abs(Al), np.abs(K)
    Bres = gamma(3 * n + 1) * ((np.abs(L) @ np.abs(L).T) @ aS) + gamma(2) * np.diag(M)[:, None] * aS
    ES = aS @ Bres
    EK = gamma(n) * (aS @ aA) + ES @ aA
    g2 = gamma(n + 2)
    ref.update(r=rl, S=S, K=K, ES=ES, EK=EK,
               dofs=np.trace(K), Bdofs=g2 * np.abs(np.diag(K)).sum() + np.diag(EK).sum(),
               N=(K * S).sum(axis=1), BN=g2 * (aK * aS).sum(axis=1) + (aK * ES + EK * aS + EK * ES).sum(axis=1),
               Q=(S * S) @ rl, BQ=g2 * ((S * S) @ rl) + (2 * aS * ES + ES * ES) @ rl)
    return ref


def check_system(A, r, got, ref=None):
    """The bounds of the module docstring on the live elements, the exact properties everywhere; returns the worst error /
    allowed ratios as a dict."""
    sigma, noise, smooth, kdiag, dofs, status, S, K = got
    ref = ref or reference(A, r)
    live, n = ref["live"], ref["n"]
    assert status == 0
    assert np.array_equal(S.view(np.uint64), S.T.copy().view(np.uint64)), "S and its transpose differ"
    bits(kdiag, np.diag(K).copy(), "avk_diag against the diagonal of avk")
    bits(sigma, np.sqrt(np.diag(S)), "sigma against sqrt(diag S)")
    dead = np.flatnonzero(~live)
    for x in (S[dead, :], S[:, dead], K[dead, :], K[:, dead], sigma[dead], noise[dead], smooth[dead], kdiag[dead]):
        assert is_plus_zero(x), "a dead element's output is not +0.0"
    if n == 0:
        assert is_plus_zero(dofs)
        return {}
    ix = np.ix_(live, live)
    tiny = np.finfo(LD).tiny
    worst = {}

    def within(what, got, want, bound):
        err = np.abs(np.asarray(got, LD) - want)
        worst[what] = float(np.max(err / np.maximum(2 * bound, tiny)))
        assert np.all(err <= 2 * bound), (what, len(A), n, float(np.max(err)), float(np.max(bound)))

    def root(what, got, want, bound):
        within(what, np.asarray(got, LD) ** 2, want, bound + gamma(2) * np.abs(want))

    within("S", S[ix], ref["S"], ref["ES"])
    within("avk", K[ix], ref["K"], ref["EK"])
    within("dofs", dofs, ref["dofs"], ref["Bdofs"])
    root("sigma", sigma[live], np.diag(ref["S"]), np.diag(ref["ES"]))
    root("sigma_noise", noise[live], ref["N"], ref["BN"])
    root("sigma_smooth", smooth[live], ref["Q"], ref["BQ"])
    return worst


def merged(a, b):
    return {k: max(a.get(k, 0.0), b.get(k, 0.0)) for k in set(a) | set(b)}


def report(what, worst):
    print("DIAGNOSE %s: worst error / allowed %s" % (what, ", ".join("%s %.3f" % (k, worst[k]) for k in sorted(worst))))


_batch = {}


def batch():
    """the ragged batch of test 1: (mats, wptr, aptr, A), and the scaled copy with its prior (mats, A, r), made once"""
    if not _batch:
        rng = np.random.default_rng(2025)
        mats = [spd(rng, w) for w in WIDTHS]
        wptr, aptr, A, _ = pack(mats, [np.zeros(w) for w in WIDTHS])
        r = 10.0 ** rng.uniform(-2.0, 1.0, int(wptr[-1]))
        small = [m * 1e-2 for m in mats]
        for a in mats + small + [A, r]:
            a.setflags(write=False)
        _batch["v"] = (mats, wptr, aptr, A, small, np.concatenate([m.ravel() for m in small]), r)
    return _batch["v"]


_done = {}


def diagnosed(model, prior):
    """the batch of test 1 without (0) or with (1) the prior: (the matrices, r or None, the result, the references)"""
    if prior not in _done:
        mats, wptr, aptr, A, small, As, r = batch()
        if prior:
            res = model.diagnose_slices(wptr, As, prior_ivar=r, want_S=True, want_avk=True)
            refs = [reference(small[s], r[wptr[s]:wptr[s + 1]]) for s in range(len(WIDTHS))]
            _done[prior] = (small, r, res, refs)
        else:
            res = model.diagnose_slices(wptr, A, want_S=True, want_avk=True)
            _done[prior] = (mats, None, res, [reference(m, None) for m in mats])
    return _done[prior]


# ---- 1. constructed systems ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior", [0, 1])
def test_constructed_systems(model, prior):
    _, wptr, aptr, _, _, _, _ = batch()
    mats, r, res, refs = diagnosed(model, prior)
    assert res["sigma"].shape == (wptr[-1],) and res["dofs"].shape == res["status"].shape == (len(WIDTHS),)
    assert res["S"].shape == res["avk"].shape == (aptr[-1],)
    assert np.all(res["status"] == 0)
    worst = {}
    for s, w in enumerate(WIDTHS):
        rs = r[wptr[s]:wptr[s + 1]] if prior else None
        worst = merged(worst, check_system(mats[s], rs, system(res, wptr, aptr, s), refs[s]))
        if prior:
            assert 0 < res["dofs"][s] < 0.9 * w                      # the prior matters
        else:
            assert is_plus_zero(res["sigma_smooth"][wptr[s]:wptr[s + 1]])
    report("constructed, %s" % ("with a prior" if prior else "no prior"), worst)


# ---- 2. wider than a workgroup and than one tile row -----------------------------------------------------------------
def test_wider_than_a_workgroup(model):
    """257 and 300 columns: more than 256 rows, more than four 64-row chunks below a diagonal block, five tiles a side"""
    rng = np.random.default_rng(8)
    mats = [spd(rng, w) * 1e-2 for w in (257, 300)]
    wptr, aptr, A, _ = pack(mats, [np.zeros(257), np.zeros(300)])
    r = 10.0 ** rng.uniform(-2.0, 1.0, int(wptr[-1]))
    res = model.diagnose_slices(wptr, A, prior_ivar=r, want_S=True, want_avk=True)
    worst = {}
    for s in range(2):
        worst = merged(worst, check_system(mats[s], r[wptr[s]:wptr[s + 1]], system(res, wptr, aptr, s)))
    report("wide", worst)


# ---- 3. dead elements and breakdown ----------------------------------------------------------------------------------
def test_dead_elements_and_breakdown(model):
    rng = np.random.default_rng(6)
    holes = spd(rng, 40)
    for i in (0, 16, 39):
        holes[i, :] = 0.0
        holes[:, i] = 0.0
    nan_diag = spd(rng, 33)
    nan_diag[20, 20] = np.nan                                      # not > 0: element 20 is dead, with what its row holds
    indefinite = np.array([[1.0, 2.0], [2.0, 1.0]])
    with_nan = spd(rng, 33)
    with_nan[20, 3] = with_nan[3, 20] = np.nan                     # between live elements: the pivot of column 20 is NaN
    good = spd(rng, 33)
    mats = [holes, nan_diag, indefinite, good, with_nan]
    wptr, aptr, A, _ = pack(mats, [np.zeros(len(m)) for m in mats])
    r = 10.0 ** rng.uniform(-2.0, 0.0, int(wptr[-1]))
    r[wptr[0]:wptr[1]][[0, 16, 39]] = 0.0                           # (D = 0 there)
    r[wptr[2]:wptr[3]] = 0.0
    worst = {}
    for prior in (None, r):
        res = model.diagnose_slices(wptr, A, prior_ivar=prior, want_S=True, want_avk=True)
        for s in (0, 1, 3):
            rs = None if prior is None else prior[wptr[s]:wptr[s + 1]]
            ref = reference(mats[s], rs)
            assert ref["n"] == len(mats[s]) - (3, 1, 0, 0)[s]
            worst = merged(worst, check_system(mats[s], rs, system(res, wptr, aptr, s), ref))
        for s, column in ((2, 1), (4, 20)):
            got = system(res, wptr, aptr, s)
            assert got[5] == 1 + column
            for x in got[:5] + got[6:]:
                assert is_plus_zero(x), "an output of a system that broke down is not +0.0"
        solo = model.diagnose_slices([0, 33], good, prior_ivar=None if prior is None else prior[wptr[3]:wptr[4]], want_S=True,
                                     want_avk=True)
        for got, want, f in zip(system(res, wptr, aptr, 3), system(solo, [0, 33], [0, 33 * 33], 0), OUTS):
            bits(np.asarray(got), np.asarray(want), "%s of the good system between two breakdowns" % f)
    report("dead elements", worst)


# ---- 4. independence -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior", [0, 1])
def test_independence(model, prior):
    _, wptr, aptr, A0, _, As, r = batch()
    A = As if prior else A0
    mats, _, res, _ = diagnosed(model, prior)
    ns = len(WIDTHS)
    pr = lambda sel: dict(prior_ivar=np.concatenate([r[wptr[s]:wptr[s + 1]] for s in sel])) if prior else {}
    for s in range(ns):                                             # each system alone
        w = WIDTHS[s]
        solo = model.diagnose_slices([0, w], mats[s], want_S=True, want_avk=True, **pr([s]))
        for got, want, f in zip(system(res, wptr, aptr, s), system(solo, [0, w], [0, w * w], 0), OUTS):
            bits(np.asarray(got), np.asarray(want), "%s of system %d alone" % (f, s))
    order = list(range(ns))[::-1]                                   # the batch reversed
    rw, ra, rA, _ = pack([mats[s] for s in order], [np.zeros(WIDTHS[s]) for s in order])
    rev = model.diagnose_slices(rw, rA, want_S=True, want_avk=True, **pr(order))
    for s in range(ns):
        for got, want, f in zip(system(res, wptr, aptr, s), system(rev, rw, ra, ns - 1 - s), OUTS):
            bits(np.asarray(got), np.asarray(want), "%s of system %d reversed" % (f, s))
    for want_S, want_avk in ((False, False), (True, False), (False, True)):
        part = model.diagnose_slices(wptr, A, want_S=want_S, want_avk=want_avk, **pr(range(ns)))
        assert ("S" in part) == want_S and ("avk" in part) == want_avk
        for f in part:
            bits(part[f], res[f], "%s with want_S %s, want_avk %s" % (f, want_S, want_avk))


# ---- 5. limits with closed forms -------------------------------------------------------------------------------------
def test_limits(model):
    rng = np.random.default_rng(9)
    n = 20
    A = spd(rng, n) / n                                            # of order 1
    assert 0.5 < np.abs(A).max() < 4
    res = model.diagnose_slices([0, n], A, prior_ivar=np.full(n, 1e30), want_avk=True)
    assert res["status"][0] == 0
    assert np.all(np.abs(res["sigma"] / 1e-15 - 1) <= 1e-12)
    assert np.all(np.abs(res["avk"]) < 1e-28) and 0 < res["dofs"][0] < 1e-28
    res = model.diagnose_slices([0, n], A, want_S=True, want_avk=True)
    ref = reference(A, None)
    worst = check_system(A, None, system(res, [0, n], [0, n * n], 0), ref)
    K = res["avk"].reshape(n, n).astype(LD)
    assert np.all(np.abs(K - np.eye(n)) <= 2 * ref["EK"])
    assert abs(LD(res["dofs"][0]) - n) <= 2 * ref["Bdofs"]
    assert is_plus_zero(res["sigma_smooth"])
    report("no prior, well conditioned", worst)


# ---- 6. the scene entry ----------------------------------------------------------------------------------------------
VIEWS = {"all": lambda g: np.ones(len(g), bool), "limb": lambda g: (g[:, 1] > 700.0) & (g[:, 4] > 1.0),
         "nadir": lambda g: np.abs(g[:, 4]) <= 1.0}


def seeded_r(out):
    """prior_ivar as tests/test_scene_solve_gpu.py::test_priors makes it: 1e-3 .. 1e-1 of the mean diagonal of A_s"""
    rng = np.random.default_rng(3)
    return np.concatenate([10.0 ** rng.uniform(-3.0, -1.0, len(bs)) * np.diag(As).mean()
                           for As, bs in (slice_of(out, s) for s in range(len(out["sfirst"])))])


@pytest.mark.parametrize("name,view", [("ragged", "all"), ("ragged", "limb"), ("ragged", "nadir"), ("lone_ends", "all")])
def test_scene_entry_equals_its_halves(hip, name, view):
    """six rays per time stamp of the scene (limb views from orbit, nadir views, observers inside the atmosphere), or its
    limb views or its nadir views alone: three or four slices of 33 to 104 columns, a few dozen rays"""
    case, geom, y, weight = inputs(hip, name)
    sel = VIEWS[view](geom)
    assert sel.sum() >= 12
    geom, y, weight = geom[sel], y[sel], weight[sel]
    want = fresh_formod(hip, case, case.atm, case.geom)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        out = blocks_and_sums(hip, name)[1] if view == "all" else model.normal_scene(case.atm, geom, y, weight, want_k=True)
        ns, wptr, aptr = len(out["sfirst"]), out["wptr"], out["aptr"]
        assert ns >= 2 and np.diff(wptr).max() > 32
        r = seeded_r(out)
        worst = {}
        for prior in (None, r):
            full = model.diagnose_scene(case.atm, geom, y, weight, prior_ivar=prior, want_S=True, want_avk=True, want_normal=True,
                                        want_k=True)
            sequences.same_bits(formod_on(model, case.geom), want, "after diagnose_scene")
            for f in SUMS + ("k", "rad", "tau", "tp", "np", "rowptr", "sid", "wptr", "aptr"):
                bits(full[f], out[f], "%s against normal_scene" % f)
            half = model.diagnose_slices(wptr, out["A"], prior_ivar=prior, want_S=True, want_avk=True)
            for f in OUTS:
                bits(full[f], half[f], "%s against diagnose_slices" % f)
            for cap in (1, 257):
                bare = model.diagnose_scene(case.atm, geom, y, weight, prior_ivar=prior, max_rays_per_pass=cap)
                assert not any(f in bare for f in ("A", "b", "k", "S", "avk"))
                for f in VECTORS + ("dofs", "status", "cost", "nlive", "rad", "tau", "tp", "np"):
                    bits(bare[f], full[f], "%s with nothing wanted, cap %d" % (f, cap))
            if prior is not None:                                   # (without one most A_s are rank-deficient)
                assert np.all(full["status"] == 0)
                for s in range(ns):
                    As, _ = slice_of(out, s)
                    worst = merged(worst, check_system(As, prior[wptr[s]:wptr[s + 1]], system(full, wptr, aptr, s)))
        report("scene %s, %s views" % (name, view), worst)
    finally:
        model.close()


def test_after_a_retrieval(hip):
    """diagnose_scene on the atm of retrieve_scene's result with that call's prior: for every slice that converged,
    0 < dofs < the number of live elements, and sigma <= 1 / sqrt(r) within sigma's bound -- S <= R^-1 in the Loewner
    order because A is positive semi-definite, so the posterior is never wider than the prior."""
    import test_scene_retrieve_gpu as T
    name, mode = "ragged", hip.DAMP_PRIOR
    case, geom, y, weight = inputs(hip, name)
    lay, iq, ip, x0 = T.layout(hip, name)
    r, xa = T.seeded_prior(hip, name, lay, x0)
    got = T.retrieved(hip, name, mode, settings=dict(T.FLOW, tol=0.5, max_iter=8))
    converged = np.flatnonzero(got["state"] == hip.RET_CONVERGED)
    assert len(converged) > 0
    wptr, aptr = lay["wptr"], lay["aptr"]
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(got["atm"])
        res = model.diagnose_scene(got["atm"], geom, y, weight, prior_ivar=r, want_S=True, want_avk=True, want_normal=True)
        sequences.same_bits(formod_on(model, case.geom), got["after"], "the model holds atm_ret afterwards")
    finally:
        model.close()
    for s in converged:
        sl = slice(wptr[s], wptr[s + 1])
        As, _ = slice_of(res, s)
        ref = reference(As, r[sl])
        check_system(As, r[sl], system(res, wptr, aptr, s), ref)
        assert 0 < res["dofs"][s] < ref["n"]
        live = ref["live"]
        prior_var = 1 / r[sl][live].astype(LD)
        assert np.all(res["sigma"][sl][live].astype(LD) ** 2 <= prior_var + 2 * (np.diag(ref["ES"]) + gamma(2) * prior_var))
        print("DIAGNOSE retrieved slice %d: dofs %.3f of %d live elements, sigma / prior sigma %.3g .. %.3g"
              % (s, res["dofs"][s], ref["n"], np.min(res["sigma"][sl][live] * np.sqrt(r[sl][live])),
                 np.max(res["sigma"][sl][live] * np.sqrt(r[sl][live]))))


# ---- 7. refusals and empty calls -------------------------------------------------------------------------------------
def test_refusals_and_state(hip):
    case, geom, y, weight = inputs(hip, "ragged")
    _, out = blocks_and_sums(hip, "ragged")
    want = fresh_formod(hip, case, case.atm, case.geom)
    n, ns, na = int(out["wptr"][-1]), len(out["sfirst"]), int(out["aptr"][-1])
    ones = np.ones(n)

    def changed(a, at, v):
        a = a.copy()
        a[at] = v
        return a

    at = int(out["wptr"][1]) + 2                                    # element 2 of slice 1
    refused = [(changed(ones, at, -1.0), r"prior_ivar of slice 1, element 2 is -1"),
               (changed(ones, at, np.inf), r"prior_ivar of slice 1, element 2 is inf"),
               (changed(ones, at, np.nan), r"prior_ivar of slice 1, element 2 is nan")]
    lp_ = C.POINTER(C.c_long)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        good = model.diagnose_scene(case.atm, geom, y, weight, prior_ivar=ones)
        for r, message in refused:
            with pytest.raises(hip.JurassicError, match=r"error %d: jur_diagnose_scene_host: .*%s" % (hip.EINVAL, message)):
                model.diagnose_scene(case.atm, geom, y, weight, prior_ivar=r)
            sequences.same_bits(formod_on(model, case.geom), want, "after the refusal '%s'" % message)
            with pytest.raises(hip.JurassicError, match=r"error %d: jur_diagnose_slices_host: .*%s" % (hip.EINVAL, message)):
                model.diagnose_slices(out["wptr"], out["A"], prior_ivar=r)
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_diagnose_slices_host: wptr is not an ascending.*slice 1" % hip.EINVAL):
            model.diagnose_slices([0, 3, 2], np.zeros(10))
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_diagnose_slices_host: wptr is not an ascending.*slice 0" % hip.EINVAL):
            model.diagnose_slices([1, 2], np.zeros(1))
        # what jur_normal_scene_host refuses
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_diagnose_scene_host: rowptr is not" % hip.EINVAL):
            model.diagnose_scene(case.atm, geom, y, weight, rowptr=out["rowptr"] + 1)
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_diagnose_scene_host: the weight of ray 1, channel 0 is -1" % hip.EINVAL):
            model.diagnose_scene(case.atm, geom, y, changed(weight, (1, 0), -1.0))
        sequences.same_bits(formod_on(model, case.geom), want, "after the inherited refusals")
        # a NULL among the required outputs: only the C interface can pass one
        garr = (hip.dp * 7)(*[hip._p(g) for g in np.ascontiguousarray(geom.T)])
        for field in VECTORS + ("dofs", "status"):
            dout, keep, _ = hip._diag_structs(ns, n, na, None, False, False)
            setattr(dout, field, None)
            rc = hip.lib().jur_diagnose_slices_host(model.h, ns, out["wptr"].ctypes.data_as(lp_), hip._p(out["A"]), None, C.byref(dout))
            assert rc == hip.EINVAL and ("jur_diagnose_slices_host: null argument (%s)" % field) in hip.lib().jur_last_error().decode()
            rad, tau, tp = np.zeros(y.shape), np.zeros(y.shape), np.zeros((3, len(geom)))
            rc = hip.lib().jur_diagnose_scene_host(model.h, C.byref(case.atm), len(geom), garr, hip._p(rad), hip._p(tau),
                                                   (hip.dp * 3)(*[hip._p(t) for t in tp]), None, out["rowptr"].ctypes.data_as(lp_),
                                                   hip._p(y), hip._p(weight), None, C.byref(dout), None, None, None, None, None, 0)
            assert rc == hip.EINVAL and ("jur_diagnose_scene_host: null argument (%s)" % field) in hip.lib().jur_last_error().decode()
            sequences.same_bits(formod_on(model, case.geom), want, "after a NULL %s" % field)
        rc = hip.lib().jur_diagnose_slices_host(model.h, ns, out["wptr"].ctypes.data_as(lp_), hip._p(out["A"]), None, None)
        assert rc == hip.EINVAL and "null argument (out)" in hip.lib().jur_last_error().decode()
        # empty calls: nothing is written
        none = model.diagnose_slices([0], np.zeros(0), want_S=True, want_avk=True)   # nslice == 0
        assert none["sigma"].shape == (0,) and none["dofs"].shape == (0,) and none["S"].shape == (0,)
        empty = model.diagnose_slices([0, 0, 2, 2], np.eye(2), want_S=True)            # systems of width 0 beside one of 2
        assert list(empty["status"]) == [0, 0, 0] and list(empty["dofs"]) == [0, 2, 0] and is_plus_zero(empty["dofs"][[0, 2]])
        bits(empty["S"], np.eye(2).ravel(), "S of the identity")
        no_rays = model.diagnose_scene(case.atm, geom[:0], y[:0], weight[:0])         # nr == 0
        assert no_rays["sigma"].shape == (0,) and no_rays["dofs"].shape == (0,)
        sequences.same_bits(formod_on(model, case.geom), want, "after the empty calls")
        half = model.diagnose_slices(out["wptr"], out["A"], prior_ivar=ones)
        sequences.same_bits(formod_on(model, case.geom), want, "after diagnose_slices")
        again = model.diagnose_scene(case.atm, geom, y, weight, prior_ivar=ones)
        for f in VECTORS + ("dofs", "status"):
            bits(again[f], good[f], "%s in the call after the refusals" % f)
            bits(half[f], good[f], "%s of diagnose_slices" % f)
    finally:
        model.close()

    stateless = scene_case("lone_up", windows=None)                 # a state of zero elements: no retrieval window
    g = stateless.geom[:6]
    model = hip.Model(stateless.ctl, stateless.lib_tables())
    try:
        model.set_atm(stateless.atm)
        res = model.diagnose_scene(stateless.atm, g, np.zeros((6, stateless.ctl.nd)), np.ones((6, stateless.ctl.nd)))
        assert res["sigma"].shape == (0,) and res["dofs"].shape == (0,)
        sequences.same_bits(dict(rc=0, **{f: res[f] for f in ("rad", "tau", "tp", "np")}), formod_on(model, g), "state of zero elements")
    finally:
        model.close()

    hyd, _ = R.jacobian_case("jacobian_hydz10")
    shape = (len(hyd.geom), hyd.ctl.nd)
    want = fresh_formod(hip, hyd, hyd.atm, hyd.geom)
    model = hip.Model(hyd.ctl, hyd.lib_tables())
    try:
        model.set_atm(hyd.atm)
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_diagnose_scene_host: hydz" % hip.EINVAL):
            model.diagnose_scene(hyd.atm, hyd.geom, np.zeros(shape), np.ones(shape))
        sequences.same_bits(formod_on(model, hyd.geom), want, "after the hydz refusal")
    finally:
        model.close()


def test_scratch_beyond_the_budget_is_refused(hip):
    """The construction of tests/test_scene_solve_gpu.py::test_solver_scratch_beyond_the_budget_is_refused: one slice of
    1120 columns whose stacked copies (16.3 MB) and normal matrix (10.0 MB) fit into half of the smallest workspace budget
    (32 MiB of 64); the factor, S and AVK -- three more copies of the matrix -- do not fit beside them: JUR_ENOMEM before
    anything is launched, and the model answers as a fresh one."""
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
        with pytest.raises(hip.JurassicError, match=r"error -3: jur_diagnose_scene_host: .*the factor, S, AVK and the vectors"):
            model.diagnose_scene(case.atm, geom, y, weight)
        sequences.same_bits(formod_on(model, geom), want, "after the refusal")
    finally:
        model.close()
