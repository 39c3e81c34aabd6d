"""Model.solve_slices (jur_solve_slices_host) and Model.step_scene (jur_step_scene_host): the batched, ragged Cholesky
solve of the damped, optionally regularised normal equations of a scene's slices, on the device.

The error bounds are derived, not measured (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.).  With
u = 2^-53, gamma_m = m u / (1 - m u) and everything compared in np.longdouble, for a system of n live elements:
  Cholesky (Thm 10.3):       |M - L L^T| <= gamma_{n+1} |L| |L^T| + gamma_2 diag(M)
  solution (Thms 8.5, 10.4): |g - M dx|  <= gamma_{3n+1} |L| |L^T| |dx| + gamma_2 diag(M) |dx| + u |g|
  pred (dot product):        |pred - sum dx_i (g_i + lam s_i dx_i)| <= gamma_{n+3} sum (|dx_i g_i| + |lam s_i dx_i^2|)
The constants are the textbook ones: the kernel divides by the diagonal of L (true divisions, no reciprocals), takes one
correctly rounded square root per column, forms every inner product as a chain of fused multiply-adds (one rounding per
term, fewer than the bounds count) and uses no MFMA.  gamma_2 diag(M) covers the two roundings of
M_ii = fma(lam, s_i, A_ii + r_i), u |g| the one of g_i = fma(r_i, d_i, b_i).  A term of pred carries at most four roundings
(s_i, lam s_i, the inner fma, the product) and the sum of n terms at most n - 1 more, in whatever order.  The reference
M, g and s are formed in np.longdouble from the inputs.  Twice each bound is allowed.  Everything else is bit identity."""
import ctypes as C
import numpy as np
import pytest
import common
import sequences
from jurassic_hip import synth
from test_scene_jacobian_gpu import bits, formod_on, fresh_formod, scene_case
from test_scene_normal_gpu import SUMS, blocks_and_sums, bumped, copy_atm, inputs, slice_of

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
LD = np.longdouble
WIDTHS = (1, 2, 15, 16, 17, 31, 32, 33, 64, 100, 182)
LAMS = (0.0, 1e-3, 10.0)
STEP_LAMS = (1e-2, 1.0, 1e2)
OUTS = ("dx", "pred", "status", "L")


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


def gamma(m):
    return m * U / (1 - m * U)


def spd(rng, w):
    """G^T G + I of a seeded (w + 3) x w matrix, its two triangles bit-identical"""
    G = rng.standard_normal((w + 3, w))
    A = np.tril(G.T @ G + np.eye(w))
    return A + np.tril(A, -1).T


def pack(mats, vecs):
    """wptr, aptr, flat A, flat b of a list of systems"""
    w = np.array([len(v) for v in vecs], dtype=np.int64)
    wptr, aptr = np.concatenate([[0], np.cumsum(w)]), np.concatenate([[0], np.cumsum(w * w)])
    A = np.concatenate([m.ravel() for m in mats]) if mats else np.zeros(0)
    return wptr, aptr, A, np.concatenate(vecs) if vecs else np.zeros(0)


def system(res, wptr, aptr, l, s):
    """dx, pred, status, L (or None) of damping l, system s of a result"""
    w = int(wptr[s + 1] - wptr[s])
    L = res["L"][l, aptr[s]:aptr[s + 1]].reshape(w, w) if "L" in res else None
    return res["dx"][l, wptr[s]:wptr[s + 1]], res["pred"][l, s], int(res["status"][l, s]), L


def is_plus_zero(x):
    return np.all(np.ascontiguousarray(x, dtype=np.float64).view(np.uint64) == 0)


def check_system(A, b, lam, mode, r, d, dx, pred, status, L):
    """The three bounds of the module docstring on the live elements, the exact properties on the dead ones and above
    the diagonal; returns the worst error / allowed ratio."""
    w = len(b)
    r = np.zeros(w) if r is None else r
    d = np.zeros(w) if d is None else d
    live = (np.diag(A) + r) > 0
    n = int(live.sum())
    assert status == 0
    assert np.all(np.triu(L, 1) == 0), "L above the diagonal"
    assert np.all(np.diag(L) > 0)
    dead = np.flatnonzero(~live)
    assert is_plus_zero(dx[dead]) and np.all(np.diag(L)[dead] == 1)
    for i in dead:
        assert np.all(np.delete(L[i], i) == 0) and np.all(np.delete(L[:, i], i) == 0)
    if n == 0:
        assert pred == 0
        return 0.0
    ix = np.ix_(live, live)
    low = np.tril(A)
    Ms = (low + np.tril(low, -1).T).astype(LD)[ix]                  # (only the diagonal and the lower triangle are read)
    rl, dl, bl = r[live].astype(LD), d[live].astype(LD), b[live].astype(LD)
    D = np.diag(Ms) + rl
    s = rl if mode == 1 else D
    M = Ms.copy()
    M[np.diag_indices(n)] = D + LD(lam) * s
    g = rl * dl + bl
    Ll, x = L[ix].astype(LD), dx[live].astype(LD)
    LLa = np.abs(Ll) @ np.abs(Ll).T
    worst = 0.0
    tiny = np.finfo(LD).tiny

    def within(err, bound, what):
        nonlocal worst
        worst = max(worst, float(np.max(err / np.maximum(2 * bound, tiny))))
        assert np.all(err <= 2 * bound), (what, w, lam, float(np.max(err)), float(np.max(bound)))

    within(np.abs(M - Ll @ Ll.T), gamma(n + 1) * LLa + gamma(2) * np.diag(np.diag(M)), "factor")
    within(np.abs(g - M @ x), gamma(3 * n + 1) * (LLa @ np.abs(x)) + gamma(2) * np.diag(M) * np.abs(x) + U * np.abs(g), "solution")
    t1, t2 = x * g, LD(lam) * s * x * x
    within(np.abs(LD(pred) - (t1 + t2).sum()), gamma(n + 3) * (np.abs(t1) + np.abs(t2)).sum(), "pred")
    return worst


_batch = {}


def batch():
    """the ragged batch of test 1: (mats, vecs, wptr, aptr, A, b, prior_ivar, prior_dx), made once"""
    if not _batch:
        rng = np.random.default_rng(2024)
        mats = [spd(rng, w) for w in WIDTHS]
        vecs = [rng.standard_normal(w) for w in WIDTHS]
        wptr, aptr, A, b = pack(mats, vecs)
        r = 10.0 ** rng.uniform(-2.0, 1.0, len(b))
        d = rng.standard_normal(len(b))
        for a in mats + vecs + [A, b, r, d]:
            a.setflags(write=False)
        _batch["v"] = (mats, vecs, wptr, aptr, A, b, r, d)
    return _batch["v"]


def prior_of(mode):
    _, _, _, _, _, _, r, d = batch()
    return dict(mode=mode, prior_ivar=r, prior_dx=d) if mode == 1 else dict(mode=mode)


_solved = {}


def solved(model, mode):
    if mode not in _solved:
        _, _, wptr, _, A, b, _, _ = batch()
        _solved[mode] = model.solve_slices(wptr, A, b, LAMS, want_factor=True, **prior_of(mode))
    return _solved[mode]


@pytest.mark.parametrize("mode", [0, 1])
def test_constructed_systems(hip, model, mode):
    assert (hip.DAMP_MARQUARDT, hip.DAMP_PRIOR) == (0, 1)
    mats, vecs, wptr, aptr, _, _, r, d = batch()
    res = solved(model, mode)
    assert res["dx"].shape == (3, wptr[-1]) and res["pred"].shape == res["status"].shape == (3, len(WIDTHS))
    assert np.all(res["status"] == 0)
    worst = 0.0
    for l, lam in enumerate(LAMS):
        for s in range(len(WIDTHS)):
            pr = (r[wptr[s]:wptr[s + 1]], d[wptr[s]:wptr[s + 1]]) if mode == 1 else (None, None)
            worst = max(worst, check_system(mats[s], vecs[s], lam, mode, pr[0], pr[1], *system(res, wptr, aptr, l, s)))
    print("SOLVE constructed, mode %d: worst error / allowed %.3f" % (mode, worst))


def test_wider_than_a_workgroup(model):
    """257 and 300 columns: more rows than the 256 lanes, more than four 64-row chunks of a panel (not one of the
    issue's widths: the strided loops of the kernel take a second turn only from here on)"""
    rng = np.random.default_rng(7)
    mats = [spd(rng, w) for w in (257, 300)]
    vecs = [rng.standard_normal(w) for w in (257, 300)]
    wptr, aptr, A, b = pack(mats, vecs)
    res = model.solve_slices(wptr, A, b, (0.0, 10.0), want_factor=True)
    worst = 0.0
    for l, lam in enumerate((0.0, 10.0)):
        for s in range(2):
            worst = max(worst, check_system(mats[s], vecs[s], lam, 0, None, None, *system(res, wptr, aptr, l, s)))
    print("SOLVE wide: worst error / allowed %.3f" % worst)


def test_dead_elements_and_breakdown(model):
    rng = np.random.default_rng(5)
    holes = spd(rng, 40)
    for i in (0, 16, 39):
        holes[i, :] = 0.0
        holes[:, i] = 0.0
    zero_diag = spd(rng, 20)
    zero_diag[5, 5] = 0.0                                           # D_5 = 0 with non-zero off-diagonals: a caller's matrix
    cleared = zero_diag.copy()
    cleared[5, :] = 0.0
    cleared[:, 5] = 0.0
    indefinite = np.array([[1.0, 2.0], [2.0, 1.0]])
    edge = np.eye(17)
    edge[16, 0] = edge[0, 16] = 2.0
    with_nan = spd(rng, 33)
    with_nan[20, 3] = np.nan
    mats = [holes, zero_diag, cleared, indefinite, edge, with_nan, spd(rng, 33)]
    vecs = [rng.standard_normal(len(m)) for m in mats]
    vecs[2] = vecs[1]
    wptr, aptr, A, b = pack(mats, vecs)
    lams = (0.0, 10.0)
    res = model.solve_slices(wptr, A, b, lams, want_factor=True)
    get = lambda l, s: system(res, wptr, aptr, l, s)

    worst = 0.0
    for l, lam in enumerate(lams):
        dx, pred, status, L = get(l, 0)
        assert is_plus_zero(dx[[0, 16, 39]]) and np.all(np.diag(L)[[0, 16, 39]] == 1)
        worst = max(worst, check_system(holes, vecs[0], lam, 0, None, None, dx, pred, status, L))   # (against the compacted 37)
        assert np.count_nonzero(dx) == 37
        for got, want, f in zip(get(l, 1), get(l, 2), OUTS):       # ignored, not propagated
            bits(np.asarray(got), np.asarray(want), "%s of a dead element with off-diagonals" % f)
        worst = max(worst, check_system(zero_diag, vecs[1], lam, 0, None, None, *get(l, 1)))
    print("SOLVE dead elements: worst error / allowed %.3f" % worst)

    dx, pred, status, L = get(0, 3)
    assert status == 2 and is_plus_zero(dx) and is_plus_zero(pred) and is_plus_zero(L)
    dx, pred, status, L = get(1, 3)
    assert status == 0 and np.all(dx != 0) and pred > 0
    check_system(indefinite, vecs[3], 10.0, 0, None, None, dx, pred, status, L)
    dx, pred, status, L = get(0, 4)
    assert status == 17 and is_plus_zero(dx) and is_plus_zero(pred) and is_plus_zero(L)   # across a 16-column panel edge
    assert get(1, 4)[2] == 0
    for l in range(2):
        dx, pred, status, L = get(l, 5)
        assert status != 0 and is_plus_zero(dx) and is_plus_zero(pred) and is_plus_zero(L)
    for s in (0, 1, 2, 6):                                         # the other systems of the batch: as their solo solves
        solo = model.solve_slices([0, len(vecs[s])], mats[s], vecs[s], lams, want_factor=True)
        for l in range(2):
            for got, want, f in zip(get(l, s), system(solo, [0, len(vecs[s])], [0, len(vecs[s]) ** 2], l, 0), OUTS):
                bits(np.asarray(got), np.asarray(want), "%s of system %d beside a NaN" % (f, s))
            assert get(l, s)[2] == 0


@pytest.mark.parametrize("mode", [0, 1])
def test_independence(model, mode):
    mats, vecs, wptr, aptr, A, b, r, d = batch()
    res = solved(model, mode)
    ns = len(WIDTHS)
    for s in range(ns):                                             # each system alone
        kw = dict(mode=mode)
        if mode == 1:
            kw.update(prior_ivar=r[wptr[s]:wptr[s + 1]], prior_dx=d[wptr[s]:wptr[s + 1]])
        w = WIDTHS[s]
        solo = model.solve_slices([0, w], mats[s], vecs[s], LAMS, want_factor=True, **kw)
        for l in range(3):
            for got, want, f in zip(system(res, wptr, aptr, l, s), system(solo, [0, w], [0, w * w], l, 0), OUTS):
                bits(np.asarray(got), np.asarray(want), "%s of system %d alone" % (f, s))
    rw, ra, rA, rb = pack(mats[::-1], vecs[::-1])                    # the batch reversed
    kw = dict(mode=mode)
    if mode == 1:
        kw.update(prior_ivar=np.concatenate([r[wptr[s]:wptr[s + 1]] for s in range(ns)][::-1]),
                  prior_dx=np.concatenate([d[wptr[s]:wptr[s + 1]] for s in range(ns)][::-1]))
    rev = model.solve_slices(rw, rA, rb, LAMS, want_factor=True, **kw)
    for s in range(ns):
        for l in range(3):
            for got, want, f in zip(system(res, wptr, aptr, l, s), system(rev, rw, ra, l, ns - 1 - s), OUTS):
                bits(np.asarray(got), np.asarray(want), "%s of system %d reversed" % (f, s))
    for l, lam in enumerate(LAMS):                                  # one call per damping
        one = model.solve_slices(wptr, A, b, lam, want_factor=True, **prior_of(mode))
        for f in OUTS:
            bits(one[f][0], res[f][l], "%s with nlam = 1, damping %g" % (f, lam))


@pytest.mark.parametrize("name", ["ragged", "lone_ends"])
def test_fused_entry_equals_its_halves(hip, name):
    case, geom, y, weight = inputs(hip, name)
    _, out = blocks_and_sums(hip, name)
    assert np.diff(out["wptr"]).max() > 32 and 257 < out["rowptr"][-1] + len(geom)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        full = model.step_scene(case.atm, geom, y, weight, STEP_LAMS, want_normal=True, want_k=True, want_factor=True)
        for f in SUMS + ("k", "rad", "tau", "tp", "np", "rowptr", "sid", "wptr", "aptr"):
            bits(full[f], out[f], "%s against normal_scene" % f)
        half = model.solve_slices(out["wptr"], out["A"], out["b"], STEP_LAMS, want_factor=True)
        for f in OUTS:
            bits(full[f], half[f], "%s against solve_slices" % f)
        assert np.all(full["status"] == 0) and np.all(full["pred"] >= 0) and np.any(full["pred"] > 0)
        for cap in (1, 257, 0):
            bare = model.step_scene(case.atm, geom, y, weight, STEP_LAMS, max_rays_per_pass=cap)
            assert not any(f in bare for f in ("A", "b", "k", "L"))
            for f in ("dx", "pred", "status", "cost", "nlive", "rad", "tau", "tp", "np"):
                bits(bare[f], full[f], "%s with nothing wanted, cap %d" % (f, cap))
    finally:
        model.close()


def test_priors(hip):
    """ragged has 12 measurements per time stamp, so every A_s wider than that is rank-deficient; a prior with r > 0 on
    every element (here 1e-3 .. 1e-1 of the mean diagonal of A_s, seeded) makes A_s + R positive definite, so every
    slice is solved at lambda = 0 in both modes.  Without a prior, under Marquardt damping, the elements no ray feels
    have D = 0: dead, exact zeros.  (The six rays per time stamp of the other tests include nadir views, which feel every
    element; the scene's limb views with tangent heights of 28 to 39 km alone pass above most of the retrieval windows.)"""
    case, geom, y, weight = inputs(hip, "ragged")
    _, out = blocks_and_sums(hip, "ragged")
    ns, wptr, aptr = len(out["sfirst"]), out["wptr"], out["aptr"]
    assert np.any(np.diff(wptr) > out["nlive"])                     # fewer measurements than elements: rank-deficient
    rng = np.random.default_rng(3)
    r = np.concatenate([10.0 ** rng.uniform(-3.0, -1.0, len(bs)) * np.diag(As).mean() for As, bs in (slice_of(out, s) for s in range(ns))])
    d = rng.standard_normal(len(r)) * 1e-3
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        worst = 0.0
        for mode in (hip.DAMP_MARQUARDT, hip.DAMP_PRIOR):
            res = model.step_scene(case.atm, geom, y, weight, 0.0, mode=mode, prior_ivar=r, prior_dx=d, want_normal=True,
                                   want_factor=True)
            for f in ("A", "b"):
                bits(res[f], out[f], f)
            for s in range(ns):
                As, bs = slice_of(out, s)
                sl = slice(wptr[s], wptr[s + 1])
                worst = max(worst, check_system(As, bs, 0.0, mode, r[sl], d[sl], *system(res, wptr, aptr, 0, s)))
        print("SOLVE priors: worst error / allowed %.3f" % worst)
        g = case.geom
        high = g[(g[:, 1] > 700.0) & (g[:, 4] > 28.0) & (g[:, 4] < 39.0)]
        assert len(high) >= 4
        y_high = fresh_formod(hip, case, bumped(case), high)["rad"]
        model.set_atm(case.atm)
        res = model.step_scene(case.atm, high, y_high, np.ones(y_high.shape), 1.0, want_normal=True, want_factor=True)
    finally:
        model.close()
    ns, wptr, aptr = len(res["sfirst"]), res["wptr"], res["aptr"]
    unfelt = np.concatenate([np.diag(slice_of(res, s)[0]) == 0 for s in range(ns)])
    assert ns >= 2 and unfelt.any() and not unfelt.all()
    assert np.all(res["status"] == 0)
    assert is_plus_zero(res["dx"][0][unfelt]) and np.any(res["dx"][0][~unfelt] != 0)
    worst = 0.0
    for s in range(ns):
        As, bs = slice_of(res, s)
        worst = max(worst, check_system(As, bs, 1.0, 0, None, None, *system(res, wptr, aptr, 0, s)))   # (L_ii = 1 where dead)
    print("SOLVE unfelt elements: %d of %d, worst error / allowed %.3f" % (unfelt.sum(), len(unfelt), worst))


def test_closing_the_loop_on_the_device(hip):
    """test_scene_normal_gpu.py::test_closing_the_loop with the steps of all three dampings from ONE step_scene call and
    no linear algebra on the host: written back through scene_elements, the summed cost falls for at least one damping
    (the condition argued there: M is positive definite on the live elements and b = -1/2 grad cost, so dx is a descent
    direction, and for a large enough lambda the step is short enough for the cost to follow its slope)."""
    case, geom, y, weight = inputs(hip, "ragged")
    ratios = {}
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        step = model.step_scene(case.atm, geom, y, weight, STEP_LAMS)
        assert np.all(step["status"] == 0)
        before = float(step["cost"].sum())
        for l, lam in enumerate(STEP_LAMS):
            atm = copy_atm(case.atm)
            rows = [np.ctypeslib.as_array(atm.p), np.ctypeslib.as_array(atm.t)]
            rows += list(np.ctypeslib.as_array(atm.q)[:case.ctl.ng]) + list(np.ctypeslib.as_array(atm.k)[:case.ctl.nw])
            for s in range(len(step["sfirst"])):
                dx = step["dx"][l, step["wptr"][s]:step["wptr"][s + 1]]
                el = hip.scene_elements(case.ctl, case.atm, step["sfirst"][s], step["slen"][s])
                assert len(dx) == len(el["cols"])
                for e in range(len(dx)):
                    rows[el["iq"][e]][el["ip"][e]] += dx[e]
            model.set_atm(atm)
            after = float(model.normal_scene(atm, geom, y, weight)["cost"].sum())
            ratios[lam] = after / before
            print("SOLVE step: lambda %g cost after / before %.4e, predicted decrease / before %.4e"
                  % (lam, ratios[lam], step["pred"][l].sum() / before))
    finally:
        model.close()
    assert before > 0 and any(q < 1.0 for q in ratios.values()), ratios


def test_refusals_and_state(hip):
    case, geom, y, weight = inputs(hip, "ragged")
    _, out = blocks_and_sums(hip, "ragged")
    want = fresh_formod(hip, case, case.atm, case.geom)
    n, ns = int(out["wptr"][-1]), len(out["sfirst"])
    ones, zeros = np.ones(n), np.zeros(n)

    def changed(a, at, v):
        a = a.copy()
        a[at] = v
        return a

    at = int(out["wptr"][1]) + 2                                    # element 2 of slice 1
    lam2 = np.ones((2, ns))
    refused = [
        (dict(lam=np.zeros(0)), r"nlam = 0"),
        (dict(lam=1.0, mode=7), r"unknown mode 7"),
        (dict(lam=changed(lam2, (1, 1), -1.0)), r"lam of slice 1, damping 1 is -1"),
        (dict(lam=changed(lam2, (0, 1), np.nan)), r"lam of slice 1, damping 0 is nan"),
        (dict(lam=changed(lam2, (1, 0), np.inf)), r"lam of slice 0, damping 1 is inf"),
        (dict(lam=1.0, prior_ivar=changed(ones, at, -1.0), prior_dx=zeros), r"prior_ivar of slice 1, element 2 is -1"),
        (dict(lam=1.0, prior_ivar=changed(ones, at, np.inf), prior_dx=zeros), r"prior_ivar of slice 1, element 2 is inf"),
        (dict(lam=1.0, prior_ivar=changed(ones, at, np.nan), prior_dx=zeros), r"prior_ivar of slice 1, element 2 is nan"),
        (dict(lam=1.0, prior_ivar=ones, prior_dx=changed(zeros, at, np.nan)), r"prior_dx of slice 1, element 2 is nan"),
        (dict(lam=1.0, prior_ivar=ones), r"prior_ivar without prior_dx"),
        (dict(lam=1.0, prior_dx=zeros), r"prior_dx without prior_ivar"),
        (dict(lam=1.0, mode=hip.DAMP_PRIOR), r"JUR_DAMP_PRIOR without a prior"),
    ]
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        good = model.step_scene(case.atm, geom, y, weight, STEP_LAMS)
        sequences.same_bits(formod_on(model, case.geom), want, "after a call")
        for kw, message in refused:
            kw = dict(kw)
            lam = kw.pop("lam")
            with pytest.raises(hip.JurassicError, match=r"error %d: jur_step_scene_host: .*%s" % (hip.EINVAL, message)):
                model.step_scene(case.atm, geom, y, weight, lam, **kw)
            sequences.same_bits(formod_on(model, case.geom), want, "after the refusal '%s'" % message)
            with pytest.raises(hip.JurassicError, match=r"error %d: jur_solve_slices_host: .*%s" % (hip.EINVAL, message)):
                model.solve_slices(out["wptr"], out["A"], out["b"], lam, **kw)
        # a NULL among lam, dx, pred, status: only the C interface can pass one
        lp_ = C.POINTER(C.c_long)
        columns = np.ascontiguousarray(geom.T)
        garr = (hip.dp * 7)(*[hip._p(g) for g in columns])
        for field in ("lam", "dx", "pred", "status"):
            sin, sout, _, keep = hip._solve_structs(ns, n, int(out["aptr"][-1]), 1.0, 0, None, None, False)
            setattr(sin if field == "lam" else sout, field, None)
            rc = hip.lib().jur_solve_slices_host(model.h, ns, out["wptr"].ctypes.data_as(lp_), hip._p(out["A"]), hip._p(out["b"]),
                                                 C.byref(sin), C.byref(sout))
            assert rc == hip.EINVAL and ("null argument (%s)" % field) in hip.lib().jur_last_error().decode()
            rad, tau, tp = np.zeros(y.shape), np.zeros(y.shape), np.zeros((3, len(geom)))
            cost, nlive = np.zeros(ns), np.zeros(ns, dtype=np.int64)
            rc = hip.lib().jur_step_scene_host(model.h, C.byref(case.atm), len(geom), garr, hip._p(rad), hip._p(tau),
                                               (hip.dp * 3)(*[hip._p(t) for t in tp]), None, out["rowptr"].ctypes.data_as(lp_),
                                               hip._p(y), hip._p(weight), C.byref(sin), C.byref(sout), None, None,
                                               hip._p(cost), nlive.ctypes.data_as(lp_), None, 0)
            assert rc == hip.EINVAL and ("jur_step_scene_host: null argument (%s)" % field) in hip.lib().jur_last_error().decode()
            sequences.same_bits(formod_on(model, case.geom), want, "after a NULL %s" % field)
        none = model.solve_slices([0], np.zeros(0), np.zeros(0), 1.0)                 # nslice == 0
        assert none["dx"].shape == (1, 0) and none["pred"].shape == (1, 0)
        half = model.solve_slices(out["wptr"], out["A"], out["b"], STEP_LAMS)
        sequences.same_bits(formod_on(model, case.geom), want, "after solve_slices")
        again = model.step_scene(case.atm, geom, y, weight, STEP_LAMS)
        for f in ("dx", "pred", "status"):
            bits(again[f], good[f], "%s in the call after the refusals" % f)
            bits(half[f], good[f], "%s of solve_slices" % f)
    finally:
        model.close()


def test_solver_scratch_beyond_the_budget_is_refused(hip):
    """The construction of test_scene_normal_gpu.py::test_accumulators_beyond_the_budget_are_refused with a profile of 140
    levels: 1120 columns.  Its stacked copies (16.3 MB) and the 1120^2 doubles of its normal matrix (10.0 MB) fit into
    half of the smallest workspace budget (32 MiB of 64) together, a second copy of the matrix, the solver's scratch,
    does not fit beside them: normal_scene is accepted and runs, step_scene returns JUR_ENOMEM before anything is
    launched, and the model answers as a fresh one."""
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
        # stacked atmosphere: 6 + ng + nw rows and the pressure slopes for the base points and one copy of the slice per element
        stack = 8 * (7 + c.ng + c.nw) * (case.atm.np + int((np.diff(lay["wptr"]) * lay["slen"]).sum()))
        matrix, half, small = 8 * int(lay["aptr"][-1]), (64 << 20) // 2, 1 << 20
        assert stack + matrix + small < half < stack + 2 * matrix       # (small: b, y, weight, the running sums, the outputs)
        out = model.normal_scene(case.atm, geom, y, weight)
        assert out["nlive"][0] == 2 * c.nd
        with pytest.raises(hip.JurassicError, match=r"error -3: jur_step_scene_host: .*solver scratch"):
            model.step_scene(case.atm, geom, y, weight, 1.0)
        sequences.same_bits(formod_on(model, geom), want, "after the refusal")
    finally:
        model.close()
