"""Model.param_slices (jur_param_slices_host), Model.set_ret_windows and lib.param_error_scene: the cross-state matrix
C_s = G_s^T Kb_s of every slice over the ragged blocks and the parameter-error budget sigma_param = sqrt(diag(C Sigma C^T)),
on the device.

The error bounds are derived, not measured (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.).  With
u = 2^-53 and gamma_n = n u / (1 - n u); the references are formed in np.longdouble from the gain and the blocks that were
passed in (their own error, of the order n 2^-64, is 2^-11 of what follows):
  C.  c^ is a chain of fused multiply-adds over the m live measurements of the slice (what is not live adds exact zeros):
      |C^ - C*| <= EC = gamma_m |G|^T |Kb|                                               (Higham 3.1, 3.4)
  diagonal radicand.  q^ is a chain of wb fused multiply-adds whose terms carry one more rounding (c * c is rounded
      first), on the c^ the first kernel wrote; c^2 is within 2 |c*| EC + EC^2 of c*^2:
      |q^ - q*| <= BD = gamma_{wb+2} sum_j (|c*| + EC)^2 v_j + sum_j (2 |c*| EC + EC^2) v_j
  full radicand.  t^_j is a chain of wb fused multiply-adds and q^ a chain of wb more on the t^_j, nested inner
      products: |q^ - c^ Sigma c^T| <= gamma_{2 wb} |c^| |Sigma| |c^|^T, and c^ Sigma c^T is within
      2 |c*| |Sigma| EC^T + EC |Sigma| EC^T of q* = c* Sigma c*^T:
      |q^ - q*| <= BF = gamma_{2 wb} (|c*| + EC) |Sigma| (|c*| + EC)^T + 2 |c*| |Sigma| EC^T + EC |Sigma| EC^T
  a correctly rounded square root: sigma_param^2 is held to q* within B + gamma_2 |q*| (where q^ <= 0 the entry writes
      +0.0, and q* is then within B of 0).  Every Sigma of these tests is positive definite, so q* >= 0.
Twice each bound is allowed, as in tests/test_scene_gain_gpu.py.  The kernels form every inner product as a chain of fused
multiply-adds in the documented order and use no MFMA.  Everything else is bit identity.

Test 1 pairs the widths 1, 7, 63, 64, 65, 130 and 300 so that w and wb differ in every slice and each crosses the tile
edge (64) on its own, with 1, 7, 15, 16, 17, 63, 64, 65 and 130 measurement rows a slice (the staging depth 16 and the
tile): exactly with nd = 1; with nd = 3 a slice has whole rays, so 3, 9, 15, 18, 18, 63, 66, 66 and 132 rows.  A tenth of
the measurements is not live, one ray without a slice leads, one slice has wb = 0.

Test 5, with the notation of tests/test_scene_gain_gpu.py (identity 1 of its docstring): the device sum C^ replaces the
host's sum_m G^_mi K_mj, so  |C^_ij - AVK^_ij| <= (E_S |A^| + |S^| gamma_{M+4} |K|^T W |K| + E^T |K| + E_K)_ij
+ gamma_M (|G^|^T |K|)_ij.  It runs on the ragged scene that tests/test_scene_gain_gpu.py builds on common.limb_case()."""
import ctypes as C
import numpy as np
import pytest
import common
from jurassic_hip import abi
from test_scene_jacobian_gpu import bits, scene_case, six_per_time_stamp
from test_scene_normal_gpu import inputs, interleaved
from test_scene_solve_gpu import gamma, is_plus_zero, spd
from test_scene_diagnose_gpu import reference as diag_reference
import test_scene_gain_gpu as G

pytestmark = pytest.mark.gpu
LD = np.longdouble
WIDTHS = (1, 7, 63, 64, 65, 130, 300)
ROWS = (1, 7, 15, 16, 17, 63, 64, 65, 130)
SENT = -7.25


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


# ---- synthetic problems ----------------------------------------------------------------------------------------------
def shapes_of_test_1(nd):
    """(w, wb, rays): every width meets two others as wb, every row count is met; the last slice has wb = 0"""
    out = []
    for i, w in enumerate(WIDTHS):
        out += [(w, WIDTHS[(i + 2) % 7], ROWS[(2 * i) % 9]), (w, WIDTHS[(i + 5) % 7], ROWS[(2 * i + 1) % 9])]
    out += [(64, 65, 130), (7, 0, 17)]
    return [(w, wb, -(-rows // nd)) for w, wb, rows in out]


def running(a):
    return np.concatenate([[0], np.cumsum(a)]).astype(np.int64)


def problem(hip, seed, shapes, nd, nvar, ncov):
    """A ragged problem: slice s has w = shapes[s][0] state elements, wb = shapes[s][1] parameters and shapes[s][2] rays
    of nd channels; one ray without a slice leads (two columns in rowptr_b: not looked at).  A tenth of the measurements
    is not live (weight 0).  The full covariances are positive definite with bit-identical triangles."""
    rng = np.random.default_rng(seed)
    sid = np.concatenate([[-1]] + [np.full(n, s) for s, (_, _, n) in enumerate(shapes)]).astype(np.int32)
    w = np.array([0 if s < 0 else shapes[s][0] for s in sid])
    wb = np.array([2 if s < 0 else shapes[s][1] for s in sid])
    wptr = running([x[0] for x in shapes])
    rowptr, rowptr_b = running(w), running(wb)
    nr = len(sid)
    gain = rng.standard_normal(int(rowptr[-1]) * nd)
    kb = rng.standard_normal(int(rowptr_b[-1]) * nd)
    weff = 10.0 ** rng.uniform(-1.0, 1.0, (nr, nd))
    weff[rng.uniform(size=(nr, nd)) < 0.1] = 0.0
    lay = hip.param_layout(wptr, rowptr, rowptr_b, sid)
    assert list(np.diff(lay["bwptr"])) == [x[1] for x in shapes]
    var = 10.0 ** rng.uniform(-2.0, 0.0, (nvar, int(lay["bwptr"][-1])))
    cov = np.zeros((ncov, int(lay["bbptr"][-1])))
    for c in range(ncov):
        cov[c] = np.concatenate([np.zeros(0)] + [(spd(rng, x[1]) * 10.0 ** rng.uniform(-2.0, 0.0)).ravel() for x in shapes])
    return dict(lay, wptr=wptr, rowptr=rowptr, rowptr_b=rowptr_b, sid=sid, gain=gain, kb=kb, weff=weff, var=var, cov=cov, nd=nd)


def call(model, p, **kw):
    args = dict(var=p["var"] if p["var"].shape[0] else None, cov=p["cov"] if p["cov"].shape[0] else None)
    args.update(kw)
    return model.param_slices(p["wptr"], p["rowptr"], p["rowptr_b"], p["sid"], p["gain"], p["kb"], p["weff"], **args)


def rows_of(p, flat, rowptr, s):
    """the rows of slice s of an array laid out as blocks under rowptr, (measurements, width), in measurement order"""
    nd = p["nd"]
    rays = np.flatnonzero(p["sid"] == s)
    width = int(rowptr[rays[0] + 1] - rowptr[rays[0]]) if len(rays) else 0
    if len(rays) == 0:
        return np.zeros((0, 0))
    return np.concatenate([flat[rowptr[r] * nd:rowptr[r + 1] * nd].reshape(nd, width) for r in rays])


def C_of(p, res, s):
    w, wb = int(p["wptr"][s + 1] - p["wptr"][s]), int(p["bwptr"][s + 1] - p["bwptr"][s])
    return res["C"][p["cptr"][s]:p["cptr"][s + 1]].reshape(w, wb)


def sigma_of(p, res, s):
    return res["sigma_param"][:, p["wptr"][s]:p["wptr"][s + 1]]


def sym(flat, wb):
    """Sigma as the entry reads it: the diagonal and the lower triangle, mirrored"""
    L = np.tril(flat.reshape(wb, wb))
    return L + np.tril(L, -1).T


def param_reference(p, s):
    """C*, EC and per component q*, B of the module docstring for slice s, in np.longdouble"""
    w, wb = int(p["wptr"][s + 1] - p["wptr"][s]), int(p["bwptr"][s + 1] - p["bwptr"][s])
    rays = np.flatnonzero(p["sid"] == s)
    with np.errstate(invalid="ignore"):
        lm = (p["weff"][rays] > 0).ravel()
    m = int(lm.sum())
    if len(rays) and wb:
        Gm = rows_of(p, p["gain"], p["rowptr"], s)[lm].astype(LD)
        Km = rows_of(p, p["kb"], p["rowptr_b"], s)[lm].astype(LD)
    else:
        Gm, Km = np.zeros((0, w), dtype=LD), np.zeros((0, wb), dtype=LD)
    Cs = Gm.T @ Km
    EC = gamma(m) * (np.abs(Gm).T @ np.abs(Km))
    a = np.abs(Cs)
    q, B = [], []
    for v in p["var"]:
        vs = v[p["bwptr"][s]:p["bwptr"][s + 1]].astype(LD)
        q.append((Cs * Cs) @ vs)
        B.append(gamma(wb + 2) * (((a + EC) ** 2) @ vs) + (2 * a * EC + EC * EC) @ vs)
    for f in p["cov"]:
        Sg = sym(f[p["bbptr"][s]:p["bbptr"][s + 1]], wb).astype(LD)
        aS = np.abs(Sg)
        q.append(((Cs @ Sg) * Cs).sum(axis=1))
        eS = EC @ aS
        B.append(gamma(2 * wb) * (((a + EC) @ aS) * (a + EC)).sum(axis=1) + (2 * a * eS).sum(axis=1) + (EC * eS).sum(axis=1))
    ncomp = len(q)
    return dict(C=Cs, EC=EC, m=m, q=np.array(q, dtype=LD).reshape(ncomp, w), B=np.array(B, dtype=LD).reshape(ncomp, w))


def check_slice(p, res, s, worst, ref=None):
    ref = ref or param_reference(p, s)
    tiny = np.finfo(LD).tiny
    Cs = C_of(p, res, s)
    assert np.all(np.isfinite(Cs))
    err = np.abs(Cs.astype(LD) - ref["C"])
    print("PARAM slice %d: C %s, m %d, worst error %.3g, bound %.3g" % (s, Cs.shape, ref["m"], float(err.max()) if err.size else 0.0,
                                                                       float(ref["EC"].max()) if err.size else 0.0))
    assert np.all(err <= 2 * ref["EC"]), ("C", s, float(err.max()), float(ref["EC"].max()))
    if Cs.size:
        worst["C"] = max(worst.get("C", 0.0), float(np.max(err / np.maximum(2 * ref["EC"], tiny))))
    sig = sigma_of(p, res, s)
    if sig.size:
        assert np.all(np.isfinite(sig)) and np.all(sig >= 0)
        bound = ref["B"] + gamma(2) * np.abs(ref["q"])
        err = np.abs(sig.astype(LD) ** 2 - ref["q"])
        print("PARAM slice %d: sigma_param worst error %.3g, bound %.3g" % (s, float(err.max()), float(bound.max())))
        assert np.all(err <= 2 * bound), ("sigma_param", s, float(err.max()), float(bound.max()))
        worst["sigma_param"] = max(worst.get("sigma_param", 0.0), float(np.max(err / np.maximum(2 * bound, tiny))))
    return ref


def report(what, worst):
    print("PARAM %s: worst error / allowed %s" % (what, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


# ---- 1. synthetic systems against np.longdouble ----------------------------------------------------------------------
_made = {}


def made(hip, model, nd):
    if nd not in _made:
        p = problem(hip, 70 + nd, shapes_of_test_1(nd), nd, 2 if nd == 1 else 1, 1 if nd == 1 else 2)
        _made[nd] = (p, call(model, p))
    return _made[nd]


@pytest.mark.parametrize("nd", [1, 3])
def test_synthetic_systems(hip, model, nd):
    p, res = made(hip, model, nd)
    ns = len(p["wptr"]) - 1
    assert res["C"].shape == (p["cptr"][-1],) and res["sigma_param"].shape == (3, p["wptr"][-1])
    worst, rows, pairs = {}, set(), set()
    for s in range(ns):
        check_slice(p, res, s, worst)
        rows.add(int((p["sid"] == s).sum()) * nd)
        pairs.add((int(np.diff(p["wptr"])[s]), int(np.diff(p["bwptr"])[s])))
    assert rows >= (set(ROWS) if nd == 1 else {3, 9, 15, 18, 63, 66, 132})
    assert all(a != b for a, b in pairs) and {a for a, _ in pairs} >= set(WIDTHS) and {b for _, b in pairs} >= set(WIDTHS) | {0}
    assert C_of(p, res, ns - 1).size == 0 and is_plus_zero(sigma_of(p, res, ns - 1)), "a slice with wb == 0"
    assert np.abs(res["C"]).max() > 0 and res["sigma_param"].max() > 0
    report("synthetic, nd %d, %d slices" % (nd, ns), worst)


# ---- 2. rows that are not live are never read --------------------------------------------------------------------------
def poisoned(p):
    """NaN in gain and kb on every row that is not live"""
    q = dict(p, gain=p["gain"].copy(), kb=p["kb"].copy())
    nd = p["nd"]
    for r in range(len(p["sid"])):
        for flat, rp in ((q["gain"], p["rowptr"]), (q["kb"], p["rowptr_b"])):
            width = int(rp[r + 1] - rp[r])
            for i in range(nd):
                if not p["weff"][r, i] > 0 or p["sid"][r] < 0:
                    flat[rp[r] * nd + i * width:rp[r] * nd + (i + 1) * width] = np.nan
    return q


def test_rows_that_are_not_live_are_never_read(hip, model):
    p, res = made(hip, model, 3)
    nd = 3
    q = poisoned(p)
    assert np.isnan(q["kb"]).sum() > 0 and np.isnan(q["gain"]).sum() > 0
    # anything not > 0 is "not live": a negative weight and a NaN
    dead = np.argwhere(~(p["weff"] > 0) & (p["sid"] >= 0)[:, None])
    q["weff"] = p["weff"].copy()
    q["weff"][tuple(dead[0])] = -1.0
    q["weff"][tuple(dead[1])] = np.nan
    got = call(model, q)
    assert np.all(np.isfinite(got["C"])) and np.all(np.isfinite(got["sigma_param"]))
    bits(got["C"], res["C"], "C with NaN on the rows that are not live")
    bits(got["sigma_param"], res["sigma_param"], "sigma_param with NaN on the rows that are not live")
    # a NaN in one live row of kb, column j: exactly column j of that slice's C, and the components over that slice
    s, j = 4, 5
    w, wb = int(np.diff(p["wptr"])[s]), int(np.diff(p["bwptr"])[s])
    assert wb > j and w > 1
    rays = np.flatnonzero(p["sid"] == s)
    r, i = next((r, i) for r in rays for i in range(nd) if p["weff"][r, i] > 0)
    q["kb"][p["rowptr_b"][r] * nd + i * wb + j] = np.nan
    got = call(model, q)
    Cs = C_of(p, got, s)
    assert np.all(np.isnan(Cs[:, j])) and np.all(np.isfinite(np.delete(Cs, j, axis=1)))
    bits(np.delete(Cs, j, axis=1), np.delete(C_of(p, res, s), j, axis=1), "the other columns of the slice")
    assert np.all(np.isnan(sigma_of(p, got, s)))
    for t in range(len(p["wptr"]) - 1):
        if t != s:
            bits(C_of(p, got, t), C_of(p, res, t), "C of slice %d beside a NaN" % t)
            bits(sigma_of(p, got, t), sigma_of(p, res, t), "sigma_param of slice %d beside a NaN" % t)


# ---- 3. invariance, bit for bit ---------------------------------------------------------------------------------------
def sub(p, order, perm=None):
    """the slices `order` of a problem, in that order, with their rays (and those without a slice) in the order perm
    gives them (default: as they lie)"""
    nd = p["nd"]
    new = {int(s): j for j, s in enumerate(order)}
    rays = [int(r) for r in (range(len(p["sid"])) if perm is None else perm) if p["sid"][r] < 0 or int(p["sid"][r]) in new]
    sid = np.array([-1 if p["sid"][r] < 0 else new[int(p["sid"][r])] for r in rays], dtype=np.int32)
    w, wb = np.diff(p["wptr"]), np.diff(p["bwptr"])
    cut = lambda flat, rp: np.concatenate([flat[rp[r] * nd:rp[r + 1] * nd] for r in rays] + [np.zeros(0)])
    return dict(wptr=running([w[s] for s in order]), bwptr=running([wb[s] for s in order]),
                cptr=running([w[s] * wb[s] for s in order]), bbptr=running([wb[s] ** 2 for s in order]), sid=sid,
                rowptr=running([p["rowptr"][r + 1] - p["rowptr"][r] for r in rays]),
                rowptr_b=running([p["rowptr_b"][r + 1] - p["rowptr_b"][r] for r in rays]),
                gain=cut(p["gain"], p["rowptr"]), kb=cut(p["kb"], p["rowptr_b"]), weff=p["weff"][rays], nd=nd,
                var=np.concatenate([p["var"][:, p["bwptr"][s]:p["bwptr"][s + 1]] for s in order] + [np.zeros((p["var"].shape[0], 0))], axis=1),
                cov=np.concatenate([p["cov"][:, p["bbptr"][s]:p["bbptr"][s + 1]] for s in order] + [np.zeros((p["cov"].shape[0], 0))], axis=1))


@pytest.mark.parametrize("nd", [1, 3])
def test_invariance(hip, model, nd):
    p, res = made(hip, model, nd)
    ns = len(p["wptr"]) - 1

    def same(q, got, order, what):
        for name in ("bwptr", "cptr", "bbptr"):
            assert np.array_equal(got[name], q[name]), (name, what)
        for j, s in enumerate(order):
            bits(C_of(q, got, j), C_of(p, res, s), "C of slice %d %s" % (s, what))
            bits(sigma_of(q, got, j), sigma_of(p, res, s), "sigma_param of slice %d %s" % (s, what))

    for s in range(ns):                                             # each slice alone
        q = sub(p, [s])
        same(q, call(model, q), [s], "alone")
    order = list(range(ns))[::-1]                                   # the slices in reversed order, the rays where they were
    q = sub(p, order)
    same(q, call(model, q), order, "reversed")
    perm = interleaved(p["sid"])                                    # the rays of the slices dealt out in turn
    assert np.any(np.diff(p["sid"][perm][:6]) != 0)
    q = sub(p, list(range(ns)), perm)
    same(q, call(model, q), list(range(ns)), "interleaved")
    bare = call(model, p, want_C=False)                             # C not asked for
    assert "C" not in bare
    bits(bare["sigma_param"], res["sigma_param"], "sigma_param with C not asked for")
    only = call(model, p, var=None, cov=None)                       # no component: C alone
    assert only["sigma_param"].shape == (0, p["wptr"][-1])
    bits(only["C"], res["C"], "C without components")


def test_one_component_among_eight(hip, model):
    p = problem(hip, 9, [(65, 130, 7), (130, 63, 3), (7, 17, 2)], 3, 5, 3)
    res = call(model, p)
    assert res["sigma_param"].shape[0] == 8 and np.all(res["sigma_param"] > 0)
    for c in range(5):
        alone = call(model, p, var=p["var"][c:c + 1], cov=None)
        bits(alone["sigma_param"][0], res["sigma_param"][c], "diagonal component %d alone" % c)
    for c in range(3):
        alone = call(model, p, var=None, cov=p["cov"][c:c + 1])
        bits(alone["sigma_param"][0], res["sigma_param"][5 + c], "full component %d alone" % c)
    worst = {}
    for s in range(3):
        check_slice(p, res, s, worst)
    report("eight components", worst)


# ---- 4. exact scaling ---------------------------------------------------------------------------------------------------
def test_exact_scaling_and_a_diagonal_full_component(hip, model):
    p, res = made(hip, model, 3)
    four = call(model, p, var=4 * p["var"], cov=4 * p["cov"])
    bits(four["sigma_param"], 2 * res["sigma_param"], "sigma_param under 4 Sigma")
    bits(four["C"], res["C"], "C under 4 Sigma")
    # a full component whose matrix is diagonal against the diagonal component: the chains differ, the bounds hold
    ns = len(p["wptr"]) - 1
    d = dict(p, var=p["var"][:1], cov=np.zeros((1, p["bbptr"][-1])))
    for s in range(ns):
        wb = int(np.diff(p["bwptr"])[s])
        d["cov"][0, p["bbptr"][s]:p["bbptr"][s + 1]] = np.diag(p["var"][0, p["bwptr"][s]:p["bwptr"][s + 1]]).ravel()
    got = call(model, d)
    worst = 0.0
    for s in range(ns):
        ref = param_reference(d, s)
        sig = sigma_of(d, got, s).astype(LD) ** 2
        bound = ref["B"].sum(axis=0) + 2 * gamma(2) * np.abs(ref["q"][0])
        assert np.all(np.abs(ref["q"][0] - ref["q"][1]) <= gamma(2) * np.abs(ref["q"][0]))   # (one q*, but for the reference's own error)
        err = np.abs(sig[0] - sig[1])
        assert np.all(err <= 2 * bound), (s, float(err.max()), float(bound.max()))
        if err.size:
            worst = max(worst, float(np.max(err / np.maximum(2 * bound, np.finfo(LD).tiny))))
    print("PARAM diagonal against full: worst error / allowed %.3f" % worst)


# ---- 5. the averaging kernel by the second route ------------------------------------------------------------------------------
def test_averaging_kernel_by_the_second_route(hip):
    case, geom, y, _ = inputs(hip, "ragged")
    nd = y.shape[1]
    _, weight = hip.error_components(y, np.full(nd, 2e-5), np.full(nd, 0.5))
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        first = model.normal_scene(case.atm, geom, y, weight)
        prior = G.seeded_prior(first)
        res = model.gain_scene(case.atm, geom, y, weight, prior_ivar=prior, want_gain=True, want_S=True, want_avk=True,
                               want_normal=True, want_k=True)
        pe = hip.param_error_scene(model, model.ret_windows(), case.atm, geom, y, weight, prior_ivar=prior)
    finally:
        model.close()
    assert np.all(res["status"] == 0) and np.all(np.isfinite(res["k"]))
    bits(pe["gain"], res["gain"], "the gain of param_error_scene")
    bits(pe["rowptr_b"], res["rowptr"], "rowptr_b under the model's own windows")
    wptr, aptr = res["wptr"], res["aptr"]
    assert np.array_equal(pe["bwptr"], wptr) and np.array_equal(pe["cptr"], aptr) and np.array_equal(pe["bbptr"], aptr)
    assert pe["sigma_param"].shape == (0, wptr[-1])
    weff = G.effective_weights(res, y, weight, np.zeros(y.shape))
    bits(pe["weight_eff"], weff, "the effective weights")
    p = dict(wptr=wptr, aptr=aptr, S=res["S"], sid=res["sid"], rowptr=res["rowptr"], k=res["k"], weff=weff,
             var=np.zeros((1,) + y.shape), nd=nd)
    worst, tiny = {}, np.finfo(LD).tiny
    for s in range(len(wptr) - 1):
        w = int(wptr[s + 1] - wptr[s])
        sl = slice(wptr[s], wptr[s + 1])
        As = res["A"][aptr[s]:aptr[s + 1]].reshape(w, w)
        dref = diag_reference(As, prior[sl])
        live = dref["live"]
        ix = np.ix_(live, live)
        gref = G.gain_reference(p, s)
        Gm, K, om = G.rows_of(p, res["gain"], s).astype(LD), gref["K"], gref["om"]
        M = Gm.shape[0]
        absA, absS = np.abs(As.astype(LD))[ix], np.abs(res["S"][aptr[s]:aptr[s + 1]].reshape(w, w).astype(LD))
        dA = gamma(M + 4) * (np.abs(K).T @ (np.abs(K) * om[:, None]))
        avk = res["avk"][aptr[s]:aptr[s + 1]].reshape(w, w).astype(LD)
        slack = (gref["E"].T @ np.abs(K) + absS @ dA)[ix] + dref["ES"] @ absA + dref["EK"] + gamma(M) * (np.abs(Gm).T @ np.abs(K))[ix]
        Cs = pe["C"][aptr[s]:aptr[s + 1]].reshape(w, w).astype(LD)
        el = pe["elements_b"][s]
        own = hip.scene_elements(case.ctl, case.atm, int(res["sfirst"][s]), int(res["slen"][s]))
        assert np.array_equal(el["iq"], own["iq"]) and np.array_equal(el["ip"], own["ip"]) and len(el["iq"]) == w
        err = np.abs(Cs[ix] - avk[ix])
        print("PARAM avk slice %d: worst error %.3g, allowed %.3g" % (s, float(err.max()), float(2 * slack.max())))
        assert np.all(err <= 2 * slack), ("avk", s, float(err.max()), float(slack.max()))
        worst["avk"] = max(worst.get("avk", 0.0), float(np.max(err / np.maximum(2 * slack, tiny))))
        assert np.abs(Cs[ix]).max() > 0
    report("the averaging kernel by the second route", worst)


# ---- 6. a real parameter ----------------------------------------------------------------------------------------------------
def copy_ctl(c):
    out = abi.ctl_t()
    C.memmove(C.byref(out), C.byref(c), C.sizeof(abi.ctl_t))
    return out


def no_windows(c):
    c.retp_zmin = c.retp_zmax = c.rett_zmin = c.rett_zmax = -999.0
    for g in range(c.ng):
        c.retq_zmin[g] = c.retq_zmax[g] = -999.0
    for w in range(c.nw):
        c.retk_zmin[w] = c.retk_zmax[w] = -999.0


def window_fields(c):
    return ([c.retp_zmin, c.retp_zmax, c.rett_zmin, c.rett_zmax] + [c.retq_zmin[g] for g in range(c.ng)]
            + [c.retq_zmax[g] for g in range(c.ng)] + [c.retk_zmin[w] for w in range(c.nw)] + [c.retk_zmax[w] for w in range(c.nw)])


@pytest.mark.parametrize("fov", [False, True], ids=["pencil", "fov"])
def test_a_real_parameter(hip, fov, name="ragged"):
    """One gas retrieved, T the parameter; with fov the scene of tests/test_scene_fov_gpu.py under its shape"""
    import test_scene_fov_gpu as F
    if fov:
        case, geom = F.scene(hip, name)[:2]
    else:
        case = scene_case(name)
        geom = six_per_time_stamp(case.geom)
    ctl_x, ctl_b = copy_ctl(case.ctl), copy_ctl(case.ctl)
    no_windows(ctl_x)
    no_windows(ctl_b)
    ctl_x.retq_zmin[2], ctl_x.retq_zmax[2] = 15.0, 35.0             # O3 retrieved
    ctl_b.rett_zmin, ctl_b.rett_zmax = 10.0, 40.0                   # T the parameter

    def new_model(c):
        m = hip.Model(c, case.lib_tables())
        if fov:
            m.set_fov(F.DZ, F.W)
        m.set_atm(case.atm)
        return m

    fresh = new_model(ctl_b)
    try:
        kb_fresh = fresh.kernel_scene(case.atm, geom)
    finally:
        fresh.close()
    model = new_model(ctl_x)
    try:
        before = model.kernel_scene(case.atm, geom)
        nr, nd = before["rad"].shape
        rng = np.random.default_rng(21)
        y = before["rad"] * (1 + 1e-3 * rng.standard_normal((nr, nd)))
        weight = 10.0 ** rng.uniform(0.0, 3.0, (nr, nd))
        first = model.normal_scene(case.atm, geom, y, weight)
        prior = G.seeded_prior(first)
        ns = len(first["sfirst"])
        assert ns >= 3
        rad_in = np.zeros((nr, nd))
        rad_in[np.flatnonzero(first["sid"] >= 0)[2], 0] = np.nan    # a masked channel: kb holds NaN there
        gs = model.gain_scene(case.atm, geom, y, weight, prior_ivar=prior, want_gain=True, rad_in=rad_in)
        assert np.all(gs["status"] == 0)
        lay = hip.param_layout(gs["wptr"], gs["rowptr"], kb_fresh["rowptr"], gs["sid"])
        rs = np.random.default_rng(22)
        nbw = int(lay["bwptr"][-1])
        var_b = np.stack([np.ones(nbw), 10.0 ** rs.uniform(-1.0, 1.0, nbw)])
        iq, z = [], []
        for s in range(ns):
            el = hip.scene_elements(ctl_b, case.atm, int(gs["sfirst"][s]), int(gs["slen"][s]))
            assert len(el["iq"]) == lay["bwptr"][s + 1] - lay["bwptr"][s] and np.all(el["iq"] == 1)
            iq.append(el["iq"]); z.append([case.atm.z[i] for i in el["ip"]])
        iq, z = np.concatenate(iq), np.concatenate(z)
        cz = np.zeros(2 + ctl_b.ng + ctl_b.nw)
        cz[1] = 5.0                                                 # sigma_i sigma_j exp(-|dz| / 5 km) for T
        pc = hip.prior_corr_slices(model, lay["bwptr"], iq, z, np.ones(nbw), cz, want_Sa=True)
        assert np.all(pc["status"] == 0)
        cov_b = pc["Sa"][None, :]
        set_before = window_fields(model.ret_windows())
        pe = hip.param_error_scene(model, ctl_b, case.atm, geom, y, weight, var_b=var_b, cov_b=cov_b, prior_ivar=prior, rad_in=rad_in)
        # the model's windows afterwards are the ones before, and kernel_scene under them returns the same bits
        assert window_fields(model.ret_windows()) == set_before == window_fields(ctl_x)
        after = model.kernel_scene(case.atm, geom)
        for f in ("k", "rad", "rowptr"):
            bits(after[f], before[f], "%s of kernel_scene after param_error_scene" % f)
        # ... and after a refusal
        with pytest.raises(hip.JurassicError):
            hip.param_error_scene(model, ctl_b, case.atm, geom, y, weight, var_b=-var_b, prior_ivar=prior, rad_in=rad_in)
        assert window_fields(model.ret_windows()) == set_before
        # a model whose windows were set answers as a fresh model created with them
        model.set_ret_windows(ctl_b)
        assert window_fields(model.ret_windows()) == window_fields(ctl_b)
        moved = model.kernel_scene(case.atm, geom)
        for f in ("k", "rad", "tau", "rowptr", "first", "len"):
            bits(moved[f], kb_fresh[f], "%s under set_ret_windows against a fresh model" % f)
        # a refusal leaves what was set
        bad = copy_ctl(ctl_x)
        bad.retq_zmax[1] = np.nan
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_model_set_ret_windows: the window of gas 1 is NaN" % hip.EINVAL):
            model.set_ret_windows(bad)
        assert window_fields(model.ret_windows()) == window_fields(ctl_b)
        kb_masked = model.kernel_scene(case.atm, geom, rad_in=rad_in)
    finally:
        model.close()
    for f in ("gain", "sigma", "rad", "cost", "status", "wptr", "rowptr", "sid"):
        bits(pe[f], gs[f], "%s of param_error_scene against gain_scene" % f)
    bits(pe["rowptr_b"], kb_fresh["rowptr"], "rowptr_b")
    for name in ("bwptr", "cptr", "bbptr"):
        assert np.array_equal(pe[name], lay[name]), name
    assert np.isnan(kb_masked["k"]).sum() > 0
    mask = np.where(hip.scene_fov_live(geom[:, 0], rad_in), 0.0, np.nan) if fov else rad_in
    weff = G.effective_weights(gs, y, weight, mask)
    bits(pe["weight_eff"], weff, "the effective weights")
    p = dict(lay, wptr=gs["wptr"], rowptr=gs["rowptr"], rowptr_b=kb_fresh["rowptr"], sid=gs["sid"], gain=gs["gain"],
             kb=kb_masked["k"], weff=weff, var=var_b, cov=cov_b, nd=nd)
    assert pe["sigma_param"].shape == (3, gs["wptr"][-1])
    worst = {}
    for s in range(ns):
        ref = check_slice(p, pe, s, worst)
        assert ref["m"] > 0 and np.abs(C_of(p, pe, s)).max() > 0
        el = pe["elements_b"][s]
        assert len(el["iq"]) == np.diff(lay["bwptr"])[s] and np.all(el["iq"] == 1)
    assert pe["sigma_param"].max() > 0
    report("a real parameter%s%s" % (", a field of view" if fov else "", "" if name == "ragged" else ", " + name), worst)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(hip, model):
    p = problem(hip, 4, [(7, 3, 2), (5, 4, 3), (3, 0, 1)], 2, 2, 1)
    lp_, ip_ = C.POINTER(C.c_long), C.POINTER(C.c_int)
    n, nc = int(p["wptr"][-1]), int(p["cptr"][-1])
    good = call(model, p)

    def raw(pin=None, pout=None, null=(), **kw):
        """the C entry with sentinels in the outputs -> (rc, message, C, sigma_param)"""
        a = dict(p)
        a.update(kw)
        Cs, sig = np.full(nc, SENT), np.full((3, n), SENT)
        pin = pin or hip.ParamIn(2, 1, hip._p(a["var"]), hip._p(a["cov"]))
        pout = pout or hip.ParamOut(hip._p(Cs), hip._p(sig))
        keep = [np.ascontiguousarray(a[k], dtype=np.int64) for k in ("wptr", "bwptr", "rowptr", "rowptr_b")]
        ptr = {k: (None if k in null else v.ctypes.data_as(lp_)) for k, v in zip(("wptr", "bwptr", "rowptr", "rowptr_b"), keep)}
        sd = np.ascontiguousarray(a["sid"], dtype=np.int32)
        dbl = {k: (None if k in null else hip._p(a[k])) for k in ("gain", "kb", "weff")}
        rc = hip.lib().jur_param_slices_host(model.h, kw.get("nslice", len(a["wptr"]) - 1), ptr["wptr"], ptr["bwptr"],
                                             kw.get("nr", len(sd)), a["nd"], ptr["rowptr"], ptr["rowptr_b"],
                                             None if "sid" in null else sd.ctypes.data_as(ip_), dbl["gain"], dbl["kb"], dbl["weff"],
                                             None if "in" in null else C.byref(pin), None if "out" in null else C.byref(pout))
        return rc, hip.lib().jur_last_error().decode(), Cs, sig

    def refused(words, **kw):
        rc, msg, Cs, sig = raw(**kw)
        assert rc == hip.EINVAL and msg == "jur_param_slices_host: " + words, (rc, msg)
        assert np.all(Cs == SENT) and np.all(sig == SENT), "outputs of a refused call were written"

    rc, _, Cs, sig = raw()
    assert rc == 0
    bits(Cs, good["C"], "C through the C entry")
    bits(sig, good["sigma_param"], "sigma_param through the C entry")
    # nslice == 0 or nr == 0 writes nothing
    for kw in (dict(nslice=0), dict(nr=0)):
        rc, _, Cs, sig = raw(**kw)
        assert rc == 0 and np.all(Cs == SENT) and np.all(sig == SENT)
    # required pointers
    refused("null argument (in)", null=("in",))
    refused("null argument (out)", null=("out",))
    for name in ("wptr", "bwptr", "rowptr", "rowptr_b", "sid"):
        refused("null argument (%s)" % name, null=(name,))
    for name, arg in (("gain", "gain"), ("kb", "kb"), ("weff", "weight_eff")):
        refused("null argument (%s)" % arg, null=(name,))
    keep = [np.full(nc, SENT), np.full((3, n), SENT)]
    refused("null argument (sigma_param) with nvar + ncov = 3", pout=hip.ParamOut(hip._p(keep[0]), None))
    refused("null argument (var)", pin=hip.ParamIn(2, 1, None, hip._p(p["cov"])))
    refused("null argument (cov)", pin=hip.ParamIn(2, 1, hip._p(p["var"]), None))
    # the number of components
    refused("nvar = 5, ncov = 4: 0 to 8 components per call", pin=hip.ParamIn(5, 4, hip._p(p["var"]), hip._p(p["cov"])))
    refused("nvar = -1, ncov = 1: 0 to 8 components per call", pin=hip.ParamIn(-1, 1, hip._p(p["var"]), hip._p(p["cov"])))
    # the layout
    refused("wptr is not an ascending running sum of widths from 0 (slice 1)", wptr=np.array([0, 7, 6, 15]))
    refused("bwptr is not an ascending running sum of widths from 0 (slice 1)", bwptr=np.array([0, 3, 2, 7]))
    refused("bwptr gives slice 1 5 columns, its rays have 4 in rowptr_b", bwptr=np.array([0, 3, 8, 8]))
    sid = p["sid"].copy()
    sid[1], sid[3] = 1, 0                                           # rays 1 and 3 swap their slices
    refused("the block of ray 1 has 7 columns, its slice 1 has 5 elements", sid=sid)
    rb = p["rowptr_b"].copy()
    rb[5:] += 1                                                     # ray 4, the second of slice 1, one column wider
    refused("rays 3 and 4 of slice 1 have 4 and 5 columns in rowptr_b", rowptr_b=rb)
    # the values
    for bad, word in ((-1.0, "-1"), (np.nan, "nan"), (np.inf, "inf")):
        v = p["var"].copy()
        v[1, p["bwptr"][1] + 2] = bad
        refused("the variance of component 1, slice 1, element 2 is %s: negative or not finite" % word, var=v)
    for bad, word in ((np.nan, "nan"), (-np.inf, "-inf")):
        c = p["cov"].copy()
        c[0, p["bbptr"][1] + 2 * 4 + 1] = bad
        refused("cov of component 2, slice 1, element (2, 1) is %s: not finite" % word, cov=c)
    c = p["cov"].copy()
    c[0, p["bbptr"][1] + 3 * 4 + 3] = -0.5
    refused("the diagonal of cov of component 2, slice 1, element 3 is -0.5: negative", cov=c)
    c = p["cov"].copy()
    c[0, p["bbptr"][1] + 1 * 4 + 2] = np.nan                        # above the diagonal: never read
    rc, _, Cs, sig = raw(cov=c)
    assert rc == 0
    bits(sig, good["sigma_param"], "sigma_param with a NaN above the diagonal of cov")
    # the wrapper raises what the library says
    with pytest.raises(hip.JurassicError, match=r"error %d: jur_param_slices_host: the variance of component 0, slice 0, element 0 is -2"
                       % hip.EINVAL):
        v = p["var"].copy()
        v[0, 0] = -2.0
        call(model, p, var=v)
    with pytest.raises(hip.JurassicError, match=r"error %d: jur_param_layout: rays 3 and 4 of slice 1 have 4 and 5 columns" % hip.EINVAL):
        model.param_slices(p["wptr"], p["rowptr"], rb, p["sid"], p["gain"], np.concatenate([p["kb"], np.zeros(2)]), p["weff"])
    again = call(model, p)
    bits(again["C"], good["C"], "C in the call after the refusals")
    bits(again["sigma_param"], good["sigma_param"], "sigma_param in the call after the refusals")
