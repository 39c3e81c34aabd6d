"""Model.gain_slices (jur_gain_slices_host) and Model.gain_scene (jur_gain_scene_host): the gain matrix G = S K^T W of every
slice over the ragged blocks and the retrieval error per source, sigma_comp = sqrt(diag(G V_c G^T)), on the device.

The error bounds are derived, not measured (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.).  With
u = 2^-53 and gamma_m = m u / (1 - m u); the references are formed in np.longdouble from the S that was passed in (their
own error, of the order w 2^-64, is 2^-11 of what follows):
  gain.  c^ is a chain of w fused multiply-adds (dead j and the padding add exact zeros), then one multiplication by omega:
      |G^ - G*| <= E = omega gamma_{w+1} (|S| |K|)                                      (Higham 3.1, 3.4)
  radicand.  With m live measurements, q^ is a chain of m fused multiply-adds whose terms carry one more rounding (g * g
      is rounded first), on the g^ the gain kernel wrote: gamma_{m+2} sum g^2 v, and g^2 is within 2 |g*| E + E^2 of g*^2:
      |q^ - q*| <= B = gamma_{m+2} sum (|g*| + E)^2 v + sum (2 |g*| E + E^2) v
  a correctly rounded square root: sigma_comp^2 is held to q* within B + gamma_2 q*.
Twice each bound is allowed, as in tests/test_scene_diagnose_gpu.py.  The kernels form every inner product as a chain of
fused multiply-adds in the documented order and use no MFMA.  Everything else is bit identity.

Test 1 takes the widths of tests/test_scene_diagnose_gpu.py and 300 (wider than a workgroup of the budget kernel) with 1, 7,
63, 64, 65 and 130 measurement rows a slice: exactly with nd = 1; with nd = 3 a slice has whole rays, so 3, 9, 63, 66, 66
and 132 rows.  Every width meets two of the row counts, and 63, 64 and 65 meet themselves.

The identities of test 5, with A^ the returned normal matrix (A^ = K^T W K + dA, |dA| <= gamma_{M+4} |K|^T W |K| over the M
measurements of the slice: tests/test_scene_normal_gpu.py), S^ = S* + dS and AVK^ = S* A^ + dK the returned diagnostics
(|dS| <= E_S, |dK| <= E_K: tests/test_scene_diagnose_gpu.py, whose reference takes A^ as its input) and G^ = W K S^ + dG:
  sum_m G^_mi K_mj - AVK^_ij = (dS A^ - S^ dA + dG^T K - dK)_ij
      <= (E_S |A^| + |S^| gamma_{M+4} |K|^T W |K| + E^T |K| + E_K)_ij
  sum_c q*_c = sum_m G*_mi^2 (v_noise + v_formod), and 1 / omega is that sum of variances within two roundings (the sum, the
      reciprocal), so sum_c q*_c = diag(S^ K^T W K S^) (1 + theta_2); against N* = diag(S* A^ S*):
      <= gamma_2 sum_c q*_c + diag(2 E_S |A^| |S*| + E_S |A^| E_S + |S^| gamma_{M+4} |K|^T W |K| |S^|)
      and sigma_comp_c^2, sigma_noise^2 are held to q*_c, N* within their radicands' bounds (B above; BN there)."""
import ctypes as C
import numpy as np
import pytest
import common
import sequences
from jurassic_hip import synth
from test_scene_jacobian_gpu import bits, formod_on, fresh_formod
from test_scene_normal_gpu import blocks_and_sums, inputs, interleaved
from test_scene_solve_gpu import gamma, is_plus_zero, pack, spd
from test_scene_diagnose_gpu import WIDTHS, OUTS, reference as diag_reference

pytestmark = pytest.mark.gpu
LD = np.longdouble
ROWS = (1, 7, 63, 64, 65, 130)
ALL_WIDTHS = WIDTHS + (300,)
FORWARD = ("rad", "tau", "tp", "np", "cost", "nlive", "rowptr", "sid", "wptr", "aptr")


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
    pairs = []
    for i, w in enumerate(ALL_WIDTHS):
        pairs += [(w, ROWS[i % 6]), (w, ROWS[(i + 3) % 6])]
    pairs += [(63, 63), (64, 64), (65, 65), (300, 130)]
    return [(w, -(-rows // nd)) for w, rows in pairs]


def problem(model, seed, shapes, nd, ncomp, mats=None):
    """A ragged problem: slice s has width shapes[s][0] and shapes[s][1] rays of nd channels; one ray without a slice leads.
    S comes from diagnose_slices on spd matrices; a tenth of the measurements is not live (weight 0)."""
    rng = np.random.default_rng(seed)
    mats = mats or [spd(rng, w) for w, _ in shapes]
    wptr, aptr, A, _ = pack(mats, [np.zeros(w) for w, _ in shapes])
    d = model.diagnose_slices(wptr, A, want_S=True)
    sid = np.concatenate([[-1]] + [np.full(n, s) for s, (_, n) in enumerate(shapes)]).astype(np.int32)
    widths = np.array([0 if s < 0 else shapes[s][0] for s in sid])
    rowptr = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    nr = len(sid)
    k = rng.standard_normal(int(rowptr[-1]) * nd)
    weff = 10.0 ** rng.uniform(-1.0, 1.0, (nr, nd))
    weff[rng.uniform(size=(nr, nd)) < 0.1] = 0.0
    var = 10.0 ** rng.uniform(-2.0, 0.0, (ncomp, nr, nd))
    return dict(wptr=wptr, aptr=aptr, S=d["S"], status=d["status"], sid=sid, rowptr=rowptr, k=k, weff=weff, var=var, nd=nd,
                mats=mats)


def call(model, p, **kw):
    args = dict(var=p["var"], status=p["status"])
    args.update(kw)
    return model.gain_slices(p["wptr"], p["S"], p["rowptr"], p["sid"], p["k"], p["weff"], **args)


def rows_of(p, flat, s):
    """the rows of slice s of an array laid out as the blocks, (measurements, w), in measurement order"""
    nd, w = p["nd"], int(p["wptr"][s + 1] - p["wptr"][s])
    rays = np.flatnonzero(p["sid"] == s)
    if len(rays) == 0:
        return np.zeros((0, w))
    return np.concatenate([flat[p["rowptr"][r] * nd:p["rowptr"][r + 1] * nd].reshape(nd, w) for r in rays])


def per_measurement(p, a, s):
    """(..., measurements) of an array (..., nr, nd)"""
    rays = np.flatnonzero(p["sid"] == s)
    return a[..., rays, :].reshape(a.shape[:-2] + (-1,))


def sigma_of(p, res, s):
    return res["sigma_comp"][:, p["wptr"][s]:p["wptr"][s + 1]]


def gain_reference(p, s):
    """G*, E, q*, B of the module docstring for slice s, in np.longdouble"""
    w = int(p["wptr"][s + 1] - p["wptr"][s])
    S = p["S"][p["aptr"][s]:p["aptr"][s + 1]].reshape(w, w)
    K, om, V = rows_of(p, p["k"], s), per_measurement(p, p["weff"], s), per_measurement(p, p["var"], s)
    with np.errstate(invalid="ignore"):
        alive, lm = np.diag(S) > 0, om > 0
    Sl = np.where(alive[:, None] & alive[None, :], S, 0.0).astype(LD)
    Kl = np.where(lm[:, None] & alive[None, :], K, 0.0).astype(LD)
    oml = np.where(lm, om, 0.0).astype(LD)
    G = oml[:, None] * (Kl @ Sl.T)
    E = oml[:, None] * gamma(w + 1) * (np.abs(Kl) @ np.abs(Sl).T)
    Vl = np.where(lm, V, 0.0).astype(LD)
    m = int(lm.sum())
    q = Vl @ (G * G)
    B = gamma(m + 2) * (Vl @ ((np.abs(G) + E) ** 2)) + Vl @ (2 * np.abs(G) * E + E * E)
    return dict(G=G, E=E, q=q, B=B, alive=alive, lm=lm, m=m, K=Kl, om=oml)


def check_slice(p, res, s, worst):
    ref = gain_reference(p, s)
    tiny = np.finfo(LD).tiny
    G = rows_of(p, res["gain"], s)
    assert np.all(np.isfinite(G))
    err = np.abs(G.astype(LD) - ref["G"])
    assert np.all(err <= 2 * ref["E"]), ("gain", s, float(err.max()), float(ref["E"].max()))
    assert is_plus_zero(G[~ref["lm"]]) and is_plus_zero(G[:, ~ref["alive"]])
    if G.size:
        worst["gain"] = max(worst.get("gain", 0.0), float(np.max(err / np.maximum(2 * ref["E"], tiny))))
    sig = sigma_of(p, res, s)
    if sig.shape[0]:
        bound = ref["B"] + gamma(2) * np.abs(ref["q"])
        err = np.abs(sig.astype(LD) ** 2 - ref["q"])
        assert np.all(err <= 2 * bound), ("sigma_comp", s, float(err.max()), float(bound.max()))
        assert is_plus_zero(sig[:, ~ref["alive"]])
        worst["sigma_comp"] = max(worst.get("sigma_comp", 0.0), float(np.max(err / np.maximum(2 * bound, tiny))))
    return ref


def report(what, worst):
    print("GAIN %s: worst error / allowed %s" % (what, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


# ---- 1. synthetic systems against np.longdouble ----------------------------------------------------------------------
_made = {}


def made(model, nd):
    if nd not in _made:
        p = problem(model, 40 + nd, shapes_of_test_1(nd), nd, 2 if nd == 1 else 3)
        _made[nd] = (p, call(model, p))
    return _made[nd]


@pytest.mark.parametrize("nd", [1, 3])
def test_synthetic_systems(model, nd):
    p, res = made(model, nd)
    ns = len(p["wptr"]) - 1
    assert res["gain"].shape == p["k"].shape and res["sigma_comp"].shape == (p["var"].shape[0], p["wptr"][-1])
    assert np.all(p["status"] == 0)
    worst, rows = {}, set()
    for s in range(ns):
        ref = check_slice(p, res, s, worst)
        rows.add(len(ref["lm"]))
    assert rows >= ({1, 7, 63, 64, 65, 130} if nd == 1 else {3, 9, 63, 66, 132})
    assert np.abs(res["gain"]).max() > 0 and res["sigma_comp"].max() > 0
    report("synthetic, nd %d, %d slices" % (nd, ns), worst)


# ---- 2. the exact rules -----------------------------------------------------------------------------------------------
def test_exact_rules(model):
    rng = np.random.default_rng(5)
    holes = spd(rng, 40)
    for i in (0, 16, 39):
        holes[i, :] = 0.0
        holes[:, i] = 0.0
    indefinite = np.array([[1.0, 2.0], [2.0, 1.0]])
    mats = [spd(rng, 33), holes, indefinite, spd(rng, 70)]
    shapes = [(33, 5), (40, 30), (2, 4), (70, 23)]
    nd = 3
    p = problem(model, 6, shapes, nd, 2, mats=mats)
    assert list(p["status"]) == [0, 0, 2, 0]
    # NaN in the block columns of the dead elements of slice 1, NaN block rows and NaN variances on what is not live
    for r in np.flatnonzero(p["sid"] == 1):
        blk = p["k"][p["rowptr"][r] * nd:p["rowptr"][r + 1] * nd].reshape(nd, 40)
        blk[:, [0, 16, 39]] = np.nan
    rays3 = np.flatnonzero(p["sid"] == 3)
    p["weff"][rays3[::2], 1] = 0.0
    p["weff"][rays3[4], 2] = -1.0                                   # anything not > 0 is "not live"
    p["weff"][rays3[5], 2] = np.nan
    for r in range(len(p["sid"])):
        w = int(p["rowptr"][r + 1] - p["rowptr"][r])
        for i in range(nd):
            if not p["weff"][r, i] > 0:
                p["k"][p["rowptr"][r] * nd + i * w:p["rowptr"][r] * nd + (i + 1) * w] = np.nan
                p["var"][:, r, i] = np.nan
    res = call(model, p)
    assert np.all(np.isfinite(res["gain"])) and np.all(np.isfinite(res["sigma_comp"]))
    worst = {}
    for s in (0, 1, 3):
        ref = check_slice(p, res, s, worst)
        assert (~ref["lm"]).sum() > 0
    assert is_plus_zero(rows_of(p, res["gain"], 1)[:, [0, 16, 39]]) and is_plus_zero(sigma_of(p, res, 1)[:, [0, 16, 39]])
    assert is_plus_zero(rows_of(p, res["gain"], 2)) and is_plus_zero(sigma_of(p, res, 2)), "a system that broke down is not +0.0"
    # the neighbours of the breakdown are untouched: the same bits without it
    keep = [0, 1, 3]
    q = sub(p, keep)
    alone = call(model, q)
    for j, s in enumerate(keep):
        bits(rows_of(q, alone["gain"], j), rows_of(p, res["gain"], s), "gain of slice %d beside a breakdown" % s)
        bits(sigma_of(q, alone, j), sigma_of(p, res, s), "sigma_comp of slice %d beside a breakdown" % s)
    # the status the caller passes rules: slice 0 marked as broken down is +0.0 throughout
    marked = p["status"].copy()
    marked[0] = 7
    res2 = call(model, p, status=marked)
    assert is_plus_zero(rows_of(p, res2["gain"], 0)) and is_plus_zero(sigma_of(p, res2, 0))
    bits(rows_of(p, res2["gain"], 3), rows_of(p, res["gain"], 3), "gain of slice 3 beside a marked system")
    # ncomp == 0, want_gain off and on
    only = call(model, p, var=None)
    assert only["sigma_comp"].shape == (0, p["wptr"][-1])
    bits(only["gain"], res["gain"], "gain with ncomp == 0")
    bare = call(model, p, want_gain=False)
    assert "gain" not in bare
    bits(bare["sigma_comp"], res["sigma_comp"], "sigma_comp with want_gain off")
    report("exact rules", worst)


# ---- 3. independence ---------------------------------------------------------------------------------------------------
def sub(p, order, perm=None):
    """the slices `order` of a problem, in that order, with their rays (and those without a slice) in the order perm
    gives them (default: as they lie)"""
    nd = p["nd"]
    new = {int(s): j for j, s in enumerate(order)}
    rays = [int(r) for r in (range(len(p["sid"])) if perm is None else perm) if p["sid"][r] < 0 or int(p["sid"][r]) in new]
    sid = np.array([-1 if p["sid"][r] < 0 else new[int(p["sid"][r])] for r in rays], dtype=np.int32)
    widths = np.array([p["rowptr"][r + 1] - p["rowptr"][r] for r in rays])
    wptr = np.concatenate([[0], np.cumsum([p["wptr"][s + 1] - p["wptr"][s] for s in order])]).astype(np.int64)
    aptr = np.concatenate([[0], np.cumsum([p["aptr"][s + 1] - p["aptr"][s] for s in order])]).astype(np.int64)
    return dict(wptr=wptr, aptr=aptr, S=np.concatenate([p["S"][p["aptr"][s]:p["aptr"][s + 1]] for s in order]),
                status=p["status"][[int(s) for s in order]], sid=sid,
                rowptr=np.concatenate([[0], np.cumsum(widths)]).astype(np.int64),
                k=np.concatenate([p["k"][p["rowptr"][r] * nd:p["rowptr"][r + 1] * nd] for r in rays] + [np.zeros(0)]),
                weff=p["weff"][rays], var=p["var"][:, rays], nd=nd)


@pytest.mark.parametrize("nd", [1, 3])
def test_independence(model, nd):
    p, res = made(model, nd)
    ns = len(p["wptr"]) - 1

    def same(q, got, order, what):
        for j, s in enumerate(order):
            bits(rows_of(q, got["gain"], j), rows_of(p, res["gain"], s), "gain of slice %d %s" % (s, what))
            bits(sigma_of(q, got, j), sigma_of(p, res, s), "sigma_comp of slice %d %s" % (s, what))

    for s in (0, 5, 11, 14, ns - 1):                                # a system alone
        q = sub(p, [s])
        same(q, call(model, q), [s], "alone")
    order = [int(s) for s in np.random.default_rng(3).permutation(ns)]   # the slices shuffled, the rays where they were
    q = sub(p, order)
    same(q, call(model, q), order, "shuffled")
    perm = interleaved(p["sid"])                                    # the rays of the slices dealt out in turn
    assert np.any(np.diff(p["sid"][perm][:6]) != 0)
    q = sub(p, list(range(ns)), perm)
    same(q, call(model, q), list(range(ns)), "interleaved")


# ---- 4. the scene entry against its pieces -----------------------------------------------------------------------------------
def effective_weights(out, y, weight, mask):
    """omega formed in numpy by jur_normal_scene_host's rule (mask: the input radiances or the effective mask)"""
    live = np.isfinite(mask) & np.isfinite(out["rad"]) & np.isfinite(y) & (weight > 0) & (out["sid"] >= 0)[:, None]
    return np.where(live, weight, 0.0)


def against_the_pieces(model, atm, geom, y, weight, var, prior, rad_in=None, mask=None, caps=(), what=""):
    """gain_scene against diagnose_scene and gain_slices on the same model -> (the diagnostics, the gain result, omega)"""
    kw = dict(prior_ivar=prior, rad_in=rad_in)
    diag = model.diagnose_scene(atm, geom, y, weight, want_S=True, want_avk=True, want_normal=True, want_k=True, **kw)
    full = model.gain_scene(atm, geom, y, weight, var=var, want_gain=True, want_S=True, want_avk=True, want_normal=True, want_k=True, **kw)
    for f in FORWARD + OUTS + ("A", "b", "k"):
        bits(full[f], diag[f], "%s against diagnose_scene%s" % (f, what))
    if mask is None:
        mask = np.zeros(y.shape) if rad_in is None else rad_in
    weff = effective_weights(diag, y, weight, mask)
    half = model.gain_slices(diag["wptr"], diag["S"], diag["rowptr"], diag["sid"], diag["k"], weff, var=var, status=diag["status"])
    bits(full["gain"], half["gain"], "gain against gain_slices" + what)
    bits(full["sigma_comp"], half["sigma_comp"], "sigma_comp against gain_slices" + what)
    for cap in caps:
        bare = model.gain_scene(atm, geom, y, weight, var=var, max_rays_per_pass=cap, **kw)
        assert not any(f in bare for f in ("A", "b", "k", "S", "avk", "gain"))
        bits(bare["sigma_comp"], full["sigma_comp"], "sigma_comp, cap %d%s" % (cap, what))
        for f in ("sigma", "sigma_noise", "dofs", "status", "rad", "cost", "nlive"):
            bits(bare[f], full[f], "%s, cap %d%s" % (f, cap, what))
        only = model.gain_scene(atm, geom, y, weight, want_gain=True, max_rays_per_pass=cap, **kw)
        assert only["sigma_comp"].shape[0] == 0
        bits(only["gain"], full["gain"], "gain with ncomp == 0, cap %d%s" % (cap, what))
    return diag, full, weff


def seeded_prior(out):
    rng = np.random.default_rng(3)
    wptr, aptr = out["wptr"], out["aptr"]
    return np.concatenate([10.0 ** rng.uniform(-3.0, -1.0, int(wptr[s + 1] - wptr[s]))
                           * np.diag(out["A"][aptr[s]:aptr[s + 1]].reshape(int(wptr[s + 1] - wptr[s]), -1)).mean()
                           for s in range(len(wptr) - 1)])


def components(hip, y):
    return hip.error_components(y, np.full(y.shape[1], 1e-5), np.full(y.shape[1], 1.0))[0]


def test_scene_entry_against_its_pieces(hip, name="ragged"):
    case, geom, y, weight = inputs(hip, name)
    _, clear = blocks_and_sums(hip, name)
    nr, nd = y.shape
    last = nd - 1
    live, dead = np.flatnonzero(clear["sid"] >= 0), np.flatnonzero(clear["sid"] < 0)
    assert len(dead) > 0                                            # rays without a slice
    rad_in = np.zeros((nr, nd))
    rad_in[live[1], 0] = rad_in[dead[0], 0] = np.nan                # a masked channel
    w2 = weight.copy()
    w2[live[5], last] = 0.0                                         # a zero weight, in the last channel
    var = components(hip, y)
    var[:, live[1], 0] = np.nan                                     # not live: never read
    want = fresh_formod(hip, case, case.atm, case.geom)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        prior = seeded_prior(clear)
        ns = len(clear["sfirst"])
        assert nr + clear["rowptr"][-1] > 3 * 150                   # a cap of 150 slots: three passes or more
        diag, full, weff = against_the_pieces(model, case.atm, geom, y, w2, var, prior, rad_in=rad_in, caps=(150, 1))
        sequences.same_bits(formod_on(model, case.geom), want, "after gain_scene")
        assert np.all(diag["status"] == 0) and np.all(np.isfinite(full["gain"]))
        assert np.all(full["sigma_comp"] >= 0) and full["sigma_comp"].max() > 0
        rp = diag["rowptr"]
        for r, i in ((live[1], 0), (live[5], last)):
            w = int(rp[r + 1] - rp[r])
            assert w > 0 and is_plus_zero(full["gain"][rp[r] * nd + i * w:rp[r] * nd + (i + 1) * w])
        assert np.all(np.isnan(diag["k"][rp[live[1]] * nd:rp[live[1]] * nd + int(rp[live[1] + 1] - rp[live[1]])]))
        # the bounds of the module docstring on the scene's own blocks
        p = dict(wptr=diag["wptr"], aptr=diag["aptr"], S=diag["S"], sid=diag["sid"], rowptr=rp, k=diag["k"], weff=weff,
                 var=var, nd=nd)
        worst = {}
        for s in range(ns):
            check_slice(p, full, s, worst)
        report("scene %s" % name, worst)
    finally:
        model.close()


def test_beside_a_field_of_view(hip):
    import test_scene_fov_gpu as F
    case, geom, y, weight, lay, iq, ip, x0 = F.scene(hip)
    r, _ = F.seeded_prior(hip)
    rad_in = np.zeros(y.shape)
    rad_in[np.flatnonzero(lay["sid"] >= 0)[2], 0] = np.nan          # masks the channel on every ray of the window
    mask = np.where(hip.scene_fov_live(geom[:, 0], rad_in), 0.0, np.nan)
    assert np.isnan(mask[:, 0]).sum() > 1
    model = F.with_shape(hip, case)
    try:
        diag, full, _ = against_the_pieces(model, case.atm, geom, y, weight, components(hip, y), r, rad_in=rad_in, mask=mask,
                                           caps=(1,), what=", a field of view")
        assert np.abs(full["gain"]).max() > 0
    finally:
        model.close()


def test_beside_the_hydrostatic_balance(hip):
    import test_scene_hydro_gpu as H
    case, geom, y, weight, lay, iq, ip = H.scene(hip, "ragged")
    r, _ = H.diagonal_prior(hip, "ragged")
    on = H.switched_on(hip, case)
    try:
        diag, full, _ = against_the_pieces(on, case.atm, geom, y, weight, components(hip, y), r, caps=(1,), what=", balanced")
        assert np.abs(full["gain"]).max() > 0
    finally:
        on.close()


def test_beside_a_full_prior_precision(hip):
    import test_prior_full_gpu as P
    import test_scene_recomp_gpu as RC
    sc = RC.scene_T(hip, "ragged")
    case, geom, y, weight, lay = sc[:5]
    pc, r, xa = P.scene_prior(hip, "ragged")
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        model.set_prior_precision(lay["wptr"], pc["R"])
        diag, full, _ = against_the_pieces(model, case.atm, geom, y, weight, components(hip, y), r, caps=(1,), what=", a full prior")
        assert np.abs(full["gain"]).max() > 0
    finally:
        model.close()


# ---- 5. identities --------------------------------------------------------------------------------------------------------
def test_identities(hip):
    """sum_m G_im K_m[j] against the returned avk, and with weight and var from error_components sum_c sigma_comp_c^2
    against sigma_noise^2, within the bounds derived in the module docstring"""
    case, geom, y, _ = inputs(hip, "ragged")
    nd = y.shape[1]
    var, weight = hip.error_components(y, np.full(nd, 2e-5), np.full(nd, 0.5))
    assert np.all(weight > 0) and np.all(np.isfinite(weight))
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        first = model.normal_scene(case.atm, geom, y, weight)
        prior = seeded_prior(first)
        res = model.gain_scene(case.atm, geom, y, weight, var=var, prior_ivar=prior, want_gain=True, want_S=True, want_avk=True,
                               want_normal=True, want_k=True)
    finally:
        model.close()
    assert np.all(res["status"] == 0) and np.all(np.isfinite(res["k"]))
    wptr, aptr = res["wptr"], res["aptr"]
    weff = effective_weights(res, y, weight, np.zeros(y.shape))
    p = dict(wptr=wptr, aptr=aptr, S=res["S"], sid=res["sid"], rowptr=res["rowptr"], k=res["k"], weff=weff, var=var, nd=nd)
    worst = {}
    tiny = np.finfo(LD).tiny
    for s in range(len(wptr) - 1):
        w = int(wptr[s + 1] - wptr[s])
        sl = slice(wptr[s], wptr[s + 1])
        As = res["A"][aptr[s]:aptr[s + 1]].reshape(w, w)
        dref = diag_reference(As, prior[sl])
        live = dref["live"]
        ix = np.ix_(live, live)
        gref = gain_reference(p, s)
        assert np.array_equal(live, gref["alive"])
        G, K, om = rows_of(p, res["gain"], s).astype(LD), gref["K"], gref["om"]
        M = G.shape[0]
        absA, absS = np.abs(As.astype(LD))[ix], np.abs(res["S"][aptr[s]:aptr[s + 1]].reshape(w, w).astype(LD))
        dA = gamma(M + 4) * (np.abs(K).T @ (np.abs(K) * om[:, None]))
        # the averaging kernel
        avk = res["avk"][aptr[s]:aptr[s + 1]].reshape(w, w).astype(LD)
        slack = (gref["E"].T @ np.abs(K) + absS @ dA)[ix] + dref["ES"] @ absA + dref["EK"]
        err = np.abs((G.T @ K)[ix] - avk[ix])
        assert np.all(err <= 2 * slack), ("avk", s, float(err.max()), float(slack.max()))
        worst["avk"] = max(worst.get("avk", 0.0), float(np.max(err / np.maximum(2 * slack, tiny))))
        # the budget
        total = (sigma_of(p, res, s).astype(LD) ** 2).sum(axis=0)[live]
        noise = res["sigma_noise"][sl].astype(LD)[live] ** 2
        qsum = gref["q"].sum(axis=0)[live]
        to_q = gref["B"].sum(axis=0)[live] + gamma(2) * qsum
        between = gamma(2) * qsum + np.diag(2 * dref["ES"] @ absA @ np.abs(dref["S"]) + dref["ES"] @ absA @ dref["ES"]) \
            + np.diag(absS @ dA @ absS)[live]
        to_N = dref["BN"] + gamma(2) * np.abs(dref["N"])
        bound = to_q + between + to_N
        err = np.abs(total - noise)
        assert np.all(err <= 2 * bound), ("budget", s, float(err.max()), float(bound.max()))
        worst["budget"] = max(worst.get("budget", 0.0), float(np.max(err / np.maximum(2 * bound, tiny))))
        assert np.all(total > 0)
    report("identities", worst)


# ---- 6. state and refusals ---------------------------------------------------------------------------------------------
def test_refusals_and_state(hip):
    case, geom, y, weight = inputs(hip, "ragged")
    _, out = blocks_and_sums(hip, "ragged")
    want = fresh_formod(hip, case, case.atm, case.geom)
    nr, nd = y.shape
    n, ns, na = int(out["wptr"][-1]), len(out["sfirst"]), int(out["aptr"][-1])
    var = np.ones((2, nr, nd))
    live = np.flatnonzero(out["sid"] >= 0)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        good = model.gain_scene(case.atm, geom, y, weight, var=var, prior_ivar=np.ones(n), want_gain=True)
        sequences.same_bits(formod_on(model, case.geom), want, "after gain_scene")
        for bad, word in ((-1.0, "-1"), (np.nan, "nan"), (np.inf, "inf")):
            v = var.copy()
            v[1, live[3], 1] = bad
            with pytest.raises(hip.JurassicError, match=r"error %d: jur_gain_scene_host: the variance of component 1, ray %d, channel 1 is %s"
                               % (hip.EINVAL, live[3], word)):
                model.gain_scene(case.atm, geom, y, weight, var=v, prior_ivar=np.ones(n))
            sequences.same_bits(formod_on(model, case.geom), want, "after the refusal of a variance of %s" % word)
        v = var.copy()
        v[0, np.flatnonzero(out["sid"] < 0)[0], 0] = -1.0           # a ray without a slice is not live: accepted
        w0 = weight.copy()
        w0[live[3], 1] = 0.0
        v[1, live[3], 1] = -1.0                                     # a zero weight: not live, accepted
        model.gain_scene(case.atm, geom, y, w0, var=v, prior_ivar=np.ones(n))
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_gain_scene_host: ncomp = 9: 0 to 8" % hip.EINVAL):
            model.gain_scene(case.atm, geom, y, weight, var=np.ones((9, nr, nd)))
        # what the diagnostics and the normal equations refuse, in this entry's name
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_gain_scene_host: rowptr is not" % hip.EINVAL):
            model.gain_scene(case.atm, geom, y, weight, var=var, rowptr=out["rowptr"] + 1)
        bad_r = np.ones(n)
        bad_r[int(out["wptr"][1]) + 2] = -1.0
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_gain_scene_host: .*prior_ivar of slice 1, element 2 is -1" % hip.EINVAL):
            model.gain_scene(case.atm, geom, y, weight, var=var, prior_ivar=bad_r)
        sequences.same_bits(formod_on(model, case.geom), want, "after the inherited refusals")
        # only the C interface can pass these
        lp_, ip_ = C.POINTER(C.c_long), C.POINTER(C.c_int)
        S = np.zeros(na)
        weff = np.where((out["sid"] >= 0)[:, None], weight, 0.0)

        def slices_rc(gin, gout):
            return hip.lib().jur_gain_slices_host(model.h, ns, out["wptr"].ctypes.data_as(lp_), hip._p(S), None, nr, nd,
                                                  out["rowptr"].ctypes.data_as(lp_), out["sid"].ctypes.data_as(ip_), hip._p(out["k"]),
                                                  hip._p(weff), C.byref(gin), C.byref(gout))

        sig = np.zeros((2, n))
        for gin, gout, message in ((hip.GainIn(-1, hip._p(var)), hip.GainOut(None, hip._p(sig)), "ncomp = -1: 0 to 8"),
                                   (hip.GainIn(9, hip._p(var)), hip.GainOut(None, hip._p(sig)), "ncomp = 9: 0 to 8"),
                                   (hip.GainIn(2, hip._p(var)), hip.GainOut(None, None), "null argument (sigma_comp)"),
                                   (hip.GainIn(2, None), hip.GainOut(None, hip._p(sig)), "null argument (var)")):
            rc = slices_rc(gin, gout)
            assert rc == hip.EINVAL and ("jur_gain_slices_host: " + message) in hip.lib().jur_last_error().decode(), message
        v = var.copy()
        v[0, live[0], 1] = -2.0
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_gain_slices_host: the variance of component 0, ray %d, channel 1 is -2"
                           % (hip.EINVAL, live[0])):
            model.gain_slices(out["wptr"], S, out["rowptr"], out["sid"], out["k"], weff, var=v)
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_gain_slices_host: the block of ray" % hip.EINVAL):
            model.gain_slices(out["wptr"], S, out["rowptr"], np.roll(out["sid"], 1), out["k"], weff, var=var)
        empty = model.gain_slices([0], np.zeros(0), [0], np.zeros(0, np.int32), np.zeros(0), np.zeros((0, nd)))   # nothing to do
        assert empty["gain"].shape == (0,)
        sequences.same_bits(formod_on(model, case.geom), want, "after gain_slices and its refusals")
        again = model.gain_scene(case.atm, geom, y, weight, var=var, prior_ivar=np.ones(n), want_gain=True)
        for f in ("gain", "sigma_comp", "sigma", "sigma_noise", "dofs", "rad"):
            bits(again[f], good[f], "%s in the call after the refusals" % f)
    finally:
        model.close()


def test_retained_blocks_beyond_the_budget_are_refused(hip):
    """One profile of 140 levels with p and T retrieved on all of them and as many rays as make the retained blocks and
    the gain larger than half of the smallest budget (32 MiB of 64): diagnose_scene, which holds the blocks of one pass
    only, still runs; gain_scene is refused with JUR_ENOMEM before anything is launched, and the model answers as a
    fresh one."""
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
    nr = half // (2 * 8 * w * c.nd) + 1                             # the blocks and the gain together exceed the half
    assert w >= 200 and 2 * 8 * nr * w * c.nd > half and nr < 20000
    geom = np.repeat(one, nr, axis=0)
    y, weight = np.zeros((nr, c.nd)), np.ones((nr, c.nd))
    probe = case.geom[:2].copy()
    probe[:, 0] = 0.0
    want = fresh_formod(hip, case, small, probe)
    cap = 64 * (w + 1)
    model = hip.Model(c, case.lib_tables())
    try:
        model.set_workspace_budget(64 << 20)
        model.set_atm(small)
        ok = model.diagnose_scene(small, geom, y, weight, prior_ivar=np.ones(w), max_rays_per_pass=cap)
        assert ok["status"][0] == 0
        with pytest.raises(hip.JurassicError, match=r"error -3: jur_gain_scene_host: the retained blocks of all rays \(%d columns" % (nr * w)):
            model.gain_scene(small, geom, y, weight, var=np.ones((2, nr, c.nd)), prior_ivar=np.ones(w), max_rays_per_pass=cap)
        sequences.same_bits(formod_on(model, probe), want, "after the refusal")
    finally:
        model.close()
