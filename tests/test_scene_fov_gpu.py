"""The field of view inside the scene entries (Model.set_fov): kernel_scene, normal_scene, step_scene, trial_scene,
retrieve_scene and diagnose_scene on tangent-height scans, with the convolution done on the device between the forward
model and everything that reads its radiances.

The yardstick is a replay on the host with the project's own merged entries: Model.formod_host on a model without a
shape, lib.fov_apply on its results, one subtraction and one division per perturbed atmosphere.  Everything is compared
bit for bit; the one bound (the sums of normal_scene against np.longdouble) is the one tests/test_scene_normal_gpu.py
derives for the same comparison.

The scene: the `ragged` atmosphere with one scan per profile (13, 7, 2, 7 and 13 rays, 1 - 3 km apart, the fourth from
the top down) and a scan of 3 whose time stamp matches no profile; two channels; narrow retrieval windows (a slice has
at most a few dozen state elements); a shape of 13 points over +-1.5 km, out of order, one weight 0.  One test widens
the T window to all levels and takes a shape of 150 points: the sizes at which the kernel stages the shape in more than
one chunk and a ray has more values than its workgroup has lanes."""
import numpy as np
import pytest
import sequences
from jurassic_hip import synth
import common
from test_scene_jacobian_gpu import bits, channels_of, formod_on, fresh_formod, scene_case
from test_scene_normal_gpu import U, bumped, copy_atm, slice_of, sums_in_longdouble
from test_scene_retrieve_gpu import elements, prior_chain, rows_of, slice_mask, state_of, written_back

pytestmark = pytest.mark.gpu
LENGTHS = (13, 7, 2, 7, 13)
_order = np.random.default_rng(2).permutation(13)
DZ = np.linspace(-1.5, 1.5, 13)[_order]
W = np.exp(-0.5 * (DZ / 0.6) ** 2)
W[3] = 0.0
LAMS = (1e-2, 1.0, 1e2)
SETTINGS = dict(max_iter=3, tol=0.0, lam0=10.0, fac=(0.1, 1.0, 10.0), lam_min=1e-6, lam_max=100.0)
PER_SLICE = ("lam", "cost", "prior", "nlive", "state", "iters")
HISTORY = ("h_cost", "h_prior", "h_lam", "h_tcost", "h_tprior", "h_status", "h_best", "h_accept", "h_work")


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def windows(c):
    c.retp_zmin, c.retp_zmax = 20.0, 24.0
    c.rett_zmin, c.rett_zmax = 16.0, 28.0
    for g in range(c.ng):
        c.retq_zmin[g], c.retq_zmax[g] = -999.0, -999.0
    c.retq_zmin[2], c.retq_zmax[2] = 18.0, 24.0
    c.retk_zmin[0], c.retk_zmax[0] = 12.0, 16.0


def limb_scan(time, lon, lat, heights, azimuth, obsz=750.0):
    """(n, 7) limb rays of one scan: tangent points above (lon, lat) at `heights`, seen from obsz in one azimuth"""
    up = synth._cart(0.0, lon, lat)
    up /= np.linalg.norm(up)
    a = np.array([np.cos(azimuth), np.sin(azimuth), 0.3])
    a -= up * (a @ up)
    h = a / np.linalg.norm(a)
    g = np.zeros((len(heights), 7))
    for i, zt in enumerate(heights):
        xt = (synth.RE + zt) * up
        xo = xt - np.sqrt((synth.RE + obsz) ** 2 - (synth.RE + zt) ** 2) * h
        g[i] = (time,) + tuple(float(x) for x in synth._geo(xo)) + tuple(float(x) for x in synth._geo(xt))
    return g


def wide_windows(c):
    """T on all levels: slices of up to 150 elements, more than 256 values a ray"""
    windows(c)
    c.retp_zmin = c.retq_zmin[2] = c.retk_zmin[0] = -999.0
    c.retp_zmax = c.retq_zmax[2] = c.retk_zmax[0] = -999.0
    c.rett_zmin, c.rett_zmax = -10.0, 1000.0


def scan_geometry(case):
    """the scans on the `ragged` atmosphere of `case`"""
    spec = [s for s in synth.SCENES["ragged"][0] if s["n"] > 1]
    assert len(spec) == len(LENGTHS)
    rng = np.random.default_rng(4)
    scans = []
    for i, (s, n) in enumerate(zip(spec, LENGTHS)):
        heights = 14.0 + np.concatenate([[0.0], np.cumsum(rng.uniform(1.0, 3.0, n - 1))])
        scans.append(limb_scan(s["time"], s["lon"], s["lat"], heights[::-1] if i == 3 else heights, 0.7 * i))
    scans.append(limb_scan(1.5, spec[0]["lon"], spec[0]["lat"], 15.0 + 2.0 * np.arange(3), 0.3))
    assert np.all(np.diff(scans[3][:, 4]) < 0) and np.all(np.diff(scans[0][:, 4]) > 0)
    return np.vstack(scans)


_scene = {}


def scene(hip, name="ragged"):
    """(case, geom, y, weight, lay, iq, ip, x0), made once per name (`ragged`, or `ragged@channels` on one of
    common.CHANNELS): y the convolved forward model on the bumped atmosphere"""
    if name not in _scene:
        assert channels_of(name)[0] == "ragged"
        case = scene_case(name, windows=windows)
        geom = scan_geometry(case)
        _scene[name] = scene_of(hip, case, geom)
        assert np.diff(_scene[name][4]["wptr"]).max() <= 48
    return _scene[name]


def scene_of(hip, case, geom, shape=None):
    lay = hip.scene_slices(case.ctl, case.atm, geom[:, 0])
    lay.update(hip.scene_layout(case.ctl, case.atm, geom[:, 0]))
    widths = np.diff(lay["wptr"])
    assert len(widths) >= 3 and 0 < widths.min()
    iq, ip = elements(hip, case, lay)
    y = convolved(hip, case, bumped(case), geom, shape=shape)["rad"]
    assert np.all(np.isfinite(y))
    weight = 10.0 ** np.random.default_rng(11).uniform(0.0, 3.0, y.shape)
    for a in (geom, y, weight):
        a.setflags(write=False)
    return (case, geom, y, weight, lay, iq, ip, state_of(case, case.atm, iq, ip))


def apply_fov(hip, geom, out, shape=None):
    rad, tau = out["rad"].copy(), out["tau"].copy()
    hip.fov_apply(geom[:, 0], geom[:, 4], rad, tau, *(shape or (DZ, W)))
    return dict(out, rad=rad, tau=tau)


def convolved(hip, case, atm, geom, rad_in=None, model=None, shape=None):
    """formod_host on atm (a fresh model, or `model`: one without a shape) followed by lib.fov_apply"""
    if model is None:
        model = hip.Model(case.ctl, case.lib_tables())
        try:
            return convolved(hip, case, atm, geom, rad_in, model, shape)
        finally:
            model.close()
    model.set_atm(atm)
    return apply_fov(hip, geom, model.formod_host(geom, rad_in), shape)


def with_shape(hip, case):
    model = hip.Model(case.ctl, case.lib_tables())
    model.set_fov(DZ, W)
    model.set_atm(case.atm)
    return model


def masked_input(lay, shape):
    """rad_in with a NaN on the seventh ray of the first scan, in the last channel"""
    rad_in = np.zeros(shape)
    rad_in[6, shape[1] - 1] = np.nan
    assert lay["sid"][6] >= 0
    return rad_in


_normal = {}


def normal_with_mask(hip, name="ragged"):
    """normal_scene(want_k=True) with the shape set and masked_input, once per name"""
    if name not in _normal:
        case, geom, y, weight, lay = scene(hip, name)[:5]
        model = with_shape(hip, case)
        try:
            _normal[name] = model.normal_scene(case.atm, geom, y, weight, rad_in=masked_input(lay, y.shape), want_k=True)
        finally:
            model.close()
    return _normal[name]


def seeded_prior(hip, name="ragged"):
    case, geom, y, weight, lay, iq, ip, x0 = scene(hip, name)
    out = normal_with_mask(hip, name)
    rng = np.random.default_rng(3)
    r = [10.0 ** rng.uniform(-3.0, -1.0, len(np.diag(slice_of(out, s)[0]))) * np.diag(slice_of(out, s)[0]).mean()
         for s in range(len(lay["sfirst"]))]
    return np.concatenate(r), x0.copy()


# ---- 1. the blocks against the host replay ------------------------------------------------------------------------------
def step_of(iq, x):
    """the reference's step (jurassic.c:833-836) as jur_scene_stack_kernel states it"""
    if iq == 0:
        return max(abs(0.01 * x), 1e-7)
    if iq == 1:
        return 1.0
    return max(abs(0.01 * x), 1e-15) if iq < 2 + 5 else 1e-4


def test_kernel_scene_against_the_host_replay(hip, name="ragged"):
    case, geom, y, weight, lay, iq, ip, x0 = scene(hip, name)
    channels = channels_of(name)[1]
    assert case.ctl.ng == 5 and case.ctl.nd == (len(common.CHANNELS[channels]["nu"]) if channels else 2)
    nd = case.ctl.nd
    model = with_shape(hip, case)
    try:
        out = model.kernel_scene(case.atm, geom)
        one = model.kernel_scene(case.atm, geom, max_rays_per_pass=1)
        sequences.same_bits(formod_on(model, geom), fresh_formod(hip, case, case.atm, geom), "the model holds atm afterwards: pencil beams")
    finally:
        model.close()
    for f in ("k", "rad", "tau", "tp", "np"):
        bits(one[f], out[f], "%s, a scan per pass" % f)
    plain = hip.Model(case.ctl, case.lib_tables())
    try:
        plain.set_atm(case.atm)
        pencil = plain.formod_host(geom)
        base = apply_fov(hip, geom, pencil)
        bits(out["rad"], base["rad"], "rad against formod_host + fov_apply")
        bits(out["tau"], base["tau"], "tau against formod_host + fov_apply")
        bits(out["tp"], pencil["tp"], "tp")
        bits(out["np"], pencil["np"], "np")
        assert np.any(out["rad"] != pencil["rad"])
        rp, seen = lay["rowptr"], 0
        for s in range(len(lay["sfirst"])):
            rays = np.flatnonzero(lay["sid"] == s)
            w = int(lay["wptr"][s + 1] - lay["wptr"][s])
            want = np.zeros((len(rays), nd, w))
            for e in range(w):
                at = lay["wptr"][s] + e
                h = step_of(iq[at], x0[at])
                atm1 = copy_atm(case.atm)
                rows = rows_of(case, atm1)
                rows[iq[at]][ip[at]] = x0[at] + h
                g1 = convolved(hip, case, atm1, geom, model=plain)["rad"]
                want[:, :, e] = (g1[rays] - base["rad"][rays]) / h
                others = np.setdiff1d(np.arange(len(geom)), rays)
                bits(g1[others], base["rad"][others], "the other slices' rays do not see element %d of slice %d" % (e, s))
            for j, r in enumerate(rays):
                bits(out["k"][rp[r] * nd:rp[r + 1] * nd].reshape(nd, w), want[j], "block of ray %d" % r)
                seen += nd * w
            assert np.abs(want).max() > 0
        assert seen == len(out["k"]) > 0
    finally:
        plain.close()


def test_a_long_shape_and_wide_slices(hip, name="ragged"):
    """A shape of 150 points is staged 64 points at a time, and a slice of 150 elements gives a ray 302 values, more than
    the 256 lanes of its workgroup take at once: rad and tau, and the blocks of the first, the middle and the last
    element of every slice, against the host replay; the sums in passes of a scan against the default."""
    rng = np.random.default_rng(8)
    shape = (rng.uniform(-2.0, 2.0, 150), rng.uniform(0.0, 1.0, 150))
    case = scene_case(name, windows=wide_windows)
    case, geom, y, weight, lay, iq, ip, x0 = scene_of(hip, case, scan_geometry(case), shape)
    nd = case.ctl.nd
    assert (np.diff(lay["rowptr"]).max() + 1) * nd > 256 and np.all(iq == 1)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_fov(*shape)
        model.set_atm(case.atm)
        out = model.normal_scene(case.atm, geom, y, weight, want_k=True)
        one = model.normal_scene(case.atm, geom, y, weight, want_k=True, max_rays_per_pass=1)
        trial = model.trial_scene(case.atm, geom, y, weight, np.zeros((3, len(x0))))
    finally:
        model.close()
    for f in ("A", "b", "cost", "nlive", "k", "rad", "tau", "tp", "np"):
        bits(one[f], out[f], "%s, a scan per pass" % f)
    bits(trial["cost"], np.vstack([out["cost"]] * 3), "three trials dx = 0 against the cost")
    plain = hip.Model(case.ctl, case.lib_tables())
    try:
        base = convolved(hip, case, case.atm, geom, model=plain, shape=shape)
        bits(out["rad"], base["rad"], "rad")
        bits(out["tau"], base["tau"], "tau")
        rp = lay["rowptr"]
        for s in range(len(lay["sfirst"])):
            rays = np.flatnonzero(lay["sid"] == s)
            w = int(lay["wptr"][s + 1] - lay["wptr"][s])
            for e in sorted({0, w // 2, w - 1}):
                at = lay["wptr"][s] + e
                atm1 = copy_atm(case.atm)
                rows_of(case, atm1)[1][ip[at]] = x0[at] + 1.0
                g1 = convolved(hip, case, atm1, geom, model=plain, shape=shape)["rad"]
                for r in rays:
                    bits(out["k"][rp[r] * nd:rp[r + 1] * nd].reshape(nd, w)[:, e], (g1[r] - base["rad"][r]) / 1.0,
                         "column %d of the block of ray %d" % (e, r))
    finally:
        plain.close()


# ---- 2. the sums against the blocks -------------------------------------------------------------------------------------
def test_normal_scene_against_its_blocks(hip, name="ragged"):
    case, geom, y, weight, lay = scene(hip, name)[:5]
    out = normal_with_mask(hip, name)
    rad_in = masked_input(lay, y.shape)
    live = hip.scene_fov_live(geom[:, 0], rad_in)
    last = y.shape[1] - 1
    # the ray, five before it and five after it in its scan of 13, in the last channel alone
    assert live[:, :last].all() and np.array_equal(np.flatnonzero(~live[:, last]), np.arange(1, 12))
    host = convolved(hip, case, case.atm, geom, rad_in)
    bits(out["rad"], host["rad"], "rad: the NaN spreads where fov_apply spreads it")
    bits(out["tau"], host["tau"], "tau")
    assert np.isnan(out["rad"][:, last]).sum() >= 2 and not np.isnan(out["rad"][:, :last]).any()
    assert not np.any(live & np.isnan(out["rad"])), "the effective mask covers every NaN of G"
    ref = sums_in_longdouble(out, out["k"], y, weight, live)
    worst = 0.0
    for s in range(len(out["sfirst"])):
        A, b = slice_of(out, s)
        n = ref[s]["n"]
        assert out["nlive"][s] == n == live[out["sid"] == s].sum() and n > 0
        gamma = (n + 4) * U / (1 - (n + 4) * U)
        assert np.array_equal(A.view(np.uint64), A.T.copy().view(np.uint64))
        for got, want, mag in ((A, ref[s]["A"], ref[s]["Aabs"]), (b, ref[s]["b"], ref[s]["babs"]),
                               (out["cost"][s], ref[s]["cost"], ref[s]["cost"])):
            err = np.abs(np.asarray(got, np.longdouble) - want)
            bound = 2 * gamma * np.asarray(mag)
            worst = max(worst, float(np.max(err / np.maximum(bound, np.finfo(np.longdouble).tiny))))
            assert np.all(err <= bound), (s, float(err.max()), float(np.max(bound)))
        assert np.abs(A).max() > 0 and np.abs(b).max() > 0 and out["cost"][s] > 0
    print("FOV NORMAL %s: worst error / allowed %.3f" % (name, worst))
    s0 = out["sid"][6]
    assert out["nlive"][s0] == (out["sid"] == s0).sum() * case.ctl.nd - 11
    model = with_shape(hip, case)
    try:
        for cap in (1, 40):
            other = model.normal_scene(case.atm, geom, y, weight, rad_in=rad_in, want_k=True, max_rays_per_pass=cap)
            for f in ("A", "b", "cost", "nlive", "k", "rad", "tau", "tp", "np"):
                bits(other[f], out[f], "%s, passes of %d" % (f, cap))
    finally:
        model.close()


# ---- 3. closing the loop ------------------------------------------------------------------------------------------------
def test_the_convolved_forward_model_of_the_truth_costs_nothing(hip):
    case, geom, y, weight = scene(hip)[:4]
    truth = bumped(case)
    model = with_shape(hip, case)
    try:
        on = model.normal_scene(truth, geom, y, weight)
        model.set_fov(None)
        off = model.normal_scene(truth, geom, y, weight)
    finally:
        model.close()
    assert np.all(on["cost"].view(np.uint64) == 0), on["cost"]
    assert np.all(on["nlive"] > 0) and np.all(on["b"] == 0)
    assert np.all(off["cost"] > 0)


# ---- 4. the trial entry -------------------------------------------------------------------------------------------------
def test_trial_costs_are_normal_scene_on_the_written_back_atmosphere(hip, name="ragged"):
    case, geom, y, weight, lay, iq, ip, x0 = scene(hip, name)
    ns = len(lay["sfirst"])
    rad_in = masked_input(lay, y.shape)
    model = with_shape(hip, case)
    try:
        step = model.step_scene(case.atm, geom, y, weight, LAMS, rad_in=rad_in)
        assert np.all(step["status"] == 0)
        dx = step["dx"]
        want = np.zeros((len(LAMS), ns))
        for t in range(len(LAMS)):
            atm = written_back(case, case.atm, iq, ip, dx[t])
            model.set_atm(atm)
            want[t] = model.normal_scene(atm, geom, y, weight, rad_in=rad_in)["cost"]
        model.set_atm(case.atm)
        got = model.trial_scene(case.atm, geom, y, weight, dx, rad_in=rad_in)
        bits(got["cost"], want, "cost against normal_scene")
        assert np.all(want > 0) and np.any(want[1] < step["cost"])
        for cap in (1, 20):
            other = model.trial_scene(case.atm, geom, y, weight, dx, rad_in=rad_in, max_rays_per_pass=cap)
            bits(other["cost"], want, "cost, passes of %d" % cap)
        still = model.trial_scene(case.atm, geom, y, weight, np.zeros(len(x0)), rad_in=rad_in)
        bits(still["cost"][0], step["cost"], "a trial dx = 0 against the cost of the base")
        sequences.same_bits(formod_on(model, geom), fresh_formod(hip, case, case.atm, geom), "the model holds atm afterwards")
        model.set_fov(None)
        off = model.trial_scene(case.atm, geom, y, weight, dx, rad_in=rad_in)
        assert np.any(off["cost"] != want)
    finally:
        model.close()


# ---- 5. the loop against a replay on the host ---------------------------------------------------------------------------
def replay(hip, model, y, prior):
    """the loop of jur_retrieve_scene_host over step_scene, trial_scene and retrieve_decide of `model` (shape set)"""
    case, geom, _, weight, lay, iq, ip, x0 = scene(hip)
    s_ = SETTINGS
    ns = len(lay["sfirst"])
    fac = np.array(s_["fac"])
    nlam, mi = len(fac), s_["max_iter"]
    wptr, sid = lay["wptr"], lay["sid"]
    widths = np.diff(lay["rowptr"])
    r, xa = prior
    atm = copy_atm(case.atm)
    lam, state, iters = np.full(ns, s_["lam0"]), np.zeros(ns, dtype=np.int32), np.zeros(ns, dtype=np.int32)
    cost, pri, nlive = np.zeros(ns), np.zeros(ns), np.zeros(ns, dtype=np.int64)
    nan = np.nan
    h = dict(h_cost=np.zeros((mi, ns)), h_prior=np.zeros((mi, ns)), h_lam=np.full((mi, nlam, ns), nan),
             h_tcost=np.full((mi, nlam, ns), nan), h_tprior=np.full((mi, nlam, ns), nan),
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
        assert sorted(full_of) == list(np.flatnonzero(active))
        els = np.concatenate([np.arange(wptr[s], wptr[s + 1]) for s in full_of])
        x = state_of(case, atm, iq, ip)
        lamt = np.minimum(np.maximum(lam[None, :] * fac[:, None], s_["lam_min"]), s_["lam_max"])
        model.set_atm(atm)
        step = model.step_scene(atm, geom[rays], y[rays], weight[rays], lamt[:, full_of], prior_ivar=r[els], prior_dx=(xa - x)[els])
        trial = model.trial_scene(atm, geom[rays], y[rays], weight[rays], step["dx"], prior_ivar=r[els], prior_xa=xa[els])
        dx = np.zeros((nlam, len(x)))
        dx[:, els] = step["dx"]
        tcost, tpri, status = np.zeros((nlam, ns)), np.zeros((nlam, ns)), np.zeros((nlam, ns), dtype=np.int32)
        status[:, full_of], tcost[:, full_of], tpri[:, full_of] = step["status"], trial["cost"], trial["prior"]
        for j, s in enumerate(full_of):
            sl = slice(wptr[s], wptr[s + 1])
            cost[s], nlive[s], iters[s] = step["cost"][j], step["nlive"][j], iters[s] + 1
            pri[s] = prior_chain(r[sl], xa[sl], x[sl])
        h["h_cost"][it], h["h_prior"][it] = cost, pri
        for f, v in (("h_lam", lamt), ("h_tcost", tcost), ("h_tprior", tpri), ("h_status", status)):
            h[f][it][:, active] = v[:, active]
        h["h_work"][it] = (widths[rays] + 1).sum(), nlam * rays.sum()
        d = hip.retrieve_decide(cost + pri, tcost + tpri, lamt, status, lam, state, s_["tol"], s_["lam_max"], fac.max())
        lam, state = d["lam"], d["state"]
        h["h_best"][it], h["h_accept"][it] = d["best"], d["accept"]
        for s in np.flatnonzero(d["accept"] == 1):
            b = d["best"][s]
            atm = written_back(case, atm, iq, ip, dx[b], only=slice_mask(lay, s))
            cost[s], pri[s] = tcost[b, s], tpri[b, s]
    state[state == hip.RET_ACTIVE] = hip.RET_MAXITER
    return dict(h, x=state_of(case, atm, iq, ip), atm=atm, lam=lam, cost=cost.copy(), prior=pri.copy(), nlive=nlive, state=state, iters=iters)


def test_retrieve_scene_against_the_host_loop(hip):
    """Slice 1's y is the convolved forward model on the first guess and the prior's xa is the first guess: its b is 0,
    nothing is accepted, lam grows 10 -> 100 = lam_max and the second rejection ends it, so the third iteration runs on
    the rays that remain, whole scans fewer."""
    case, geom, y, weight, lay, iq, ip, x0 = scene(hip)
    prior = seeded_prior(hip)
    s0 = 1
    y2 = y.copy()
    y2[lay["sid"] == s0] = convolved(hip, case, case.atm, geom)["rad"][lay["sid"] == s0]
    s = dict(SETTINGS)
    mi, fac = s.pop("max_iter"), s.pop("fac")
    model = with_shape(hip, case)
    try:
        got = model.retrieve_scene(case.atm, geom, y2, weight, mi, fac, history=True, prior_ivar=prior[0], prior_xa=prior[1], **s)
        after = formod_on(model, geom)
        small = model.retrieve_scene(case.atm, geom, y2, weight, mi, fac, history=True, prior_ivar=prior[0], prior_xa=prior[1],
                                     max_rays_per_pass=1, **s)
        want = replay(hip, model, y2, prior)
    finally:
        model.close()
    for f in HISTORY + ("x",) + PER_SLICE:
        bits(got[f], want[f], f)
        bits(small[f], got[f], "%s, a scan per pass" % f)
    assert got["state"][s0] == hip.RET_STALLED and got["iters"][s0] == 2
    assert np.any(got["h_accept"] == 1) and got["h_work"][2, 0] < got["h_work"][0, 0]
    others = np.arange(len(lay["sfirst"])) != s0
    assert np.all(got["state"][others] == hip.RET_MAXITER)
    bits(state_of(case, got["atm"], iq, ip), got["x"], "atm_ret holds x")
    final = convolved(hip, case, got["atm"], geom)
    pencil = fresh_formod(hip, case, got["atm"], geom)
    for f in ("rad", "tau"):
        bits(got[f], final[f], "%s against formod_host + fov_apply on atm_ret" % f)
        bits(small[f], final[f], "%s, a scan per pass" % f)
    for f in ("tp", "np"):
        bits(got[f], pencil[f], f)
    sequences.same_bits(after, pencil, "the model holds atm_ret: pencil beams")


# ---- 6. the diagnostics -------------------------------------------------------------------------------------------------
def test_diagnose_scene_is_diagnose_slices_on_the_sums(hip):
    case, geom, y, weight, lay = scene(hip)[:5]
    out = normal_with_mask(hip)
    r = seeded_prior(hip)[0]
    model = with_shape(hip, case)
    try:
        got = model.diagnose_scene(case.atm, geom, y, weight, prior_ivar=r, want_normal=True, rad_in=masked_input(lay, y.shape))
        want = model.diagnose_slices(lay["wptr"], out["A"], prior_ivar=r)
    finally:
        model.close()
    for f in ("A", "b", "cost", "nlive", "rad", "tau"):
        bits(got[f], out[f], f)
    for f in ("sigma", "sigma_noise", "sigma_smooth", "avk_diag", "dofs", "status"):
        bits(got[f], want[f], f)
    assert np.all(got["status"] == 0) and np.all(got["dofs"] > 0)


# ---- 7. off again -------------------------------------------------------------------------------------------------------
def test_switching_the_shape_off_gives_a_fresh_models_bits(hip):
    case, geom = scene(hip)[:2]
    fresh = hip.Model(case.ctl, case.lib_tables())
    try:
        assert fresh.fov() is None
        fresh.set_atm(case.atm)
        want = fresh.kernel_scene(case.atm, geom)
    finally:
        fresh.close()
    model = with_shape(hip, case)
    try:
        dz, w = model.fov()
        bits(dz, DZ, "dz")
        bits(w, W, "w")
        on = model.kernel_scene(case.atm, geom)
        model.set_fov(None)
        assert model.fov() is None
        off = model.kernel_scene(case.atm, geom)
    finally:
        model.close()
    for f in ("k", "rad", "tau", "tp", "np"):
        bits(off[f], want[f], f)
    assert np.any(on["k"] != want["k"]) and np.any(on["rad"] != want["rad"])


# ---- 8. refusals --------------------------------------------------------------------------------------------------------
def test_refusals_and_state(hip):
    case, geom, y, weight, lay, iq, ip, x0 = scene(hip)
    want = fresh_formod(hip, case, case.atm, geom)
    n = len(x0)
    lone = np.vstack([geom, limb_scan(9.0, 10.0, 45.0, [20.0], 0.1)])
    pad = lambda a: np.vstack([a, a[:1]])
    two = np.vstack([geom, geom[20:22]])                                 # the second scan's time stamp again, at the end
    assert geom[19, 0] != geom[20, 0] == geom[21, 0] != geom[22, 0]
    pad2 = lambda a: np.vstack([a, a[:2]])
    einval = r"error %d: " % hip.EINVAL
    model = with_shape(hip, case)
    try:
        for who, call in (("jur_kernel_scene_host", lambda g, p: model.kernel_scene(case.atm, g)),
                          ("jur_normal_scene_host", lambda g, p: model.normal_scene(case.atm, g, p(y), p(weight))),
                          ("jur_trial_scene_host", lambda g, p: model.trial_scene(case.atm, g, p(y), p(weight), np.zeros(n))),
                          ("jur_retrieve_scene_host", lambda g, p: model.retrieve_scene(case.atm, g, p(y), p(weight), 2, (0.1, 10.0)))):
            with pytest.raises(hip.JurassicError, match=einval + who + r": .*ray %d is alone in its window: Cannot apply FOV convolution!" % len(geom)):
                call(lone, pad)
            sequences.same_bits(formod_on(model, geom), want, "%s after the lone ray" % who)
            with pytest.raises(hip.JurassicError, match=einval + who + r": .*ray %d starts a second run of rays with the time stamp" % len(geom)):
                call(two, pad2)
            sequences.same_bits(formod_on(model, geom), want, "%s after the time stamp in two runs" % who)
        for dz, w, message in ((np.zeros(3), np.array([1.0, np.nan, 1.0]), r"point 1 of the shape is \(0, nan\)"),
                               (np.array([0.0, np.inf]), np.ones(2), r"point 1 of the shape is \(inf, 1\)"),
                               (np.zeros(2), np.array([1.0, -1.0]), r"the weights sum to 0"),
                               (np.zeros(2), np.array([1e308, 1e308]), r"the weights sum to inf"),
                               (np.zeros(2049), np.ones(2049), r"n = 2049")):
            with pytest.raises(hip.JurassicError, match=einval + r"jur_model_set_fov: " + message):
                model.set_fov(dz, w)
            bits(model.fov()[0], DZ, "the shape that was set stays")
        sequences.same_bits(formod_on(model, geom), want, "after the bad shapes")
        bits(model.kernel_scene(case.atm, geom)["rad"], apply_fov(hip, geom, want)["rad"], "a call after the refusals")
    finally:
        model.close()
