"""Model.param_scene (jur_param_scene_host): the parameter errors of a scene in one call, with the gain and the blocks K_b
of the parameters left on the device, against lib.param_error_scene -- gain_scene, kernel_scene under the parameters'
windows and param_slices -- on the same model.  Everything is bit identity: the entry runs the code of the three calls,
and the chains of C are those of jur_param_slices_host continued pass by pass (the one corner, a partial chain that is
exactly -0.0 where a pass ends, takes products that underflow and does not occur on these scenes).

The passes.  With 20 rays per time stamp a slice has 40 measurement rows at nd = 2 and 60 at nd = 3, so the 16-deep staging
of the cross kernel is crossed more than twice; max_rays_per_pass = 1 sends every ray alone (2 or 3 rows a pass), and the
test looks for a cap under which the rays of some slice fall into three or more passes of the parameter blocks whose row
counts are no multiples of 16, and asserts that it found one."""
import numpy as np
import pytest
from test_scene_jacobian_gpu import bits, per_time_stamp, scene_case
from test_scene_param_gpu import copy_ctl, no_windows, window_fields
from test_scene_gain_gpu import seeded_prior
from test_scene_fov_gpu import DZ, W, scene
from test_scene_solve_gpu import is_plus_zero

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def windows_x(case):
    """O3 retrieved over 15 - 35 km"""
    c = copy_ctl(case.ctl)
    no_windows(c)
    c.retq_zmin[2], c.retq_zmax[2] = 15.0, 35.0
    return c


def windows_t(case):
    """T the parameter over 10 - 40 km"""
    c = copy_ctl(case.ctl)
    no_windows(c)
    c.rett_zmin, c.rett_zmax = 10.0, 40.0
    return c


def new_model(hip, case, ctl, fov=False):
    m = hip.Model(ctl, case.lib_tables())
    if fov:
        m.set_fov(DZ, W)
    m.set_atm(case.atm)
    return m


def problem(hip, model, case, geom, ctl_b, ncov=1, with_prior=True, mask=True):
    """y, weight, a seeded prior, one masked channel, two diagonal components and ncov full ones (c_z = 5 km) for the
    parameters of ctl_b: the set-up of test_scene_param_gpu.test_a_real_parameter"""
    before = model.kernel_scene(case.atm, geom)
    nr, nd = before["rad"].shape
    rng = np.random.default_rng(21)
    y = before["rad"] * (1 + 1e-3 * rng.standard_normal((nr, nd)))
    weight = 10.0 ** rng.uniform(0.0, 3.0, (nr, nd))
    first = model.normal_scene(case.atm, geom, y, weight)
    ns = len(first["sfirst"])
    rad_in = np.zeros((nr, nd))
    if mask:
        rad_in[np.flatnonzero(first["sid"] >= 0)[2], 0] = np.nan
    rowptr_b = hip.scene_layout(ctl_b, case.atm, geom[:, 0])["rowptr"]
    lay = hip.param_layout(first["wptr"], first["rowptr"], rowptr_b, first["sid"])
    nbw = int(lay["bwptr"][-1])
    var_b = np.stack([np.ones(nbw), 10.0 ** np.random.default_rng(22).uniform(-1.0, 1.0, nbw)])
    cov_b = None
    if ncov:
        iq, z, sigma = [], [], []
        for s in range(ns):
            el = hip.scene_elements(ctl_b, case.atm, int(first["sfirst"][s]), int(first["slen"][s]))
            assert len(el["iq"]) == lay["bwptr"][s + 1] - lay["bwptr"][s]
            iq.append(el["iq"]); z.append([case.atm.z[i] for i in el["ip"]])
        iq, z = np.concatenate(iq), np.concatenate(z)
        pc = hip.prior_corr_slices(model, lay["bwptr"], iq, z, np.ones(nbw), np.full(2 + ctl_b.ng + ctl_b.nw, 5.0), want_Sa=True)
        assert np.all(pc["status"] == 0)
        cov_b = np.repeat(pc["Sa"][None, :], ncov, axis=0)
    return dict(y=y, weight=weight, prior=seeded_prior(first) if with_prior else None, rad_in=rad_in, var_b=var_b, cov_b=cov_b,
                lay=dict(lay, rowptr_b=rowptr_b), first=first, before=before)


def route(hip, model, case, geom, ctl_b, p, **kw):
    return hip.param_error_scene(model, ctl_b, case.atm, geom, p["y"], p["weight"], var_b=p["var_b"], cov_b=p["cov_b"],
                                 prior_ivar=p["prior"], rad_in=p["rad_in"], **kw)


def entry(model, case, geom, ctl_b, p, **kw):
    args = dict(var_b=p["var_b"], cov_b=p["cov_b"], prior_ivar=p["prior"], rad_in=p["rad_in"])
    args.update(kw)
    return model.param_scene(ctl_b, case.atm, geom, p["y"], p["weight"], **args)


def same(got, ref, what, absent=()):
    """every key of ref in got with the same bits; the keys in `absent` in neither"""
    for key, v in ref.items():
        if key in absent:
            assert key not in got, (key, what)
            continue
        assert key in got, (key, what)
        if key == "elements_b":
            assert len(got[key]) == len(v)
            for a, b in zip(got[key], v):
                assert set(a) == set(b)
                for f in b:
                    bits(a[f], b[f], "elements_b.%s %s" % (f, what))
        else:
            bits(got[key], v, "%s %s" % (key, what))


# ---- 1. against the three calls ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fov", [False, True], ids=["pencil", "fov"])
def test_against_the_three_calls(hip, fov):
    if fov:
        case, geom = scene(hip, "ragged")[:2]
    else:
        case = scene_case("ragged")
        geom = per_time_stamp(case.geom, 6)
    ctl_x, ctl_b = windows_x(case), windows_t(case)
    model = new_model(hip, case, ctl_x, fov)
    try:
        p = problem(hip, model, case, geom, ctl_b)
        assert len(p["first"]["sfirst"]) >= 3
        set_before = window_fields(model.ret_windows())
        ref = route(hip, model, case, geom, ctl_b, p)
        got = entry(model, case, geom, ctl_b, p, want_gain=True, want_kb=True)
        assert window_fields(model.ret_windows()) == set_before == window_fields(ctl_x)
        after = model.kernel_scene(case.atm, geom)
        model.set_ret_windows(ctl_b)
        kb = model.kernel_scene(case.atm, geom, rad_in=p["rad_in"])
        model.set_ret_windows(ctl_x)
    finally:
        model.close()
    assert np.all(ref["status"] == 0) and ref["sigma_param"].shape[0] == 3 and ref["sigma_param"].max() > 0
    assert np.abs(ref["C"]).max() > 0 and np.isnan(kb["k"]).sum() > 0
    same(got, ref, "against param_error_scene")
    bits(got["kb"], kb["k"], "kb against kernel_scene under ctl_b")
    bits(got["rowptr_b"], kb["rowptr"], "rowptr_b")
    for f in ("k", "rad", "tau", "rowptr"):
        bits(after[f], p["before"][f], "%s of kernel_scene after param_scene" % f)


# ---- 2. passes --------------------------------------------------------------------------------------------------------------
def splitting_cap(hip, lay, sid, nd):
    """a cap under which the rays of one slice fall into >= 3 passes of the parameter blocks, none of a multiple of 16 rows"""
    rb = lay["rowptr_b"]
    for cap in range(8, int(rb[-1]) + len(sid)):
        cuts = hip.scene_passes(rb, cap)[0]
        for s in range(int(sid.max()) + 1):
            rows = [int((sid[a:b] == s).sum()) * nd for a, b in zip(cuts[:-1], cuts[1:])]
            rows = [r for r in rows if r]
            if len(rows) >= 3 and all(r % 16 and r > nd for r in rows):   # (more than one ray of the slice in each)
                return cap, s, rows
    return None


@pytest.mark.parametrize("name", ["ragged", "ragged@nd3"])
def test_passes(hip, name):
    case = scene_case(name)
    geom = per_time_stamp(case.geom, 20)
    ctl_x, ctl_b = windows_x(case), windows_t(case)
    model = new_model(hip, case, ctl_x)
    try:
        p = problem(hip, model, case, geom, ctl_b)
        sid, nd = p["first"]["sid"], p["y"].shape[1]
        assert nd == (3 if name.endswith("nd3") else 2)
        assert max(int((sid == s).sum()) for s in range(int(sid.max()) + 1)) * nd >= 40
        found = splitting_cap(hip, p["lay"], sid, nd)
        assert found is not None, "no cap splits a slice into three passes"
        cap, s, rows = found
        print("PARAM_SCENE %s: cap %d puts slice %d into passes of %s rows" % (name, cap, s, rows))
        one = int(p["lay"]["rowptr_b"][-1] + p["first"]["rowptr"][-1]) + len(sid) + 1
        assert len(hip.scene_passes(p["lay"]["rowptr_b"], one)[0]) == 2 and len(hip.scene_passes(p["first"]["rowptr"], one)[0]) == 2
        assert len(hip.scene_passes(p["lay"]["rowptr_b"], 1)[0]) == len(sid) + 1
        assert len(hip.scene_passes(p["lay"]["rowptr_b"], cap)[0]) > 3
        ref = route(hip, model, case, geom, ctl_b, p)
        for c in (0, 1, cap, one):
            got = entry(model, case, geom, ctl_b, p, want_gain=True, max_rays_per_pass=c)
            same(got, ref, "with max_rays_per_pass %d" % c)
    finally:
        model.close()
    assert np.abs(ref["C"]).max() > 0


def test_passes_between_scans(hip):
    case, geom = scene(hip, "ragged")[:2]
    ctl_x, ctl_b = windows_x(case), windows_t(case)
    model = new_model(hip, case, ctl_x, fov=True)
    try:
        p = problem(hip, model, case, geom, ctl_b)
        rb = p["lay"]["rowptr_b"]
        cap = next(c for c in range(8, int(rb[-1]) + len(geom)) if 2 < len(hip.scene_passes(rb, c, time=geom[:, 0])[0]) < len(geom))
        cuts = hip.scene_passes(rb, cap, time=geom[:, 0])[0]
        assert all(geom[c, 0] != geom[c - 1, 0] for c in cuts[1:-1]), "a scan was split"
        whole = entry(model, case, geom, ctl_b, p, want_gain=True, want_kb=True)
        cut = entry(model, case, geom, ctl_b, p, want_gain=True, want_kb=True, max_rays_per_pass=cap)
    finally:
        model.close()
    same(cut, whole, "cut between scans")
    assert np.abs(whole["C"]).max() > 0


# ---- 3. widths --------------------------------------------------------------------------------------------------------------
def test_widths(hip):
    case = scene_case("ragged")
    geom = per_time_stamp(case.geom, 6)
    ctl_x = windows_x(case)
    ctl_b = copy_ctl(case.ctl)
    no_windows(ctl_b)
    # every quantity but the windows' extinction above 60.5 km: the profile that ends at 60 km has no parameter
    ctl_b.retp_zmin = ctl_b.rett_zmin = 60.5
    ctl_b.retp_zmax = ctl_b.rett_zmax = 1000.0
    for g in range(ctl_b.ng):
        ctl_b.retq_zmin[g], ctl_b.retq_zmax[g] = 60.5, 1000.0
    model = new_model(hip, case, ctl_x)
    try:
        p = problem(hip, model, case, geom, ctl_b, with_prior=True)
        w, wb = np.diff(p["first"]["wptr"]), np.diff(p["lay"]["bwptr"])
        print("PARAM_SCENE widths: w %s, wb %s" % (list(w), list(wb)))
        used = np.isin(np.arange(len(w)), p["first"]["sid"])
        assert np.any((wb == 0) & used) and np.any(wb > 128) and np.any((w < 64) != (wb < 64))
        ref = route(hip, model, case, geom, ctl_b, p)
        got = entry(model, case, geom, ctl_b, p, want_gain=True)
    finally:
        model.close()
    same(got, ref, "wide and empty parameter sets")
    for s in np.flatnonzero((wb == 0) & used):
        sl = slice(p["first"]["wptr"][s], p["first"]["wptr"][s + 1])
        assert is_plus_zero(got["sigma_param"][:, sl]), "a slice with wb == 0"
    assert got["sigma_param"].max() > 0


# ---- 4. switches held by the model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full_prior", [False, True], ids=["hydz", "hydz+precision"])
def test_switches(hip, full_prior):
    from test_prior_full_gpu import scene_sigma
    from test_scene_hydro_gpu import HYDZ
    case = scene_case("ragged")
    geom = per_time_stamp(case.geom, 6)
    ctl_x = windows_x(case)
    ctl_b = copy_ctl(case.ctl)
    no_windows(ctl_b)
    ctl_b.rett_zmin, ctl_b.rett_zmax = 10.0, 40.0                   # T and the pressure at the reference level
    ctl_b.retp_zmin, ctl_b.retp_zmax = 21.3, 22.65
    model = new_model(hip, case, ctl_x)
    try:
        model.set_scene_hydz(HYDZ)
        if full_prior:
            pc = hip.prior_corr(model, ctl_x, case.atm, geom[:, 0], scene_sigma(case), [5.0] * (2 + ctl_x.ng + ctl_x.nw))
            assert np.all(pc["status"] == 0)
            model.set_prior_precision(pc["wptr"], pc["R"])
        p = problem(hip, model, case, geom, ctl_b, with_prior=not full_prior)
        if full_prior:
            p["prior"] = np.zeros(int(p["first"]["wptr"][-1]))
        ref = route(hip, model, case, geom, ctl_b, p)
        got = entry(model, case, geom, ctl_b, p, want_gain=True, want_kb=True, max_rays_per_pass=300)
        model.set_ret_windows(ctl_b)
        kb = model.kernel_scene(case.atm, geom, rad_in=p["rad_in"])
    finally:
        model.close()
    assert np.any(np.diff(p["lay"]["bwptr"]) > 0) and np.all(ref["status"] == 0) and ref["sigma_param"].max() > 0
    same(got, ref, "with the balance%s" % (" and a prior precision" if full_prior else ""))
    bits(got["kb"], kb["k"], "kb under the balance")


# ---- 5. optional outputs ------------------------------------------------------------------------------------------------------
def test_optional_outputs(hip):
    case = scene_case("ragged")
    geom = per_time_stamp(case.geom, 6)
    ctl_x, ctl_b = windows_x(case), windows_t(case)
    model = new_model(hip, case, ctl_x)
    try:
        p = problem(hip, model, case, geom, ctl_b)
        full = entry(model, case, geom, ctl_b, p, want_gain=True, want_kb=True, want_C=True)
        for gain, kb, Cm in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
            got = entry(model, case, geom, ctl_b, p, want_gain=gain, want_kb=kb, want_C=Cm)
            absent = [k for k, on in (("gain", gain), ("kb", kb), ("C", Cm)) if not on]
            same(got, full, "with gain %r, kb %r, C %r" % (gain, kb, Cm), absent=absent)
        bare = entry(model, case, geom, ctl_b, p, var_b=None, cov_b=None)
        assert bare["sigma_param"].shape == (0, full["sigma_param"].shape[1])
        bits(bare["C"], full["C"], "C without components")
    finally:
        model.close()
    assert full["sigma_param"].max() > 0


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    case = scene_case("ragged")
    geom = per_time_stamp(case.geom, 6)
    ctl_x, ctl_b = windows_x(case), windows_t(case)
    model = new_model(hip, case, ctl_x)
    einval = r"error %d: jur_param_scene_host: " % hip.EINVAL
    try:
        p = problem(hip, model, case, geom, ctl_b)
        gs = lambda: model.gain_scene(case.atm, geom, p["y"], p["weight"], prior_ivar=p["prior"], want_gain=True, rad_in=p["rad_in"])
        before, set_before = gs(), window_fields(model.ret_windows())

        def unharmed(what):
            assert window_fields(model.ret_windows()) == set_before, what
            again = gs()
            for f in ("gain", "sigma", "rad", "tau", "cost", "status", "sigma_noise"):
                bits(again[f], before[f], "%s of gain_scene after %s" % (f, what))

        with pytest.raises(hip.JurassicError, match=einval + r"the variance of component 1, slice 0, element 0 is -"):
            v = p["var_b"].copy()
            v[1, 0] *= -1
            entry(model, case, geom, ctl_b, p, var_b=v)
        unharmed("a negative var_b")
        with pytest.raises(hip.JurassicError, match=einval + r"cov of component 2, slice 0, element \(1, 0\) is nan: not finite"):
            c = p["cov_b"].copy()
            wb0 = int(p["lay"]["bwptr"][1])
            assert wb0 > 1
            c[0, wb0] = np.nan                                            # (1, 0): below the diagonal, read
            entry(model, case, geom, ctl_b, p, cov_b=c)
        unharmed("a NaN in cov_b")
        c = p["cov_b"].copy()
        c[0, 1] = np.nan                                                  # (0, 1): above the diagonal, never read
        bits(entry(model, case, geom, ctl_b, p, cov_b=c)["sigma_param"], entry(model, case, geom, ctl_b, p)["sigma_param"],
             "sigma_param with a NaN above the diagonal of cov_b")
        # a rowptr_b that is not the layout's: the C entry, with the binding's own structs
        full = entry(model, case, geom, ctl_b, p)
        rb = full["rowptr_b"].copy()
        rb[-1] += 1
        rc, msg = raw_call(hip, model, case, geom, ctl_b, p, full, rb)
        assert rc == hip.EINVAL and msg == ("jur_param_scene_host: rowptr_b is not jur_scene_layout's for these rays, this "
                                            "atmosphere and the windows of ctl_b"), msg
        unharmed("a rowptr_b that is not the layout's")
        rc, msg = raw_call(hip, model, case, geom, ctl_b, p, full, full["rowptr_b"], bwptr=full["bwptr"] + np.arange(len(full["bwptr"])))
        assert rc == hip.EINVAL and msg.startswith("jur_param_scene_host: bwptr gives slice 0 "), msg
        unharmed("a bwptr that is not the layout's")
        rc, msg = raw_call(hip, model, case, geom, ctl_b, p, full, full["rowptr_b"])
        assert rc == 0, msg
        # half a prior: a precision in the model, no prior_ivar in the call
        from test_prior_full_gpu import scene_sigma
        pc = hip.prior_corr(model, ctl_x, case.atm, geom[:, 0], scene_sigma(case), [5.0] * (2 + ctl_x.ng + ctl_x.nw))
        model.set_prior_precision(pc["wptr"], pc["R"])
        with pytest.raises(hip.JurassicError, match=einval + r"a prior precision is set in the model: prior_ivar"):
            entry(model, case, geom, ctl_b, p, prior_ivar=None)
        model.set_prior_precision(None)
        unharmed("half a prior")
        again = entry(model, case, geom, ctl_b, p)
        same(again, full, "after the refusals")
    finally:
        model.close()


def raw_call(hip, model, case, geom, ctl_b, p, full, rowptr_b, bwptr=None):
    """jur_param_scene_host through ctypes with a rowptr_b and a bwptr of the caller's -> (rc, message)"""
    import ctypes as C
    dp, lp_ = C.POINTER(C.c_double), C.POINTER(C.c_long)
    g = np.ascontiguousarray(geom.T)
    nr, nd = p["y"].shape
    n, ns = int(full["wptr"][-1]), len(full["sfirst"])
    rad, tau, tp = p["rad_in"].copy(), np.zeros((nr, nd)), np.zeros((3, nr))
    y, weight, prior = (np.ascontiguousarray(x) for x in (p["y"], p["weight"], p["prior"]))
    vec = [np.zeros(n) for _ in range(4)]
    dofs, status = np.zeros(ns), np.zeros(ns, dtype=np.int32)
    dout = hip.DiagOut(*[hip._p(v) for v in vec], hip._p(dofs), status.ctypes.data_as(C.POINTER(C.c_int)), None, None)
    gin, gout = hip.GainIn(0, None), hip.GainOut(None, None)
    var, cov = np.ascontiguousarray(p["var_b"]), np.ascontiguousarray(p["cov_b"])
    sig = np.zeros((var.shape[0] + cov.shape[0], n))
    pin = hip.ParamIn(var.shape[0], cov.shape[0], hip._p(var), hip._p(cov))
    pout = hip.ParamOut(None, hip._p(sig))
    rb = np.ascontiguousarray(rowptr_b, dtype=np.int64)
    bw = None if bwptr is None else np.ascontiguousarray(bwptr, dtype=np.int64)
    sin = hip.ParamSceneIn(C.addressof(ctl_b), rb.ctypes.data_as(lp_), None if bw is None else bw.ctypes.data_as(lp_), C.pointer(pin))
    sout = hip.ParamSceneOut(C.pointer(pout), None, None)
    garr = (dp * 7)(*[hip._p(g[i]) for i in range(7)])
    tarr = (dp * 3)(*[hip._p(tp[i]) for i in range(3)])
    rp = np.ascontiguousarray(full["rowptr"], dtype=np.int64)
    rc = hip.lib().jur_param_scene_host(model.h, C.byref(case.atm), nr, garr, hip._p(rad), hip._p(tau), tarr, None, rp.ctypes.data_as(lp_),
                                        hip._p(y), hip._p(weight), hip._p(prior), C.byref(dout), C.byref(gin), C.byref(gout),
                                        C.byref(sin), C.byref(sout), None, None, None, None, None, 0)
    msg = hip.lib().jur_last_error().decode()
    if rc == 0:
        bits(sig, full["sigma_param"], "sigma_param through the C entry")
    return rc, msg
