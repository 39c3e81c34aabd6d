"""Model.normal_scene (jur_normal_scene_host): the Gauss-Newton normal equations of a scene per slice -- K^T W K,
K^T W (y - F), (y - F)^T W (y - F) and the number of terms -- accumulated on the device from the blocks of
Model.kernel_scene.

The error bound is derived, not measured.  A sum of n products formed in any order, fused or not, from the same inputs
differs from the exact sum by at most gamma_{n+4} * sum |terms| with gamma_m = m u / (1 - m u), u = 2^-53 (the dot-product
bound; the four spare roundings cover the products inside a term: K_i K_j, y - F, weight (y - F)).  The reference sums
and sum |terms| are formed from the blocks in np.longdouble; twice the bound is allowed.  Everything else is bit
identity: the sums run in ascending ray and channel order in accumulators that stay on the device, so neither the
passes nor the place of a ray in the call nor the copy of the blocks may change a bit."""
import ctypes as C
import numpy as np
import pytest
import common
import refcases as R
import sequences
from jurassic_hip import abi, synth
from test_scene_jacobian_gpu import NAMES, bits, formod_on, fresh_formod, scene_case, six_per_time_stamp

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
SUMS = ("A", "b", "cost", "nlive")


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def copy_atm(a):
    out = abi.atm_t()
    C.memmove(C.byref(out), C.byref(a), C.sizeof(abi.atm_t))
    return out


def bumped(case):
    """the scene's atmosphere with T raised by a smooth 2 K bump inside the T window"""
    atm = copy_atm(case.atm)
    n = atm.np
    z = np.ctypeslib.as_array(atm.z)[:n]
    lo, hi = case.ctl.rett_zmin, case.ctl.rett_zmax
    inside = (z >= lo) & (z <= hi)
    np.ctypeslib.as_array(atm.t)[:n][inside] += 2.0 * np.sin(np.pi * (z[inside] - lo) / (hi - lo)) ** 2
    return atm


_inputs = {}


def inputs(hip, name):
    """(case, geom, y, weight) of a scene, made once: six rays per time stamp, y the forward model on the bumped
    atmosphere, weights from a seeded generator over three decades."""
    if name not in _inputs:
        case = scene_case(name)
        geom = six_per_time_stamp(case.geom)
        y = fresh_formod(hip, case, bumped(case), geom)["rad"]
        assert np.all(np.isfinite(y))
        weight = 10.0 ** np.random.default_rng(11).uniform(0.0, 3.0, y.shape)
        for a in (geom, y, weight):
            a.setflags(write=False)
        _inputs[name] = (case, geom, y, weight)
    return _inputs[name]


_calls = {}


def blocks_and_sums(hip, name, arith="fast"):
    """Model.kernel_scene and Model.normal_scene(want_k=True) on the scene's rays (once per scene and mode)"""
    key = (name, arith)
    if key not in _calls:
        case, geom, y, weight = inputs(hip, name)
        model = hip.Model(case.ctl, case.lib_tables())
        try:
            model.set_arithmetic(hip.ARITH_EXACT if arith == "exact" else hip.ARITH_FAST)
            model.set_atm(case.atm)
            ks = model.kernel_scene(case.atm, geom)
            out = model.normal_scene(case.atm, geom, y, weight, want_k=True)
        finally:
            model.close()
        _calls[key] = (ks, out)
    return _calls[key]


def sums_in_longdouble(out, k, y, weight, live):
    """Per slice, in ascending ray and channel order: (A, b, cost) and the sums of the absolute terms, n"""
    ld = np.longdouble
    nd = y.shape[1]
    rp, res = out["rowptr"], []
    for s in range(len(out["sfirst"])):
        w = int(out["wptr"][s + 1] - out["wptr"][s])
        A, Aabs, b, babs = np.zeros((w, w), ld), np.zeros((w, w), ld), np.zeros(w, ld), np.zeros(w, ld)
        c, n = ld(0), 0
        for r in np.flatnonzero(out["sid"] == s):
            K = k[rp[r] * nd:rp[r + 1] * nd].reshape(nd, w).astype(ld)
            for i in range(nd):
                if not live[r, i]:
                    continue
                wt, d = ld(weight[r, i]), ld(y[r, i]) - ld(out["rad"][r, i])
                t = wt * np.outer(K[i], K[i])
                A, Aabs = A + t, Aabs + np.abs(t)
                t = wt * K[i] * d
                b, babs = b + t, babs + np.abs(t)
                c, n = c + wt * d * d, n + 1
        res.append(dict(A=A, Aabs=Aabs, b=b, babs=babs, cost=c, n=n))
    return res


def slice_of(out, s):
    w = int(out["wptr"][s + 1] - out["wptr"][s])
    return out["A"][out["aptr"][s]:out["aptr"][s + 1]].reshape(w, w), out["b"][out["wptr"][s]:out["wptr"][s + 1]]


@pytest.mark.parametrize("arith", ["fast", "exact"])
@pytest.mark.parametrize("name", NAMES)
def test_against_the_blocks(hip, name, arith):
    case, geom, y, weight = inputs(hip, name)
    ks, out = blocks_and_sums(hip, name, arith)
    for f in ("k", "rad", "tau", "tp", "np", "rowptr", "first", "len"):
        bits(out[f], ks[f], f)
    ns = len(out["sfirst"])
    assert ns >= 2 and np.diff(out["wptr"]).max() > 32             # more than one slice, more than two tiles a side
    ref = sums_in_longdouble(out, out["k"], y, weight, np.ones(y.shape, bool))
    worst = 0.0
    for s in range(ns):
        A, b = slice_of(out, s)
        n = ref[s]["n"]
        assert out["nlive"][s] == n == (out["sid"] == s).sum() * case.ctl.nd and n > 0
        gamma = (n + 4) * U / (1 - (n + 4) * U)
        assert np.array_equal(A.view(np.uint64), A.T.copy().view(np.uint64)), "A_s and its transpose differ"
        for got, want, mag in ((A, ref[s]["A"], ref[s]["Aabs"]), (b, ref[s]["b"], ref[s]["babs"]),
                               (out["cost"][s], ref[s]["cost"], ref[s]["cost"])):
            err = np.abs(np.asarray(got, np.longdouble) - want)
            bound = 2 * gamma * np.asarray(mag)
            worst = max(worst, float(np.max(err / np.maximum(bound, np.finfo(np.longdouble).tiny))))
            assert np.all(err <= bound), (s, float(err.max()), float(np.max(bound)))
        assert np.abs(A).max() > 0 and np.abs(b).max() > 0 and out["cost"][s] > 0
    print("NORMAL %s %s: worst error / allowed %.3f" % (name, arith, worst))


def interleaved(sid):
    """a permutation that deals the rays of the slices (and those without one) out in turn, each slice's in order"""
    groups = [list(np.flatnonzero(sid == s)) for s in np.unique(sid)]
    perm = []
    while any(groups):
        perm += [g.pop(0) for g in groups if g]
    return np.array(perm)


@pytest.mark.parametrize("name", ["ragged", "lone_ends"])
def test_arrangements(hip, name):
    case, geom, y, weight = inputs(hip, name)
    _, out = blocks_and_sums(hip, name)
    assert 257 < out["rowptr"][-1] + len(geom)                      # (257 ends a pass inside the scene)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        other = model.normal_scene(case.atm, geom, y, weight)
        assert "k" not in other
        for f in SUMS + ("rad", "tau", "tp", "np"):
            bits(other[f], out[f], "%s without k" % f)
        for cap in (1, 257, 0):
            for want_k in (False, True):
                other = model.normal_scene(case.atm, geom, y, weight, max_rays_per_pass=cap, want_k=want_k)
                for f in SUMS + ("rad", "tau", "tp", "np") + (("k",) if want_k else ()):
                    bits(other[f], out[f], "%s cap %d k %d" % (f, cap, want_k))
        perm = interleaved(out["sid"])
        assert not np.array_equal(perm, np.arange(len(perm)))
        assert np.any(np.diff(out["sid"][perm]) != 0) and np.all(np.diff(out["sid"][perm][:4]) != 0)
        other = model.normal_scene(case.atm, geom[perm], y[perm], weight[perm], max_rays_per_pass=257)
        for f in ("rad", "tau", "tp", "np"):
            bits(other[f], out[f][perm], "%s permuted" % f)
        where = {(int(a), int(b)): s for s, (a, b) in enumerate(zip(other["sfirst"], other["slen"]))}
        assert len(where) == len(out["sfirst"])
        for s, key in enumerate(zip(out["sfirst"], out["slen"])):
            p = where[(int(key[0]), int(key[1]))]
            for got, want, f in zip(slice_of(other, p), slice_of(out, s), ("A", "b")):
                bits(got, want, "%s of slice %d permuted" % (f, s))
            bits(other["cost"][p:p + 1], out["cost"][s:s + 1], "cost permuted")
            assert other["nlive"][p] == out["nlive"][s]
    finally:
        model.close()


def test_live_rule(hip, name="ragged"):
    case, geom, y, weight = inputs(hip, name)
    _, clear = blocks_and_sums(hip, name)
    nr, nd = y.shape
    live = np.flatnonzero(clear["sid"] >= 0)
    dead = np.flatnonzero(clear["sid"] < 0)
    assert len(dead) > 0
    # masked with NaN, masked with NaN, y = NaN, weight 0, masked with +inf, masked with -inf (the forward model masks
    # every channel whose input is not finite), in turn on the first and on the last channel; with more than two
    # channels every channel between them is masked with NaN on a further ray
    last = nd - 1
    gone = [(live[1], 0), (live[7], last), (live[3], 0), (live[5], last), (live[9], 0), (live[11], last)]
    between = [(live[13 + 2 * j], 1 + j) for j in range(nd - 2)]
    assert len(live) > 11 + 2 * max(nd - 2, 0) and {i for _, i in gone + between} == set(range(nd))
    masks = gone[:2] + gone[4:] + between
    rad_in = np.zeros((nr, nd))
    rad_in[gone[0]] = rad_in[gone[1]] = rad_in[dead[0], 0] = np.nan
    rad_in[gone[4]], rad_in[gone[5]] = np.inf, -np.inf
    for g in between:
        rad_in[g] = np.nan
    gone = gone + between
    y2, w2 = y.copy(), weight.copy()
    y2[gone[2]] = np.nan
    w2[gone[3]] = 0.0
    y2[dead[-1]] += 1e6                                             # a ray of width 0 with a large residual
    w0 = weight.copy()
    for g in gone:
        w0[g] = 0.0
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        out = model.normal_scene(case.atm, geom, y2, w2, rad_in=rad_in, want_k=True)
        want = model.normal_scene(case.atm, geom, y, w0)
    finally:
        model.close()
    for f in SUMS:
        bits(out[f], want[f], f)
        assert np.all(np.isfinite(out[f])), f
    removed = np.zeros(len(clear["nlive"]), dtype=np.int64)
    for r, _ in gone:
        removed[clear["sid"][r]] += 1
    assert removed.sum() == len(gone) == 6 + max(nd - 2, 0) and np.array_equal(out["nlive"], clear["nlive"] - removed)
    assert np.array_equal(np.isnan(out["rad"]), ~np.isfinite(rad_in))
    rp = out["rowptr"]
    for r, i in masks:                                           # the masked channel's row of the block is NaN, as kernel_scene's
        w = rp[r + 1] - rp[r]
        assert np.all(np.isnan(out["k"][rp[r] * nd + i * w:rp[r] * nd + (i + 1) * w]))


def test_refusals_and_state(hip):
    case, geom, y, weight = inputs(hip, "ragged")
    _, out = blocks_and_sums(hip, "ragged")
    want = fresh_formod(hip, case, case.atm, case.geom)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        good = model.normal_scene(case.atm, geom, y, weight)
        sequences.same_bits(formod_on(model, case.geom), want, "after a call")
        for bad in (-1.0, np.nan):
            w = weight.copy()
            w[17, 1] = bad
            with pytest.raises(hip.JurassicError, match=r"error %d: .*ray 17\b" % hip.EINVAL):
                model.normal_scene(case.atm, geom, y, w)
            sequences.same_bits(formod_on(model, case.geom), want, "after a weight of %g" % bad)
        wrong = out["rowptr"].copy()
        wrong[len(wrong) // 2:] += 1
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_normal_scene_host: .*rowptr" % hip.EINVAL):
            model.normal_scene(case.atm, geom, y, weight, rowptr=wrong)
        sequences.same_bits(formod_on(model, case.geom), want, "after a wrong rowptr")
        again = model.normal_scene(case.atm, geom, y, weight)
        for f in SUMS:
            bits(again[f], good[f], "%s in the call after the refusals" % f)
            bits(good[f], out[f], f)
        none = model.normal_scene(case.atm, geom[:0], y[:0], weight[:0], want_k=True)          # nr == 0
        assert none["rad"].shape == (0, case.ctl.nd) and all(len(none[f]) == 0 for f in SUMS + ("k",))
        sequences.same_bits(formod_on(model, case.geom), want, "after a call of no rays")
    finally:
        model.close()

    unsorted = scene_case("unsorted")
    g = six_per_time_stamp(unsorted.geom)
    want = fresh_formod(hip, unsorted, unsorted.atm, unsorted.geom)
    model = hip.Model(unsorted.ctl, unsorted.lib_tables())
    try:
        model.set_atm(unsorted.atm)
        with pytest.raises(hip.JurassicError, match=r"error %d: .*ascending" % hip.EINVAL):
            model.normal_scene(unsorted.atm, g, np.zeros((len(g), unsorted.ctl.nd)), np.ones((len(g), unsorted.ctl.nd)))
        sequences.same_bits(formod_on(model, unsorted.geom), want, "after unsorted time stamps")
    finally:
        model.close()

    hyd, _ = R.jacobian_case("jacobian_hydz10")
    want = fresh_formod(hip, hyd, hyd.atm, hyd.geom)
    model = hip.Model(hyd.ctl, hyd.lib_tables())
    try:
        model.set_atm(hyd.atm)
        shape = (len(hyd.geom), hyd.ctl.nd)
        with pytest.raises(hip.JurassicError, match=r"error %d: .*hydz" % hip.EINVAL):
            model.normal_scene(hyd.atm, hyd.geom, np.zeros(shape), np.ones(shape))
        sequences.same_bits(formod_on(model, hyd.geom), want, "after the hydz refusal")
    finally:
        model.close()


def all_temperatures(c):
    c.rett_zmin, c.rett_zmax = -10.0, 100.0


def test_time_stamps_that_share_a_slice(hip):
    """short_last with T retrieved at all altitudes: the rays of the time stamps 1.5 (which matches no profile) and 2.0
    are traced through the same two-level slice of width 2, and they do not lie next to each other in the call -- one
    ray list of mixed time stamps with a gap.  Sums against the blocks as in test_against_the_blocks; the same bits
    with every ray a pass of its own."""
    case = scene_case("short_last", windows=all_temperatures)
    geom = six_per_time_stamp(case.geom)
    t = geom[:, 0]
    order = np.concatenate([np.flatnonzero(t == 2.0)[:3], np.flatnonzero((t != 2.0) & (t != 1.5)), np.flatnonzero(t == 1.5),
                            np.flatnonzero(t == 2.0)[3:]])
    geom, t = geom[order], t[order]
    y = fresh_formod(hip, case, bumped(case), geom)["rad"]
    weight = 10.0 ** np.random.default_rng(12).uniform(0.0, 3.0, y.shape)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        out = model.normal_scene(case.atm, geom, y, weight, want_k=True)
        single = model.normal_scene(case.atm, geom, y, weight, max_rays_per_pass=1)
        ks = model.kernel_scene(case.atm, geom)
    finally:
        model.close()
    bits(out["k"], ks["k"], "k")
    shared = [s for s in range(len(out["sfirst"])) if len(np.unique(t[out["sid"] == s])) > 1]
    assert len(shared) == 1 and set(t[out["sid"] == shared[0]]) == {1.5, 2.0}
    rays = np.flatnonzero(out["sid"] == shared[0])
    assert len(rays) == 12 and np.diff(rays).max() > 1 and out["wptr"][shared[0] + 1] - out["wptr"][shared[0]] == 2
    ref = sums_in_longdouble(out, out["k"], y, weight, np.ones(y.shape, bool))
    for s in range(len(out["sfirst"])):
        A, b = slice_of(out, s)
        n = ref[s]["n"]
        assert out["nlive"][s] == n == (out["sid"] == s).sum() * case.ctl.nd
        gamma = (n + 4) * U / (1 - (n + 4) * U)
        for got, want, mag in ((A, ref[s]["A"], ref[s]["Aabs"]), (b, ref[s]["b"], ref[s]["babs"]),
                               (out["cost"][s], ref[s]["cost"], ref[s]["cost"])):
            assert np.all(np.abs(np.asarray(got, np.longdouble) - want) <= 2 * gamma * np.asarray(mag)), s
    assert np.abs(slice_of(out, shared[0])[0]).max() > 0
    for f in SUMS:
        bits(single[f], out[f], "%s, a pass per ray" % f)


def test_accumulators_beyond_the_budget_are_refused(hip):
    """One profile of 180 levels with p, T, all five gases and the extinction retrieved on every level: 1440 columns.  Its
    stacked copies (1440 x 180 points of 13 rows: 27 MB) fit into half of the smallest workspace budget (32 MiB of 64),
    the 1440^2 doubles of its normal matrix (16.6 MB) do not fit beside them: kernel_scene's layout is accepted,
    normal_scene returns JUR_ENOMEM before anything is launched, and the model answers as a fresh one."""
    case = common.limb_case()
    spec = [synth._spec(0.0, 10.0, 45.0, 180, 0.0, 90.0), synth._spec(1.0, 20.0, 30.0, 20, 0.0, 60.0)]
    case.atm = synth.ragged_atmosphere(case.ctl, spec, seed=0, base=case.atm, order=None)
    c = case.ctl
    c.retp_zmin, c.retp_zmax, c.rett_zmin, c.rett_zmax = -10.0, 100.0, -10.0, 100.0
    for g in range(c.ng):
        c.retq_zmin[g], c.retq_zmax[g] = -10.0, 100.0
    c.retk_zmin[0], c.retk_zmax[0] = -10.0, 100.0
    geom = case.geom[:2].copy()
    geom[:, 0] = 0.0
    want = fresh_formod(hip, case, case.atm, geom)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_workspace_budget(64 << 20)
        model.set_atm(case.atm)
        lay = hip.scene_slices(case.ctl, case.atm, geom[:, 0])
        assert list(np.diff(lay["wptr"])) == [1440]
        with pytest.raises(hip.JurassicError, match=r"error -3: jur_normal_scene_host: .*normal matrices"):
            model.normal_scene(case.atm, geom, np.zeros((2, c.nd)), np.ones((2, c.nd)))
        sequences.same_bits(formod_on(model, geom), want, "after the refusal")
    finally:
        model.close()


def test_no_windows_is_the_forward_model(hip):
    case = scene_case("lone_up", windows=None)
    shape = (len(case.geom), case.ctl.nd)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        out = model.normal_scene(case.atm, case.geom, np.ones(shape), np.ones(shape), want_k=True)
        assert len(out["sfirst"]) == 0 and np.all(out["sid"] == -1) and all(len(out[f]) == 0 for f in SUMS + ("k",))
        fm = formod_on(model, case.geom)
        sequences.same_bits(dict(rc=0, **{f: out[f] for f in ("rad", "tau", "tp", "np")}), fm, "state of zero elements")
    finally:
        model.close()


def test_closing_the_loop(hip):
    """A Levenberg-Marquardt step per slice from the outputs, written back through scene_elements: for at least one
    damping the summed cost falls.  (A_s + lambda diag A_s) is positive semi-definite and b_s = -1/2 grad cost, so dx
    is a descent direction, and for a large enough lambda the step is short enough for the cost to follow its slope:
    the assertion is that condition, not a size.  Elements no ray of the scene feels have a zero row, a zero b and get
    dx = 0 from the least-squares solve."""
    case, geom, y, weight = inputs(hip, "ragged")
    _, out = blocks_and_sums(hip, "ragged")
    before = float(out["cost"].sum())
    ratios = {}
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        for lam in (1e-2, 1.0, 1e2):
            atm = copy_atm(case.atm)
            rows = [np.ctypeslib.as_array(atm.p), np.ctypeslib.as_array(atm.t)]
            rows += list(np.ctypeslib.as_array(atm.q)[:case.ctl.ng]) + list(np.ctypeslib.as_array(atm.k)[:case.ctl.nw])
            for s in range(len(out["sfirst"])):
                A, b = slice_of(out, s)
                dx = np.linalg.lstsq(A + lam * np.diag(np.diag(A)), b, rcond=None)[0]
                el = hip.scene_elements(case.ctl, case.atm, out["sfirst"][s], out["slen"][s])
                assert len(dx) == len(el["cols"])
                for e in range(len(dx)):
                    rows[el["iq"][e]][el["ip"][e]] += dx[e]
            model.set_atm(atm)
            after = float(model.normal_scene(atm, geom, y, weight)["cost"].sum())
            ratios[lam] = after / before
            print("NORMAL step: lambda %g cost after / before %.4e" % (lam, ratios[lam]))
    finally:
        model.close()
    assert before > 0 and any(r < 1.0 for r in ratios.values()), ratios
