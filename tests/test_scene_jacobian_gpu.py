"""Model.kernel_scene (jur_kernel_scene_host): the Jacobian of a scene as per-ray blocks, with the perturbed slices, the
replicated rays and the difference quotients made on the device.

Both Jacobian entries put the same values through the same forward model, whose results do not depend on where a ray
sits in a call (tests/test_scenes_gpu.py::test_ray_order) nor on the arrangement of the kernels: the bar against
Model.kernel and Model.formod_host is bit-identity, and a single differing bit means that the stacking is wrong.
Against the reference's stored Jacobians the bound is the one tests/test_reference_gpu.py applies to Model.kernel."""
import numpy as np
import pytest
import common
import refcases as R
import sequences
from jurassic_hip import abi, synth

pytestmark = pytest.mark.gpu
NAMES = ["ragged", "lone_ends", "lone_up", "short_last"]


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def retrieval_windows(c):
    """as common.retrieval_case: p, T, one gas and the extinction"""
    c.retp_zmin, c.retp_zmax = 20.0, 25.0
    c.rett_zmin, c.rett_zmax = 10.0, 40.0
    for g in range(c.ng):
        c.retq_zmin[g], c.retq_zmax[g] = -999.0, -999.0
    c.retq_zmin[2], c.retq_zmax[2] = 15.0, 35.0
    c.retk_zmin[0], c.retk_zmax[0] = 10.0, 20.0


def narrow_windows(c):
    """T and one gas over a few kilometres: what keeps a case of many channels quick"""
    c.rett_zmin, c.rett_zmax = 10.0, 30.0
    for g in range(c.ng):
        c.retq_zmin[g], c.retq_zmax[g] = -999.0, -999.0
    c.retq_zmin[2], c.retq_zmax[2] = 18.0, 24.0


# what a channel configuration changes besides the channels: nd65 takes five rays per time stamp and narrow_windows
# in place of retrieval_windows (the widest slice of `ragged` then has 42 elements, that of `lone_ends` 19, and the
# rays and columns of either scene still exceed a pass of 257)
REDUCED = {"nd65": dict(per_time_stamp=5, windows=narrow_windows)}


def channels_of(name):
    """'ragged@nd3' -> ('ragged', 'nd3'): a scene's name may carry one of common.CHANNELS; 'ragged' -> ('ragged', '')"""
    base, _, channels = name.partition("@")
    return base, channels


def scene_case(name, nrays=180, windows=retrieval_windows):
    """The named scene of synth.SCENES on the limb example's two channels, or, as 'name@channels', on one of
    common.CHANNELS: every helper and cache keyed by the name carries the configuration with it."""
    base, channels = channels_of(name)
    reduced = REDUCED.get(channels, {})
    case = common.limb_case(**common.CHANNELS[channels]) if channels else common.limb_case()
    case.atm, case.geom, _ = synth.scene(base, case.ctl, case.atm, nrays=nrays)
    if "per_time_stamp" in reduced:
        case.geom = per_time_stamp(case.geom, reduced["per_time_stamp"])
    if windows is retrieval_windows:
        windows = reduced.get("windows", windows)
    if windows:
        windows(case.ctl)
    return case


def per_time_stamp(geom, n):
    return np.vstack([geom[geom[:, 0] == t][:n] for t in np.unique(geom[:, 0])])


def six_per_time_stamp(geom):
    return per_time_stamp(geom, 6)


def obs_result(obs, nd):
    n = obs.nr
    tp = np.column_stack([np.ctypeslib.as_array(getattr(obs, f))[:n] for f in ("tpz", "tplon", "tplat")])
    return dict(rad=np.ctypeslib.as_array(obs.rad)[:n, :nd].copy(), tau=np.ctypeslib.as_array(obs.tau)[:n, :nd].copy(), tp=tp)


def bits(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    if a.dtype.kind != "f":
        assert np.array_equal(a, b), what
        return
    assert np.array_equal(np.isnan(a), np.isnan(b)), (what, "NaN mask")
    m = ~np.isnan(a)
    bad = a[m].view(np.uint64) != b[m].view(np.uint64)
    assert not bad.any(), (what, int(bad.sum()), "values differ", float(np.abs(a[m] - b[m]).max()))


def in_block(hip, case, out, n):
    """(nr * nd, n) mask: the columns of every ray's block"""
    nd = case.ctl.nd
    m = np.zeros((len(out["first"]) * nd, n), dtype=bool)
    for r, (f, l) in enumerate(zip(out["first"], out["len"])):
        if out["rowptr"][r + 1] > out["rowptr"][r]:
            m[r * nd:(r + 1) * nd, hip.scene_columns(case.ctl, case.atm, f, l)] = True
    return m


_pairs = {}


def dense_and_blocks(hip, name, arith):
    """Model.kernel and Model.kernel_scene on the scene's rays, six per time stamp (computed once per scene and mode)."""
    key = (name, arith)
    if key not in _pairs:
        case = scene_case(name)
        geom = six_per_time_stamp(case.geom)
        obs = common.obs_from_geom(geom, case.ctl.nd)
        np.ctypeslib.as_array(obs.rad)[:] = 0.0
        model = hip.Model(case.ctl, case.lib_tables())
        try:
            model.set_arithmetic(hip.ARITH_EXACT if arith == "exact" else hip.ARITH_FAST)
            model.set_atm(case.atm)
            k = model.kernel(case.atm, obs)
            out = model.kernel_scene(case.atm, geom)
        finally:
            model.close()
        _pairs[key] = (case, geom, k, obs_result(obs, case.ctl.nd), out)
    return _pairs[key]


@pytest.mark.parametrize("arith", ["fast", "exact"])
@pytest.mark.parametrize("name", NAMES)
def test_same_doubles_as_the_dense_jacobian(hip, name, arith):
    case, geom, k, obs, out = dense_and_blocks(hip, name, arith)
    nd = case.ctl.nd
    assert k.shape[0] == len(geom) * nd                              # every measurement is finite: no row is dropped
    dense = hip.scene_blocks_to_dense(case.ctl, case.atm, out, n=k.shape[1])
    inside = in_block(hip, case, out, k.shape[1])
    assert inside.sum() == len(out["k"]) and inside.any() and not inside.all()
    assert np.all(k[~inside] == 0)                                   # outside the blocks the dense entries are exactly 0
    bits(dense[inside], k[inside], "blocks")
    assert (np.abs(k).max(axis=0) > 0).sum() >= 25
    for f in ("rad", "tau", "tp"):
        bits(out[f], obs[f], f)


@pytest.mark.parametrize("name", ["ragged", "lone_ends"])
def test_passes(hip, name):
    """Every ray a pass of its own (1), passes that end inside the scene (257: a ray of these scenes has up to ~150
    columns) and the model's own choice (0)."""
    case, geom, _, _, out = dense_and_blocks(hip, name, "fast")
    assert 257 < out["rowptr"][-1] + len(geom)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        for cap in (1, 257, 0):
            other = model.kernel_scene(case.atm, geom, max_rays_per_pass=cap)
            for f in ("k", "rad", "tau", "tp", "np", "rowptr"):
                bits(other[f], out[f], "%s cap %d" % (f, cap))
    finally:
        model.close()


def three_thousand_rays(geom, nextra):
    """The first 3000 - nextra of the scene's rays that the forward model takes, and the nextra rays of the extra time
    stamps behind them.  About one limb ray in a thousand of synth.global_geometry on this scene needs JUR_NLOS = 400
    LOS points or more, which every entry refuses (JUR_ENLOS: formod_host and the dense Model.kernel too): a limb ray
    (kinds 0 and 1) through the 150-level profile (time stamp 1.25, 2 - 95 km) whose tangent point lies in the
    profile's lowest 5 km.  The oracle's tracer counts 395 points at a tangent height of 6.3 km and 393 at 6.8 km,
    falling with height, and ends at 400 from 5.0 km down; rays that end on the profile's bottom need far fewer."""
    main, extra = geom[:len(geom) - nextra], geom[len(geom) - nextra:]
    nlive = sum(s["n"] > 1 for s in synth.SCENES["ragged"][0])
    kind = (np.arange(len(main)) // nlive) % 6
    too_long = (main[:, 0] == 1.25) & (kind < 2) & (main[:, 4] >= 2.0) & (main[:, 4] < 7.0)
    assert 0 < too_long.sum() < len(main) // 100
    return np.vstack([main[~too_long][:3000 - nextra], extra])


def test_beyond_one_package(hip):
    """3000 rays (jur_kernel takes 1088): blocks against Model.kernel on the three packages of 1000, np and tp against
    Model.formod_host."""
    def windows(c):
        c.rett_zmin, c.rett_zmax = 10.0, 40.0
    case = scene_case("ragged", nrays=3100, windows=windows)
    geom, nd = three_thousand_rays(case.geom, 6 * len(synth.SCENES["ragged"][1])), case.ctl.nd
    assert len(geom) == 3000
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        out = model.kernel_scene(case.atm, geom)
        fm = model.formod_host(geom)
        assert fm["np"].max() < abi.NLOS                            # three_thousand_rays: every ray kept fits (392 in the oracle)
        for f in ("np", "tp", "rad", "tau"):
            bits(out[f], fm[f], f)
        dense = hip.scene_blocks_to_dense(case.ctl, case.atm, out)
        inside = in_block(hip, case, out, dense.shape[1])
        assert inside.sum() == len(out["k"])
        for a in range(0, 3000, 1000):
            obs = common.obs_from_geom(geom[a:a + 1000], nd)
            np.ctypeslib.as_array(obs.rad)[:] = 0.0
            k = model.kernel(case.atm, obs)
            rows = slice(a * nd, (a + 1000) * nd)
            assert np.all(k[~inside[rows]] == 0)
            bits(dense[rows][inside[rows]], k[inside[rows]], "package at %d" % a)
    finally:
        model.close()


def test_nan_mask(hip, name="ragged"):
    case, geom, _, _, clear = dense_and_blocks(hip, name, "fast")
    nd, nr = case.ctl.nd, len(geom)
    rad_in = np.zeros((nr, nd))
    live = np.flatnonzero(np.diff(clear["rowptr"]))                  # two masked rays that have a block, one that has none
    assert np.diff(clear["rowptr"])[nr - 1] == 0                     # (the first channel, the last, the first)
    rad_in[live[1], 0] = rad_in[live[7], nd - 1] = rad_in[nr - 1, 0] = np.nan
    obs = common.obs_from_geom(geom, nd)
    np.ctypeslib.as_array(obs.rad)[:nr, :nd] = rad_in
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        out = model.kernel_scene(case.atm, geom, rad_in=rad_in)
        k = model.kernel(case.atm, obs)
    finally:
        model.close()
    n = k.shape[1]
    dense, ref = hip.scene_blocks_to_dense(case.ctl, case.atm, out, n=n), hip.scene_blocks_to_dense(case.ctl, case.atm, clear, n=n)
    inside = in_block(hip, case, out, n)
    masked = np.isnan(rad_in).ravel()
    assert np.all(np.isnan(dense[masked][inside[masked]]))           # the whole row of the block
    bits(dense[~masked], ref[~masked], "rows of the other channels")
    assert k.shape[0] == (~masked).sum()
    bits(dense[~masked][inside[~masked]], k[inside[~masked]], "rows kept against the dense rows kept")
    assert np.array_equal(np.isnan(out["rad"]).ravel(), masked)


@pytest.mark.parametrize("arith", ["fast", "exact"])
@pytest.mark.parametrize("name", ["jacobian", "jacobian_extinction"])
def test_blocks_against_stored_reference(hip, tmp_path, name, arith):
    """The reference's own kernel() on the limb example (one profile: one block per ray, all columns), tables read
    from the files the reference read.  Bound as tests/test_reference_gpu.py: 1e-6 of each column's largest entry."""
    case, obs = R.jacobian_case(name)
    case.write_files(str(tmp_path))
    k_ref = R.stored(name)
    nd, nr = case.ctl.nd, len(case.geom)
    rad_in = np.ctypeslib.as_array(obs.rad)[:nr, :nd].copy()
    model = hip.Model(case.ctl)
    try:
        model.set_arithmetic(hip.ARITH_EXACT if arith == "exact" else hip.ARITH_FAST)
        model.set_atm(case.atm)
        out = model.kernel_scene(case.atm, case.geom, rad_in=rad_in)
    finally:
        model.close()
    k = hip.scene_blocks_to_dense(case.ctl, case.atm, out)[np.isfinite(out["rad"]).ravel()]
    assert nr == 66 and k.shape == k_ref.shape == (66 * nd - 1, 6 + 31 + 21 + 11)
    scale = np.abs(k_ref).max(axis=0)
    live = scale > 0
    assert live.sum() >= 31 + 21 + 11 and np.all(k[:, ~live] == 0)
    worst = np.max(np.abs(k[:, live] - k_ref[:, live]) / scale[live])
    print("REFGPU %s kernel_scene %s jac_rel %.3e" % (name, arith, worst))
    assert worst < 1e-6


def test_hydrostatic_adjustment_is_refused(hip):
    case, obs = R.jacobian_case("jacobian_hydz10")
    want = fresh_formod(hip, case, case.atm, case.geom)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        with pytest.raises(hip.JurassicError, match=r"error %d: .*hydz" % hip.EINVAL):
            model.kernel_scene(case.atm, case.geom)
        sequences.same_bits(formod_on(model, case.geom), want, "after the hydz refusal")
    finally:
        model.close()


def formod_on(model, geom):
    return dict(model.formod_host(geom), rc=0)


def fresh_formod(hip, case, atm, geom):
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(atm)
        return formod_on(model, geom)
    finally:
        model.close()


def test_refusals_leave_the_model_as_a_fresh_one(hip):
    """After a successful call and after every refused one the model answers formod_host as a fresh model does: neither
    the stacked atmosphere nor anything else of the call stays behind."""
    case = scene_case("ragged")
    geom = six_per_time_stamp(case.geom)
    want = fresh_formod(hip, case, case.atm, case.geom)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        out = model.kernel_scene(case.atm, geom)
        sequences.same_bits(formod_on(model, case.geom), want, "after a call")
        wrong = out["rowptr"].copy()
        wrong[len(wrong) // 2:] += 1
        with pytest.raises(hip.JurassicError, match=r"error %d: .*rowptr" % hip.EINVAL):
            model.kernel_scene(case.atm, geom, rowptr=wrong)
        sequences.same_bits(formod_on(model, case.geom), want, "after a wrong rowptr")
        again = model.kernel_scene(case.atm, geom)
        bits(again["k"], out["k"], "the call after the refusal")
    finally:
        model.close()
    unsorted = scene_case("unsorted")
    want = fresh_formod(hip, unsorted, unsorted.atm, unsorted.geom)
    model = hip.Model(unsorted.ctl, unsorted.lib_tables())
    try:
        model.set_atm(unsorted.atm)
        with pytest.raises(hip.JurassicError, match=r"error %d: .*ascending" % hip.EINVAL):
            model.kernel_scene(unsorted.atm, six_per_time_stamp(unsorted.geom))
        sequences.same_bits(formod_on(model, unsorted.geom), want, "after unsorted time stamps")
    finally:
        model.close()


def test_no_windows_is_the_forward_model(hip):
    case = scene_case("lone_up", windows=None)
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        out = model.kernel_scene(case.atm, case.geom)
        assert len(out["k"]) == 0 and np.all(out["rowptr"] == 0)
        sequences.same_bits(dict(out, rc=0), formod_on(model, case.geom), "state of zero elements")
        none = model.kernel_scene(case.atm, case.geom[:0])
        assert len(none["k"]) == 0 and none["rad"].shape == (0, case.ctl.nd)
    finally:
        model.close()
