"""The CPU oracle against the reference's OWN CPU forward model: src/jurassic.c + src/CPUdrivers.c compiled where the
reference tree lies (oracle/Makefile, target `ref`; stand-in GSL headers with libm's expm1 / log1p), run in a fresh
process per configuration (oracle/ref.py), both programs reading the same table and filter files.

Live tests need oracle/_ref/libjurassic_ref.so.  Where the reference tree is present a missing library FAILS them
(build() makes it); where neither exists they skip.  The fixture tests need nothing but the repository: the results
the reference wrote are stored under tests/golden/reference_runs/ (tools/make_reference_goldens.py).

Bounds (refcases.py): transmittances, tangent points and finite masks bit-identical, radiances within 1e-14 relative
(measured 4.3e-16: one or two units in the last place on 9 of the limb example's 132 radiances, none on the nadir
example's; the operation that rounds differently has not been tracked down, so equality is not asserted), Jacobians within 1e-10 of each column's largest entry (measured 4.2e-12: that
last bit divided by the step h).  The rays named by refcases.departing -- from the inputs alone -- are the ones on
which the reference reads los[-1]: there the oracle's documented answer is asserted, and every
ray on which the programs differ must be one of them.  Measured maxima per group: tests/golden/README.md."""
import ctypes as C
import os
import numpy as np
import pytest
import common
import refcases as R
from jurassic_hip import abi, synth

ALL = list(R.FORMOD)
_cache = {}


@pytest.fixture(scope="module")
def ref():
    from oracle import ref as r
    if r.available():
        return r
    if r.required():
        pytest.fail("the reference tree is present but oracle/_ref/libjurassic_ref.so is not: make -C oracle ref")
    pytest.skip("neither oracle/_ref/libjurassic_ref.so nor the reference tree (JUR_REFERENCE) is here")


def prepared(name, oracle, tmp_path_factory):
    """-> dict(case, rad_in, hash, oracle result) of a formod case, its files written once per session."""
    if name not in _cache:
        case, rad_in = R.FORMOD[name]()
        d = str(tmp_path_factory.mktemp(name))
        case.write_files(d)
        _cache[name] = dict(case=case, rad_in=rad_in, hash=R.input_hash(case, d, rad_in),
                            oracle=R.run_oracle(oracle, case, rad_in))
    return _cache[name]


def live(name, ref, oracle, tmp_path_factory):
    c = prepared(name, oracle, tmp_path_factory)
    if "live" not in c:
        c["live"] = R.run_reference(ref, c["case"], c["rad_in"])
    return c


def differing_rays(o, r):
    """Boolean per ray: the oracle's result misses one of the bounds against the reference's; and the largest relative
    radiance error per ray."""
    fo, fr = np.isfinite(o["rad"]), np.isfinite(r["rad"])
    err = np.where(fo & fr, common.rel_err(o["rad"], r["rad"]), 0.0)
    bad = np.any(fo != fr, axis=1) | np.any(o["tau"] != r["tau"], axis=1) | np.any(o["tp"] != r["tp"], axis=1) | \
        np.any(err > R.RAD_RTOL, axis=1)
    return bad, err.max(axis=1, initial=0.0)


def check_against_reference(name, c, r):
    case, o = c["case"], c["oracle"]
    dep = R.departing(case)
    bad, err = differing_rays(o, r)
    print("%s: %d rays, %d departing, %d differing, oracle np = 0 on %d, largest relative radiance error outside the "
          "departing rays %.3g" % (name, len(dep), dep.sum(), bad.sum(), (o["np"] == 0).sum(), err[~dep].max(initial=0.0)))
    if dep.any():
        print("   reference on the departing rays: rad %.3g .. %.3g, tau %.3g .. %.3g, tpz %.4g .. %.4g km"
              % (np.nanmin(r["rad"][dep]), np.nanmax(r["rad"][dep]), r["tau"][dep].min(), r["tau"][dep].max(),
                 r["tp"][dep, 0].min(), r["tp"][dep, 0].max()))
    assert np.array_equal(bad, dep), ("differ, not selected", np.nonzero(bad & ~dep)[0],
                                      "selected, do not differ", np.nonzero(dep & ~bad)[0])
    if name not in ("scene_ragged", "scene_lone_ends", "scene_lone_up", "scene_short_last", "scene_unsorted",
                    "scene_ragged_extinction"):
        assert not dep.any()
    assert dep.sum() <= 0.12 * len(dep)
    # what the oracle documents for a slice it does not enter
    assert np.all(o["np"][dep] == 0) and np.all(o["rad"][dep] == 0) and np.all(o["tau"][dep] == 1)
    assert np.array_equal(o["tp"][dep], case.geom[dep][:, 4:7])


@pytest.mark.parametrize("name", ALL)
def test_oracle_formod_against_live_reference(ref, oracle, tmp_path_factory, name):
    c = live(name, ref, oracle, tmp_path_factory)
    check_against_reference(name, c, c["live"])


@pytest.mark.parametrize("name", ALL)
def test_stored_results_equal_a_live_run(ref, oracle, tmp_path_factory, name):
    """Bit for bit, NaN masks included.  On the departing rays the reference's result depends on memory it does not
    own (los[-1]): what it returned when the fixtures were written is stored, but not compared."""
    c = live(name, ref, oracle, tmp_path_factory)
    s, ok = R.stored(name), ~R.departing(c["case"])
    for k in ("rad", "tau", "tp"):
        assert s[k].shape == c["live"][k].shape
        assert np.array_equal(s[k][ok], c["live"][k][ok], equal_nan=True), k


@pytest.mark.parametrize("name", ALL + list(R.JACOBIANS))
def test_manifest_hash_equals_the_regenerated_inputs(oracle, tmp_path_factory, tmp_path, name):
    """A drift of synth, of the shipped example files or of the table writer reads "regenerate the fixtures"
    (tools/make_reference_goldens.py), not "radiance wrong"."""
    entry = R.manifest()[name]
    if name in R.JACOBIANS:
        case, obs = R.jacobian_case(name)
        case.write_files(str(tmp_path))
        digest = R.input_hash(case, str(tmp_path), np.ctypeslib.as_array(obs.rad)[:obs.nr, :case.ctl.nd])
        assert entry["shape"] == list(R.stored(name).shape)
    else:
        digest = prepared(name, oracle, tmp_path_factory)["hash"]
        assert entry["shape"] == [len(_cache[name]["case"].geom), 2 * _cache[name]["case"].ctl.nd + 3]
    assert digest == entry["sha256"], "inputs of %s changed: regenerate tests/golden/reference_runs" % name


def test_manifest_lists_every_case_and_nothing_else():
    assert sorted(R.manifest()) == sorted(ALL + list(R.JACOBIANS))
    files = sorted(f for f in os.listdir(R.STORE) if f.endswith(".npy"))
    want = sorted([n + ".npy" for n in ALL] + ["%s.rows_%s.npy" % (n, h) for n in R.JACOBIANS for h in "ab"])
    assert files == want
    sizes = [os.path.getsize(os.path.join(R.STORE, f)) for f in os.listdir(R.STORE)]
    assert max(sizes) < 64 * 1024 and sum(sizes) < 1024 * 1024


@pytest.mark.parametrize("name", ALL)
def test_oracle_formod_against_stored_reference(oracle, tmp_path_factory, name):
    """The same bounds where only the fixtures are: the oracle stays pinned without the reference tree."""
    c = prepared(name, oracle, tmp_path_factory)
    check_against_reference(name, c, R.stored(name))


# ---------------------------------------------------------------------------------------------------------------------
# kernel()

def jacobian_pair(name, oracle, d):
    case, obs = R.jacobian_case(name)
    case.write_files(d)
    obs_o = abi.obs_t.from_buffer_copy(bytes(obs))
    k = oracle.kernel(case.ctl, case.atm, obs_o, R.oracle_tables(oracle, case))
    assert len(case.geom) == 66 and k.shape == (66 * case.ctl.nd - 1, 6 + 31 + 21 + 11)
    return case, obs, obs_o, k


def check_jacobian(name, k, k_ref):
    scale = np.abs(k_ref).max(axis=0)
    live_cols = scale > 0
    assert live_cols.sum() >= 31 + 21 + 11
    assert np.array_equal(live_cols, np.abs(k).max(axis=0) > 0)          # all-zero columns are the same columns
    worst = float(np.max(np.abs(k[:, live_cols] - k_ref[:, live_cols]) / scale[live_cols]))
    print("%s: largest Jacobian difference %.3g of the column maximum, %d all-zero columns" % (name, worst, (~live_cols).sum()))
    assert worst < R.JAC_RTOL


@pytest.mark.parametrize("name", list(R.JACOBIANS))
def test_oracle_kernel_against_live_reference(ref, oracle, tmp_path, name):
    case, obs, obs_o, k = jacobian_pair(name, oracle, str(tmp_path))
    k_ref, obs_r = ref.kernel(case.ctl, case.atm, obs, *k.shape)
    check_jacobian(name, k, k_ref)
    a, b = ref.arrays(obs_o, case.ctl.nd), ref.arrays(obs_r, case.ctl.nd)
    fin = np.isfinite(b["rad"])
    assert np.array_equal(fin, np.isfinite(a["rad"])) and (~fin).sum() == 1
    assert common.rel_err(a["rad"][fin], b["rad"][fin]).max() <= R.RAD_RTOL
    assert np.array_equal(a["tau"], b["tau"]) and np.array_equal(a["tp"], b["tp"])
    assert np.array_equal(R.stored(name), k_ref)                         # the stored matrix is what a live run gives


@pytest.mark.parametrize("name", list(R.JACOBIANS))
def test_oracle_kernel_against_stored_reference(oracle, tmp_path, name):
    _, _, _, k = jacobian_pair(name, oracle, str(tmp_path))
    check_jacobian(name, k, R.stored(name))


# ---------------------------------------------------------------------------------------------------------------------
# formod_fov, intpol_atm, hydrostatic

def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("descending", [False, True])
def test_oracle_fov_convolution_against_live_reference(ref, oracle, tmp_path, descending):
    """The inputs of test_fov_convolution_matches_the_restatement.  The same operations in the same order: equal bits."""
    from test_abi_cpu import _fov_obs
    from jurassic_hip import lib
    nd = 3
    ctl = abi.make_ctl(["CO2"], [700.0, 800.0, 900.0])
    dz = np.linspace(-1.5, 1.5, 21)
    w = np.exp(-0.5 * (dz / 0.6) ** 2)
    shape = tmp_path / "fov.shape"
    shape.write_text("# dz [km]  weight\n" + "".join(f"{a:.6f} {b:.8g}\n" for a, b in zip(dz, w)))
    rdz, rw = lib.fov_read_shape(str(shape))
    ctl.fov = str(shape).encode()
    a = _fov_obs(nd, descending=descending)
    before = ref.arrays(a, nd)
    assert oracle.formod_fov(ctl, a, rdz, rw) == 0
    b = ref.formod_fov(ctl, _fov_obs(nd, descending=descending))
    x, y = ref.arrays(a, nd), ref.arrays(b, nd)
    assert not np.array_equal(x["rad"], before["rad"])
    assert same_bits(x["rad"], y["rad"]) and same_bits(x["tau"], y["tau"])


def test_oracle_intpol_atm_against_live_reference(ref, oracle):
    """The inputs of tests/test_intpol.py, IP = 1, 2, 3: pure IEEE arithmetic in the reference's order for t, q, k
    (equal bits); the pressure goes through exp / log (IP = 1, 2), where the reference's EXP macro and the oracle's
    restatement call the same libm in the same order -- equal bits as well.  What the reference aborts on, the
    oracle reports with its error number."""
    import test_intpol as T
    z, p, t, q, k = T._profile()
    one = T._fill(abi.atm_t(), z, 0 * z, 0 * z, p, t, q, k)
    cases = [(T._ctl(1), one, T.targets(5000, 5)), (T._ctl(2), T.track(), T.targets(6000, 6)),
             (T._ctl(3, cx=300.0, cz=4.0), T.cloud(), T.targets(4000, 7, lat=(38, 52), lon=(-7, 7), z=(-3, 66)))]
    for ctl, src, dest in cases:
        mine = abi.atm_t.from_buffer_copy(bytes(dest))
        src_o = abi.atm_t.from_buffer_copy(bytes(src))
        assert oracle.intpol_atm(ctl, mine, src_o) == 0
        theirs, log = ref.intpol_atm(ctl, dest, src)
        assert theirs is not None, log
        a, b = T.values(mine), T.values(theirs)
        nan = np.isnan(b["t"])
        assert np.array_equal(np.isnan(a["t"]), nan) and (ctl.ip != 3 or 0 < nan.sum() < len(nan))
        for key in ("p", "t", "q", "k"):
            assert same_bits(a[key][..., ~nan], b[key][..., ~nan]), (ctl.ip, key)
    bad = T._fill(abi.atm_t(), np.array([1.0, 2.0, 3.0]), np.array([0.0, 0.0, 1.0]), np.array([0.0, 0.0, 1.0]), np.ones(3),
                  np.ones(3), np.ones((T.NG, 3)), np.ones((1, 3)))
    far = T.track(3)
    np.ctypeslib.as_array(far.lat)[len(z):2 * len(z)] = 40.0
    for ctl, src, code, words in ((T._ctl(2), bad, -2, "Cannot identify profiles"), (T._ctl(2), far, -3, "Distance of profiles"),
                                  (T._ctl(4), far, -4, "Unknown interpolation")):
        assert oracle.intpol_atm(ctl, T.targets(4, 1), abi.atm_t.from_buffer_copy(bytes(src))) == code
        theirs, log = ref.intpol_atm(ctl, T.targets(4, 1), src)
        assert theirs is None and words in log, log


HYDRO_PTOL = 1e-13


def test_oracle_hydrostatic_against_live_reference(ref, oracle):
    """hydrostatic() of jurassic.c:263-310 (one call of hydrostatic_1d per profile) against the oracle's
    restatement of what formod() itself applies, hydrostatic_1d_h2o over the whole array (jr_common.h:713-761,
    CPUdrivers.c:98-103), on ONE profile, where the two cover the same points.  Not the same expression: the former
    divides the running sum by R, by T and by the number of points one after the other (jurassic.c:294,303), the latter
    by their product (jr_common.h:744,757), so each of the 20 terms of a layer's mean may differ in the last bit and
    the pressures, products of up to ~90 layers' exponentials, by a few 1e-16 per layer: 1e-13 relative bounds
    sqrt(90 * 20) ulp with a factor ~20 to spare (the measured figure is in tests/golden/README.md).  Everything but
    the pressure is untouched, bit for bit."""
    for hydz in (10.0, 0.0, 35.5):
        case = common.limb_case(hydz=hydz)
        mine = abi.atm_t.from_buffer_copy(bytes(case.atm))
        oracle.lib().orc_hydrostatic(C.byref(case.ctl), C.byref(mine))
        theirs = ref.hydrostatic(case.ctl, case.atm)
        n = case.atm.np
        g = lambda atm, k: np.ctypeslib.as_array(getattr(atm, k))[..., :n]
        for k in ("time", "z", "lon", "lat", "t", "q", "k"):
            assert same_bits(g(mine, k), g(theirs, k)) and same_bits(g(mine, k), g(case.atm, k)), k
        err = float(np.abs(g(mine, "p") / g(theirs, "p") - 1).max())
        moved = float(np.abs(g(theirs, "p") / g(case.atm, "p") - 1).max())
        print("hydrostatic hydz = %g: largest relative pressure difference %.3g (the call moves pressures by up to %.3g)"
              % (hydz, err, moved))
        assert moved > 1e-4 and err < HYDRO_PTOL
