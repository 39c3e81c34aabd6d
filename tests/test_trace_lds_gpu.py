"""The batched ray tracer with the profile slice of a workgroup's rays staged in LDS (jur_trace_slice_kernel,
jur_tune_trace_slice(2)) against the tracer that reads the model's arrays (jur_tune_trace_slice(1)): the same values
read from another place by the same operations, so every output is the same double -- rad, tau, tp, np of the forward
model, and p, T, ds, q_H2O, k, u[ng], tsurf, tp, np and the status word of the LOS records (jur_kat_traceray, the
entry tests/test_kat_gpu.py::test_los_records_against_the_oracle reads), point by point.

The LOS entry traces the rays in the order given, 256 to a workgroup, so the geometry's order decides which
workgroups hold one slice (staged) and which straddle two (they read the model's arrays).  The slab holds 1280
doubles: rows z, p, T, ln-p slope, q[ng], k[nw] of the longest slice (include/jurassic_hip.h)."""
import numpy as np
import pytest
import common
import losrecords as L
from jurassic_hip import abi, synth

pytestmark = pytest.mark.gpu

SLAB_DOUBLES = 1280


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def both_ways(hip, case, forward=True, overflow_ok=False):
    """-> (records, forward results or None) with the slice in LDS and without; the forward model on the batched
    kernels whatever the call's size."""
    m = hip.Model(case.ctl, case.lib_tables())
    m.set_atm(case.atm)
    m.set_pencil(0)
    out = {}
    try:
        hip.tune_trace(1)                                   # a lane per ray: the arrangement that has the LDS variant
        for mode in (2, 1):
            hip.tune_trace_slice(mode)
            out[mode] = (m.kat_traceray(case.geom, overflow_ok=overflow_ok), m.formod_host(case.geom) if forward else None)
    finally:
        hip.tune_trace_slice(0)
        hip.tune_trace(0)
        m.close()
    return out[2], out[1]


def assert_same(on, off, what):
    (rec_on, fwd_on), (rec_off, fwd_off) = on, off
    for key in ("p", "t", "ds", "qh2o", "k", "u", "tsurf", "tp"):
        assert np.array_equal(bits(rec_on[key]), bits(rec_off[key])), (what, "records", key)
    assert np.array_equal(rec_on["np"], rec_off["np"]) and rec_on["status"] == rec_off["status"], (what, "np / status")
    if fwd_on is not None:
        for key in ("rad", "tau", "tp"):
            assert np.array_equal(bits(fwd_on[key]), bits(fwd_off[key])), (what, "forward", key)
        assert np.array_equal(fwd_on["np"], fwd_off["np"]), (what, "forward np")
        assert np.array_equal(fwd_on["np"], rec_on["np"]), (what, "np of the two entries")


def limb(nprofiles, per_profile):
    """`per_profile` limb rays on each of `nprofiles` profiles, sorted by (profile, tangent altitude)."""
    g = np.vstack([synth.limb_geometry(per_profile, scan=True, zmin=-8.0, zmax=70.0) for _ in range(nprofiles)])
    g[:, 0] = np.repeat(np.arange(nprofiles), per_profile)
    case = common.limb_case(geom=g)
    common.extinction_profile(case.atm)
    if nprofiles > 1:
        case.atm = synth.stack_profiles(case.atm, case.ctl, nprofiles, seed=7)
    return case


@pytest.mark.parametrize("nprofiles,per_profile", [(1, 300),     # (a) a full workgroup and a partial one, one slice
                                                   (2, 1100),    # (b) workgroup 4 (rays 1024 .. 1279) straddles the boundary
                                                   (3, 100)])    # (b') both workgroups straddle
def test_sorted_limb_rays(hip, nprofiles, per_profile):
    case = limb(nprofiles, per_profile)
    on, off = both_ways(hip, case)
    assert_same(on, off, (nprofiles, per_profile))
    assert on[0]["status"] == 0 and (on[0]["np"] > 100).any() and (on[0]["tsurf"] != -999).any()


@pytest.mark.parametrize("extra", [0, 1])
def test_slice_that_fills_the_slab_and_one_level_more(hip, tmp_path, extra):
    """(c) Eight emitters, one window: 13 rows; 98 levels are the most that fit 1280 doubles, 99 must fall back."""
    case = common.Case(L.EMITTERS8, [792.0, 832.0], L.generated_profiles(str(tmp_path), L.EMITTERS8),
                       synth.limb_geometry(300, scan=True, zmin=-8.0, zmax=70.0), table_kw=dict(nlev=2, ntemp=2))
    common.extinction_profile(case.atm)
    nrow = 4 + case.ctl.ng + case.ctl.nw
    n = SLAB_DOUBLES // nrow + extra
    assert nrow == 13 and (n * nrow > SLAB_DOUBLES) == bool(extra) and (n - 1) * nrow <= SLAB_DOUBLES
    case.atm = synth.ragged_atmosphere(case.ctl, [dict(time=0.0, lon=0.0, lat=0.0, n=n, z0=0.0, z1=90.0)], base=case.atm)
    on, off = both_ways(hip, case)
    assert_same(on, off, n)
    assert on[0]["status"] == 0 and (on[0]["np"] > 100).any()


def test_altitude_axis_that_is_not_monotone(hip):
    """(d) Two neighbouring levels change places: atm_sorted = 0, every bracket is found by bisection -- in LDS too."""
    case = limb(1, 300)
    a, n = case.atm, case.atm.np
    for name in ("z", "p", "t"):
        x = np.ctypeslib.as_array(getattr(a, name))[:n]
        x[[40, 41]] = x[[41, 40]]
    for name in ("q", "k"):
        x = np.ctypeslib.as_array(getattr(a, name))[:, :n]
        x[:, [40, 41]] = x[:, [41, 40]]
    on, off = both_ways(hip, case)
    assert_same(on, off, "not monotone")
    assert (on[0]["np"] > 100).any()


def test_edge_geometries(hip):
    """(e) Rays that miss, an observer inside or below the atmosphere, zenith and ground hits, short paths."""
    case = common.limb_case(geom=np.vstack([L.edge_rays(), synth.nadir_geometry(13, seed=4), L.SHORT_PATHS]))
    common.extinction_profile(case.atm)
    on, off = both_ways(hip, case)
    assert_same(on, off, "edges")
    assert (on[0]["np"] == 0).any() and (on[0]["tsurf"] != -999).any()


def test_ray_that_needs_nlos_points(hip):
    """(e) The ray of test_los_records_of_a_ray_that_needs_nlos_points among ordinary ones: status and clamped count."""
    g = np.vstack([synth.limb_geometry(1, scan=True, zmin=1.9, zmax=1.9), synth.limb_geometry(70, scan=True, zmin=5.0, zmax=70.0)])
    case = common.limb_case(geom=g)
    np.ctypeslib.as_array(case.atm.z)[:case.atm.np] *= 1.08
    common.extinction_profile(case.atm)
    on, off = both_ways(hip, case, forward=False, overflow_ok=True)
    assert_same(on, off, "overflow")
    assert on[0]["status"] == hip.ENLOS and on[0]["np"][0] == abi.NLOS - 1
