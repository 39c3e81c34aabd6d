"""Point-cloud atmosphere along the line of sight (IP 3), the part that needs no GPU.

  * tests/cloud_model.py's restatement of intpol_atm_3d equals the oracle's orc_intpol_atm under ip = 3 bit for bit on
    destination points spread through the cloud (a destination's x0 is the oracle's own geo2cart);
  * the model's tracer under the 1-D rule equals orc.traceray bit for bit;
  * jur_cloud_points, the host function behind every upload under ip = 3, equals the model's table bit for bit, and
    refuses NULL;
  * the condition on the inputs of tests/test_cloud_gpu.py: over every evaluation the model makes for the main case
    wsum >= 1e-3, a thousand times the rule's threshold, and no record is NaN -- the GPU comparison never sits on the
    threshold.
"""
import ctypes as C
import numpy as np
import pytest
import common
import cloud_model as CM
import track_model as T
from jurassic_hip import abi, lib
from test_track_cpu import base_case, points_atm, same_doubles


def cloud_case(**kw):
    """The fixed rays (cloud_model.RAYS8 of track_model.track_rays()) on the two-block test cloud, ip = 3.  cx: the
    issue's 150 km leaves most of these rays in holes -- a limb ray runs some 1000 km through the atmosphere on either
    side of its tangent point, the four columns span 1.5 degrees -- so the influence radius is enlarged, as the issue
    provides, until the condition test_inputs_stay_clear_of_the_threshold asserts holds: 1500 km."""
    kw.setdefault("ip", 3)
    kw.setdefault("cx", CM.CX)
    kw.setdefault("cz", CM.CZ)
    case = base_case(**kw)
    case.geom = case.geom[CM.RAYS8]
    case.base = case.atm
    case.atm = CM.cloud_atmosphere(case.ctl, case.base)
    return case


@pytest.mark.parametrize("cx,cz", [(150.0, 3.0), (CM.CX, CM.CZ), (60.0, 0.7)])
def test_3d_restatement_equals_the_oracle(oracle, cx, cz):
    """1 200 destination points against orc.intpol_atm under ip = 3 on block A (upstream's ip 3 knows one block):
    random ones through and around the cloud, points exactly on a parcel, points beyond the influence radius."""
    case = base_case(ip=3, cx=cx, cz=cz)
    src = CM.cloud_atmosphere(case.ctl, case.atm, second_block=False)
    a = CM.Cloud(src, case.ctl)
    rng = np.random.default_rng(12)
    on = rng.integers(0, a.np, 200)
    z = np.concatenate([rng.uniform(-2.0, 93.0, 800), a.Z[on], rng.uniform(0.0, 90.0, 200)])
    lat = np.concatenate([rng.uniform(-1.5, 1.5, 800), a.LAT[on], rng.uniform(-14.0, 14.0, 200)])
    lon = np.concatenate([rng.uniform(-0.5, 0.5, 800), np.array(a.lon)[on], rng.uniform(-3.0, 3.0, 200)])
    dest = points_atm(z, lon, lat)
    assert oracle.intpol_atm(case.ctl, dest, src) == 0
    n = len(z)
    got = [CM.mean_3d(a, 0, a.np, float(z[i]), float(lon[i]), float(lat[i])) for i in range(n)]
    p = np.array([g[0] for g in got])
    assert same_doubles(p, np.ctypeslib.as_array(dest.p)[:n])
    assert same_doubles([g[1] for g in got], np.ctypeslib.as_array(dest.t)[:n])
    for ig in range(case.ctl.ng):
        assert same_doubles([g[2][ig] for g in got], np.ctypeslib.as_array(dest.q)[ig, :n]), ig
    assert same_doubles([g[3][0] for g in got], np.ctypeslib.as_array(dest.k)[0, :n])
    assert np.isfinite(p).sum() > 100
    if cx < 1000:
        assert np.isnan(p).sum() > 50, "no destination point lies in a hole"


@pytest.mark.parametrize("refrac", [1, 0])
def test_tracer_1d_rule_equals_the_oracle(oracle, refrac):
    """The code object the 3-D model runs, under the 1-D rule on the one-profile atmosphere: orc.traceray bit for bit."""
    case = base_case(refrac=refrac)
    a = CM.Cloud(case.atm, case.ctl)
    a.altitude_range = lambda a0, n: T.Atm.altitude_range(a, a0, n)        # one column: upstream's rule
    for g in case.geom[CM.RAYS8]:
        g = g.copy()
        g[0] = 0.0
        ref = oracle.traceray(case.ctl, case.atm, g)
        got = CM.traceray(case.ctl, a, g, rule=1)
        assert got["np"] == ref["np"] and ref["np"] > 0, g
        for f in ("z", "lon", "lat", "p", "t", "ds"):
            assert same_doubles(got[f], ref[f]), (f, g)
        assert same_doubles(got["k"][0], ref["k"]) and same_doubles(got["q"], ref["q"]) and same_doubles(got["u"], ref["u"]), g
        assert same_doubles([got["tsurf"]], [ref["tsurf"]]) and same_doubles(got["tp"], ref["tp"]), g


def test_whole_slice_range_agrees_with_the_first_column_rule_on_columns():
    """Rule 2 on a slice made of columns on one altitude grid is upstream's first-column rule."""
    case = base_case(ip=3, cx=CM.CX, cz=CM.CZ)
    atm = CM.join(CM.columns(case.ctl, case.atm, CM.CLOUD_LATS, seed=5, jitter=False))
    a = CM.Cloud(atm, case.ctl)
    assert a.altitude_range(0, a.np) == T.Atm.altitude_range(a, 0, a.np)
    b = CM.Cloud(CM.cloud_atmosphere(case.ctl, case.atm), case.ctl)
    assert b.altitude_range(0, 364) != T.Atm.altitude_range(b, 0, 364)     # a cloud: the first column is one point


def test_cloud_points_against_the_model():
    case = cloud_case()
    got = lib.cloud_points(case.atm)
    a = CM.Cloud(case.atm, case.ctl)
    assert got.shape == (case.atm.np, 3) and case.atm.np == 364 + 182
    assert same_doubles(got, a.x1)


def test_cloud_points_refusals_and_bindings():
    L = lib.lib()
    assert hasattr(L, "jur_cloud_points") and L.jur_cloud_points.restype is C.c_long
    assert lib.cloud_lds_points() >= 256
    case = cloud_case()
    x1 = np.zeros((case.atm.np, 3))
    assert L.jur_cloud_points(None, x1.ctypes.data_as(C.POINTER(C.c_double))) == -1
    assert L.jur_cloud_points(C.byref(case.atm), None) == -1
    empty = abi.atm_t()
    empty.np = 0
    with pytest.raises(lib.JurassicError, match="jur_cloud_points"):
        lib.cloud_points(empty)


@pytest.mark.parametrize("refrac", [1, 0])
def test_inputs_stay_clear_of_the_threshold(refrac):
    """Every evaluation of the main case -- points, probes; the redone columns repeat a point's evaluation -- has
    wsum >= 1e-3, and no record is NaN."""
    case = cloud_case(refrac=refrac)
    a = CM.Cloud(case.atm, case.ctl)
    recs = [CM.traceray(case.ctl, a, g) for g in case.geom]
    print("IP 3 main case refrac=%d: %d evaluations, smallest wsum %.4g, points per ray %s" % (refrac, a.evals, a.wsum_min, [r["np"] for r in recs]))
    assert a.evals > 100 * len(recs) * (1 + 4 * refrac) / 5 and a.wsum_min >= 1e-3
    for r in recs:
        assert r["np"] >= 2
        for f in ("p", "t", "ds", "q", "k", "u", "tp"):
            assert np.all(np.isfinite(r[f])), f
