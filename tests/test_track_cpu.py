"""2-D atmosphere along the line of sight (IP 2), the part that needs no GPU.

  * tests/track_model.py's restatement of intpol_atm_2d equals the oracle's orc_intpol_atm under ip = 2 bit for bit;
  * its restatement of traceray, with the 1-D point rule, equals the oracle's traceray on the test's rays: point
    counts and records bit for bit -- the interpreter's math functions are the C library's the oracle is linked to;
  * jur_track_profiles, the host function behind every upload under ip = 2: counts, firsts, lengths and x1 against the
    model, the two refusals, two time blocks, a profile that comes back to an earlier position;
  * how many rays of the fixed ray set the yardstick of the GPU test's LOS-record comparison leaves out.
"""
import ctypes as C
import numpy as np
import pytest
import common
import track_model as T
from jurassic_hip import abi, lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_doubles(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a)[~np.isnan(a)], bits(b)[~np.isnan(b)])


def base_case(**kw):
    kw.setdefault("rayds", 10.0)
    kw.setdefault("raydz", 1.0)
    case = common.limb_case(geom=T.track_rays(), table_kw=dict(nlev=2, ntemp=2), **kw)
    common.extinction_profile(case.atm)
    return case


def points_atm(z, lon, lat):
    d = abi.atm_t()
    d.np = len(z)
    for f, v in (("z", z), ("lon", lon), ("lat", lat)):
        np.ctypeslib.as_array(getattr(d, f))[:len(z)] = v
    return d


def test_2d_restatement_equals_the_oracle(oracle):
    """About 2 000 points against orc.intpol_atm under ip = 2 on the graded track (one profile with fewer levels):
    random ones, points exactly over a profile, exactly midway between two, beyond both ends of the track, on level
    altitudes, below and above every profile."""
    case = base_case(ip=2)
    src = T.track_atmosphere(case.ctl, case.atm, second_block=False)      # upstream's ip 2 knows one block
    rng = np.random.default_rng(11)
    levels = np.ctypeslib.as_array(src.z)[:91]
    z = np.concatenate([rng.uniform(-2.0, 95.0, 1400), rng.choice(levels, 300), rng.uniform(0.0, 90.0, 300)])
    special = [-3.0, -1.0, 1.0, 3.0, -2.0, 0.0, 2.0, -4.0, -9.5, 3.5, 9.0, 12.9, -12.9, np.nextafter(0.0, 1), np.nextafter(-2.0, 0)]
    lat = np.concatenate([rng.uniform(-9.0, 9.0, 1400), rng.uniform(-5.0, 5.0, 300), rng.choice(special, 300)])
    lon = np.concatenate([rng.uniform(-2.0, 2.0, 1700), np.zeros(300)])
    dest = points_atm(z, lon, lat)
    assert oracle.intpol_atm(case.ctl, dest, src) == 0
    a = T.Atm(src, case.ctl)
    n = len(z)
    got = [T.interp_2d(a, 0, a.np, float(z[i]), float(lon[i]), float(lat[i])) for i in range(n)]
    assert same_doubles([g[0] for g in got], np.ctypeslib.as_array(dest.p)[:n])
    assert same_doubles([g[1] for g in got], np.ctypeslib.as_array(dest.t)[:n])
    for ig in range(case.ctl.ng):
        assert same_doubles([g[2][ig] for g in got], np.ctypeslib.as_array(dest.q)[ig, :n]), ig
    assert same_doubles([g[3][0] for g in got], np.ctypeslib.as_array(dest.k)[0, :n])
    r = np.array([T.weights(a.profiles(0, a.np), float(lon[i]), float(lat[i]))[2] for i in range(n)])
    assert (r == 0).any() and (r == 1).sum() == 0 and ((r > 0.4) & (r <= 0.5)).any(), "the points do not cover the rule's branches"


@pytest.mark.parametrize("refrac", [1, 0])
def test_python_tracer_1d_rule_equals_the_oracle(oracle, refrac):
    """One-profile atmosphere, the fixed rays: equal point counts, records bit for bit (no libm difference shows: the
    interpreter and the oracle call the same C library)."""
    case = base_case(refrac=refrac)
    a = T.Atm(case.atm, case.ctl)
    geom = case.geom.copy()
    geom[:, 0] = 0.0
    entered = 0
    for g in geom:
        ref = oracle.traceray(case.ctl, case.atm, g)
        got = T.traceray(case.ctl, a, g, two_d=False)
        assert got["np"] == ref["np"], g
        entered += ref["np"] > 0
        for f in ("z", "lon", "lat", "p", "t", "ds"):
            assert same_doubles(got[f], ref[f]), (f, g)
        assert same_doubles(got["k"][0], ref["k"]) and same_doubles(got["q"], ref["q"]) and same_doubles(got["u"], ref["u"]), g
        assert same_doubles([got["tsurf"]], [ref["tsurf"]]) and same_doubles(got["tp"], ref["tp"]), g
    assert entered == len(geom)


def model_table(atm, ctl):
    return T.profile_table(T.Atm(atm, ctl))


def test_track_profiles_against_the_model():
    case = base_case(ip=2)
    atm = T.track_atmosphere(case.ctl, case.atm)            # two time blocks: 4 profiles and 1
    got = lib.track_profiles(atm)
    first, length, x1, block_of = model_table(atm, case.ctl)
    assert len(got["first"]) == 5 and got["block_of"].tolist() == [0, 0, 0, 0, 1] == block_of
    assert got["first"].tolist() == first and got["len"].tolist() == length
    assert got["len"].tolist() == [91, 91, 76, 91, 91]
    assert same_doubles(got["x1"], x1)


def test_track_profiles_refusals():
    case = base_case(ip=2)
    atm = T.track_atmosphere(case.ctl, case.atm)
    lone = T.track_atmosphere(case.ctl, case.atm)
    np.ctypeslib.as_array(lone.lat)[91] = -1.5              # the first level of profile 1 becomes a profile of its own
    with pytest.raises(lib.JurassicError, match="Cannot identify profiles"):
        lib.track_profiles(lone)
    far = T.track_atmosphere(case.ctl, case.atm, lats=(-3.0, -1.0, 9.5, 12.0))
    with pytest.raises(lib.JurassicError, match="Distance of profiles is too large"):
        lib.track_profiles(far)
    # more than 10 degrees between the LAST profile of one block and the first of the next is no refusal
    np.ctypeslib.as_array(atm.lat)[atm.np - 91:atm.np] = 40.0
    assert len(lib.track_profiles(atm)["first"]) == 5
    with pytest.raises(ValueError, match="Cannot identify profiles"):
        model_table(lone, case.ctl)
    with pytest.raises(ValueError, match="Distance of profiles is too large"):
        model_table(far, case.ctl)


def test_track_profiles_returning_profile_is_a_new_run():
    """A track that comes back to an earlier position lists that position twice: runs, not places."""
    case = base_case(ip=2)
    atm = T.track_atmosphere(case.ctl, case.atm, lats=(-1.0, 1.0, -1.0), thinned=None, second_block=False)
    got = lib.track_profiles(atm)
    assert got["first"].tolist() == [0, 91, 182] and got["len"].tolist() == [91, 91, 91] and got["block_of"].tolist() == [0, 0, 0]
    assert same_doubles(got["x1"][0], got["x1"][2]) and not same_doubles(got["x1"][0], got["x1"][1])
    first, length, x1, _ = model_table(atm, case.ctl)
    assert got["first"].tolist() == first and same_doubles(got["x1"], x1)


def test_track_symbol_and_binding():
    L = lib.lib()
    assert hasattr(L, "jur_track_profiles") and L.jur_track_profiles.restype is C.c_long


def nudged_out(ctl, a, geom):
    """Rays of geom whose point count changes when the geometry moves one ulp up or down (tests/losrecords.py)."""
    from losrecords import _nudged
    out = []
    for i, g in enumerate(geom):
        n0 = T.traceray(ctl, a, g, two_d=True)["np"]
        if any(T.traceray(ctl, a, _nudged(g, s), two_d=True)["np"] != n0 for s in (+1, -1)):
            out.append(i)
    return out


@pytest.mark.parametrize("refrac", [1, 0])
def test_nudge_leaves_out_at_most_one_ray_in_eight(refrac):
    case = base_case(ip=2, refrac=refrac)
    atm = T.track_atmosphere(case.ctl, case.atm)
    out = nudged_out(case.ctl, T.Atm(atm, case.ctl), case.geom)
    print("rays left out by the nudge:", out)
    assert 8 * len(out) <= len(case.geom), out
