"""jur_scene_hydrostatic and jur_scene_ray_slices (host arithmetic, no GPU): the rule that the scene entries' hydrostatic
balance follows -- upstream's hydrostatic_1d_h2o on every slice of a scene by itself.

Against the live reference the partner is upstream's per-profile hydrostatic() (jurassic.c:263-307).  The two are not
the same expression, exactly as in tests/test_reference_cpu.py::test_oracle_hydrostatic_against_live_reference: upstream
divides each of the 20 terms of a layer's mean by R, by T and by the number of points one after the other and forms
exp(log(p) - x), the rule divides by the product of the three and forms p * exp(-x).  Per layer that is up to 20 terms
whose last bit may differ (each a relative 1.1e-16 of a mean whose exponent is below 1: below 1.1e-16 on the factor even
if all fell the same way), one rounding of log(p) (|log p| < 7 between 1e-3 and 1000 hPa: below 8.9e-16 absolute on the
exponent, the same relative on the pressure) and three further roundings of 1.1e-16.  Over the 149 layers of the longest
profile of the scenes (150 levels) a linear worst case is 149 * 1.3e-15 = 2e-13 and the expected random walk
sqrt(149) * 1.3e-15 = 1.6e-14: HYDRO_PTOL = 1e-13, the bound of that test, sits a factor 6 above the walk.  The measured
maximum is printed and recorded in DESIGN.md."""
import ctypes as C
import numpy as np
import pytest
import common
from jurassic_hip import abi, lib, synth

HYDRO_PTOL = 1e-13
HYDZ = (10.0, 0.0, 35.5, 200.0)        # a level hit, the bottom end (no downward loop), between levels, above every level


def rows(atm, k):
    return np.ctypeslib.as_array(getattr(atm, k))[..., :atm.np]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def scene(name, **kw):
    case = common.limb_case(**kw)
    case.atm, case.geom, spec = synth.scene(name, case.ctl, case.atm)
    return case, spec


def place_runs(atm):
    """upstream's profiles: runs of equal (lon, lat)"""
    lon, lat = rows(atm, "lon"), rows(atm, "lat")
    start = np.r_[0, np.flatnonzero((np.diff(lon) != 0) | (np.diff(lat) != 0)) + 1]
    return start, np.diff(np.r_[start, atm.np])


@pytest.fixture(scope="module")
def ref():
    from oracle import ref as r
    if r.available():
        return r
    if r.required():
        pytest.fail("the reference tree is present but oracle/_ref/libjurassic_ref.so is not: make -C oracle ref")
    pytest.skip("neither oracle/_ref/libjurassic_ref.so nor the reference tree (JUR_REFERENCE) is here")


@pytest.mark.parametrize("name", ["ragged", "short_last"])
def test_against_upstreams_hydrostatic_per_profile(ref, name):
    case, spec = scene(name)
    assert case.ctl.ctm_h2o == 1 and "H2O" in common.LIMB_EMITTERS      # both sides read the H2O emitter
    rs = lib.scene_ray_slices(case.ctl, case.atm, case.geom[:, 0])
    start, length = place_runs(case.atm)
    order = np.argsort(rs["sfirst"])
    assert np.array_equal(rs["sfirst"][order], start) and np.array_equal(rs["slen"][order], length)   # upstream's runs are the slices
    assert length.max() == max(s["n"] for s in spec) and (name != "ragged" or length.max() == 150)
    for hydz in HYDZ:
        ctl = abi.ctl_t.from_buffer_copy(bytes(case.ctl))
        ctl.hydz = hydz
        theirs = ref.hydrostatic(ctl, case.atm)
        mine = lib.scene_hydrostatic(case.ctl, hydz, case.atm, rs["sfirst"], rs["slen"])
        for k in ("time", "z", "lon", "lat", "t", "q", "k"):
            assert same_bits(rows(mine, k), rows(case.atm, k)) and same_bits(rows(theirs, k), rows(case.atm, k)), k
        err = float(np.abs(rows(mine, "p") / rows(theirs, "p") - 1).max())
        moved = float(np.abs(rows(theirs, "p") / rows(case.atm, "p") - 1).max())
        print("HYDRO cpu %s hydz = %g: largest relative pressure difference %.3g (the call moves pressures by up to %.3g)"
              % (name, hydz, err, moved))
        assert moved > 1e-4 and err < HYDRO_PTOL


def by_hand(ctl, hydz, atm, first, n, wet):
    """the rule restated with numpy doubles, one operation at a time (jr_common.h:713-761)"""
    z, lat, t, p = (rows(atm, k)[first:first + n].copy() for k in ("z", "lat", "t", "p"))
    q = rows(atm, "q")[common.LIMB_EMITTERS.index("H2O"), first:first + n]
    ipref = int(np.argmin(np.abs(z - hydz)))                           # (argmin: the first of several)
    rad = np.pi / 180.0
    x, y = np.sin(lat[ipref] * rad), np.sin(2 * lat[ipref] * rad)

    def layer(a, b):
        mean = 0.0
        for i in range(20):
            zz = z[a] + (i - 0.0) * (z[b] - z[a]) / 19.0
            grav = 9.780318 * (1. + 0.0053024 * x * x - 5.8e-6 * y * y) - 3.086e-3 * zz
            e = q[a] + (i - 0.0) * (q[b] - q[a]) / 19.0 if wet else 0.0
            temp = t[a] + (i - 0.0) * (t[b] - t[a]) / 19.0
            mean += (e * 18.0153e-3 + (1 - e) * 28.96456e-3) * grav / (8.314472 * temp * 20)
        p[b] = p[a] * np.exp(-1000 * mean * (z[b] - z[a]))
    for ip in range(ipref + 1, n):
        layer(ip - 1, ip)
    for ip in range(ipref - 1, -1, -1):
        layer(ip + 1, ip)
    return ipref, p


def test_descending_profiles_and_the_two_point_slice():
    """ragged holds ascending and descending profiles and one of two points; the restatement agrees to the libm's exp
    and sin (numpy's may differ from it in the last bit: 4 ulp per layer at the most, 149 layers)."""
    case, spec = scene("ragged")
    rs = lib.scene_ray_slices(case.ctl, case.atm, case.geom[:, 0])
    assert 2 in rs["slen"] and any(s.get("descending") for s in spec) and not all(s.get("descending") for s in spec)
    for hydz in HYDZ:
        out = lib.scene_hydrostatic(case.ctl, hydz, case.atm, rs["sfirst"], rs["slen"])
        for f, n in zip(rs["sfirst"], rs["slen"]):
            ipref, want = by_hand(case.ctl, hydz, case.atm, f, n, wet=True)
            got = rows(out, "p")[f:f + n]
            assert got[ipref] == rows(case.atm, "p")[f + ipref]         # the parcel keeps its pressure, bit for bit
            assert np.abs(got / want - 1).max() < 149 * 4 * 2.3e-16
        z = rows(case.atm, "z")
        down = [f for f, n in zip(rs["sfirst"], rs["slen"]) if z[f + 1] < z[f]]
        assert down                                                     # (the parcel of a descending profile: found by value)
    untouched = np.ones(case.atm.np, dtype=bool)
    for f, n in zip(rs["sfirst"], rs["slen"]):
        untouched[f:f + n] = False
    assert same_bits(rows(out, "p")[untouched], rows(case.atm, "p")[untouched])


def test_a_tie_picks_the_lower_index():
    case, _ = scene("short_last")
    z = rows(case.atm, "z")
    z[4:40] += 10.0
    z[0:4] = [8.0, 9.0, 11.0, 12.0]                                     # |z - 10| = 1 at the points 1 and 2, more elsewhere
    assert abs(z[1] - 10.0) == abs(z[2] - 10.0) == np.abs(z[:40] - 10.0).min() and np.all(np.diff(z[:40]) > 0)
    out = lib.scene_hydrostatic(case.ctl, 10.0, case.atm, [0], [40])
    p0, p1 = rows(case.atm, "p")[:40], rows(out, "p")[:40]
    assert p1[1] == p0[1] and p1[2] != p0[2]
    ipref, want = by_hand(case.ctl, 10.0, case.atm, 0, 40, wet=True)
    assert ipref == 1 and np.abs(p1 / want - 1).max() < 39 * 4 * 2.3e-16


def test_both_h2o_settings():
    wet, _ = scene("ragged")
    dry, _ = scene("ragged", ctm_h2o=0)
    assert wet.ctl.ctm_h2o == 1 and dry.ctl.ctm_h2o == 0
    rs = lib.scene_ray_slices(wet.ctl, wet.atm, wet.geom[:, 0])
    a = lib.scene_hydrostatic(wet.ctl, 10.0, wet.atm, rs["sfirst"], rs["slen"])
    b = lib.scene_hydrostatic(dry.ctl, 10.0, dry.atm, rs["sfirst"], rs["slen"])
    assert same_bits(rows(wet.atm, "p"), rows(dry.atm, "p"))
    assert not same_bits(rows(a, "p"), rows(b, "p"))
    f, n = int(rs["sfirst"][0]), int(rs["slen"][0])
    _, want = by_hand(dry.ctl, 10.0, dry.atm, f, n, wet=False)          # e = 0
    assert np.abs(rows(b, "p")[f:f + n] / want - 1).max() < 149 * 4 * 2.3e-16


def test_balancing_twice_gives_the_same_bits():
    case, _ = scene("ragged")
    rs = lib.scene_ray_slices(case.ctl, case.atm, case.geom[:, 0])
    for hydz in HYDZ:
        once = lib.scene_hydrostatic(case.ctl, hydz, case.atm, rs["sfirst"], rs["slen"])
        twice = lib.scene_hydrostatic(case.ctl, hydz, once, rs["sfirst"], rs["slen"])
        assert same_bits(rows(once, "p"), rows(twice, "p"))
        assert not same_bits(rows(once, "p"), rows(case.atm, "p"))
    ip_ = C.POINTER(C.c_int)                                            # in place: out may be in
    sf, sn = rs["sfirst"].astype(np.int32), rs["slen"].astype(np.int32)
    inplace = abi.atm_t.from_buffer_copy(bytes(case.atm))
    assert lib.lib().jur_scene_hydrostatic(C.byref(case.ctl), 200.0, C.byref(inplace), len(sf), sf.ctypes.data_as(ip_),
                                           sn.ctypes.data_as(ip_), C.byref(inplace)) == 0
    assert same_bits(rows(inplace, "p"), rows(once, "p"))


def test_segments_of_fewer_than_two_points_are_left_alone():
    case, _ = scene("ragged")
    out = lib.scene_hydrostatic(case.ctl, 10.0, case.atm, [0, 5, 9, 9], [1, 0, 1, 1])      # (and they may share points)
    assert same_bits(rows(out, "p"), rows(case.atm, "p"))


def test_every_refusal_names_what_is_wrong():
    case, _ = scene("ragged")
    n = case.atm.np
    for bad in (-1.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(lib.JurassicError, match=r"error %d: jur_scene_hydrostatic: hydz is .*negative or not finite" % lib.EINVAL):
            lib.scene_hydrostatic(case.ctl, bad, case.atm, [0], [60])
    for f, l in ((-1, 5), (n - 3, 4), (0, -2)):
        with pytest.raises(lib.JurassicError, match=r"error %d: .*segment 1, \[%d, .*outside the %d points" % (lib.EINVAL, f, n)):
            lib.scene_hydrostatic(case.ctl, 10.0, case.atm, [0, f], [60, l])
    with pytest.raises(lib.JurassicError, match=r"error %d: .*segments 0, \[0, 60\), and 2, \[59, 70\), share point 59" % lib.EINVAL):
        lib.scene_hydrostatic(case.ctl, 10.0, case.atm, [0, 100, 59], [60, 20, 11])
    before = bytes(case.atm)
    with pytest.raises(lib.JurassicError, match=r"share point 10 "):
        lib.scene_hydrostatic(case.ctl, 10.0, case.atm, [10, 10], [2, 2])
    assert bytes(case.atm) == before


@pytest.mark.parametrize("name", ["ragged", "lone_ends", "lone_up", "short_last"])
def test_ray_slices_are_the_slices_with_elements_plus_those_without(name):
    case, _ = scene(name)
    time = case.geom[:, 0]
    none = lib.scene_ray_slices(case.ctl, case.atm, time)               # no retrieval window: every slice has width 0
    assert len(lib.scene_slices(case.ctl, case.atm, time)["sfirst"]) == 0 and len(none["sfirst"]) >= 3
    case.ctl.rett_zmin, case.ctl.rett_zmax = 62.0, 75.0                 # T above 62 km: some profiles end below
    sl = lib.scene_slices(case.ctl, case.atm, time)
    rs = lib.scene_ray_slices(case.ctl, case.atm, time)
    assert np.array_equal(rs["sfirst"], none["sfirst"]) and np.array_equal(rs["slen"], none["slen"])   # (windows play no part)
    with_elements = set(zip(sl["sfirst"].tolist(), sl["slen"].tolist()))
    all_of_them = list(zip(rs["sfirst"].tolist(), rs["slen"].tolist()))
    assert with_elements <= set(all_of_them) and len(set(all_of_them)) == len(all_of_them)
    assert [s for s in all_of_them if s in with_elements] == list(zip(sl["sfirst"].tolist(), sl["slen"].tolist()))   # same order
    lay = lib.scene_layout(case.ctl, case.atm, time)
    for f, l in set(all_of_them) - with_elements:                       # the added ones: traced through, width 0
        hit = (lay["first"] == f) & (lay["len"] == l)
        assert l >= 2 and hit.any() and np.all(np.diff(lay["rowptr"])[hit] == 0)
    if name in ("ragged", "short_last"):
        assert set(all_of_them) - with_elements
    assert set(zip(lay["first"][lay["len"] >= 2].tolist(), lay["len"][lay["len"] >= 2].tolist())) == set(all_of_them)
    owner = np.zeros(case.atm.np, dtype=int)
    for f, l in all_of_them:
        owner[f:f + l] += 1
    assert owner.max() == 1                                             # no named scene has overlapping ray slices
