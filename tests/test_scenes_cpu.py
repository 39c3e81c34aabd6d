"""The oracle on ragged multi-profile scenes across the globe (synth.SCENES): properties it must have by physics or by
definition, without the reference.

  * rotation invariance: the atmosphere is one-dimensional (ctl.ip == 1), so turning every ray and every profile's
    location about any axis leaves radiances, transmittances and LOS point counts unchanged and turns the tangent
    point with them;
  * straight rays (refrac = 0): the tangent point is the line's closest approach to the Earth's centre, and the LOS
    point count follows from the path length and the step rules (rayds, raydz);
  * degenerate slices: a slice without vertical extent is not entered, and a LOS that leaves its
    slice at the first point is that point alone -- no read before los[0]."""
import ctypes as C
import math
import numpy as np
import pytest
import common
import losrecords as L
from jurassic_hip import abi, synth


def scene_case(name, **ctl_kw):
    case = common.limb_case(**ctl_kw)
    atm, geom, spec = synth.scene(name, case.ctl, case.atm)
    case.atm, case.geom = atm, geom
    return case, spec


def rotation(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = math.radians(deg)
    return np.eye(3) + math.sin(t) * k + (1 - math.cos(t)) * k @ k


def rotated(atm, geom, r):
    """Copy of the scene turned by the rotation matrix r: every profile point's location, every observer and view point."""
    a = abi.atm_t()
    C.memmove(C.byref(a), C.byref(atm), C.sizeof(abi.atm_t))
    n = a.np
    lon, lat = np.ctypeslib.as_array(a.lon), np.ctypeslib.as_array(a.lat)
    _, lon[:n], lat[:n] = synth._geo(synth._cart(0.0, lon[:n], lat[:n]) @ r.T)
    g = geom.copy()
    for k in (1, 4):
        g[:, k], g[:, k + 1], g[:, k + 2] = synth._geo(synth._cart(g[:, k], g[:, k + 1], g[:, k + 2]) @ r.T)
    return a, g


ROTATIONS = {"earth_axis_37deg": ([0, 0, 1], 37.3), "oblique_71deg": ([1, 2, -0.5], 71.0)}


@pytest.mark.parametrize("refrac", [0, 1])
@pytest.mark.parametrize("rot", sorted(ROTATIONS))
@pytest.mark.parametrize("name", ["ragged", "unsorted", "lone_ends"])
def test_rotation_invariance(oracle, name, rot, refrac):
    """Bounds, with what set them (all three scenes, both rotations):
      refrac = 0: measured 3.7e-11 relative on radiances, tangent points 3.4e-9 km apart.  The rotated inputs are the
        turned scene only to rounding (~1e-16 relative in the coordinates); rays that end on the ground at a shallow
        angle, where the exit clipping divides by a small altitude difference, amplify that most.  So 1e-10, not the
        1e-12 of a well-conditioned ray (the limb rays from orbit stay within 6e-12).
      refrac = 1: measured 2.0e-5 relative on radiances, tangent points 0.114 km apart.  The refractivity gradient
        is a forward difference along the Cartesian AXES with h = 0.02 km (jr_common.h:665-681): turned, it probes
        other points and carries a different truncation error of the second derivative of the refractivity.
    No ray's LOS point count changes with either rotation (a flip of a discrete decision -- entry bisection, step
    rule, exit -- would show there first); rays that never enter give 0 points and their view point as tangent point."""
    case, _ = scene_case(name, refrac=refrac)
    tb = case.oracle_tables(oracle)
    ref = oracle.formod_rays(case.ctl, case.atm, tb, case.geom)
    r = rotation(*ROTATIONS[rot])
    atm2, g2 = rotated(case.atm, case.geom, r)
    out = oracle.formod_rays(case.ctl, atm2, tb, g2)
    assert np.array_equal(out["np"], ref["np"])
    assert (ref["np"] > 0).sum() >= 25
    rtol, dmax = (1e-10, 1e-8) if refrac == 0 else (5e-5, 0.25)
    fin = np.isfinite(ref["rad"])
    assert np.array_equal(fin, np.isfinite(out["rad"]))
    assert common.rel_err(out["rad"][fin], ref["rad"][fin]).max() < rtol
    tau_atol = 1e-11 if refrac == 0 else 5e-5      # measured 3.5e-12 and 1.8e-5 absolute
    assert np.abs(out["tau"] - ref["tau"]).max() <= tau_atol
    d = np.linalg.norm(synth._cart(*ref["tp"].T) @ r.T - synth._cart(*out["tp"].T), axis=1)
    assert d.max() < dmax


def test_straight_limb_rays_tangent_point_and_point_count(oracle):
    """refrac = 0, limb rays of the ragged scene whose closest approach lies inside their profile's range: the tangent
    point is the closest approach of the straight line x_obs + s e, altitude |x_obs x e| - RE.  The reference finds it
    as the vertex of the parabola through the three lowest LOS points (jr_common.h:502-539): measured 9.1e-10 km in
    altitude and 3.1e-6 km in position on these 46 rays (near its vertex the altitude along a straight line is a
    parabola to third order in the distance), bounded by 2e-9 km and 1e-5 km.
    The LOS point count: every step is min(rayds, raydz / |cos a|) long (a: zenith angle) and a straight line through
    the shell between the tangent altitude zt and the top zmax is L = 2 sqrt((RE + zmax)^2 - (RE + zt)^2) long, so
    L / rayds <= np - 1 and np - 1 <= L / rayds + 2 (zmax - zt) / raydz + 2 (raydz-limited steps climb raydz each)."""
    case, spec = scene_case("ragged", refrac=0)
    live = [s for s in spec if s["n"] > 1]
    g = case.geom[:len(live) * 30]
    kind = (np.arange(len(g)) // len(live)) % 6
    prof = np.arange(len(g)) % len(live)
    zlo = np.array([min(s["z0"], s["z1"]) for s in live])[prof]
    zhi = np.array([max(s["z0"], s["z1"]) for s in live])[prof]
    xo = synth._cart(g[:, 1], g[:, 2], g[:, 3])
    e = synth._cart(g[:, 4], g[:, 5], g[:, 6]) - xo
    e /= np.linalg.norm(e, axis=1)[:, None]
    zt = np.linalg.norm(np.cross(xo, e), axis=1) - synth.RE
    use = (kind <= 1) & (zt > zlo + 0.5) & (zt < zhi - 0.5)
    assert use.sum() >= 20
    ref = oracle.formod_rays(case.ctl, case.atm, case.oracle_tables(oracle), g[use])
    xt = xo[use] - (xo[use] * e[use]).sum(axis=1)[:, None] * e[use]
    assert np.abs(ref["tp"][:, 0] - zt[use]).max() < 2e-9
    assert np.linalg.norm(synth._cart(*ref["tp"].T) - xt, axis=1).max() < 1e-5
    L = 2 * np.sqrt((synth.RE + zhi[use]) ** 2 - (synth.RE + zt[use]) ** 2)
    steps = ref["np"] - 1
    assert np.all(steps >= np.floor(L / case.ctl.rayds))
    assert np.all(steps <= L / case.ctl.rayds + 2 * (zhi[use] - zt[use]) / case.ctl.raydz + 2)


def test_degenerate_slices_are_not_entered(oracle):
    """Ray time stamps below the first profile, between profiles and above the last, and the time stamps of the
    one-point profiles at both ends of lone_ends (0.0 and 5.0): locate_atm gives each a slice of one point
    (zmin == zmax), which is not entered -- 0 LOS points, the view point as tangent point, nothing emitted -- where the
    reference would step out at the first point and read los[-1].  The rays of the other profiles are traced."""
    case, spec = scene_case("lone_ends")
    t = case.geom[:, 0]
    degenerate = np.isin(t, [-2.0, 0.0, 0.5, 3.0, 4.5, 5.0, 9.0])
    assert np.isin([0.0, 5.0], t).all() and degenerate.sum() >= 42
    ref = oracle.formod_rays(case.ctl, case.atm, case.oracle_tables(oracle), case.geom)
    assert np.all(ref["np"][degenerate] == 0)
    assert np.array_equal(ref["tp"][degenerate], case.geom[degenerate][:, 4:7])
    assert np.all(ref["rad"][degenerate] == 0) and np.all(ref["tau"][degenerate] == 1)
    assert (ref["np"][~degenerate] > 1).sum() >= 150


def test_one_point_end_profiles_join_the_next_slice(oracle):
    """lone_up: locate_atm hands the rays of the profile after a one-point first profile, and of the profile before a
    one-point last profile, a slice that includes that point (jr_common.h:127-154).  Both lie at that profile's
    place, so they widen its altitude range: the 0-60 km profile's rays from orbit enter at 75 km (the foreign point),
    and rays of the 0-70 km profile that reach the ground are clipped at -1 km.  short_last: a ray time stamp between
    the profiles before a two-level last profile and it (1.5) is traced through that last profile."""
    case, spec = scene_case("lone_up")
    t = case.geom[:, 0]
    for i in np.nonzero((t == 4.0) & (case.geom[:, 1] > 700))[0][:8]:
        tr = oracle.traceray(case.ctl, case.atm, case.geom[i])
        if tr["np"] > 0:
            assert 75.0 - 0.001 < tr["z"][0] <= 75.0
    low = [oracle.traceray(case.ctl, case.atm, g) for g in case.geom[t == 1.0]]
    ground = [tr for tr in low if tr["tsurf"] != -999]
    assert len(ground) >= 3 and all(abs(tr["z"][-1] + 1.0) < 1e-4 for tr in ground)   # (clipped through a geo round trip)
    case, spec = scene_case("short_last")
    ref = oracle.formod_rays(case.ctl, case.atm, case.oracle_tables(oracle), case.geom)
    t = case.geom[:, 0]
    assert np.all(ref["np"][np.isin(t, [0.5, 3.0])] == 0) and (ref["np"][t == 1.5] > 1).sum() >= 3


def test_leaving_the_slice_at_the_first_point(oracle):
    """A slice 1 cm thick, seen from above: the entry bisection stops within 1 m below its top, which is below its
    bottom.  The LOS is that one point with ds = 0 (no segment before it to cut), the surface below it -- defined, and
    the same on every call, where the reference reads los[-1]."""
    case = common.limb_case()
    spec = [dict(time=0.0, lon=0.0, lat=0.0, n=2, z0=10.0, z1=10.00001), dict(time=1.0, lon=0.0, lat=0.0, n=30, z0=0.0, z1=60.0)]
    atm = synth.ragged_atmosphere(case.ctl, spec, base=case.atm)
    geom = np.array([[0.0, 700.0, 0.0, 0.0, 0.0, 0.0, 0.5], [0.0, 700.0, 0.0, 0.0, 9.9, 0.0, 0.0]])
    for g in geom:
        tr = oracle.traceray(case.ctl, atm, g)
        assert tr["np"] == 1 and tr["ds"][0] == 0.0 and 10.00001 - 0.001 < tr["z"][0] < 10.0
        assert tr["tsurf"] == tr["t"][0]
    a = oracle.formod_rays(case.ctl, atm, case.oracle_tables(oracle), geom)
    b = oracle.formod_rays(case.ctl, atm, case.oracle_tables(oracle), geom)
    assert np.array_equal(a["rad"], b["rad"]) and np.all(a["np"] == 1) and np.all(np.isfinite(a["rad"]))


@pytest.mark.parametrize("name", list(L.CONFIGS))
def test_los_record_yardstick_and_short_paths(oracle, tmp_path, name):
    """CPU twin of tests/test_kat_gpu.py::test_los_records_against_the_oracle: the configurations and the yardstick the
    device's LOS records are held to (tests/losrecords.py), proven without a GPU.  No ray needs NLOS points (the oracle
    would end the process); at most 2 % of the rays change their point count under a one-ulp nudge of the geometry; every
    Y_f is a few 1e-11 at most (FACTOR * Y_f is then below the 1e-9 cap for p, T, k, q and reaches it for ds and u of
    the longest limb paths); the extinction the tracer interpolates varies along the paths; and the short paths have the point counts they are
    there for."""
    case = L.CONFIGS[name](str(tmp_path))
    base, use, Y = L.yardstick(oracle, case)
    nps = np.array([tr["np"] for tr in base])
    tsurf = np.array([tr["tsurf"] for tr in base])
    print("LOS %s: %d rays, %d traced, %d left out, np <= %d, Y_f %s"
          % (name, len(nps), (nps > 0).sum(), (~use).sum(), nps.max(), " ".join("%s %.2e" % (f, Y[f]) for f in L.FIELDS)))
    assert 100 <= len(nps) <= 230 and (nps > 0).sum() >= 25 and nps.max() < abi.NLOS - 1
    assert (~use).sum() <= 0.02 * len(use)
    assert (tsurf != -999).any() and (tsurf == -999).any()
    for f in L.FIELDS:
        present = f not in ("q", "u") or (case.ctl.ng > 0 and (f == "u" or L.h2o_index(case.ctl) >= 0))
        assert (0 < Y[f] < 1e-10) if present else Y[f] == 0.0, (f, Y[f])
        assert 64 * 2.0 ** -52 <= L.bound(Y[f]) <= L.CAP
    long_ray = base[int(np.argmax(nps))]
    assert long_ray["k"].min() > 0 and long_ray["k"].max() > 20 * long_ray["k"].min()      # the profile of common.extinction_profile
    if name == "thin_slice":
        assert list(nps[:2]) == [1, 1] and all(tr["ds"][0] == 0.0 for tr in base[:2])
    elif name not in ("ragged", "unsorted", "lone_up"):
        short = base[-len(L.SHORT_PATHS):]
        want = [2, 2, 2, 2] if name == "coarse_steps" else L.SHORT_NP                       # (one step of 1 km leaves the top)
        assert [tr["np"] for tr in short] == want
        assert short[2]["tsurf"] != -999 and short[3]["tsurf"] != -999 and not np.any(short[3]["ds"])
        assert short[0]["tsurf"] == -999 and short[1]["tsurf"] == -999
