"""Seeded synthetic inputs: emissivity tables, filter functions, observation
geometries and stacked atmosphere profiles.

The geometry formulas restate the reference's generators: limb tangent-height
scan src/limb.c:49-59, nadir latitude sweep src/nadir.c:51-58; the profile
perturbation follows src/climatology.c:65-78 (p*(1+dp), T+dT per profile).
"""
import numpy as np
from . import abi

RE = 6367.421

# absorption strength per molecule/cm^2 at 1000 hPa, 250 K, by emitter
K0 = {"CO2": 5e-23, "H2O": 2e-22, "O3": 5e-21, "F11": 1e-17, "CCL4": 2e-17}


def table_rows(emitter, nu, id_=0, nlev=33, ntemp=10, descending=False, umax_eps=0.99999, ratio=1.122, dup_every=0):
    """Rows (p, T, u, eps) of one synthetic table in file order.

    p: nlev levels 0.016..1000 hPa (log-spaced, ascending unless `descending`);
    T: ntemp values per level, 15 K apart, the axis shifted by 2 K*(level%3) so
       neighbouring levels do not share their temperature brackets;
    u: geometric grid with the given ratio from eps~1e-6 to eps>umax_eps;
    eps = 1 - exp(-(k u)^0.7), k = k0 sqrt(p/1000) 250/T (1+0.3 id_) (nu/800)^2;
    dup_every = k > 0: after every k-th row a row 1e-10 (relative) above it -- larger as a double, so the
       loader keeps it, equal once stored as fp32: curves that are sorted but not strictly increasing."""
    k0 = K0.get(emitter.upper(), 1e-21) * (1 + 0.3 * id_) * (nu / 800.0) ** 2
    plev = np.exp(np.linspace(np.log(0.016), np.log(1000.0), nlev))
    if descending:
        plev = plev[::-1]
    nmax = 2 + int(np.ceil(np.log(1e12) / np.log(ratio))) if ratio > 1 else 400
    steps = np.full(nmax, ratio)
    blocks = []
    for il, p in enumerate(plev):
        for t in 180.0 + 2.0 * (il % 3) + 15.0 * np.arange(ntemp):
            k = k0 * np.sqrt(p / 1000.0) * 250.0 / t
            steps[0] = (1e-6 ** (1 / 0.7)) / k
            u = np.cumprod(steps)                      # u0, u0*r, (u0*r)*r, ... left to right
            eps = 1.0 - np.exp(-(k * u) ** 0.7)
            hit = np.nonzero(eps > umax_eps)[0]
            n = (hit[0] + 1) if len(hit) else nmax     # the row that crosses the limit is the last one
            blk = np.empty((n, 4))
            blk[:, 0] = p
            blk[:, 1] = t
            blk[:, 2] = u[:n]
            blk[:, 3] = eps[:n]
            if dup_every > 0:
                twin = blk[dup_every - 1::dup_every].copy()
                twin[:, 2:] *= 1.0 + 1e-10
                blk = np.insert(blk, np.arange(dup_every, n + 1, dup_every)[:len(twin)], twin, axis=0)
            blocks.append(blk)
    return np.vstack(blocks)


def write_table_file(path, rows):
    with open(path, "w") as fh:
        fh.write("# $1 = pressure [hPa]\n# $2 = temperature [K]\n"
                 "# $3 = column density [molecules/cm^2]\n# $4 = emissivity\n\n")
        for p, t, u, e in rows:
            fh.write("%.9g %.9g %.9g %.9g\n" % (p, t, u, e))


def parse_table_file(path):
    out = []
    with open(path) as fh:
        for line in fh:
            tok = line.split()
            if len(tok) >= 4:
                try:
                    out.append([float(x) for x in tok[:4]])
                except ValueError:
                    pass
    return np.array(out)


def boxcar_filter(nu, halfwidth=0.5, n=21):
    x = np.linspace(nu - halfwidth, nu + halfwidth, n)
    f = np.ones(n)
    f[0] = f[-1] = 0.0
    return x, f


def write_filter_file(path, x, f):
    with open(path, "w") as fh:
        fh.write("# $1 = wavenumber [cm^-1]\n# $2 = filter function\n\n")
        for a, b in zip(x, f):
            fh.write("%.4f %g\n" % (a, b))


def limb_geometry(nr, seed=0, obsz=780.0, zmin=3.0, zmax=68.0, nprofiles=1, scan=False):
    """(nr, 7) limb rays.  scan=True gives the reference's regular tangent-height
    scan (limb.c), else vpz ~ U[zmin, zmax]."""
    rng = np.random.default_rng(seed)
    vpz = np.linspace(zmin, zmax, nr) if scan else rng.uniform(zmin, zmax, nr)
    g = np.zeros((nr, 7))
    g[:, 0] = np.arange(nr) % nprofiles
    g[:, 1] = obsz
    g[:, 4] = vpz
    g[:, 6] = 180.0 / np.pi * np.arccos((RE + vpz) / (RE + obsz))
    return g


def nadir_geometry(nr, seed=0, obsz=700.0, lat0=-8.01, lat1=8.01, nprofiles=1):
    rng = np.random.default_rng(seed)
    g = np.zeros((nr, 7))
    g[:, 0] = np.arange(nr) % nprofiles
    g[:, 1] = obsz
    g[:, 6] = rng.uniform(lat0, lat1, nr)
    return g


# ---- index-addressable geometry ("splitmix64 seed 0x4A55524153534943") -----------------------------
# Ray i of a workload is a function of (seed, i) alone: output i of the splitmix64 stream started at `seed`, whose
# state after i + 1 steps is seed + (i + 1) * golden -- no sequential generator state.  A rank of a sharded run builds
# exactly its rows [lo, hi), rank 0 builds the handful of sampled global rows it re-computes, nobody builds the whole set.
SURVEY_SEED = 0x4A55524153534943
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def splitmix64_uniform(seed, idx):
    """U[0, 1) doubles number idx (array of non-negative ints) of the splitmix64 stream with the given seed."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.asarray(idx, dtype=np.uint64) + np.uint64(1)) * _GOLDEN
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def limb_rays(idx, seed=SURVEY_SEED, obsz=780.0, zmin=3.0, zmax=68.0, nprofiles=1):
    """(len(idx), 7) limb rays number idx of the workload: view-point altitude ~ U[zmin, zmax] from obsz km, looking
    at the tangent point (limb.c:49-59), profile idx mod nprofiles."""
    idx = np.asarray(idx, dtype=np.int64)
    vpz = zmin + (zmax - zmin) * splitmix64_uniform(seed, idx)
    g = np.zeros((len(idx), 7))
    g[:, 0] = idx % nprofiles
    g[:, 1] = obsz
    g[:, 4] = vpz
    g[:, 6] = 180.0 / np.pi * np.arccos((RE + vpz) / (RE + obsz))
    return g


def nadir_rays(idx, seed=SURVEY_SEED, obsz=700.0, lat0=-8.01, lat1=8.01, nprofiles=1):
    """(len(idx), 7) nadir observations number idx: sub-satellite latitude ~ U[lat0, lat1] (nadir.c:51-58)."""
    idx = np.asarray(idx, dtype=np.int64)
    g = np.zeros((len(idx), 7))
    g[:, 0] = idx % nprofiles
    g[:, 1] = obsz
    g[:, 6] = lat0 + (lat1 - lat0) * splitmix64_uniform(seed, idx)
    return g


def stack_profiles(atm, ctl, nprofiles, seed=0, dp=0.05, dt=30.0):
    """Atmosphere holding `nprofiles` perturbed copies of the first profile of
    `atm`, time stamps 0..nprofiles-1 (profile 0 unperturbed)."""
    rng = np.random.default_rng(seed)
    n = atm.np
    assert n * nprofiles <= abi.NP
    out = abi.atm_t()
    out.np = n * nprofiles
    fields = ("z", "lon", "lat", "p", "t")
    src = {f: np.ctypeslib.as_array(getattr(atm, f))[:n].copy() for f in fields}
    q = np.ctypeslib.as_array(atm.q)[:, :n].copy()
    k = np.ctypeslib.as_array(atm.k)[:, :n].copy()
    for i in range(nprofiles):
        s = slice(i * n, (i + 1) * n)
        fp = 1.0 + (rng.uniform(-dp, dp) if i else 0.0)
        ft = rng.uniform(-dt, dt) if i else 0.0
        np.ctypeslib.as_array(out.time)[s] = float(i)
        for f in ("z", "lon", "lat"):
            np.ctypeslib.as_array(getattr(out, f))[s] = src[f]
        np.ctypeslib.as_array(out.p)[s] = src["p"] * fp
        np.ctypeslib.as_array(out.t)[s] = src["t"] + ft
        np.ctypeslib.as_array(out.q)[:, s] = q
        np.ctypeslib.as_array(out.k)[:, s] = k
    return out


# ---- ragged multi-profile scenes across the globe ----------------------------------------------------------------
# The atmospheres above are copies of one profile on one z grid at one place.  These put profiles of their own length,
# vertical range, order and location side by side, and rays at every profile in any azimuth, so that the slice a ray
# is traced through (locate_atm / altitude_range_nn, jr_common.h:127-154, 411-420) is a different one per ray.

def _cart(alt, lon, lat):
    r, lo, la = RE + np.asarray(alt, dtype=np.float64), np.radians(lon), np.radians(lat)
    return np.stack([r * np.cos(la) * np.cos(lo), r * np.cos(la) * np.sin(lo), r * np.sin(la)], axis=-1)


def _geo(x):
    """(alt, lon, lat) of Cartesian points, as cart2geo forms them."""
    x = np.asarray(x, dtype=np.float64)
    r = np.sqrt((x * x).sum(axis=-1))
    return r - RE, np.degrees(np.arctan2(x[..., 1], x[..., 0])), np.degrees(np.arcsin(x[..., 2] / r))


def ragged_atmosphere(ctl, spec, seed=0, base=None, order=None):
    """atm_t holding one profile per entry of `spec`, each regridded from the first profile of `base` (an atm_t) and
    perturbed (p * (1 + U(-5 %, 5 %)), T + U(-10, 10) K per profile, then 1 % / 1 K per level).  An entry is a dict:

      time        time stamp (any double)                lon, lat   location [deg]
      n           number of levels (1 ... )              z0, z1     bottom and top altitude [km]
      descending  written top-down (default False)       p0_top     pressure 0 at the top level
      q_nonpos    list of (emitter, level, value): q <= 0 there, as retrieval iterates carry them
      move_at     level from which on the location is lon + 0.5, lat - 0.25 (altitude_range_nn stops there)

    order: permutation of the profiles in the array (default: as given)."""
    assert base is not None, "ragged_atmosphere needs a base profile"
    rng = np.random.default_rng(seed)
    nb = base.np
    bz = np.ctypeslib.as_array(base.z)[:nb]
    srt = np.argsort(bz)
    bz = bz[srt]
    blnp = np.log(np.ctypeslib.as_array(base.p)[:nb][srt])
    bt = np.ctypeslib.as_array(base.t)[:nb][srt]
    bq = np.ctypeslib.as_array(base.q)[:, :nb][:, srt]
    bk = np.ctypeslib.as_array(base.k)[:, :nb][:, srt]
    blocks = []
    for s in spec:
        n = int(s["n"])
        z = np.linspace(s["z0"], s["z1"], n) if n > 1 else np.array([float(s["z0"])])
        fp, ft = 1.0 + rng.uniform(-0.05, 0.05), rng.uniform(-10.0, 10.0)
        p = np.exp(np.interp(z, bz, blnp)) * fp * (1.0 + rng.uniform(-0.01, 0.01, n))
        t = np.interp(z, bz, bt) + ft + rng.uniform(-1.0, 1.0, n)
        q = np.array([np.interp(z, bz, bq[g]) for g in range(ctl.ng)]).reshape(ctl.ng, n)
        q *= 1.0 + rng.uniform(-0.05, 0.05, (ctl.ng, 1))
        k = np.array([np.interp(z, bz, bk[w]) for w in range(ctl.nw)]).reshape(ctl.nw, n)
        if s.get("p0_top"):
            p[np.argmax(z)] = 0.0
        for g, lev, val in s.get("q_nonpos", ()):
            q[g, lev] = val
        lon = np.full(n, float(s["lon"]))
        lat = np.full(n, float(s["lat"]))
        if s.get("descending"):
            z, p, t, q, k = z[::-1], p[::-1], t[::-1], q[:, ::-1], k[:, ::-1]
        if s.get("move_at") is not None:
            lon[s["move_at"]:] += 0.5
            lat[s["move_at"]:] -= 0.25
        blocks.append((np.full(n, float(s["time"])), z, lon, lat, p, t, q, k))
    order = range(len(spec)) if order is None else order
    cols = [np.concatenate([blocks[i][f] for i in order], axis=-1) for f in range(8)]
    n = cols[0].shape[-1]
    assert 2 <= n <= abi.NP
    out = abi.atm_t()
    out.np = n
    for f, name in enumerate(("time", "z", "lon", "lat", "p", "t")):
        np.ctypeslib.as_array(getattr(out, name))[:n] = cols[f]
    np.ctypeslib.as_array(out.q)[:ctl.ng, :n] = cols[6]
    np.ctypeslib.as_array(out.k)[:ctl.nw, :n] = cols[7]
    return out


def global_geometry(profiles, n, seed=0, obsz=750.0):
    """(n, 7) rays, ray i at profile i mod len(profiles) (its location and time stamp), kind i // len(profiles) mod 6:

      0, 1  limb in a random azimuth, tangent point within 2 deg of the profile, tangent height U(z0 - 5, z1 + 5) km
            (below ground to above the top); the view point is the tangent point
      2     nadir: view point straight below the observer, on the ground
      3     off-nadir: view point on the ground 1 - 15 deg away in a random azimuth
      4, 5  observer inside the profile's range looking up (4) or down (5) at 20 - 80 deg elevation

    Profiles at a pole or at lon +-180 put rays over the pole and across the dateline."""
    rng = np.random.default_rng(seed)
    g = np.zeros((n, 7))
    npro = len(profiles)
    for i in range(n):
        s = profiles[i % npro]
        kind = (i // npro) % 6
        zlo, zhi = min(s["z0"], s["z1"]), max(s["z0"], s["z1"])
        up = _cart(0.0, s["lon"], s["lat"])
        up /= np.linalg.norm(up)
        # a horizontal unit vector in a random azimuth (well defined at the poles too)
        a = rng.normal(size=3)
        a -= up * (a @ up)
        h = a / np.linalg.norm(a)
        if kind in (0, 1):
            off = rng.uniform(0.0, 2.0)
            b = rng.normal(size=3)
            b -= up * (b @ up)
            b /= np.linalg.norm(b)
            ut = np.cos(np.radians(off)) * up + np.sin(np.radians(off)) * b
            ht = h - ut * (h @ ut)
            ht /= np.linalg.norm(ht)
            zt = rng.uniform(zlo - 5.0, zhi + 5.0)
            xt = (RE + zt) * ut
            xo = xt - np.sqrt((RE + obsz) ** 2 - (RE + zt) ** 2) * ht
            obs, vp = _geo(xo), _geo(xt)
        elif kind == 2:
            obs, vp = (obsz, s["lon"], s["lat"]), (0.0, s["lon"], s["lat"])
        elif kind == 3:
            ang = np.radians(rng.uniform(1.0, 15.0))
            xv = RE * (np.cos(ang) * up + np.sin(ang) * h)
            obs, vp = (obsz, s["lon"], s["lat"]), _geo(xv)
        else:
            zo = rng.uniform(zlo + 0.2 * (zhi - zlo), zhi - 0.2 * (zhi - zlo))
            el = np.radians(rng.uniform(20.0, 80.0))
            xo = (RE + zo) * up
            d = np.cos(el) * h + np.sin(el) * (up if kind == 4 else -up)
            # view point half way to the top (bottom) along the ray: inside the atmosphere, below its top
            obs, vp = (zo, s["lon"], s["lat"]), _geo(xo + 0.5 * ((zhi - zo) if kind == 4 else (zo - zlo)) / np.sin(el) * d)
        g[i] = (s["time"],) + tuple(float(x) for x in obs) + tuple(float(x) for x in vp)
    return g


def _spec(time, lon, lat, n, z0, z1, **kw):
    return dict(time=time, lon=lon, lat=lat, n=n, z0=z0, z1=z1, **kw)


# Named scenes: name -> (profile specs in array order, extra ray time stamps that match no profile, order).
#   ragged    five profiles of 2 ... 150 levels, own ranges and places (a pole, lon -180, the dateline's other side),
#             ascending and descending, non-integer sorted time stamps
#   unsorted  the same kind of profiles stored out of time order (atm_sorted = 0), with p = 0 at a top level, q <= 0
#             at some levels and a location change part-way through a profile
#   lone_ends a first and a last profile of one point: locate_atm gives the slice after the first one point and the
#             slice before the last one point the foreign point too (jr_common.h:127-154); the last one lies above the
#             descending profile before it, at the same place, so that it widens that slice's altitude range
#   lone_up   the same two one-point profiles where the slices they join stay monotone: the first one 1 km below the
#             ascending profile after it, the last one 15 km above the ASCENDING profile before it, each at that
#             profile's place -- atm_sorted holds, so the fused kernel copies the joined slice (foreign point
#             included) to LDS and the tracer resumes its altitude brackets on it
#   short_last a last profile of two levels: a ray time stamp between the profiles before it and it is traced through
#             it (locate_atm's second search), though it matches no profile
#   at_cap    a slice of 315 levels: 13 rows (5 emitters, 1 window) of 315 doubles fill 32 KB of LDS as far as they
#             can (jur_pencil_kernel's profile copy is made)
#   over_cap  a slice of 316 levels: one more than fits (no copy)
SCENES = {
    "ragged": ([_spec(0.5, 10.0, 45.0, 60, 0.0, 80.0),
                _spec(1.25, -180.0, -30.0, 150, 2.0, 95.0, descending=True),
                _spec(2.0, 179.9, 0.0, 2, 0.0, 70.0),
                _spec(2.75, 45.0, 89.99, 33, 0.0, 60.0, descending=True),
                _spec(4.0, -75.0, -90.0, 41, 5.0, 85.0)],
               [0.0, 1.5, 3.5, 9.0], None),
    "unsorted": ([_spec(3.0, 120.0, 60.0, 45, 0.0, 90.0, p0_top=True, q_nonpos=[(1, 10, 0.0), (2, 20, -1e-9)]),
                  _spec(-1.5, -10.0, -89.99, 80, 0.0, 75.0, descending=True, p0_top=True),
                  _spec(7.0, 180.0, 10.0, 30, 3.0, 65.0, move_at=20),
                  _spec(0.0, 0.0, 90.0, 25, 0.0, 100.0, q_nonpos=[(0, 3, -1e-7), (1, 0, 0.0)])],
                 [2.0, 10.0], [2, 0, 3, 1]),
    "lone_ends": ([_spec(0.0, 30.0, 20.0, 1, 5.0, 5.0),
                   _spec(1.0, 30.0, 20.0, 50, 0.0, 70.0),
                   _spec(2.5, -120.0, -45.0, 40, 0.0, 80.0),
                   _spec(4.0, 60.0, 70.0, 45, 0.0, 60.0, descending=True),
                   _spec(5.0, 60.0, 70.0, 1, 75.0, 75.0)],
                  [-2.0, 0.0, 0.5, 3.0, 4.5, 5.0, 9.0], None),
    "lone_up": ([_spec(0.0, 30.0, 20.0, 1, -1.0, -1.0),
                 _spec(1.0, 30.0, 20.0, 50, 0.0, 70.0),
                 _spec(2.5, -120.0, -45.0, 40, 0.0, 80.0, descending=True),
                 _spec(4.0, 60.0, 70.0, 45, 0.0, 60.0),
                 _spec(5.0, 60.0, 70.0, 1, 75.0, 75.0)],
                [-2.0, 0.0, 0.5, 3.0, 4.5, 5.0, 9.0], None),
    "short_last": ([_spec(0.0, -60.0, 35.0, 40, 0.0, 70.0),
                    _spec(1.0, 100.0, -20.0, 30, 0.0, 85.0, descending=True),
                    _spec(2.0, 170.0, 5.0, 2, 0.0, 80.0)],
                   [0.5, 1.5, 3.0], None),
    "at_cap": ([_spec(0.0, 20.0, -10.0, 315, 0.0, 90.0),
                _spec(1.0, -150.0, 50.0, 120, 0.0, 80.0, descending=True)],
               [], None),
    "over_cap": ([_spec(0.0, 20.0, -10.0, 316, 0.0, 90.0, descending=True),
                  _spec(1.0, -150.0, 50.0, 120, 0.0, 80.0)],
                 [], None),
}


def scene(name, ctl, base, nrays=180, seed=0):
    """-> (atm_t, geom (nrays + extra, 7), profile specs) of a named scene.  The rays carry their profile's time stamp;
    after them come six limb rays per extra time stamp (one that matches no profile, or lies below the first or
    above the last), looking at the first profile's place."""
    spec, extra, order = SCENES[name]
    atm = ragged_atmosphere(ctl, spec, seed=seed, base=base, order=order)
    live = [s for s in spec if s["n"] > 1]
    geom = global_geometry(live, nrays, seed=seed + 1)
    if extra:
        g2 = global_geometry(live[:1], 6 * len(extra), seed=seed + 2)
        g2[:, 0] = np.repeat(extra, 6)
        geom = np.vstack([geom, g2])
    return atm, geom, spec
