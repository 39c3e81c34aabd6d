"""Constructed edge cases and a plain extended-precision model of the field-of-view convolution (formod_fov) and of
the atmosphere regridding (intpol_atm, IP = 1 / 2 / 3) -- a helper of tests/test_fov_edges_*.py and
tests/test_intpol_edges_*.py, no tests in it.

The rules stand in include/jurassic_hip.h and in the comments of jur_fov.c and jur_intpol.c; they are restated here from
those words, not from the kernels.  What DECIDES something -- which rays a window gathers, which bracket a point falls
into, which two profiles are nearest, every cut-off, and the weights the cut-offs are applied to (the blend weight r of
IP 2, the point weights w of IP 3 and their running sum) -- is evaluated in float64, one rounding per operation, so that
the model takes the branch the code takes; sin and cos are the interpreter's, i.e. the C library's the oracle is linked
to.  The interpolation and the averaging are carried in np.longdouble (64 significant bits here), and next to every
value the model returns the sum of the absolute values of its terms, which the bounds below scale with.

Bounds (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Lemma 3.1): u = 2^-53,
gamma_m = m u / (1 - m u), first order in u; the tests allow twice each bound, which covers the second order.

  linear interpolation   y0 + (x - x0) (y1 - y0) / (x1 - x0) rounds x - x0, y1 - y0, their product, x1 - x0, the
                         quotient and the sum: six roundings on the slope term, one on y0, and y1 - y0 enters through
                         its absolute value:                 gamma_6 (|y0| + |x - x0| |y1 - y0| / |x1 - x0|).
  field of view          a term is w_k times that: seven roundings; the first term is added to zero exactly, the other
                         n - 1 additions touch a term at most n - 1 times; the quotient by wsum rounds once:
                         gamma_{n+7} S / |wsum|.  wsum itself is a sum of n weights with n - 1 roundings, off by at
                         most gamma_{n-1} sum |w_k|, which moves the quotient by gamma_{n-1} (sum |w_k| / |wsum|)
                         S / |wsum|.  For n = 2 and weights of one sign that is gamma_{n+8}; it is 2 n + 6 in general.
  exponential (p)        y0 exp(log(y1 / y0) / (x1 - x0) (x - x0)) with E the exponent and a = (x - x0) / (x1 - x0):
                         the rounding of y1 / y0 moves E by u |a|; log (within 1 ulp: 2 u), x1 - x0, the quotient,
                         x - x0 and the product move it by gamma_6 |E|; exp (2 u) and the product with y0 add
                         gamma_3:                            |p| (gamma_6 |E| + u |a| + gamma_3).
  IP 2 blend             (1 - r) v0 + r v1 with r given: 1 - r, two products, one sum, three roundings on a term:
                         gamma_3 (|(1 - r) v0| + |r v1|) on top of |1 - r| b0 + |r| b1 of the two profiles' values.
  IP 3 mean              sum w_i x_i / wsum over m contributing points with w given (all w_i > 0): a product and at most
                         m - 1 additions on a term, m - 1 roundings in wsum, the quotient:
                         gamma_{2m} sum |w_i x_i| / |wsum|."""
import math
import numpy as np
from jurassic_hip import abi

U = 2.0 ** -53
LD = np.longdouble
NFOV = abi.NFOV
NG = 3
RE = 6367.421                    # oracle_constants.h (src/jurassic.h:126)
assert np.finfo(LD).eps <= 2.0 ** -63, "the models need an extended-precision long double"


def gamma(m):
    return m * U / (1 - m * U)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def bracket(z, x):
    """Index i of the bracket [z[i], z[i+1]] of every x on a strictly monotone axis of at least two nodes.  Ascending:
    the last node that is <= x; descending: the last node that is > x; in both cases the first bracket for an x in
    front of the axis and the last one for an x behind it (which is then extrapolated)."""
    z = np.asarray(z, dtype=np.float64)
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    d = np.diff(z)
    assert len(z) >= 2 and (np.all(d > 0) or np.all(d < 0)), "the rule is defined for a strictly monotone axis"
    inside = (z[None, :] <= x[:, None]) if d[0] > 0 else (z[None, :] > x[:, None])
    return np.clip(inside.sum(axis=1) - 1, 0, len(z) - 2)


# ----------------------------------------------------------------------------------------------------------------------
# field of view
# ----------------------------------------------------------------------------------------------------------------------
class LoneRay(ValueError):
    """fewer than two rays of a ray's time stamp within +-NFOV positions: "Cannot apply FOV convolution!" """


def fov_window(time, ir):
    """the rays ray ir is convolved from: positions ir - NFOV .. ir + NFOV inside the array, same time stamp"""
    lo, hi = max(ir - NFOV, 0), min(ir + 1 + NFOV, len(time))
    return lo, hi, np.array([j for j in range(lo, hi) if time[j] == time[ir]], dtype=np.int64)


def fov_model(time, vpz, rad0, tau0, dz, w):
    """-> dict(rad, tau: the convolved values (nr, nd) in long double; b_rad, b_tau: their bounds; trace: per ray
    lo, hi, src, idx (bracket per weight), a (position in the bracket in units of its width: < 0 or > 1 extrapolated),
    node (weights whose zfov is another ray's vpz exactly); exact: every vpz + dz is a float64 without rounding)."""
    time, vpz, dz, w = (np.asarray(x, dtype=np.float64) for x in (time, vpz, dz, w))
    nr, nd = rad0.shape
    n = len(dz)
    wl = w.astype(LD)
    W, Wabs = wl.sum(), np.abs(wl).sum()
    out = {k: np.zeros((nr, nd), LD) for k in ("rad", "tau", "b_rad", "b_tau")}
    trace, exact = [], True
    for ir in range(nr):
        lo, hi, src = fov_window(time, ir)
        if len(src) < 2:
            raise LoneRay(ir)
        z = vpz[src]
        zfov = vpz[ir] + dz                                                   # float64: the abscissa the rule names
        exact = exact and bool(np.all(LD(vpz[ir]) + dz.astype(LD) == zfov.astype(LD)))
        idx = bracket(z, zfov)
        a = (zfov.astype(LD) - z[idx].astype(LD)) / (z[idx + 1].astype(LD) - z[idx].astype(LD))
        for key, X in (("rad", rad0), ("tau", tau0)):
            x0, x1 = X[src[idx]].astype(LD), X[src[idx + 1]].astype(LD)       # (n, nd)
            out[key][ir] = (wl[:, None] * (x0 + a[:, None] * (x1 - x0))).sum(axis=0) / W
            S = (np.abs(wl)[:, None] * (np.abs(x0) + np.abs(a)[:, None] * np.abs(x1 - x0))).sum(axis=0)
            out["b_" + key][ir] = (gamma(n + 7) + gamma(n - 1) * Wabs / abs(W)) * S / abs(W)
        others = z[src != ir]
        trace.append(dict(lo=lo, hi=hi, src=src, idx=idx, a=a.astype(np.float64), node=np.isin(zfov, others)))
    out["trace"], out["exact"] = trace, exact
    return out


def fov_ratio(got_rad, got_tau, ref):
    """largest error / (twice the bound) of a result against fov_model's"""
    worst = 0.0
    tiny = np.finfo(LD).tiny
    for got, key in ((got_rad, "rad"), (got_tau, "tau")):
        err = np.abs(got.astype(LD) - ref[key])
        worst = max(worst, float(np.max(err / np.maximum(2 * ref["b_" + key], tiny))))
    return worst


_STEPS = ((1.5,), (1.5,), (0.75, 1.25, 2.0, 0.5, 1.5), (2.0, 0.5, 1.25, 0.75))


def _scan(length, kind, z0):
    """view-point altitudes of one scan, all multiples of 1/4 km: kind 0 ascending and 1 descending in steps of 1.5 km,
    2 ascending and 3 descending in unequal steps"""
    steps = _STEPS[kind]
    z = z0 + np.concatenate([[0.0], np.cumsum([steps[j % len(steps)] for j in range(length - 1)])])
    return z[::-1].copy() if kind & 1 else z


BASE_SCANS = (2, 3, 11, 12, 13)          # below, at and above the window of 2 NFOV + 1 = 11 rays
INTERLEAVED = 8                          # A B A B A B A B
NR_BASE = sum(BASE_SCANS) + INTERLEAVED + 2


def fov_batch(nr, nd, seed=0, lone=None):
    """A batch of nr >= NR_BASE rays (nr - NR_BASE != 1): scans of 2, 3, 11, 12 and 13 rays, two interleaved scans of 4
    rays each, filler scans of 5 (and one of 2 to 6) rays and a last scan of 2 rays; ascending, descending and unequally
    spaced in turn; one time stamp per scan.  Radiances over seven decades, transmittances in (0, 1] with an exact 1.
    lone: None, or "first" / "middle" / "last": one more ray that is alone in its window (the middle one carries the time
    stamp of the first scan, six and more positions away).  -> dict(time, vpz, rad, tau, scans=[(start, length, kind)],
    inter=(start, length))"""
    rest = nr - NR_BASE
    assert rest == 0 or rest >= 2
    lengths = list(BASE_SCANS)
    filler = []
    while rest >= 7:
        filler.append(5)
        rest -= 5
    if rest:
        filler.append(rest)
    time, vpz, scans = [], [], []
    stamp = 0

    def add(length, kind):
        nonlocal stamp
        scans.append((len(time), length, kind))
        vpz.extend(_scan(length, kind, 10.0 + 0.25 * (stamp % 7)))
        time.extend([float(stamp)] * length)
        stamp += 1

    for k, length in enumerate(lengths):
        add(length, (0, 1, 2, 1, 0)[k])
    inter = (len(time), INTERLEAVED)
    za, zb = _scan(INTERLEAVED // 2, 0, 12.0), _scan(INTERLEAVED // 2, 3, 30.0)
    for j in range(INTERLEAVED // 2):
        time.extend([float(stamp), float(stamp + 1)])
        vpz.extend([za[j], zb[j]])
    stamp += 2
    for k, length in enumerate(filler):
        add(length, (3, 2, 0, 1)[k % 4])
    add(2, 1)
    time, vpz = np.array(time), np.array(vpz)
    if lone is not None:
        at = {"first": 0, "middle": sum(BASE_SCANS[:3]), "last": len(time)}[lone]
        t = 0.0 if lone == "middle" else 1e3
        time, vpz = np.insert(time, at, t), np.insert(vpz, at, 20.0)
    n = len(time)
    rng = np.random.default_rng(1000 * nd + n + seed)
    rad = 10.0 ** rng.uniform(-6.0, 1.0, (n, nd))
    tau = rng.uniform(0.01, 1.0, (n, nd))
    tau[n // 2, 0] = 1.0
    return dict(time=time, vpz=vpz, rad=rad, tau=tau, scans=scans, inter=inter)


def _shapes():
    big = -8.0 + np.arange(abi.NSHAPE) / 128.0             # the largest n the device entry accepts
    return {"n1": (np.array([0.25]), np.array([2.0])),
            "n2": (np.array([-4.0, 4.5]), np.array([1.0, 3.0])),
            # exact zeros at both ends; +-1.5 lands on the neighbours of an equally spaced scan; +-7 needs the fifth
            "zeros": (np.array([-7.0, -4.0, -1.5, -0.5, 0.0, 0.5, 1.5, 4.0, 7.0]), np.array([0.0, 0.5, 1.0, 2.0, 4.0, 2.0, 1.0, 0.5, 0.0])),
            # asymmetric, with a negative side lobe
            "asym": (np.array([-7.0, -3.0, -1.5, -0.25, 0.75, 1.5, 2.5, 6.5]), np.array([0.1, 0.5, 1.0, 2.0, 0.7, 0.3, -0.2, 0.05])),
            "nmax": (big, np.exp(-0.5 * (big / 2.5) ** 2))}


SHAPES = _shapes()
# (nd, nr): nr nd = 255, 256, 257 for nd = 1 (and 256 for 2, 255 for 3); 102, 153 and 357 are no multiples of 64
FOV_SIZES = ((1, 255), (1, 256), (1, 257), (2, NR_BASE), (2, 128), (3, NR_BASE), (3, 85), (7, NR_BASE))
FOV_BIG = ((2, NR_BASE), (1, 257))       # where the 2048-point shape runs


def fov_shapes_of(nd, nr):
    return [s for s in SHAPES if s != "nmax" or (nd, nr) in FOV_BIG]


_fov_cache = {}


def fov_case(nd, nr, shape):
    """-> (batch, dz, w, fov_model's result), computed once per process and not to be changed"""
    key = (nd, nr, shape)
    if key not in _fov_cache:
        b = fov_batch(nr, nd)
        dz, w = SHAPES[shape]
        _fov_cache[key] = (b, dz, w, fov_model(b["time"], b["vpz"], b["rad"], b["tau"], dz, w))
    return _fov_cache[key]


def fov_edges(batch, ref, dz):
    """The edges a batch and a shape reach, from the model's trace (a set of names; the tests assert it)."""
    tr, nr = ref["trace"], len(batch["time"])
    hit = set()
    if ref["exact"]:
        hit.add("zfov exact")
    if tr[0]["lo"] == 0 and len(tr[0]["src"]) == 2 and tr[-1]["hi"] == nr and len(tr[-1]["src"]) == 2:
        hit.add("2-ray scans clipped at lo = 0 and hi = nr")
    if any(len(t["src"]) < min(2 * NFOV + 1, t["hi"] - t["lo"]) for t in tr):
        hit.add("scan shorter than the window")
    if any(len(t["src"]) == 2 * NFOV + 1 for t in tr):
        hit.add("full window")
    i0, ni = batch["inter"]
    if all(np.any(np.diff(tr[i]["src"]) == 2) for i in range(i0, i0 + ni)):
        hit.add("interleaved: src is not lo + k")
    beyond = far = True
    for start, length, kind in batch["scans"]:
        z = batch["vpz"][start:start + length]
        for ir in (start, start + length - 1):                      # the scan's end rays
            a = tr[ir]["a"]
            beyond = beyond and bool(np.any(a < 0) or np.any(a > 1))
            far = far and bool(np.any(a < -1) or np.any(a > 2))
        zf = z[:, None] + dz[None, :]
        if not (zf.min() < z.min() and zf.max() > z.max()):
            beyond = False
    kinds = {k for _, _, k in batch["scans"]}
    if {0, 1} <= kinds:
        hit.add("ascending and descending scans")
    if kinds & {2, 3}:
        hit.add("unequal spacing")
    if beyond:
        hit.add("dz beyond both ends of every scan")
    if far:
        hit.add("end rays extrapolated by more than one spacing")
    if any(t["node"].any() for t in tr):
        hit.add("zfov on a neighbour's vpz")
    return hit


def fov_obs(batch, nd):
    """obs_t of a batch, for the oracle's formod_fov"""
    nr = len(batch["time"])
    obs = abi.obs_t()
    obs.nr = nr
    np.ctypeslib.as_array(obs.time)[:nr] = batch["time"]
    np.ctypeslib.as_array(obs.vpz)[:nr] = batch["vpz"]
    np.ctypeslib.as_array(obs.rad)[:nr, :nd] = batch["rad"]
    np.ctypeslib.as_array(obs.tau)[:nr, :nd] = batch["tau"]
    return obs


def fov_ctl(nd):
    return abi.make_ctl(["CO2"], list(common_nu(nd)))


def common_nu(nd):
    return [650.0 + 100.0 * d for d in range(nd)]


# ----------------------------------------------------------------------------------------------------------------------
# regridding
# ----------------------------------------------------------------------------------------------------------------------
ROWS = ("p", "t", "q0", "q1", "q2", "k")


def geo2cart0(lon, lat):
    """position at altitude 0 in float64, as the host prepares it: radius cos(lat) cos(lon), .. sin(lon), radius sin(lat)"""
    deg = math.pi / 180
    clat = math.cos(lat * deg)
    return np.array([RE * clat * math.cos(lon * deg), RE * clat * math.sin(lon * deg), RE * math.sin(lat * deg)])


def dist2(a, b):
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2])


def source(z, lon, lat, p, t, q, k):
    """a source atmosphere as plain arrays: rows p, t, q0, q1, q2, k over the points"""
    z = np.asarray(z, dtype=np.float64)
    n = len(z)
    f = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)).copy()
    q = np.asarray(q, dtype=np.float64)
    assert q.shape == (NG, n)
    return dict(z=z, lon=f(lon), lat=f(lat), rows=np.vstack([f(p), f(t), q, f(k)]))


def to_atm(src):
    atm = abi.atm_t()
    n = len(src["z"])
    atm.np = n
    for name in ("z", "lon", "lat"):
        np.ctypeslib.as_array(getattr(atm, name))[:n] = src[name]
    np.ctypeslib.as_array(atm.p)[:n] = src["rows"][0]
    np.ctypeslib.as_array(atm.t)[:n] = src["rows"][1]
    np.ctypeslib.as_array(atm.q)[:NG, :n] = src["rows"][2:2 + NG]
    np.ctypeslib.as_array(atm.k)[:1, :n] = src["rows"][2 + NG:]
    return atm


def dest_atm(z, lon, lat):
    n = len(z)
    atm = abi.atm_t()
    atm.np = n
    for name, a in (("z", z), ("lon", lon), ("lat", lat)):
        np.ctypeslib.as_array(getattr(atm, name))[:n] = a
    for name in ("p", "t"):
        np.ctypeslib.as_array(getattr(atm, name))[:n] = 7.0            # stale content the call must overwrite
    np.ctypeslib.as_array(atm.q)[:NG, :n] = 7.0
    np.ctypeslib.as_array(atm.k)[:1, :n] = 7.0
    return atm


def rows_of(atm):
    """(6, n) rows p, t, q0, q1, q2, k of a regridded atmosphere"""
    n = atm.np
    return np.vstack([np.ctypeslib.as_array(atm.p)[:n], np.ctypeslib.as_array(atm.t)[:n], np.ctypeslib.as_array(atm.q)[:NG, :n],
                      np.ctypeslib.as_array(atm.k)[:1, :n]]).copy()


def intpol_ctl(ip, cx=0.0, cz=0.0):
    ctl = abi.make_ctl(["CO2", "H2O", "O3"], [792.0], ip=ip)
    ctl.cx, ctl.cz = cx, cz
    return ctl


def _profile_rule(z, rows, z0, hit):
    """One profile (points z, rows (6, n)) at altitude z0: p exponentially in altitude where both levels of the bracket
    are positive and linearly otherwise, everything else linearly.  -> value, bound, pexp (6,): pexp is |p| (1 + |E|)
    in row 0 where p went through exp and log and 0 everywhere else."""
    i = int(bracket(z, z0)[0])
    if np.any(z == z0):
        hit.add("z == node")
    if z0 < z.min() or z0 > z.max():
        hit.add("z beyond the profile")
    x0, x1, x = LD(z[i]), LD(z[i + 1]), LD(z0)
    y0, y1 = rows[:, i].astype(LD), rows[:, i + 1].astype(LD)
    a = (x - x0) / (x1 - x0)
    val = y0 + a * (y1 - y0)
    bnd = gamma(6) * (np.abs(y0) + abs(a) * np.abs(y1 - y0))
    pexp = np.zeros(len(ROWS), LD)
    if rows[0, i] > 0 and rows[0, i + 1] > 0:
        E = np.log(y1[0] / y0[0]) / (x1 - x0) * (x - x0)
        assert abs(E) <= 10, "keep the exponent of an extrapolated pressure within 10"
        val[0] = y0[0] * np.exp(E)
        bnd[0] = abs(val[0]) * (gamma(6) * abs(E) + U * abs(a) + gamma(3))
        pexp[0] = abs(val[0]) * (1 + abs(E))
    else:
        hit.add("p <= 0: linear")
    return val, bnd, pexp


def _profiles(src):
    """first point and length of every profile of a track: a profile is a run of points with one longitude and latitude"""
    first = [0]
    for i in range(1, len(src["z"])):
        if src["lon"][i] != src["lon"][i - 1] or src["lat"][i] != src["lat"][i - 1]:
            first.append(i)
    first = np.array(first)
    return first, np.diff(np.append(first, len(src["z"])))


def intpol_model(ip, src, z, lon, lat, cx=0.0, cz=0.0):
    """-> val (6, nd_) long double (NaN where the rule gives none), bnd (6, nd_), pexp (6, nd_), hits: per destination
    point the set of comparisons that were met with equality (and the other edges it reached)."""
    nd_ = len(z)
    val, bnd, pexp = (np.zeros((len(ROWS), nd_), LD) for _ in range(3))
    hits = []
    zs, rows = src["z"], src["rows"]
    if ip == 2:
        first, length = _profiles(src)
        pos = [geo2cart0(src["lon"][i], src["lat"][i]) for i in first]
    elif ip == 3:
        pos = [geo2cart0(src["lon"][i], src["lat"][i]) for i in range(len(zs))]
    for j in range(nd_):
        hit = set()
        if ip == 1:
            val[:, j], bnd[:, j], pexp[:, j] = _profile_rule(zs, rows, z[j], hit)
        elif ip == 2:
            # the two nearest profiles among those within 10 degrees of latitude; a tie goes to the later profile; with
            # fewer than two in reach the missing one is profile 0 at the distance 1e99
            x0 = geo2cart0(lon[j], lat[j])
            d0 = d1 = 1e99
            i0 = i1 = 0
            for ix in range(len(first)):
                dlat = abs(lat[j] - src["lat"][first[ix]])
                if dlat == 10:
                    hit.add("dlat == 10")
                if dlat <= 10:
                    dh = dist2(x0, pos[ix])
                    if dh == d0:
                        hit.add("dh == dhmin0")
                    elif dh == d1 and dh > d0:
                        hit.add("dh == dhmin1")
                    if dh <= d0:
                        d1, i1, d0, i0 = d0, i0, dh, ix
                    elif dh <= d1:
                        d1, i1 = dh, ix
            if d0 == 1e99:
                hit.add("no profile in reach")
            elif d1 == 1e99:
                hit.add("one profile in reach")
            if d0 == 0:
                hit.add("dhmin0 == 0")
            # the blend weight in float64: r0 the distance from profile i0 to the foot of the point on the line to
            # profile i1, r1 the rest; r = 0 before the line, 1 behind it
            with np.errstate(all="ignore"):
                x2 = np.float64(dist2(pos[i0], pos[i1]))
                x = np.sqrt(x2)
                r0 = (np.float64(d0) - np.float64(d1) + x2) / (2 * x)
                r1 = x - r0
                if r0 == 0:
                    hit.add("r0 == 0")
                if r0 <= 0:
                    r = np.float64(0.0)
                elif r1 <= 0:
                    r = np.float64(1.0)
                else:
                    r = r0 / (r0 + r1)
            if r0 < 0:
                hit.add("r0 < 0")
            h0, h1 = set(), set()
            v0, b0, e0 = _profile_rule(zs[first[i0]:first[i0] + length[i0]], rows[:, first[i0]:first[i0] + length[i0]], z[j], h0)
            v1, b1, e1 = _profile_rule(zs[first[i1]:first[i1] + length[i1]], rows[:, first[i1]:first[i1] + length[i1]], z[j], h1)
            if ("z beyond the profile" in h0) != ("z beyond the profile" in h1):
                hit.add("z beyond one of the two profiles")
            hit |= (h0 | h1) & {"z == node"}
            if np.isnan(r):
                hit.add("r is NaN")
                val[:, j] = np.nan
            else:
                rl = LD(r)
                val[:, j] = (1 - rl) * v0 + rl * v1
                bnd[:, j] = abs(1 - rl) * b0 + abs(rl) * b1 + gamma(3) * (np.abs((1 - rl) * v0) + np.abs(rl * v1))
                pexp[:, j] = abs(1 - rl) * e0 + abs(rl) * e1
        else:
            # the mean of the source points closer than cz in altitude, cx / 111.13 degrees in latitude and cx in
            # distance (all three exclusive), weighted with (1 - dz / cz) (cx^2 - dx^2) / (cx^2 + dx^2); no value where
            # the weights sum to less than 1e-6
            x0 = geo2cart0(lon[j], lat[j])
            rm2 = cx * cx
            ws, wsum = [], 0.0
            for i in range(len(zs)):
                dz = abs(zs[i] - z[j])
                if dz == cz:
                    hit.add("dz == cz")
                if dz >= cz:
                    continue
                if abs(src["lat"][i] - lat[j]) * 111.13 >= cx:
                    continue
                dx2 = dist2(x0, pos[i])
                if dx2 == rm2:
                    hit.add("dx2 == rm2")
                if dx2 >= rm2:
                    continue
                if dz == 0 and dx2 == 0:
                    hit.add("on a source point")
                if dz == np.nextafter(cz, 0.0):
                    hit.add("dz one ulp inside cz")
                w = (1 - dz / cz) * (rm2 - dx2) / (rm2 + dx2)
                ws.append((i, w))
                wsum += w
            if ws and abs(wsum - 1e-6) < 1e-15:
                hit.add("wsum just above 1e-6" if wsum >= 1e-6 else "wsum just below 1e-6")
            hit.add("m = %d" % len(ws))
            if wsum >= 1e-6:
                m = len(ws)
                wl = np.array([w for _, w in ws], dtype=LD)
                xs = rows[:, [i for i, _ in ws]].astype(LD)
                val[:, j] = (wl[None, :] * xs).sum(axis=1) / wl.sum()
                bnd[:, j] = gamma(2 * m) * (np.abs(wl[None, :] * xs)).sum(axis=1) / abs(wl.sum())
            else:
                val[:, j] = np.nan
        hits.append(hit)
    return val, bnd, pexp, hits


# --- the cases ---------------------------------------------------------------------------------------------------------
def _gases(n, scale=1.0):
    j = np.arange(n)
    return np.vstack([3.7e-4 * scale + 0 * j, 2.5e-3 * scale / (1 + j * j), 1e-6 * scale * (1 + j)])


def _pad(targets, count):
    """cycle a list of (z, lon, lat, tags) targets up to count of them"""
    return [targets[i % len(targets)] for i in range(count)] if count > len(targets) else targets[:count]


def _case(name, ip, src, targets, cx=0.0, cz=0.0):
    z, lon, lat = (np.array([t[k] for t in targets], dtype=np.float64) for k in range(3))
    return dict(name=name, ip=ip, src=src, z=z, lon=lon, lat=lat, cx=cx, cz=cz, expect=[set(t[3]) for t in targets])


def _ip1_targets(z, p_lin=()):
    """every node, both ends, one and ten spacings beyond each end, half way between the nodes; p_lin: the brackets
    (lower index) in which a level without pressure makes p linear"""
    n = len(z)
    up = z[0] < z[-1]
    lo_i, hi_i = (0, n - 1) if up else (n - 1, 0)

    def tags(x):
        t = set()
        if x in z:
            t.add("z == node")
        if x < z.min() or x > z.max():
            t.add("z beyond the profile")
        if int(bracket(z, x)[0]) in p_lin:
            t.add("p <= 0: linear")
        return t

    xs = list(z) + [(z[i] + z[i + 1]) / 2 for i in range(n - 1)]
    for end, inner in ((lo_i, lo_i + (1 if up else -1)), (hi_i, hi_i + (-1 if up else 1))):
        step = z[end] - z[inner]
        xs += [z[end] + step, z[end] + 10 * step]
    return [(x, 0.0, 0.0, tags(x)) for x in xs]


Z8 = np.arange(8) * 10.0
P8 = np.array([1000.0, 500.0, 250.0, 120.0, 60.0, 30.0, 15.0, 7.5])
T8 = np.array([288.0, 250.5, 221.0, 216.5, 230.0, 255.5, 270.0, 245.0])
K8 = np.array([3e-4, 1e-4, 5e-5, 0.0, 2e-5, 1e-5, 0.0, 0.0])


def _prof8(lon=0.0, lat=0.0, scale=1.0, dt=0.0):
    return source(Z8, lon, lat, P8 * scale, T8 + dt, _gases(8, scale), K8 * scale)


def _stack(*srcs):
    return dict(z=np.concatenate([s["z"] for s in srcs]), lon=np.concatenate([s["lon"] for s in srcs]),
                lat=np.concatenate([s["lat"] for s in srcs]), rows=np.hstack([s["rows"] for s in srcs]))


def _sub(src, idx, **kw):
    out = dict(z=src["z"][idx].copy(), lon=src["lon"][idx].copy(), lat=src["lat"][idx].copy(), rows=src["rows"][:, idx].copy())
    for k, v in kw.items():
        out[k][:] = v
    return out


def intpol_cases():
    cases = []
    # ---- IP 1 -------------------------------------------------------------------------------------------------------
    two = source([5.0, 25.0], 0.0, 0.0, [800.0, 400.0], [280.0, 220.0], _gases(2), [1e-4, 2e-5])
    cases.append(_case("ip1 ns=2, 1 target", 1, two, _pad(_ip1_targets(two["z"]), 1)))
    cases.append(_case("ip1 ns=2, 127 targets", 1, two, _pad(_ip1_targets(two["z"]), 127)))
    eight = _prof8()
    cases.append(_case("ip1 ns=8, 128 targets", 1, eight, _pad(_ip1_targets(Z8), 128)))
    holes = _prof8()
    holes["rows"][0, 3] = 0.0                                     # a level with p = 0: brackets 2 and 3 fall back
    holes["rows"][3, 5] = 0.0                                     # a level with q1 = 0
    cases.append(_case("ip1 ns=8 with p = 0 and q = 0 levels, 129 targets", 1, holes, _pad(_ip1_targets(Z8, p_lin=(2, 3)), 129)))
    down = _sub(eight, np.arange(8)[::-1])
    cases.append(_case("ip1 ns=8 descending, 129 targets", 1, down, _pad(_ip1_targets(down["z"]), 129)))
    # ---- IP 2 -------------------------------------------------------------------------------------------------------
    # nx = 2: profiles of 8 and 2 levels at 4 S and 4 N on one meridian
    south = _prof8(0.0, -4.0)
    north = source([15.0, 45.0], 0.0, 4.0, [150.0, 3.0], [210.0, 260.0], _gases(2, 1.5), [7e-5, 1e-6])
    tiny = 2.0 ** -40
    t2 = [(20.0, 0.0, -4.0, {"dhmin0 == 0", "r0 == 0", "z == node"}),            # on the southern profile, at a node
          (45.0, 0.0, 4.0, {"dhmin0 == 0", "r0 == 0", "z == node"}),             # on the northern one, its top node
          (30.0, 0.0, 0.0, {"dh == dhmin0", "z == node"}),                       # the mid-point: a tie
          (25.0, 0.0, 0.0, {"dh == dhmin0"}),
          (5.0, 0.0, 0.0, {"dh == dhmin0", "z beyond one of the two profiles"}),  # below the short profile
          (55.0, 0.0, 0.0, {"dh == dhmin0", "z beyond one of the two profiles"}),  # above it
          (25.0, 0.0, -5.5, {"r0 < 0"}),                                         # beyond the first profile
          (25.0, 0.0, 5.5, {"r0 < 0"}),                                          # beyond the last profile
          (25.0, 0.0, 6.0, {"dlat == 10", "r0 < 0"}),                            # 10 degrees from the southern profile
          (25.0, 0.0, 6.0 + tiny, {"one profile in reach", "r0 < 0"}),           # just beyond: pairs with profile 0
          (25.0, 0.0, 14.0, {"dlat == 10", "one profile in reach", "r0 < 0"}),   # 10 degrees from the northern one
          (25.0, 0.0, 14.0 + tiny, {"no profile in reach", "r is NaN"}),
          (25.0, 0.0, -14.0, {"dlat == 10", "one profile in reach", "r0 < 0"}),  # the one in reach IS profile 0
          (25.0, 0.0, -14.0 - tiny, {"no profile in reach", "r is NaN"}),
          (25.0, 1.0, 1.0, set())]
    cases.append(_case("ip2 nx=2", 2, _stack(south, north), t2))
    # nx = 5: 2, 8, 3, 8 and 5 levels; profile 2 lies at the equator 3 degrees east of the meridian of the others
    p0 = source([10.0, 30.0], 0.0, -12.0, [300.0, 12.0], [225.0, 228.0], _gases(2, 0.5), [5e-5, 0.0])
    p1 = _prof8(0.0, -4.0, 1.0, 0.0)
    p2 = source([20.0, 35.0, 50.0], 3.0, 0.0, [60.0, 6.0, 0.75], [215.0, 240.0, 268.0], _gases(3, 2.0), [2e-5, 1e-5, 0.0])
    p3 = _prof8(0.0, 4.0, 1.25, 12.5)
    p4 = source([5.0, 20.0, 35.0, 50.0, 65.0], 0.0, 12.0, [550.0, 55.0, 5.5, 0.75, 0.125], [260.0, 215.0, 235.0, 265.0, 230.0],
                _gases(5, 0.75), [1e-4, 3e-5, 0.0, 0.0, 0.0])
    t5 = [(30.0, 0.0, 0.0, {"dh == dhmin1", "z == node"}),                       # profile 2 nearest, 1 and 3 tie behind it
          (42.5, 0.0, 0.0, {"dh == dhmin1"}),
          (35.0, 3.0, 0.0, {"dhmin0 == 0", "r0 == 0", "dh == dhmin1", "z == node"}),   # on profile 2
          (12.5, 3.0, 1.0, {"z beyond one of the two profiles"}),               # 2 and 3: below the shorter one
          (57.5, 3.0, 1.0, {"z beyond one of the two profiles"}),               # above it
          (25.0, 0.0, -12.0, {"dhmin0 == 0", "r0 == 0"}),                        # on profile 0
          (25.0, 0.0, -13.0, {"r0 < 0"}),                                        # beyond the first profile
          (25.0, 0.0, 13.0, {"r0 < 0"}),                                         # beyond the last one
          (20.0, 0.0, 9.0, {"z == node"}),                                       # between 3 and 4
          (25.0, 0.0, 22.0, {"dlat == 10", "one profile in reach", "r0 < 0"}),   # only profile 4: pairs with profile 0
          (25.0, 0.0, 22.0 + tiny, {"no profile in reach", "r is NaN"}),
          (25.0, 0.0, -2.0, {"dlat == 10"}),                                     # 10 degrees from profile 0
          (25.0, 1.5, -7.0, set())]
    cases.append(_case("ip2 nx=5, ragged", 2, _stack(p0, p1, p2, p3, p4), t5))
    # ---- IP 3 -------------------------------------------------------------------------------------------------------
    # a cloud of 12 points around 45 N; cz = 2 km, cx = 200 km
    cz, cx = 2.0, 200.0
    cz_z = [10.0, 30.0, 30.5, 31.0, 50.0, 50.0, 50.0, 50.0, 70.0, 70.5, 90.0, 90.0]
    c_lon = [0.0, 0.0, 0.5, 0.0, 0.0, 0.5, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    c_lat = [45.0, 45.0, 45.0, 45.5, 45.0, 45.0, 45.5, 45.0, 45.0, 45.0, 45.0, 60.0]
    j = np.arange(12.0)
    cloud = source(cz_z, c_lon, c_lat, 1000.0 / (1 + j), 200.0 + 7.5 * j, np.vstack([3.7e-4 + 1e-5 * j, 1e-3 / (1 + j), 1e-6 * (1 + j * j)]), 1e-4 * (12 - j))
    t3 = [(12.0, 0.0, 45.0, {"dz == cz", "m = 0"}),                              # the only candidate at the cut-off: excluded
          (8.0, 0.0, 45.0, {"dz == cz", "m = 0"}),
          (10.0, 0.0, 45.0, {"on a source point", "m = 1"}),
          (30.0, 0.0, 45.0, {"on a source point", "m = 3"}),
          (30.75, 0.25, 45.25, {"m = 3"}),
          (50.0, 0.25, 45.125, {"m = 4"}),
          (50.5, 0.0, 45.0, {"m = 4"}),
          (70.25, 0.0, 45.0, {"m = 2"}),
          (72.0, 0.0, 45.0, {"dz == cz", "m = 1"}),                              # 70 at the cut-off, 70.5 inside
          (90.5, 0.0, 52.0, {"m = 0"}),                                          # too far in latitude from both
          (20.0, 0.0, 45.0, {"m = 0"})]
    cases.append(_case("ip3 cloud of 12", 3, cloud, t3, cx=cx, cz=cz))
    # the weight floor: one source point at z = 0 straight below the targets and cz = 1, so that dz is the target's z and
    # the only weight 1 - z, both without rounding; z steps in ulps around 1 - 1e-6 and to one ulp inside cz
    floor_src = source([0.0, 40.0], [0.0, 0.0], [45.0, 45.0], [900.0, 3.0], [285.0, 250.0], _gases(2), [2e-4, 0.0])
    z_lo = 1.0 - 1e-6
    while 1 - z_lo >= 1e-6:
        z_lo = float(np.nextafter(z_lo, 2.0))
    while 1 - float(np.nextafter(z_lo, 0.0)) < 1e-6:
        z_lo = float(np.nextafter(z_lo, 0.0))
    z_hi = float(np.nextafter(z_lo, 0.0))
    assert 1 - z_lo < 1e-6 <= 1 - z_hi
    tf = [(z_lo, 0.0, 45.0, {"wsum just below 1e-6", "m = 1"}),
          (z_hi, 0.0, 45.0, {"wsum just above 1e-6", "m = 1"}),
          (float(np.nextafter(1.0, 0.0)), 0.0, 45.0, {"dz one ulp inside cz", "m = 1"}),   # a weight of 2^-53: no value
          (1.0, 0.0, 45.0, {"dz == cz", "m = 0"}),
          (0.0, 0.0, 45.0, {"on a source point", "m = 1"})]
    cases.append(_case("ip3 weight floor", 3, floor_src, tf, cx=200.0, cz=1.0))
    # dx2 == rm2 exactly: a source point opposite the target on the equator, cx twice the radius -- cos and sin of 0
    # and of the float64 pi leave (RE, 0, 0) and (-RE, 1.2e-16 RE, 0), whose squared distance rounds to (2 RE)^2; the
    # point at the cut-off holds a NaN, which must not reach the result: it takes no part
    anti = source([10.0, 10.5, 12.0], [180.0, 60.0, 0.0], [0.0, 0.0, 0.0], [np.nan, 200.0, 150.0], [np.nan, 220.0, 230.0],
                  np.vstack([[np.nan, 1e-4, 2e-4]] * 3), [np.nan, 1e-5, 2e-5])
    ta = [(10.0, 0.0, 0.0, {"dx2 == rm2", "dz == cz", "m = 1"}),                 # 180 E at dx2 == rm2, 12 km at dz == cz
          (10.25, 0.0, 0.0, {"dx2 == rm2", "m = 2"})]
    cases.append(_case("ip3 dx2 == rm2, NaN at the cut-offs", 3, anti, ta, cx=2 * RE, cz=2.0))
    # the altitude cut-off alone, a NaN at dz == cz next to a point inside
    cut = source([10.0, 11.0], [0.0, 0.0], [45.0, 45.0], [np.nan, 300.0], [np.nan, 240.0], np.vstack([[np.nan, 3e-4]] * 3), [np.nan, 4e-5])
    tc = [(12.0, 0.0, 45.0, {"dz == cz", "m = 1"})]
    cases.append(_case("ip3 NaN at dz == cz", 3, cut, tc, cx=200.0, cz=2.0))
    return cases


_intpol_cache = {}


def intpol_case_names():
    return [c["name"] for c in intpol_cases()]


def intpol_ref(name):
    """-> (case, val, bnd, pexp, hits) of a case by name, computed once per process and not to be changed"""
    if not _intpol_cache:
        for c in intpol_cases():
            _intpol_cache[c["name"]] = (c,) + intpol_model(c["ip"], c["src"], c["z"], c["lon"], c["lat"], c["cx"], c["cz"])
    return _intpol_cache[name]


def intpol_check(rows, val, bnd, extra=None):
    """NaN positions equal and every finite value within twice its bound (+ extra, an absolute allowance) of the model;
    -> worst error / allowance"""
    nan = np.isnan(val.astype(np.float64))
    assert np.array_equal(np.isnan(rows), nan), "NaN positions"
    assert np.all(nan.all(axis=0) | ~nan.any(axis=0)), "p, T, q and k are NaN together or not at all"
    ok = ~nan
    allow = 2 * bnd + (0 if extra is None else extra)
    err = np.abs(rows.astype(LD) - val)
    ratio = np.where(ok, err / np.maximum(allow, np.finfo(LD).tiny), 0)
    exact = ok & (allow == 0)
    assert np.all(err[exact] == 0)
    ratio = np.where(exact, 0, ratio)
    return float(ratio.max()) if ratio.size else 0.0
