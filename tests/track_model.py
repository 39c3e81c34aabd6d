"""CPU model of the 2-D atmosphere along the line of sight (IP 2, "satellite track") -- a helper of
tests/test_track_cpu.py and tests/test_track_gpu.py, no tests in it.

The rule stands in include/jurassic_hip.h (IP 2).  Restated here in plain Python floats, one rounding per operation:

  profiles / weights / interp_2d   intpol_atm_2d (jurassic.c:704-760) on the profiles of ONE time block;
  traceray                         traceray (jr_common.h:585-711) with tangent_point (:502-539), the trapezoid rule
                                   (:437-443) and the column densities (:446-453), with a switch between the 1-D point
                                   rule (intpol_atm_1d on the block) and the 2-D one (every point and every probe at its
                                   own longitude and latitude);
  formod                           the forward model on top, as tests/cga_model.py builds it: orc.ega_eps (FORMOD 2) or
                                   cga_model.path_tau (FORMOD 1), orc.continua, orc.new_obs and orc.epilogue.

tests/test_track_cpu.py pins interp_2d to orc.intpol_atm under ip = 2 and traceray's 1-D rule to orc.traceray, bit for
bit.  sin, cos, asin, atan2, exp, log and sqrt are the interpreter's, i.e. the C library's the oracle is linked to."""
import math
import numpy as np
from jurassic_hip import abi
from cga_model import div, lip, continua_config, ega_ctl, pairs_of, path_tau

RE = 6367.421                    # oracle_constants.h (src/jurassic.h:126)
BOLTZMANN = 1.3806504e-23
RAD2GRD = 180 / math.pi
GRD2RAD = math.pi / 180
NLOS = abi.NLOS


def eip(x0, y0, x1, y1, x):
    if y0 > 0 and y1 > 0:
        return y0 * math.exp(div(math.log(div(y1, y0)), x1 - x0) * (x - x0))
    return lip(x0, y0, x1, y1, x)


def locate(xx, i0, n, x):
    """locate (jr_common.h:87-104) on xx[i0 : i0 + n] -> index relative to i0"""
    ilo, ihi, i = 0, n - 1, (n - 1) >> 1
    if xx[i0 + i] < xx[i0 + i + 1]:
        while ihi > ilo + 1:
            i = (ihi + ilo) >> 1
            if xx[i0 + i] > x:
                ihi = i
            else:
                ilo = i
    else:
        while ihi > ilo + 1:
            i = (ihi + ilo) >> 1
            if xx[i0 + i] <= x:
                ihi = i
            else:
                ilo = i
    return ilo


def norm(x):
    return math.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])


def asin_(x):
    return math.asin(x) if -1.0 <= x <= 1.0 else math.nan


def cart2geo(x):
    """-> (alt, lon, lat)"""
    radius = norm(x)
    lat = asin_(div(x[2], radius)) * RAD2GRD
    lon = math.atan2(x[1], x[0]) * RAD2GRD
    return radius - RE, lon, lat


def geo2cart(alt, lon, lat):
    radius = alt + RE
    clat = math.cos(lat * GRD2RAD)
    return [radius * clat * math.cos(lon * GRD2RAD), radius * clat * math.sin(lon * GRD2RAD), radius * math.sin(lat * GRD2RAD)]


def dist2(a, b):
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2])


class Atm:
    """The rows of an abi.atm_t as lists of Python floats."""

    def __init__(self, atm, ctl):
        n = atm.np
        self.np, self.ng, self.nw = n, ctl.ng, max(ctl.nw, 1)
        for f in ("time", "z", "lon", "lat", "p", "t"):
            setattr(self, f, np.ctypeslib.as_array(getattr(atm, f))[:n].tolist())
        self.q = [np.ctypeslib.as_array(atm.q)[g, :n].tolist() for g in range(self.ng)]
        self.k = [np.ctypeslib.as_array(atm.k)[w, :n].tolist() for w in range(self.nw)]
        self._tables = {}

    def block(self, time):
        """locate_atm (jr_common.h:127-154) -> (a0, n)"""
        t, lo, hi = self.time, 0, self.np - 1
        while hi > lo + 1:
            i = (lo + hi) // 2
            if t[i] < time:
                lo = i
            else:
                hi = i
        lower = lo if lo == 0 else hi
        lo, hi = lower, self.np - 1
        while hi > lo + 1:
            i = (lo + hi) // 2
            if t[i] > time:
                hi = i
            else:
                lo = i
        upper = self.np if hi == self.np - 1 else hi
        return lower, upper - lower

    def altitude_range(self, a0, n):
        """altitude_range_nn (jr_common.h:411-420): the block's first column"""
        zmin = zmax = self.z[a0]
        ipp = a0
        while ipp < a0 + n and self.lon[ipp] == self.lon[a0] and self.lat[ipp] == self.lat[a0]:
            zmax, zmin = max(zmax, self.z[ipp]), min(zmin, self.z[ipp])
            ipp += 1
        return zmin, zmax

    def profiles(self, a0, n):
        """The profile table of the block [a0, a0 + n): a list of (first, len, x1, lat), jurassic.c:715-725."""
        key = (a0, n)
        if key not in self._tables:
            out, lon1, lat1 = [], -999.0, -999.0
            for ip in range(a0, a0 + n):
                if self.lon[ip] != lon1 or self.lat[ip] != lat1:
                    lon1, lat1 = self.lon[ip], self.lat[ip]
                    out.append([ip, 0, geo2cart(0.0, lon1, lat1), lat1])
                out[-1][1] += 1
            self._tables[key] = out
        return self._tables[key]


def profile_table(atm_rows):
    """The profiles of a whole atmosphere by rule 2 (a profile: a run of equal time stamp, longitude and latitude; a
    block: a run of equal time stamps) -> lists first, len, x1, block_of; ValueError with upstream's words."""
    a, first, length, x1, block_of = atm_rows, [], [], [], []
    block, start = 0, 0
    for i in range(1, a.np + 1):
        if i == a.np or a.time[i] != a.time[i - 1] or a.lon[i] != a.lon[i - 1] or a.lat[i] != a.lat[i - 1]:
            if i - start <= 1:
                raise ValueError("Cannot identify profiles. Check ordering of data points!")
            same = start > 0 and a.time[start] == a.time[start - 1]
            if start > 0 and not same:
                block += 1
            if same and abs(a.lat[start - 1] - a.lat[start]) > 10:
                raise ValueError("Distance of profiles is too large!")
            first.append(start); length.append(i - start); x1.append(geo2cart(0.0, a.lon[start], a.lat[start])); block_of.append(block)
            start = i
    return first, length, x1, block_of


def weights(table, lon0, lat0):
    """jurassic.c:731-755 -> (ix0, ix1, r, dhmin0, dhmin1)"""
    dhmin0 = dhmin1 = 1e99
    ix0 = ix1 = 0
    x0 = geo2cart(0.0, lon0, lat0)
    for ix, (_, _, x1, lat1) in enumerate(table):
        if abs(lat0 - lat1) <= 10:
            dh = dist2(x0, x1)
            if dh <= dhmin0:
                dhmin1, ix1, dhmin0, ix0 = dhmin0, ix0, dh, ix
            elif dh <= dhmin1:
                dhmin1, ix1 = dh, ix
    x2 = dist2(table[ix0][2], table[ix1][2])
    x = math.sqrt(x2)
    r0 = div(dhmin0 - dhmin1 + x2, 2 * x)
    r1 = x - r0
    if r0 <= 0:
        r = 0.0
    else:
        r = 1.0 if r1 <= 0 else div(r0, r0 + r1)
    return ix0, ix1, r, dhmin0, dhmin1


def interp_1d(a, first, n, z0, want_qk=True):
    """intpol_atm_1d on points [first, first + n) -> (p, t, q[], k[])"""
    ip = first + locate(a.z, first, n, z0)
    za, zb = a.z[ip], a.z[ip + 1]
    p = eip(za, a.p[ip], zb, a.p[ip + 1], z0)
    t = lip(za, a.t[ip], zb, a.t[ip + 1], z0)
    if not want_qk:
        return p, t, None, None
    q = [lip(za, y[ip], zb, y[ip + 1], z0) for y in a.q]
    k = [lip(za, y[ip], zb, y[ip + 1], z0) for y in a.k]
    return p, t, q, k


def interp_2d(a, a0, n, z0, lon0, lat0, want_qk=True):
    """intpol_atm_2d on the block [a0, a0 + n) -> (p, t, q[], k[])"""
    table = a.profiles(a0, n)
    ix0, ix1, r, _, _ = weights(table, lon0, lat0)
    p0, t0, q0, k0 = interp_1d(a, table[ix0][0], table[ix0][1], z0, want_qk)
    p1, t1, q1, k1 = interp_1d(a, table[ix1][0], table[ix1][1], z0, want_qk)

    def mix(y0, y1):
        return (1 - r) * y0 + r * y1
    if not want_qk:
        return mix(p0, p1), mix(t0, t1), None, None
    return mix(p0, p1), mix(t0, t1), [mix(u, v) for u, v in zip(q0, q1)], [mix(u, v) for u, v in zip(k0, k1)]


def refractivity(p, t):
    return div(7.753e-05 * p, t)


def tangent_point(los, npts, ip):
    """jr_common.h:502-539 on records (z, lon, lat, ds raw)"""
    if ip <= 0 or ip >= npts - 1:
        return [los[npts - 1]["z"], los[npts - 1]["lon"], los[npts - 1]["lat"]]
    yy0, yy1, yy2 = los[ip - 1]["z"], los[ip]["z"], los[ip + 1]["z"]
    ds0, ds1 = los[ip]["ds"], los[ip + 1]["ds"]
    dyy10, dyy21 = yy1 - yy0, yy2 - yy1

    def sq(v):
        return math.sqrt(v) if v >= 0 else math.nan
    x1 = sq(ds0 * ds0 - dyy10 * dyy10)
    x2 = x1 + sq(ds1 * ds1 - dyy21 * dyy21)
    dx12 = x1 - x2
    a = div(dyy10 * x2 + (yy0 - yy2) * x1, x1 * x2 * dx12)
    b = div(dyy10, x1) - a * x1
    c = yy0
    x = div(-b, 2 * a)
    tpz = (a * x + b) * x + c
    v0 = geo2cart(los[ip - 1]["z"], los[ip - 1]["lon"], los[ip - 1]["lat"])
    v2 = geo2cart(los[ip + 1]["z"], los[ip + 1]["lon"], los[ip + 1]["lat"])
    v = [lip(0.0, v0[i], x2, v2[i], x) for i in range(3)]
    _, tplon, tplat = cart2geo(v)
    return [tpz, tplon, tplat]


def traceray(ctl, a, geom7, two_d):
    """traceray (jr_common.h:585-711) on the rows `a` (an Atm).  two_d: the point rule, False intpol_atm_1d on the ray's
    block, True intpol_atm_2d on it.  -> dict(np, z, lon, lat, p, t, ds, k (nw lists), q, u (ng lists), tsurf, tp), as
    orc.traceray returns them (arrays).  Under the 2-D rule a block that is not made of whole profiles of the
    atmosphere's table is not entered (np = 0)."""
    time, obsz, obslon, obslat, vpz, vplon, vplat = [float(v) for v in geom7]
    ng, nw = a.ng, a.nw
    tsurf, tp = -999.0, [vpz, vplon, vplat]
    los = []

    def result():
        n = len(los)
        out = {f: np.array([pt[f] for pt in los]) for f in ("z", "lon", "lat", "p", "t", "ds")}
        out["k"] = np.array([[pt["k"][w] for pt in los] for w in range(nw)]).reshape(nw, n)
        out["q"] = np.array([[pt["q"][g] for pt in los] for g in range(ng)]).reshape(ng, n)
        out["u"] = np.array([[pt["u"][g] for pt in los] for g in range(ng)]).reshape(ng, n)
        out.update(np=n, tsurf=tsurf, tp=np.array(tp))
        return out

    a0, n = a.block(time)
    zmin, zmax = a.altitude_range(a0, n)
    if obsz < zmin or vpz > zmax - 0.001 or zmin == zmax:
        return result()
    if two_d:
        first, length, _, _ = profile_table(a)
        ends = {f + l for f, l in zip(first, length)}
        if a0 not in first or (a0 + n) not in ends:
            return result()

    def point(z, lon, lat, want_qk):
        return interp_2d(a, a0, n, z, lon, lat, want_qk) if two_d else interp_1d(a, a0, n, z, want_qk)

    xobs, xvp = geo2cart(obsz, obslon, obslat), geo2cart(vpz, vplon, vplat)
    ex0 = [xvp[i] - xobs[i] for i in range(3)]
    nrm = norm(ex0)
    ex0 = [div(v, nrm) for v in ex0]
    x = list(xobs)
    if obsz > zmax:
        dmax, dmin = nrm, 0.0
        while abs(dmin - dmax) > 0.001:
            d = 0.5 * (dmax + dmin)
            x = [xobs[i] + d * ex0[i] for i in range(3)]
            z = norm(x) - RE
            if z <= zmax and z > zmax - 0.001:
                break
            if z < zmax - 0.0005:
                dmax = d
            else:
                dmin = d
    z_low, z_low_idx = 1e99, -1
    stop, done = 0, False
    for npi in range(NLOS):
        ds, dz = ctl.rayds, ctl.raydz
        if dz > 0.0:
            norm_x = div(1.0, norm(x))
            dot = 0.0
            for i in range(3):
                dot += ex0[i] * x[i] * norm_x
            cosa = abs(dot)
            if cosa != 0.0:
                ds = min(ds, div(dz, cosa))
        z, lon, lat = cart2geo(x)
        if z < zmin or z > zmax:
            stop = 2 if z < zmin else 1
            if npi > 0:
                pv = los[npi - 1]
                xh = geo2cart(pv["z"], pv["lon"], pv["lat"])
                zfrac = zmin if z < zmin else zmax
                frac = div(zfrac - pv["z"], z - pv["z"])
                x = [xh[i] + frac * (x[i] - xh[i]) for i in range(3)]
                z, lon, lat = cart2geo(x)
                pv["ds"] = ds * frac
            ds = 0.0
        p, t, q, k = point(z, lon, lat, True)
        los.append(dict(z=z, lon=lon, lat=lat, p=p, t=t, q=q, k=k, ds=ds))
        if z < z_low:
            z_low, z_low_idx = z, npi
        if stop:
            tsurf = t if stop == 2 else -999.0
            done = True
            break
        nref, ngr = 1.0, [0.0, 0.0, 0.0]
        if ctl.refrac and z <= 60.0:
            nref += refractivity(p, t)
            xh = [x[i] + 0.5 * ds * ex0[i] for i in range(3)]
            zz, llon, llat = cart2geo(xh)
            pp, tt, _, _ = point(zz, llon, llat, False)
            n2 = refractivity(pp, tt)
            for i in range(3):
                h = 0.02
                xh[i] += h
                zz, llon, llat = cart2geo(xh)
                pp, tt, _, _ = point(zz, llon, llat, False)
                ngr[i] = div(refractivity(pp, tt) - n2, h)
                xh[i] -= h
        ex1 = [ex0[i] * nref + ds * ngr[i] for i in range(3)]
        norm_ex1 = norm(ex1)
        for i in range(3):
            ex1[i] = div(ex1[i], norm_ex1)
            x[i] += 0.5 * ds * (ex0[i] + ex1[i])
            ex0[i] = ex1[i]
    assert done, "Too many LOS points!"
    npts = len(los)
    tp = tangent_point(los, npts, z_low_idx)
    for ip in range(npts - 1, 0, -1):
        los[ip]["ds"] = 0.5 * (los[ip - 1]["ds"] + los[ip]["ds"])
    los[0]["ds"] *= 0.5
    for pt in los:
        pt["u"] = [div(10.0 * pt["q"][g] * pt["p"], BOLTZMANN * pt["t"]) * pt["ds"] for g in range(ng)]
    return result()


def formod(orc, case, geom=None, atm=None, two_d=True, tables=None, records=None):
    """Forward model of the rays geom (default: the case's) on the Python tracer -> dict(rad, tau (nr, nd), tp (nr, 3),
    np, records).  case.ctl.formod chooses the band model: 2 orc.ega_eps along the path (apply_ega_core), 1 the
    Curtis-Godson rule of tests/cga_model.py fed these LOS records.  records: traced already (a list, one per ray)."""
    ctl = case.ctl
    ctl2 = ega_ctl(ctl)
    atm = case.atm if atm is None else atm
    geom = case.geom if geom is None else np.asarray(geom, dtype=np.float64)
    tables = case.oracle_tables(orc) if tables is None else tables
    pairs = pairs_of(case) if ctl.formod == 1 else None
    rows = Atm(atm, ctl)
    ng, nd = ctl.ng, ctl.nd
    ig_co2, ig_h2o, fourbit = continua_config(ctl2)
    nr = len(geom)
    rad, tau = np.zeros((nr, nd)), np.ones((nr, nd))
    tp, npts, recs = np.zeros((nr, 3)), np.zeros(nr, dtype=np.int32), []
    for ir, g in enumerate(geom):
        tr = records[ir] if records is not None else traceray(ctl, rows, g, two_d)
        recs.append(tr)
        n = int(tr["np"])
        npts[ir], tp[ir] = n, tr["tp"]
        p, t, ds = tr["p"].tolist(), tr["t"].tolist(), tr["ds"].tolist()
        for d in range(nd):
            nu = ctl.nu[d]
            r_d, t_d = np.zeros(1), np.ones(1)
            if n:
                u_co2 = tr["u"][ig_co2] if ig_co2 >= 0 else np.zeros(n)
                u_h2o = tr["u"][ig_h2o] if ig_h2o >= 0 else np.zeros(n)
                q_h2o = tr["q"][ig_h2o] if ig_h2o >= 0 else np.zeros(n)
                ctm = orc.continua(nu, tr["p"], tr["t"], q_h2o, u_co2, u_h2o)
            if ctl.formod == 1:
                paths = [path_tau(pairs.get((ig, d)), p, t, tr["u"][ig].tolist()) for ig in range(ng)]
            tau_path = [1.0] * ng
            pprev = 1.0
            for ip in range(n):
                beta_ds = float(tr["k"][ctl.window[d]][ip]) * ds[ip]
                if fourbit & 8:
                    beta_ds += float(ctm[0][ip])
                if fourbit & 4:
                    beta_ds += float(ctm[1][ip])
                if fourbit & 2:
                    beta_ds += float(ctm[2][ip]) * ds[ip]
                if fourbit & 1:
                    beta_ds += float(ctm[3][ip]) * ds[ip]
                if ctl.formod == 1:
                    pcur = 1.0
                    for ig in range(ng):
                        pcur *= paths[ig][ip]
                    tau_gas = div(pcur, pprev) if pprev > 1e-280 else 0.0
                    pprev = pcur
                else:                                       # apply_ega_core (jr_common.h:270-280)
                    tau_gas = 1.0
                    for ig in range(ng):
                        eps = float(orc.ega_eps(tables, ig, d, [tau_path[ig]], [t[ip]], [float(tr["u"][ig][ip])], [p[ip]])[0])
                        tau_path[ig] *= eps
                        tau_gas *= eps
                r_d, t_d, _ = orc.new_obs(tables, d, [t[ip]], [tau_gas], [beta_ds], r_d, t_d)
            r_d = orc.epilogue(tables, d, nu, [tr["tsurf"]], [ctl.write_bbt], r_d, t_d)
            rad[ir, d], tau[ir, d] = r_d[0], t_d[0]
    return dict(rad=rad, tau=tau, tp=tp, np=npts, records=recs)


# ---- the test atmosphere and rays (tests/test_track_cpu.py, tests/test_track_gpu.py) -----------------------------------
TRACK_LATS = (-3.0, -1.0, 1.0, 3.0)


def track_atmosphere(ctl, base, lats=TRACK_LATS, graded=True, thinned=2, second_block=True, order=None):
    """One time block (time 0) holding a track of len(lats) profiles on the meridian lon = 0, each the first profile of
    `base` (an atm_t with common.extinction_profile applied); graded: profile i has T + 2 i K, p (1 + 0.01 i), gas 2
    scaled by 1 + 0.2 i and the extinction by 1 + 0.5 i.  Profile `thinned` (None: none) loses every other level above
    60 km.  order: the profiles are listed in this order (default as lats).  second_block: one more profile at time 1,
    lat 0.5, T + 5 K.  -> atm_t"""
    n = base.np
    src = {f: np.ctypeslib.as_array(getattr(base, f))[:n].copy() for f in ("z", "p", "t")}
    q, k = np.ctypeslib.as_array(base.q)[:, :n].copy(), np.ctypeslib.as_array(base.k)[:, :n].copy()
    out = abi.atm_t()
    at = 0

    def put(time, lat, keep, dt, fp, fq, fk):
        nonlocal at
        m = int(keep.sum())
        s = slice(at, at + m)
        np.ctypeslib.as_array(out.time)[s] = time
        np.ctypeslib.as_array(out.lon)[s] = 0.0
        np.ctypeslib.as_array(out.lat)[s] = lat
        np.ctypeslib.as_array(out.z)[s] = src["z"][keep]
        np.ctypeslib.as_array(out.p)[s] = src["p"][keep] * fp
        np.ctypeslib.as_array(out.t)[s] = src["t"][keep] + dt
        qq = q[:, keep].copy()
        if ctl.ng > 2:
            qq[2] *= fq
        np.ctypeslib.as_array(out.q)[:, s] = qq
        np.ctypeslib.as_array(out.k)[:, s] = k[:, keep] * fk
        at += m

    every = np.ones(n, dtype=bool)
    thin = every.copy()
    above = np.flatnonzero(src["z"] > 60.0)
    thin[above[::2]] = False
    for i in (range(len(lats)) if order is None else order):
        g = float(i) if graded else 0.0
        put(0.0, lats[i], thin if (thinned is not None and i == thinned) else every, 2.0 * g, 1.0 + 0.01 * g, 1.0 + 0.2 * g, 1.0 + 0.5 * g)
    if second_block:
        put(1.0, 0.5, every, 5.0, 1.0, 1.0, 1.0)
    out.np = at
    return out


def limb_ray(h, vplat=0.3, obsz=780.0, time=0.0):
    """A limb ray along the meridian lon = 0 whose geometric tangent point (altitude h) lies at latitude vplat, seen
    from the south."""
    return [time, obsz, 0.0, vplat - RAD2GRD * math.acos((RE + h) / (RE + obsz)), h, 0.0, vplat]


def track_rays():
    """The fixed ray set, 14 rays: 8 limb rays from -5 to 60 km whose paths cross the track, nadir rays at -2.2, 0.4 and
    5.0 degrees (the last beyond the track's end), an observer inside the atmosphere looking north and upwards, and a
    limb and a nadir ray of the second block."""
    g = [limb_ray(h) for h in np.linspace(-5.0, 60.0, 8)]
    g += [[0.0, 700.0, 0.0, lat, 0.0, 0.0, lat] for lat in (-2.2, 0.4, 5.0)]
    g.append([0.0, 20.0, 0.0, -2.5, 45.0, 0.0, 2.0])
    g += [limb_ray(12.0, time=1.0), [1.0, 700.0, 0.0, 0.4, 0.0, 0.0, 0.4]]
    return np.array(g, dtype=np.float64)


LIMB_CROSSING = list(range(8))       # rows of track_rays()
NADIR_BEYOND = 10
SECOND_BLOCK = [12, 13]
