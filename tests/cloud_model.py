"""CPU model of the point-cloud atmosphere along the line of sight (IP 3) -- a helper of tests/test_cloud_cpu.py and
tests/test_cloud_gpu.py, no tests in it.

The rule stands in include/jurassic_hip.h (IP 3).  Restated here in IEEE doubles, one rounding per operation:

  Cloud        the rows of an atm_t (track_model.Atm) with the cached positions x1 = geo2cart(0, lon, lat), the
               influence lengths and the whole-slice altitude range (rule 2);
  mean_3d      intpol_atm_3d (jurassic.c:763-804) on the points of ONE time block (rule 4): the gates and the weights
               element by element (numpy's subtract, multiply, divide and abs round once each, as C's do), the sums in
               ascending index in Python floats;
  traceray     track_model.traceray with a third point rule: the SAME code object, run with mean_3d in the place of
               interp_2d and a profile check that accepts the ray's block as it is;
  formod       track_model.formod on these LOS records.

tests/test_cloud_cpu.py pins mean_3d to orc.intpol_atm under ip = 3 and the tracer's 1-D rule to orc.traceray, bit for
bit."""
import math
import types
import numpy as np
from jurassic_hip import abi
import track_model as T

CX, CZ = 1500.0, 3.0             # km: see cloud_case -- the issue's 150 km leaves the fixed rays in holes
CLOUD_LATS = (-0.75, -0.25, 0.25, 0.75)
RAYS8 = [0, 2, 4, 7, 8, 11, 12, 13]     # rows of track_model.track_rays(): 4 limb, 1 nadir, observer inside, 2 of block B
BLOCK_A, BLOCK_B = [0, 1, 2, 3, 4, 5], [6, 7]       # rows of RAYS8


class Cloud(T.Atm):
    def __init__(self, atm, ctl):
        super().__init__(atm, ctl)
        self.cx, self.cz = float(ctl.cx), float(ctl.cz)
        self.x1 = [T.geo2cart(0.0, lo, la) for lo, la in zip(self.lon, self.lat)]
        self.Z, self.LAT, self.X1 = np.array(self.z), np.array(self.lat), np.array(self.x1).reshape(self.np, 3)
        self.rows = [self.p, self.t] + self.q + self.k
        self.wsum_min, self.evals, self.last = math.inf, 0, None

    def block(self, time):
        self.last = super().block(time)
        return self.last

    def altitude_range(self, a0, n):
        """rule 2: all points of the slice, ascending index"""
        zmin = zmax = self.z[a0]
        for ip in range(a0, a0 + n):
            zmax, zmin = max(zmax, self.z[ip]), min(zmin, self.z[ip])
        return zmin, zmax


def weights_3d(a, a0, n, z0, lat0, x0):
    """The gates and weights of rule 4 on the points [a0, a0 + n) -> (indices that contribute, ascending; their w)"""
    s = slice(a0, a0 + n)
    rm2 = a.cx * a.cx
    dz = np.abs(a.Z[s] - z0)
    b = x0 - a.X1[s]
    dx2 = b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1] + b[:, 2] * b[:, 2]
    with np.errstate(invalid="ignore"):
        skip = (dz >= a.cz) | (np.abs(a.LAT[s] - lat0) * 111.13 >= a.cx) | (dx2 >= rm2)
        w = (1 - dz / a.cz) * (rm2 - dx2) / (rm2 + dx2)
    idx = np.flatnonzero(~skip)
    return (idx + a0).tolist(), w[idx].tolist()


def mean_3d(a, a0, n, z0, lon0, lat0, want_qk=True, x0=None):
    """intpol_atm_3d on the block [a0, a0 + n) -> (p, t, q[], k[]); x0: the position after the geometry step, if the
    caller has it (default geo2cart(0, lon0, lat0))."""
    x0 = np.array(T.geo2cart(0.0, lon0, lat0) if x0 is None else x0, dtype=np.float64)
    idx, w = weights_3d(a, a0, n, z0, lat0, x0)
    rows = a.rows if want_qk else a.rows[:2]
    y = [0.0] * len(rows)
    wsum = 0.0
    for ip, wi in zip(idx, w):
        wsum += wi
        for r, row in enumerate(rows):
            y[r] += wi * row[ip]
    a.wsum_min, a.evals = min(a.wsum_min, wsum), a.evals + 1
    y = [T.div(v, wsum) for v in y] if wsum >= 1e-6 else [math.nan] * len(rows)
    if not want_qk:
        return y[0], y[1], None, None
    return y[0], y[1], y[2:2 + a.ng], y[2 + a.ng:]


def _ray_block(a):
    """In the place of track_model.profile_table: the block the tracer has just located is taken as it is."""
    return [a.last[0]], [a.last[1]], None, None


# the names the swap relies on: track_model.traceray must look BOTH up as globals, or this model would run another rule
assert "interp_2d" in T.traceray.__code__.co_names + tuple(n for c in T.traceray.__code__.co_consts if isinstance(c, types.CodeType)
                                                           for n in c.co_names), "track_model.traceray no longer calls interp_2d"
assert "profile_table" in T.traceray.__code__.co_names, "track_model.traceray no longer calls profile_table"
_traceray_3d = types.FunctionType(T.traceray.__code__, dict(vars(T), interp_2d=mean_3d, profile_table=_ray_block), "traceray_3d",
                                  T.traceray.__defaults__, T.traceray.__closure__)


def traceray(ctl, a, geom7, rule=3):
    """track_model.traceray on the rows `a` (a Cloud): rule 3 the mean over the ray's block at every point and probe,
    rule 1 intpol_atm_1d on it."""
    return _traceray_3d(ctl, a, geom7, True) if rule == 3 else T.traceray(ctl, a, geom7, False)


def formod(orc, case, geom=None, atm=None, records=None, rows=None):
    atm = case.atm if atm is None else atm
    geom = case.geom if geom is None else np.asarray(geom, dtype=np.float64)
    if records is None:
        rows = Cloud(atm, case.ctl) if rows is None else rows
        records = [traceray(case.ctl, rows, g) for g in geom]
    return T.formod(orc, case, geom=geom, atm=atm, records=records)


# ---- the test clouds ------------------------------------------------------------------------------------------------------
def make_atm(time, z, lon, lat, p, t, q, k):
    out = abi.atm_t()
    n = len(z)
    for f, v in (("time", time), ("z", z), ("lon", lon), ("lat", lat), ("p", p), ("t", t)):
        np.ctypeslib.as_array(getattr(out, f))[:n] = v
    np.ctypeslib.as_array(out.q)[:q.shape[0], :n] = q
    np.ctypeslib.as_array(out.k)[:k.shape[0], :n] = k
    out.np = n
    return out


def columns(ctl, base, lats, seed, time=0.0, dt=0.0, keep=None, jitter=True, npoints=None):
    """The first profile of `base` copied to len(lats) columns on the meridian lon = 0 (column i: T + 2 i K + dt, the
    extinction scaled by 1 + 0.5 i), every point moved by a seeded +-0.2 km in z and +-0.05 degrees in longitude and
    latitude: no two points share a column.  keep(z): which points stay; npoints: cut to that many.  -> dict of rows"""
    n = base.np
    src = {f: np.ctypeslib.as_array(getattr(base, f))[:n].copy() for f in ("z", "p", "t")}
    q, k = np.ctypeslib.as_array(base.q)[:ctl.ng, :n].copy(), np.ctypeslib.as_array(base.k)[:max(ctl.nw, 1), :n].copy()
    rng = np.random.default_rng(seed)
    m = len(lats)
    z = np.tile(src["z"], m)
    lon, lat = np.zeros(m * n), np.repeat(np.asarray(lats, dtype=np.float64), n)
    if jitter:
        z = z + rng.uniform(-0.2, 0.2, m * n)
        lon = lon + rng.uniform(-0.05, 0.05, m * n)
        lat = lat + rng.uniform(-0.05, 0.05, m * n)
    col = np.repeat(np.arange(m, dtype=np.float64), n)
    rows = dict(time=np.full(m * n, time), z=z, lon=lon, lat=lat, p=np.tile(src["p"], m), t=np.tile(src["t"], m) + 2.0 * col + dt,
                q=np.tile(q, (1, m)), k=np.tile(k, (1, m)) * (1.0 + 0.5 * col))
    sel = np.ones(m * n, dtype=bool) if keep is None else keep(z)
    if npoints is not None:
        sel &= np.arange(m * n) < npoints
    return {f: (v[:, sel] if v.ndim == 2 else v[sel]) for f, v in rows.items()}


def join(*blocks):
    return make_atm(*[np.concatenate([b[f] for b in blocks], axis=-1) for f in ("time", "z", "lon", "lat", "p", "t", "q", "k")])


def cloud_atmosphere(ctl, base, second_block=True, lats=CLOUD_LATS, keep=None, npoints=None):
    """Block A (time 0): 4 jittered columns 0.5 degrees apart.  Block B (time 1): a different, smaller cloud -- 2 columns,
    another seed, T + 5 K."""
    blocks = [columns(ctl, base, lats, seed=5, keep=keep, npoints=npoints)]
    if second_block:
        blocks.append(block_b(ctl, base))
    return join(*blocks)


def block_b(ctl, base, time=1.0):
    return columns(ctl, base, (0.2, 0.7), seed=6, time=time, dt=5.0)
