"""Point-cloud atmosphere along the line of sight (IP 3) on the device: jur_cloud_trace_kernel behind the entries, against
the CPU model of tests/cloud_model.py (which tests/test_cloud_cpu.py pins to the oracle bit for bit).

Atmosphere: block A, four columns 0.5 degrees of latitude apart whose 364 points are each moved by a seeded +-0.2 km and
+-0.05 degrees, and block B, a smaller cloud of two columns at another time stamp.  Rays: eight of
track_model.track_rays() (cloud_model.RAYS8).  cx = 1500 km, cz = 3 km: tests/test_cloud_cpu.py asserts that no
evaluation of these rays comes within a factor 1000 of the rule's wsum threshold.  Bounds are the suite's own:
radiances 1e-9 relative, transmittances 1e-9 relative plus common.tau_atol, LOS records the scaled deviation and bound
of tests/losrecords.py with the yardstick taken from the CPU model.  Every test here fails at model creation on a
library that refuses IP 3."""
import ctypes as C
import math
import numpy as np
import pytest
import common
import cga_model as M
import cloud_model as CM
import losrecords as L
import track_model as T
from jurassic_hip import abi
from test_cloud_cpu import cloud_case
from test_track_cpu import same_doubles

pytestmark = pytest.mark.gpu
RTOL = 1e-9
FIELDS4 = ("rad", "tau", "tp", "np")
LOSF = ("p", "t", "ds", "qh2o", "k", "u", "np", "tsurf", "tp")


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def copy_atm(a):
    out = abi.atm_t()
    C.memmove(C.byref(out), C.byref(a), C.sizeof(abi.atm_t))
    return out


def with_ctl(case, **kw):
    c = abi.ctl_t()
    C.memmove(C.byref(c), C.byref(case.ctl), C.sizeof(abi.ctl_t))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def run(hip, case, atm=None, geom=None, ctl=None, arith="fast", what="formod_host"):
    m = hip.Model(case.ctl if ctl is None else ctl, case.lib_tables())
    try:
        m.set_arithmetic(hip.ARITH_EXACT if arith == "exact" else hip.ARITH_FAST)
        m.set_atm(case.atm if atm is None else atm)
        return getattr(m, what)(case.geom if geom is None else geom)
    finally:
        m.close()


def assert_parity(out, ref, what="", rows=None):
    """Device against model on the rays `rows` (default all): equal point counts, the suite's tolerances."""
    rows = slice(None) if rows is None else rows
    o, r = {f: out[f][rows] for f in FIELDS4}, {f: ref[f][rows] for f in FIELDS4}
    assert np.array_equal(o["np"], r["np"]), (what, o["np"], r["np"])
    fin = np.isfinite(r["rad"])
    assert fin.all() and np.array_equal(fin, np.isfinite(o["rad"])), what
    rerr = common.rel_err(o["rad"], r["rad"])
    terr = np.abs(o["tau"] - r["tau"])
    allow = RTOL * np.abs(r["tau"]) + common.tau_atol(r["tau"])
    print("IP 3 %s: worst rel radiance error %.3e, worst |dtau| / allowance %.3e, worst |dtp| %.3e"
          % (what, rerr.max(), (terr / allow).max(), np.abs(o["tp"] - r["tp"]).max()))
    assert rerr.max() < RTOL, (what, rerr.max())
    assert np.all(terr <= allow), (what, terr.max())
    assert np.abs(o["tp"] - r["tp"]).max() < 1e-9, what


@pytest.fixture(scope="module")
def reference(oracle):
    """The CPU model's LOS records and forward results, computed once: name -> (case, formod dict)."""
    cache = {}

    def get(name):
        if name not in cache:
            base = dict(refrac1={}, refrac0=dict(refrac=0), bbt=dict(write_bbt=1), cga=dict(formod=1))[name]
            case = cloud_case(**base)
            records = cache["refrac1"][1]["records"] if name in ("bbt", "cga") else None     # the tracer sees neither switch
            cache[name] = (case, CM.formod(oracle, case, records=records))
        return cache[name]
    get("refrac1")
    return get


# ---- 1. the mean at a position, bit for bit -------------------------------------------------------------------------------
def edge_cloud(case, npoints):
    """Block-A columns cut to npoints - 3 points, then three isolated parcels on the axis lon = lat = 0 at 200, 300 and
    400 km: nothing else lies within cz of them, and the last one is the slice's last point."""
    cols = CM.columns(case.ctl, case.base, tuple(-0.75 + 0.5 * i for i in range(12)), seed=5, npoints=npoints - 3)
    lone = CM.columns(case.ctl, case.base, (0.0, 0.0, 0.0), seed=5, jitter=False, npoints=3 * case.base.np)
    pick = [40, case.base.np + 41, 2 * case.base.np + 42]
    lone = {f: (v[:, pick] if v.ndim == 2 else v[pick]) for f, v in lone.items()}
    lone["z"] = np.array([200.0, 300.0, 400.0])
    return CM.join(cols, lone)


@pytest.mark.parametrize("size", ["staged", "global"])
def test_mean_at_positions_bit_for_bit(hip, size):
    """jur_kat_cloud_mean against mean_3d: positions through the cloud and the constructed edges.  cx = 128 km, a power
    of two: x1 + 128 and the difference back are exact, so dx2 == rm2 can be met exactly."""
    case = cloud_case(cx=128.0, cz=3.0)
    npts = 367 if size == "staged" else hip.cloud_lds_points() + 1
    atm = edge_cloud(case, npts)
    assert atm.np == npts
    a = CM.Cloud(atm, case.ctl)
    i200, i300, ilast = npts - 3, npts - 2, npts - 1
    cx, cz = a.cx, a.cz
    rng = np.random.default_rng(21)
    pos = []                                                # (z0, lat0, x0, name)

    def at(z0, lon0, lat0, name="", x0=None):
        pos.append((float(z0), float(lat0), list(T.geo2cart(0.0, lon0, lat0)) if x0 is None else list(x0), name))
    for _ in range(150):
        at(rng.uniform(-1.0, 91.0), rng.uniform(-0.3, 0.3), rng.uniform(-2.2, 2.2))
    for ip in rng.integers(0, npts - 3, 20):                # exactly on a parcel
        at(a.z[ip], a.lon[ip], a.lat[ip])
    # dz == cz exactly, and one ulp inside
    at(203.0, 0.0, 0.0, "dz==cz")
    at(np.nextafter(203.0, 0.0), 0.0, 0.0, "dz<cz")
    # dx2 == rm2 exactly: the parcel at x0 - (cx, 0, 0); one ulp inside
    x1 = a.x1[i200]
    assert (x1[0] + cx) - x1[0] == cx
    at(200.5, 0.0, 0.0, "dx2==rm2", x0=[x1[0] + cx, x1[1], x1[2]])
    at(200.5, 0.0, 0.0, "dx2<rm2", x0=[np.nextafter(x1[0] + cx, 0.0), x1[1], x1[2]])
    # the latitude gate exactly met: |0 - lat0| * 111.13 == cx, and the next double inside
    dlat = cx / 111.13
    while dlat * 111.13 >= cx:
        dlat = np.nextafter(dlat, 0.0)
    inside = dlat
    dlat = np.nextafter(dlat, np.inf)
    assert dlat * 111.13 == cx and inside * 111.13 < cx
    pos.append((300.5, -float(dlat), list(a.x1[i300]), "lat==cx"))
    pos.append((300.5, -float(inside), list(a.x1[i300]), "lat<cx"))
    # wsum just below and just above 1e-6: one parcel right below the position, w = 1 - dz / cz
    for name, f in (("wsum<1e-6", 0.999), ("wsum>1e-6", 1.001)):
        pos.append((300.0 + cz * (1.0 - 1e-6 * f), 0.0, list(a.x1[i300]), name))
    # only the last point of the slice contributes
    pos.append((401.0, 0.0, list(a.x1[ilast]), "last"))
    z0, lat0 = np.array([p[0] for p in pos]), np.array([p[1] for p in pos])
    x0 = np.array([p[2] for p in pos])
    names = [p[3] for p in pos]
    want = np.array([[v for part in CM.mean_3d(a, 0, npts, z0[i], None, lat0[i], True, x0[i])
                      for v in (part if isinstance(part, list) else [part])] for i in range(len(pos))]).T
    took = {n: CM.weights_3d(a, 0, npts, z0[i], lat0[i], x0[i])[0] for i, n in enumerate(names) if n}
    assert took["dz==cz"] == [] and took["dz<cz"] == [i200]
    assert took["dx2==rm2"] == [] and took["dx2<rm2"] == [i200]
    assert took["lat==cx"] == [] and took["lat<cx"] == [i300]
    assert took["wsum<1e-6"] == [i300] and took["wsum>1e-6"] == [i300] and took["last"] == [ilast]
    k = {n: i for i, n in enumerate(names) if n}
    assert np.isnan(want[:, k["wsum<1e-6"]]).all() and np.isfinite(want[:, k["wsum>1e-6"]]).all()
    assert np.isnan(want[:, k["dz==cz"]]).all() and np.isfinite(want[:, k["last"]]).all()
    assert np.isfinite(want[0, :150]).sum() > 100
    m = hip.Model(case.ctl, case.lib_tables())
    try:
        m.set_atm(atm)
        got = m.kat_cloud_mean(0, npts, z0, lat0, x0)
        with pytest.raises(hip.JurassicError, match="kat_cloud_mean"):
            m.kat_cloud_mean(1, npts, z0, lat0, x0)
    finally:
        m.close()
    assert got.shape == want.shape == (2 + case.ctl.ng + 1, len(pos))
    for r in range(want.shape[0]):
        assert same_doubles(got[r], want[r]), (r, [names[i] for i in np.flatnonzero(~((got[r] == want[r]) | (np.isnan(got[r]) & np.isnan(want[r]))))])


def test_mean_on_a_slice_that_does_not_start_the_atmosphere(hip):
    """Block B of the two-block cloud, points [364, 546): the staged columns are indexed from the slice's first point."""
    case = cloud_case()
    a = CM.Cloud(case.atm, case.ctl)
    a0, n = 364, 182
    assert a.block(1.0) == (a0, n)
    rng = np.random.default_rng(22)
    z0, lon0, lat0 = rng.uniform(-1.0, 91.0, 64), rng.uniform(-0.3, 0.3, 64), rng.uniform(-2.0, 3.0, 64)
    x0 = np.array([T.geo2cart(0.0, lo, la) for lo, la in zip(lon0.tolist(), lat0.tolist())])
    want = np.array([[v for part in CM.mean_3d(a, a0, n, z0[i], None, lat0[i], True, x0[i])
                      for v in (part if isinstance(part, list) else [part])] for i in range(64)]).T
    other = np.array([CM.mean_3d(a, 0, a0, z0[i], None, lat0[i], True, x0[i])[1] for i in range(64)])
    assert np.isfinite(want).all() and not same_doubles(want[1], other)
    m = hip.Model(case.ctl, case.lib_tables())
    try:
        m.set_atm(case.atm)
        got = m.kat_cloud_mean(a0, n, z0, lat0, x0)
    finally:
        m.close()
    for r in range(want.shape[0]):
        assert same_doubles(got[r], want[r]), r


# ---- 2. LOS records ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refrac", [1, 0])
def test_los_records_against_the_model(hip, reference, refrac):
    case, ref = reference("refrac%d" % refrac)
    rows = CM.Cloud(case.atm, case.ctl)
    base = ref["records"]
    use = np.ones(len(case.geom), dtype=bool)
    Y = {f: 0.0 for f in L.FIELDS}
    for i, g in enumerate(case.geom):                       # the yardstick of tests/losrecords.py, from the model
        near = [CM.traceray(case.ctl, rows, L._nudged(g, s)) for s in (+1, -1)]
        if any(t["np"] != base[i]["np"] for t in near):
            use[i] = False
            continue
        r0 = L.rows_of(case.ctl, dict(base[i], k=base[i]["k"][0]))
        for t in near:
            for f, v in L.scaled_deviation(r0, L.rows_of(case.ctl, dict(t, k=t["k"][0]))).items():
                Y[f] = max(Y[f], v)
    assert 8 * (~use).sum() <= len(use)
    m = hip.Model(case.ctl, case.lib_tables())
    try:
        m.set_atm(case.atm)
        out = m.kat_traceray(case.geom)
    finally:
        m.close()
    assert np.array_equal(out["np"], [b["np"] for b in base]), (out["np"], [b["np"] for b in base])
    assert out["np"].min() >= 2
    worst = {f: 0.0 for f in L.FIELDS}
    for i in np.flatnonzero(use):
        n = int(base[i]["np"])
        dev = L.scaled_deviation(L.rows_of(case.ctl, dict(base[i], k=base[i]["k"][0])), L.hook_rows(case.ctl, out, i, n))
        for f in L.FIELDS:
            worst[f] = max(worst[f], dev[f])
    for f in L.FIELDS:
        print("IP 3 LOS records refrac=%d field %s: scaled deviation %.3e, yardstick %.3e, bound %.3e" % (refrac, f, worst[f], Y[f], L.bound(Y[f])))
    for f in L.FIELDS:
        assert worst[f] <= L.bound(Y[f]), (f, worst[f], Y[f], L.bound(Y[f]))
    tsurf = np.array([b["tsurf"] for b in base])
    assert np.array_equal(tsurf > 0, out["tsurf"] > 0) and (tsurf > 0).any()
    hit = tsurf > 0
    assert np.abs(out["tsurf"][hit] - tsurf[hit]).max() < 1e-9 * 300
    assert np.abs(out["tp"] - np.array([b["tp"] for b in base])).max() < 1e-9


# ---- 3. radiances, transmittances, tangent points ------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_forward_model_against_the_model(hip, reference, arith):
    case, ref = reference("refrac1")
    assert_parity(run(hip, case, arith=arith), ref, "formod %s" % arith)
    assert np.any(ref["tau"] < 0.99) and np.all(ref["rad"] > 0)


def test_forward_model_in_brightness_temperatures(hip, reference):
    case, ref = reference("bbt")
    assert_parity(run(hip, case), ref, "write_bbt")
    assert np.all((ref["rad"] > 1.0) & (ref["rad"] < 350))        # kelvins, not radiances (those stay below 0.1)


def test_curtis_godson_band_model_in_the_cloud(hip, reference):
    """FORMOD 1 and IP 3 compose: tests/cga_model.py's rule fed the 3-D LOS records."""
    case, ref = reference("cga")
    assert_parity(run(hip, case), ref, "FORMOD 1")
    _, ega = reference("refrac1")
    assert not same_doubles(ref["rad"], ega["rad"])
    m = hip.Model(case.ctl, case.lib_tables())
    try:
        m.set_atm(case.atm)
        cg = m.curtis_godson(case.geom)                     # jur_curtis_godson_host runs on the same tracer
        rec = m.kat_traceray(case.geom)
    finally:
        m.close()
    assert np.array_equal(cg["np"], ref["np"])
    for i, n in enumerate(ref["np"]):
        for ig in range(case.ctl.ng):
            _, _, cgu = M.means(rec["p"][i, :n].tolist(), rec["t"][i, :n].tolist(), rec["u"][ig, i, :n].tolist())
            assert np.allclose(cg["cgu"][i, ig, :n], cgu, rtol=1e-12, atol=0), (i, ig)


# ---- 4. / 5. time blocks are separate; staged and global route give the same bits ------------------------------------------
def traced(hip, case, atm, geom):
    m = hip.Model(case.ctl, case.lib_tables())
    try:
        m.set_atm(atm)
        return m.formod_host(geom), m.kat_traceray(geom)
    finally:
        m.close()


def test_time_blocks_are_separate_and_routes_agree(hip):
    """Block A's rays on the two-block atmosphere, traced ALONE (the workgroup agrees on block A: staged), return the
    bits they return with block A uploaded alone -- a scan over the whole atmosphere would take block B's parcels in.
    The same rays in one launch with block B's (the workgroup disagrees: every lane reads the model's arrays) return
    those bits again.  And block B's rays the bits of block B alone."""
    case = cloud_case()
    ga, gb = case.geom[CM.BLOCK_A], case.geom[CM.BLOCK_B]
    only_a = CM.cloud_atmosphere(case.ctl, case.base, second_block=False)
    only_b = CM.join(CM.block_b(case.ctl, case.base))
    fa, la = traced(hip, case, only_a, ga)
    fb, lb = traced(hip, case, only_b, gb)
    f2, l2 = traced(hip, case, case.atm, ga)
    assert np.all(fa["np"] > 10) and np.all(fb["np"] > 10)
    for f in FIELDS4:
        assert same_doubles(f2[f], fa[f]), ("block A alone in the launch", f)
    for f in LOSF:
        assert same_doubles(l2[f], la[f]), ("block A alone in the launch", f)
    fb2, lb2 = traced(hip, case, case.atm, gb)              # block B alone in the launch: staged from point 364 on
    for f in FIELDS4:
        assert same_doubles(fb2[f], fb[f]), ("block B alone in the launch", f)
    for f in LOSF:
        assert same_doubles(lb2[f], lb[f]), ("block B alone in the launch", f)
    fm, lm = traced(hip, case, case.atm, case.geom)         # both blocks in one workgroup
    for f in FIELDS4:
        assert same_doubles(fm[f][CM.BLOCK_A], fa[f]) and same_doubles(fm[f][CM.BLOCK_B], fb[f]), ("mixed launch", f)
    for f in ("p", "t", "ds", "qh2o", "np", "tsurf", "tp"):
        assert same_doubles(lm[f][CM.BLOCK_A], la[f]) and same_doubles(lm[f][CM.BLOCK_B], lb[f]), ("mixed launch", f)
    for f in ("k", "u"):
        assert same_doubles(lm[f][:, CM.BLOCK_A], la[f]) and same_doubles(lm[f][:, CM.BLOCK_B], lb[f]), ("mixed launch", f)
    assert not same_doubles(fa["rad"][:2], fb["rad"])


def test_cloud_one_point_past_the_staging_limit(hip, oracle):
    """cloud_lds_points() + 1 points: every lane reads the model's arrays and finds the altitude range by its own pass."""
    case = cloud_case()
    n = hip.cloud_lds_points() + 1
    ncol = -(-n // case.base.np)
    atm = CM.join(CM.columns(case.ctl, case.base, tuple(-0.75 + 1.5 * i / (ncol - 1) for i in range(ncol)), seed=8, npoints=n))
    assert atm.np == n
    geom = case.geom[[0, 2, 4, 5]]
    ref = CM.formod(oracle, case, geom=geom, atm=atm)
    assert_parity(run(hip, case, atm=atm, geom=geom), ref, "%d points" % n)
    # one point fewer: staged; the cut point is the topmost of the last column, so the bits differ -- but not the parity
    atm2 = CM.join(CM.columns(case.ctl, case.base, tuple(-0.75 + 1.5 * i / (ncol - 1) for i in range(ncol)), seed=8, npoints=n - 1))
    assert_parity(run(hip, case, atm=atm2, geom=geom), CM.formod(oracle, case, geom=geom, atm=atm2), "%d points" % (n - 1))


# ---- 6. the whole-slice altitude rule ----------------------------------------------------------------------------------------
def test_cloud_whose_first_point_lies_mid_atmosphere_is_entered(hip):
    """Under upstream's first-column rule zmin == zmax == z of the first point and no ray would enter."""
    case = cloud_case()
    blk = CM.columns(case.ctl, case.base, CM.CLOUD_LATS, seed=5)
    order = np.roll(np.arange(len(blk["z"])), -45)          # the first point: level 45 of column 0
    blk = {f: (v[:, order] if v.ndim == 2 else v[order]) for f, v in blk.items()}
    atm = CM.join(blk)
    a = CM.Cloud(atm, case.ctl)
    assert 40.0 < a.z[0] < 50.0 and T.Atm.altitude_range(a, 0, a.np) == (a.z[0], a.z[0])
    geom = case.geom[CM.BLOCK_A]
    recs = [CM.traceray(case.ctl, a, g) for g in geom]
    m = hip.Model(case.ctl, case.lib_tables())
    try:
        m.set_atm(atm)
        out = m.kat_traceray(geom)
    finally:
        m.close()
    assert np.array_equal(out["np"], [r["np"] for r in recs]) and out["np"].min() > 10
    assert np.abs(out["tp"] - np.array([r["tp"] for r in recs])).max() < 1e-9


# ---- 7. a hole ---------------------------------------------------------------------------------------------------------------
def test_hole_gives_nan_where_the_model_has_nan(hip, oracle):
    """Refraction off, the parcels between 38 and 52 km cut out: positions between 41 and 49 km have no parcel within
    cz.  Records and radiances are NaN exactly where the model's are; where the model's radiance is finite (upstream's
    radiance update skips a segment whose gas transmittance is not > 1e-50, a NaN one included) it is met to the
    suite's tolerance.  The ray with its tangent point at 60 km reads no parcel below 57 km: it keeps the bits it has
    in the uncut cloud."""
    case = cloud_case(refrac=0)
    geom = case.geom[CM.BLOCK_A]
    full = CM.cloud_atmosphere(case.ctl, case.base, second_block=False)
    hole = CM.cloud_atmosphere(case.ctl, case.base, second_block=False, keep=lambda z: (z < 38.0) | (z > 52.0))
    a = CM.Cloud(hole, case.ctl)
    recs = [CM.traceray(case.ctl, a, g) for g in geom]
    ref = CM.formod(oracle, case, geom=geom, atm=hole, records=recs)
    crossing = [i for i, r in enumerate(recs) if np.isnan(r["p"]).any()]
    clear = [i for i, r in enumerate(recs) if not np.isnan(r["p"]).any()]
    assert len(crossing) >= 4 and clear == [3]
    fh, lh = traced(hip, case, hole, geom)
    ff, lf = traced(hip, case, full, geom)
    assert np.array_equal(lh["np"], [r["np"] for r in recs])
    for i, r in enumerate(recs):
        n = r["np"]
        for f, dev in (("p", lh["p"][i, :n]), ("t", lh["t"][i, :n]), ("k", lh["k"][0, i, :n]), ("u", lh["u"][0, i, :n])):
            want = np.asarray(r[f][0] if f in ("k", "u") else r[f])
            assert np.array_equal(np.isnan(dev), np.isnan(want)), (i, f)
            ok = ~np.isnan(want)
            assert np.allclose(dev[ok], want[ok], rtol=1e-9, atol=0), (i, f)
    assert np.array_equal(np.isnan(fh["rad"]), np.isnan(ref["rad"])) and np.array_equal(np.isnan(fh["tau"]), np.isnan(ref["tau"]))
    print("IP 3 hole: rays crossing %s, NaN radiances in the model %d of %d" % (crossing, np.isnan(ref["rad"]).sum(), ref["rad"].size))
    # the documented behaviour (rule 6 in jurassic_hip.h): the update leaves the NaN segments out, the radiance stays finite
    assert np.isfinite(ref["rad"][crossing]).all() and np.isfinite(ref["tau"][crossing]).all()
    assert np.isfinite(fh["rad"][crossing]).all() and np.isfinite(fh["tau"][crossing]).all()
    fin = ~np.isnan(ref["rad"])
    assert common.rel_err(fh["rad"][fin], ref["rad"][fin]).max() < RTOL
    fin = ~np.isnan(ref["tau"])
    assert np.all(np.abs(fh["tau"] - ref["tau"])[fin] <= (RTOL * np.abs(ref["tau"]) + common.tau_atol(ref["tau"]))[fin])
    for f in FIELDS4:
        assert same_doubles(fh[f][clear], ff[f][clear]), f
    for f in ("p", "t", "ds", "qh2o", "np", "tsurf", "tp"):
        assert same_doubles(lh[f][clear], lf[f][clear]), f


# ---- 8. dense Jacobian -------------------------------------------------------------------------------------------------------
def coarse(base, step):
    n = base.np
    keep = np.arange(0, n, step)
    out = abi.atm_t()
    for f in ("time", "z", "lon", "lat", "p", "t"):
        np.ctypeslib.as_array(getattr(out, f))[:len(keep)] = np.ctypeslib.as_array(getattr(base, f))[:n][keep]
    np.ctypeslib.as_array(out.q)[:, :len(keep)] = np.ctypeslib.as_array(base.q)[:, :n][:, keep]
    np.ctypeslib.as_array(out.k)[:, :len(keep)] = np.ctypeslib.as_array(base.k)[:, :n][:, keep]
    out.np = len(keep)
    return out


def test_dense_jacobian_on_a_two_column_cloud(hip):
    """T on all points and O3 between 10 and 30 km of a 2-column cloud.  Every column of jur_kernel equals
    (F(x + h e) - F(x)) / h from two jur_formod_host calls with upstream's steps (1 K; 1 % of a mixing ratio,
    jurassic.c:831-837) to 1e-6 of the column's largest entry, the bound of
    test_track_gpu.py::test_dense_jacobian_on_two_profiles."""
    case = cloud_case(rett_zmin=-100.0, rett_zmax=1000.0, cz=7.0)
    case.ctl.retq_zmin[2], case.ctl.retq_zmax[2] = 10.0, 30.0
    atm = CM.join(CM.columns(case.ctl, coarse(case.base, 3), (-0.25, 0.25), seed=9))
    geom = np.array([[0.0, 700.0, 0.0, -1.8, 0.0, 0.0, -1.8], [0.0, 700.0, 0.0, 0.3, 0.0, 0.0, 0.3], T.limb_ray(15.0)])
    nd = case.ctl.nd
    obs = common.obs_from_geom(geom, nd)
    np.ctypeslib.as_array(obs.rad)[:] = 0.0
    m = hip.Model(case.ctl, case.lib_tables())
    try:
        k = m.kernel(atm, obs)
        el = hip.scene_elements(case.ctl, atm, 0, atm.np)
        iq, ip, cols = np.asarray(el["iq"]), np.asarray(el["ip"]), np.asarray(el["cols"])
        assert k.shape[0] == len(geom) * nd and (iq == 1).sum() == atm.np and 4 <= (iq == 4).sum() < atm.np and len(iq) == k.shape[1]
        m.set_atm(atm)
        y0 = m.formod_host(geom)["rad"]
        assert same_doubles(y0, np.ctypeslib.as_array(obs.rad)[:len(geom), :nd])
        worst_all, nonzero = 0.0, 0
        for e in range(len(ip)):
            pert = copy_atm(atm)
            if iq[e] == 1:
                h = 1.0
                np.ctypeslib.as_array(pert.t)[ip[e]] += h
            else:
                x = float(np.ctypeslib.as_array(pert.q)[2, ip[e]])
                h = max(abs(0.01 * x), 1e-15)
                np.ctypeslib.as_array(pert.q)[2, ip[e]] = x + h
            m.set_atm(pert)
            quot = ((m.formod_host(geom)["rad"] - y0) / h).ravel()
            scale = np.abs(quot).max()
            col = k[:, cols[e]]
            if scale == 0:
                assert np.all(col == 0), e
                continue
            nonzero += 1
            worst_all = max(worst_all, np.abs(col - quot).max() / scale)
            assert np.abs(col - quot).max() < 1e-6 * scale, (e, iq[e], ip[e], np.abs(col - quot).max() / scale)
        print("IP 3 dense Jacobian: worst column deviation %.3e of the column's largest entry over %d columns (%d non-zero)" % (worst_all, len(ip), nonzero))
        assert nonzero > len(ip) // 2
    finally:
        m.close()


# ---- 9. routing --------------------------------------------------------------------------------------------------------------
def test_routing_leaves_the_bits_alone(hip):
    import torch
    case = cloud_case()
    geom = case.geom
    n = len(geom)
    m = hip.Model(case.ctl, case.lib_tables())
    try:
        m.set_atm(case.atm)
        m.enable_timing(True)
        base = m.formod_host(geom)                          # package-sized: the fused kernel's size under ip 1
        ms = m.kernel_ms()
        assert ms["pencil_launches"] == 0 and ms["trace_launches"] >= 1, ms
        m.enable_timing(False)
        m.set_pencil(1 << 16)                               # accepted, no effect
        again = m.formod_host(geom)
        for f in FIELDS4:
            assert same_doubles(again[f], base[f]), ("set_pencil", f)
        npad = 1000
        pad = np.vstack([geom] + [geom[i % n][None] for i in range(npad - n)])
        pad[n:, 4] += np.linspace(0.0, 0.5, npad - n)
        big = m.formod_host(pad)
        for f in FIELDS4:
            assert same_doubles(big[f][:n], base[f]), ("padded to %d rays" % npad, f)
        perm = np.random.default_rng(3).permutation(len(pad))
        for chunk in (64, 1 << 21):
            m.set_chunk_rays(chunk)
            for sort in (False, True):
                m.set_sort_rays(sort)
                for compact in (False, True):
                    m.set_compact_workspace(compact)
                    out = m.formod_host(pad[perm])
                    for f in FIELDS4:
                        assert same_doubles(out[f], big[f][perm]), (f, chunk, sort, compact)
        # the device entry
        dev = torch.device("cuda", 0)
        nd = case.ctl.nd
        d_geom = torch.from_numpy(np.ascontiguousarray(geom.T)).to(dev)
        d_rad = torch.zeros((n, nd), dtype=torch.float64, device=dev)
        d_tau = torch.empty((n, nd), dtype=torch.float64, device=dev)
        d_tp = torch.empty((3, n), dtype=torch.float64, device=dev)
        d_np = torch.empty(n, dtype=torch.int32, device=dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m.formod_device(n, d_geom.data_ptr(), d_rad.data_ptr(), d_tau.data_ptr(), d_tp.data_ptr(), d_np.data_ptr(), d_st.data_ptr(),
                            s.cuda_stream)
        s.synchronize()
        assert int(d_st.item()) == 0
        assert same_doubles(d_rad.cpu().numpy(), base["rad"]) and same_doubles(d_tau.cpu().numpy(), base["tau"])
        assert same_doubles(d_tp.cpu().numpy().T, base["tp"]) and np.array_equal(d_np.cpu().numpy(), base["np"])
        # contributions: the totals are the forward model's, an emitter alone is the forward model without the others
        from test_contrib_gpu import edited_atm
        ctb = m.formod_contrib_host(geom)
        for f in FIELDS4:
            assert same_doubles(ctb[f], base[f]), ("contributions", f)
        v = 2
        m.set_atm(edited_atm(case, v))
        alone = m.formod_host(geom)
        assert common.rel_err(ctb["rad_c"][v], alone["rad"]).max() < RTOL
        terr = np.abs(ctb["tau_c"][v] - alone["tau"])
        assert np.all(terr <= RTOL * np.abs(alone["tau"]) + common.tau_atol(alone["tau"]))
        # the one GPU listed twice through the multi-device entry
        m2 = hip.Model(case.ctl, case.lib_tables())
        try:
            hip.models_set_atm([m, m2], case.atm)
            multi = hip.formod_host_multi([m, m2], geom)
            for f in FIELDS4:
                assert same_doubles(multi[f], base[f]), ("multi", f)
        finally:
            m2.close()
    finally:
        m.close()


def test_drop_in_formod_and_the_tool_equal_the_model_entry(hip, tmp_path):
    case = cloud_case()
    case.write_files(str(tmp_path), base="tbl")
    m = hip.Model(case.ctl)                                  # tables from the files, as the drop-in entry reads them
    try:
        m.set_atm(case.atm)
        want = m.formod_host(case.geom)
    finally:
        m.close()
    hip.dropin_finalize()
    try:
        obs = common.obs_from_geom(case.geom, case.ctl.nd)
        hip.formod(case.ctl, case.atm, obs)
        n, nd = obs.nr, case.ctl.nd
        assert same_doubles(np.ctypeslib.as_array(obs.rad)[:n, :nd], want["rad"])
        assert same_doubles(np.ctypeslib.as_array(obs.tau)[:n, :nd], want["tau"])
    finally:
        hip.dropin_finalize()
    # the command-line tool: IP, CX and CZ from the control file, atmosphere and rays from text files written to 17 digits
    nd = case.ctl.nd
    ctl_text = "TBLBASE = ./tbl\nNG = %d\n" % case.ctl.ng + "".join("EMITTER[%d] = %s\n" % (g, e) for g, e in enumerate(common.LIMB_EMITTERS)) \
        + "ND = %d\n" % nd + "".join("NU[%d] = %.4f\n" % (d, v) for d, v in enumerate(common.LIMB_NU)) \
        + "USEGPU = -1\nWRITE_BINARY = 0\nREAD_BINARY = 0\nIP = 3\nCX = %r\nCZ = %r\nRAYDS = 10\nRAYDZ = 1\n" % (CM.CX, CM.CZ)
    (tmp_path / "cloud.ctl").write_text(ctl_text)
    a = T.Atm(case.atm, case.ctl)
    with open(tmp_path / "atm.tab", "w") as fh:
        for i in range(a.np):
            fh.write(" ".join(repr(v) for v in [a.time[i], a.z[i], a.lon[i], a.lat[i], a.p[i], a.t[i]] + [q[i] for q in a.q] + [k[i] for k in a.k]) + "\n")
    with open(tmp_path / "obs.tab", "w") as fh:
        for g in case.geom:
            fh.write(" ".join(repr(float(v)) for v in list(g) + [0.0] * (3 + 2 * nd)) + "\n")
    import os
    import subprocess
    exe = os.path.join(common.ROOT, "jurassic-gpu_amd", "formod")
    tool = subprocess.run([exe, "cloud.ctl", "obs.tab", "atm.tab", "rad.tab"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert tool.returncode == 0, tool.stdout + tool.stderr
    got = [l.split() for l in open(tmp_path / "rad.tab") if l.strip() and not l.startswith("#")]
    assert len(got) == len(case.geom)
    for row, rad, tau in zip(got, want["rad"], want["tau"]):
        assert row[10:10 + 2 * nd] == ["%g" % v for v in list(rad) + list(tau)], (row, rad, tau)


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    case = cloud_case()
    for cx, cz in ((0.0, 3.0), (150.0, 0.0), (-1.0, 3.0), (150.0, -3.0), (math.nan, 3.0), (150.0, math.nan), (math.inf, 3.0), (150.0, math.inf)):
        with pytest.raises(hip.JurassicError, match="error -1: IP 3 .*cx.*cz"):
            hip.Model(with_ctl(case, cx=cx, cz=cz), case.lib_tables())
    for ip in (0, 4):
        with pytest.raises(hip.JurassicError, match="error -1: Unknown interpolation method.*1, 2 or 3"):
            hip.Model(with_ctl(case, ip=ip), case.lib_tables())
    geom = case.geom
    y = np.ones((len(geom), case.ctl.nd))
    m = hip.Model(case.ctl, case.lib_tables())
    try:
        m.set_atm(case.atm)
        good = m.formod_host(geom)
        scene_calls = [lambda: m.kernel_scene(case.atm, geom), lambda: m.normal_scene(case.atm, geom, y, y),
                       lambda: m.gradient_scene(case.atm, geom, y, y, None), lambda: m.step_scene(case.atm, geom, y, y, [1.0]),
                       lambda: m.trial_scene(case.atm, geom, y, y, np.zeros((1, 0))),
                       lambda: m.retrieve_scene(case.atm, geom, y, y, 1, (1.0,)), lambda: m.diagnose_scene(case.atm, geom, y, y),
                       lambda: m.gain_scene(case.atm, geom, y, y), lambda: m.param_scene(case.ctl, case.atm, geom, y, y)]
        for i, call in enumerate(scene_calls):
            with pytest.raises(hip.JurassicError, match="error -1: .*ip = 3 "):
                call()
        again = m.formod_host(geom)                          # the refusals left the model's atmosphere alone
        for f in FIELDS4:
            assert same_doubles(again[f], good[f]), f
    finally:
        m.close()


# ---- 11. call sequence -------------------------------------------------------------------------------------------------------
def test_call_sequence_on_one_model_gives_fresh_model_bits(hip):
    """Clouds of 364 + 182, 182, 62 and 364 + 182 points in turn on one long-lived model: a stale position table, or one
    that did not grow, would show."""
    case = cloud_case()
    geom = case.geom[CM.BLOCK_A][:4]
    atms = [case.atm, CM.join(CM.block_b(case.ctl, case.base, time=0.0)),
            CM.join(CM.columns(case.ctl, coarse(case.base, 3), (-0.25, 0.25), seed=9)), case.atm]
    fresh = [run(hip, case, atm=a, geom=geom) for a in atms]
    assert not same_doubles(fresh[0]["rad"], fresh[1]["rad"]) and not same_doubles(fresh[1]["rad"], fresh[2]["rad"])
    m = hip.Model(case.ctl, case.lib_tables())
    try:
        for a, want in zip(atms, fresh):
            m.set_atm(a)
            out = m.formod_host(geom)
            for f in FIELDS4:
                assert same_doubles(out[f], want[f]), f
    finally:
        m.close()


def test_drop_in_follows_ip_and_influence_lengths_from_call_to_call(hip, tmp_path):
    """One drop-in lane under ip 3, ip 1, ip 3 with another cx, and the first again: each the bits of a fresh model."""
    case = cloud_case()
    case.write_files(str(tmp_path), base="tbl")
    geom = case.geom[CM.BLOCK_A][:4]
    nd = case.ctl.nd
    ctls = [case.ctl, with_ctl(case, ip=1), with_ctl(case, cx=2000.0), case.ctl]
    want = []
    for c in ctls:
        m = hip.Model(c)
        try:
            m.set_atm(case.atm)
            want.append(m.formod_host(geom))
        finally:
            m.close()
    assert not same_doubles(want[0]["rad"], want[1]["rad"]) and not same_doubles(want[0]["rad"], want[2]["rad"])
    hip.dropin_finalize()
    try:
        for c, w in zip(ctls, want):
            obs = common.obs_from_geom(geom, nd)
            hip.formod(c, case.atm, obs)
            assert same_doubles(np.ctypeslib.as_array(obs.rad)[:len(geom), :nd], w["rad"]), (c.ip, c.cx)
            assert same_doubles(np.ctypeslib.as_array(obs.tau)[:len(geom), :nd], w["tau"]), (c.ip, c.cx)
    finally:
        hip.dropin_finalize()
