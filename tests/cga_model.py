"""CPU model of the Curtis-Godson forward model (FORMOD 1) -- a helper of tests/test_cga_cpu.py and
tests/test_cga_gpu.py, no tests in it.

Look-up blocks: locate_id, locate_tbl_id, get_eps, get_u, lip, c01 (jr_common.h:43-50, 106-125, 156-185) and the
row-acceptance rules of the table reader (jurassic.c:346-395) restated in plain Python on the rows a common.Case holds;
u and eps are stored as fp32, as in the oracle's and the library's tables.  `ega_eps` is built from these blocks alone
and is what pins them to the reference (tests/test_cga_cpu.py compares it with orc.ega_eps bit for bit).

The rule (include/jurassic_hip.h, FORMOD 1) and a forward model on top: the LOS records of orc.traceray, the means
summed in the order of curtis_godson() (jr_common.h:455-473), the look-up at the means, then orc.continua, orc.new_obs
and orc.epilogue with the segment transmittance of all gases as the quotient of the products of the path
transmittances (segment_tau_gas in jur_kernels.hip: 0 where the previous product is not above 1e-280).

Python floats are IEEE doubles and every operation below is one rounding; the one exception Python makes -- a division
by zero raises -- is put back to IEEE by div()."""
import ctypes as C
import math
import numpy as np
from jurassic_hip import abi


def c01(x):
    return 1.0 if x > 1.0 else (0.0 if x < 0.0 else x)


def div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def lip(x0, y0, x1, y1, x):
    return y0 + div((x - x0) * (y1 - y0), x1 - x0)


def locate_id(xx, n, x):
    ilo, ihi = 0, n - 1
    while ihi > ilo + 1:
        i = (ihi + ilo) >> 1
        if xx[i] > x:
            ihi = i
        else:
            ilo = i
    return ilo


def locate_tbl_id(xx, n, x, i0=0):
    ilo, ihi = i0, n - 1
    while ihi > ilo + 1:
        i = (ihi + ilo) >> 1
        if xx[i] > x:
            ihi = i
        else:
            ilo = i
    return ilo


class Pair:
    """The table of one (gas, channel) pair as the reader leaves it: p[ip], t[ip][it], u[ip][it][iu], eps[ip][it][iu]
    (lists of Python floats; u and eps rounded to fp32)."""

    def __init__(self, rows, mp=abi.TBLNP, mt=abi.TBLNT, mu=abi.TBLNU):
        self.p, self.t, self.u, self.eps = [], [], [], []
        eps_old = press_old = temp_old = u_old = -999.0
        for press, temp, u, eps in np.asarray(rows, dtype=np.float64).tolist():
            if press != press_old:
                press_old = press
                assert len(self.p) < mp, "too many pressure levels"
                self.p.append(press); self.t.append([]); self.u.append([]); self.eps.append([])
            ip = len(self.p) - 1
            if temp != temp_old:
                temp_old = temp
                assert len(self.t[ip]) < mt, "too many temperatures"
                self.t[ip].append(temp); self.u[ip].append([]); self.eps[ip].append([])
            it = len(self.t[ip]) - 1
            assert it >= 0, "table block repeats previous temperature"
            cu, ce = self.u[ip][it], self.eps[ip][it]
            if (eps > eps_old and u > u_old) or not cu:
                eps_old, u_old = eps, u
                if len(cu) >= mu:
                    continue                                   # a row beyond the curve's capacity is ignored
                cu.append(0.0); ce.append(0.0)
            self.p[ip] = press
            self.t[ip][it] = temp
            cu[-1] = float(np.float32(u)); ce[-1] = float(np.float32(eps))

    @property
    def np(self):
        return len(self.p)

    def get_eps(self, ip, it, u):
        cu, ce = self.u[ip][it], self.eps[ip][it]
        i = locate_tbl_id(cu, len(cu), u)
        return lip(cu[i], ce[i], cu[i + 1], ce[i + 1], u)

    def get_u(self, ip, it, eps):
        cu, ce = self.u[ip][it], self.eps[ip][it]
        i = locate_tbl_id(ce, len(ce), eps)
        return lip(ce[i], cu[i], ce[i + 1], cu[i + 1], eps)

    def brackets(self, t, p):
        """(ipr, it0, it1) of ega_eps (jr_common.h:240-246), or None where one of its size rules answers 1."""
        if self.np < 2:
            return None
        ipr = locate_id(self.p, self.np, p)
        if len(self.t[ipr]) < 2 or len(self.t[ipr + 1]) < 2:
            return None
        it0 = locate_id(self.t[ipr], len(self.t[ipr]), t)
        if len(self.u[ipr][it0]) < 2 or len(self.u[ipr][it0 + 1]) < 2:
            return None
        it1 = locate_id(self.t[ipr + 1], len(self.t[ipr + 1]), t)
        if len(self.u[ipr + 1][it1]) < 2 or len(self.u[ipr + 1][it1 + 1]) < 2:
            return None
        return ipr, it0, it1

    def blend(self, ipr, it0, it1, e00, e01, e10, e11, t, p):
        """eps_t of ega_eps lines :259-265 from the four corner emissivities."""
        eps_p0 = c01(lip(self.t[ipr][it0], e00, self.t[ipr][it0 + 1], e01, t))
        eps_p1 = c01(lip(self.t[ipr + 1][it1], e10, self.t[ipr + 1][it1 + 1], e11, t))
        return c01(lip(self.p[ipr], eps_p0, self.p[ipr + 1], eps_p1, p))


def ega_eps(pair, tau, t, u, p):
    """ega_eps (jr_common.h:237-268) from the blocks above; pair is None where the case has no table."""
    if tau < 1e-9:
        return 0.0
    b = pair.brackets(t, p) if pair is not None else None
    if b is None:
        return 1.0
    ipr, it0, it1 = b
    eps = 1 - tau
    corners = ((ipr, it0), (ipr, it0 + 1), (ipr + 1, it1), (ipr + 1, it1 + 1))
    e = [c01(pair.get_eps(ip, it, pair.get_u(ip, it, eps) + u)) for ip, it in corners]
    return div(1.0 - pair.blend(ipr, it0, it1, *e, t, p), tau)


def cga_lookup(pair, tau, cgt, cgu, cgp):
    """Steps 1, 2 and 4 of the rule: the new path transmittance from the previous one and the means."""
    if tau < 1e-9:
        return 0.0
    b = pair.brackets(cgt, cgp) if pair is not None else None
    if b is None:
        return tau
    ipr, it0, it1 = b
    corners = ((ipr, it0), (ipr, it0 + 1), (ipr + 1, it1), (ipr + 1, it1 + 1))
    e = [c01(pair.get_eps(ip, it, cgu)) for ip, it in corners]
    return 1.0 - pair.blend(ipr, it0, it1, *e, cgt, cgp)


def means(p, t, u):
    """Curtis-Godson sums and means along one ray for one gas -> (cgp, cgt, cgu) lists; cgp, cgt are NaN where cgu is
    0 (0 / 0), as in the reference."""
    a = b = w = 0.0
    cgp, cgt, cgu = [], [], []
    for pi, ti, ui in zip(p, t, u):
        up, ut = ui * pi, ui * ti
        a, b, w = a + up, b + ut, w + ui
        cgp.append(div(a, w)); cgt.append(div(b, w)); cgu.append(w)
    return cgp, cgt, cgu


def path_tau(pair, p, t, u):
    """The gas's path transmittance after every segment of one ray (the whole rule, step 3 included)."""
    cgp, cgt, cgu = means(p, t, u)
    tau, out = 1.0, []
    for ip in range(len(cgu)):
        if tau < 1e-9:
            tau = 0.0
        elif cgu[ip] == 0.0:
            pass
        else:
            tau = cga_lookup(pair, tau, cgt[ip], cgu[ip], cgp[ip])
        out.append(tau)
    return out


def pairs_of(case):
    return {gd: Pair(rows) for gd, rows in case.rows.items()}


def ega_ctl(ctl):
    """A copy of the control block with FORMOD 2: the oracle's tracer asserts FORMOD != 1, as upstream does."""
    c = abi.ctl_t()
    C.memmove(C.byref(c), C.byref(ctl), C.sizeof(abi.ctl_t))
    c.formod = 2
    return c


def continua_config(ctl):
    names = [ctl.emitter[g].value.decode().upper() for g in range(ctl.ng)]
    ig_h2o = names.index("H2O") if ctl.ctm_h2o and "H2O" in names else -999
    ig_co2 = names.index("CO2") if ctl.ctm_co2 and "CO2" in names else -999
    fourbit = (ctl.ctm_co2 == 1 and ig_co2 >= 0) * 8 + (ctl.ctm_h2o == 1 and ig_h2o >= 0) * 4 + (ctl.ctm_n2 == 1) * 2 \
        + (ctl.ctm_o2 == 1) * 1
    return ig_co2, ig_h2o, fourbit


def formod(orc, case, geom=None, atm=None, pairs=None, tables=None, want_paths=False):
    """CGA forward model of the rays geom (default: the case's) -> dict(rad, tau (nr, nd), tp (nr, 3), np, and with
    want_paths paths[ray][(g, d)] = list of path transmittances)."""
    ctl2 = ega_ctl(case.ctl)
    atm = case.atm if atm is None else atm
    geom = case.geom if geom is None else np.asarray(geom, dtype=np.float64)
    pairs = pairs_of(case) if pairs is None else pairs
    tables = case.oracle_tables(orc) if tables is None else tables
    ng, nd = ctl2.ng, ctl2.nd
    ig_co2, ig_h2o, fourbit = continua_config(ctl2)
    nr = len(geom)
    rad, tau = np.zeros((nr, nd)), np.ones((nr, nd))
    tp, npts, paths = np.zeros((nr, 3)), np.zeros(nr, dtype=np.int32), []
    for ir, g in enumerate(geom):
        tr = orc.traceray(ctl2, atm, g)
        n = int(tr["np"])
        npts[ir], tp[ir] = n, tr["tp"]
        p, t, ds = tr["p"].tolist(), tr["t"].tolist(), tr["ds"]
        cg = orc.curtis_godson(ctl2, atm, g)
        ray_paths = {}
        for ig in range(ng):
            u = tr["u"][ig].tolist()
            cgp, cgt, cgu = means(p, t, u)
            for mine, theirs in ((cgp, cg["cgp"]), (cgt, cg["cgt"]), (cgu, cg["cgu"])):   # bit for bit, NaN where 0 / 0
                # (curtis_godson() starts its sums with the first product, the rule with 0 + the first product: the same
                # doubles except that a first column of -0.0 -- a path without length -- stays -0.0 there; w == 0
                # does not see the sign, so it is taken out here: x + 0.0)
                a, b = np.array(mine) + 0.0, theirs[ig, :n] + 0.0
                assert n == cg["np"] and np.array_equal(np.isnan(a), np.isnan(b)), (ir, ig)
                assert np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64)), (ir, ig)
            for d in range(nd):
                ray_paths[(ig, d)] = path_tau(pairs.get((ig, d)), p, t, u)
        paths.append(ray_paths)
        for d in range(nd):
            nu = ctl2.nu[d]
            r_d, t_d = np.zeros(1), np.ones(1)
            if n:
                u_co2 = tr["u"][ig_co2] if ig_co2 >= 0 else np.zeros(n)
                u_h2o = tr["u"][ig_h2o] if ig_h2o >= 0 else np.zeros(n)
                q_h2o = tr["q"][ig_h2o] if ig_h2o >= 0 else np.zeros(n)
                ctm = orc.continua(nu, tr["p"], tr["t"], q_h2o, u_co2, u_h2o)
            pprev = 1.0
            for ip in range(n):
                beta_ds = float(tr["k"][ip]) * float(ds[ip])          # (abi.NW == 1: one extinction window)
                if fourbit & 8:
                    beta_ds += float(ctm[0][ip])
                if fourbit & 4:
                    beta_ds += float(ctm[1][ip])
                if fourbit & 2:
                    beta_ds += float(ctm[2][ip]) * float(ds[ip])
                if fourbit & 1:
                    beta_ds += float(ctm[3][ip]) * float(ds[ip])
                pcur = 1.0
                for ig in range(ng):
                    pcur *= ray_paths[(ig, d)][ip]
                tau_gas = div(pcur, pprev) if pprev > 1e-280 else 0.0
                pprev = pcur
                r_d, t_d, _ = orc.new_obs(tables, d, [t[ip]], [tau_gas], [beta_ds], r_d, t_d)
            r_d = orc.epilogue(tables, d, nu, [tr["tsurf"]], [ctl2.write_bbt], r_d, t_d)
            rad[ir, d], tau[ir, d] = r_d[0], t_d[0]
    out = dict(rad=rad, tau=tau, tp=tp, np=npts)
    if want_paths:
        out["paths"] = paths
    return out
