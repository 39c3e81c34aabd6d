"""2-D atmosphere along the line of sight (IP 2) on the device: jur_track_trace_kernel behind the entries, against the CPU
model of tests/track_model.py (which tests/test_track_cpu.py pins to the oracle bit for bit).

Atmosphere: a track of four graded profiles at latitudes -3, -1, 1, 3 on one meridian (one of them with fewer levels)
in one time block, a single profile in a second block.  Rays: T.track_rays(), 14 of them.  Bounds are the suite's own:
radiances 1e-9 relative, transmittances 1e-9 relative plus common.tau_atol, LOS records the scaled deviation and bound
of tests/losrecords.py with the yardstick taken from the CPU model.  Every test here fails at model creation on a
library that refuses IP 2."""
import ctypes as C
import numpy as np
import pytest
import common
import cga_model as M
import losrecords as L
import track_model as T
from jurassic_hip import abi
from test_track_cpu import base_case, same_doubles

pytestmark = pytest.mark.gpu
RTOL = 1e-9
FIELDS4 = ("rad", "tau", "tp", "np")


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


def track_case(**kw):
    """The fixed rays on the graded track (+ the one-profile second block), ip = 2 unless said otherwise."""
    kw.setdefault("ip", 2)
    case = base_case(**kw)
    case.base = case.atm
    case.atm = T.track_atmosphere(case.ctl, case.base)
    return case


def with_ip(case, ip):
    c = abi.ctl_t()
    C.memmove(C.byref(c), C.byref(case.ctl), C.sizeof(abi.ctl_t))
    c.ip = ip
    return c


def run(hip, case, atm=None, geom=None, ctl=None, arith="fast", what="formod_host"):
    m = hip.Model(case.ctl if ctl is None else ctl, case.lib_tables())
    try:
        m.set_arithmetic(hip.ARITH_EXACT if arith == "exact" else hip.ARITH_FAST)
        m.set_atm(case.atm if atm is None else atm)
        return getattr(m, what)(case.geom if geom is None else geom)
    finally:
        m.close()


def assert_parity(out, ref, what=""):
    assert np.array_equal(out["np"], ref["np"]), (what, out["np"], ref["np"])
    fin = np.isfinite(ref["rad"])
    assert fin.all() and np.array_equal(fin, np.isfinite(out["rad"])), what
    rerr = common.rel_err(out["rad"], ref["rad"])
    terr = np.abs(out["tau"] - ref["tau"])
    allow = RTOL * np.abs(ref["tau"]) + common.tau_atol(ref["tau"])
    print("IP 2 %s: worst rel radiance error %.3e, worst |dtau| / allowance %.3e, worst |dtp| %.3e"
          % (what, rerr.max(), (terr / allow).max(), np.abs(out["tp"] - ref["tp"]).max()))
    assert rerr.max() < RTOL, (what, rerr.max())
    assert np.all(terr <= allow), (what, terr.max())
    assert np.abs(out["tp"] - ref["tp"]).max() < 1e-9, what


@pytest.fixture(scope="module")
def reference(oracle):
    """The CPU model's LOS records and forward results, computed once: name -> (case, formod dict)."""
    cache = {}

    def get(name):
        if name not in cache:
            base = dict(refrac1={}, refrac0=dict(refrac=0), bbt=dict(write_bbt=1), cga=dict(formod=1))[name]
            case = track_case(**base)
            records = cache["refrac1"][1]["records"] if name in ("bbt", "cga") else None     # the tracer sees neither switch
            cache[name] = (case, T.formod(oracle, case, records=records))
        return cache[name]
    get("refrac1")
    return get


# ---- 1. LOS records ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refrac", [1, 0])
def test_los_records_against_the_model(hip, reference, refrac):
    case, ref = reference("refrac%d" % refrac)
    rows = T.Atm(case.atm, case.ctl)
    base = ref["records"]
    use = np.ones(len(case.geom), dtype=bool)
    Y = {f: 0.0 for f in L.FIELDS}
    for i, g in enumerate(case.geom):                       # the yardstick of tests/losrecords.py, from the model
        near = [T.traceray(case.ctl, rows, L._nudged(g, s), two_d=True) for s in (+1, -1)]
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
        print("IP 2 LOS records refrac=%d field %s: scaled deviation %.3e, yardstick %.3e, bound %.3e" % (refrac, f, worst[f], Y[f], L.bound(Y[f])))
    for f in L.FIELDS:
        assert worst[f] <= L.bound(Y[f]), (f, worst[f], Y[f], L.bound(Y[f]))
    tsurf = np.array([b["tsurf"] for b in base])
    assert np.array_equal(tsurf > 0, out["tsurf"] > 0) and (tsurf > 0).any()
    hit = tsurf > 0
    assert np.abs(out["tsurf"][hit] - tsurf[hit]).max() < 1e-9 * 300
    assert np.abs(out["tp"] - np.array([b["tp"] for b in base])).max() < 1e-9


# ---- 2. radiances, transmittances, tangent points ------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_forward_model_against_the_model(hip, reference, arith):
    case, ref = reference("refrac1")
    assert_parity(run(hip, case, arith=arith), ref, "formod %s" % arith)
    assert np.any(ref["tau"] < 0.99) and np.all(ref["rad"] > 0)


def test_forward_model_in_brightness_temperatures(hip, reference):
    case, ref = reference("bbt")
    assert_parity(run(hip, case), ref, "write_bbt")
    assert np.all((ref["rad"] > 1.0) & (ref["rad"] < 350))        # kelvins, not radiances (those stay below 0.1)


def test_curtis_godson_band_model_on_the_track(hip, reference):
    """FORMOD 1 and IP 2 compose: tests/cga_model.py's rule fed the 2-D LOS records."""
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


# ---- 3. one-profile blocks --------------------------------------------------------------------------------------------------
def test_one_profile_blocks_have_the_bits_of_ip_1(hip):
    case = track_case()
    geom = case.geom[T.SECOND_BLOCK]
    res = []
    for ip in (2, 1):
        m = hip.Model(with_ip(case, ip), case.lib_tables())
        try:
            m.set_atm(case.atm)
            res.append((m.formod_host(geom), m.kat_traceray(geom)))
        finally:
            m.close()
    (f2, l2), (f1, l1) = res
    assert np.all(f2["np"] > 10)
    for f in FIELDS4:
        assert same_doubles(f2[f], f1[f]), f
    for f in ("p", "t", "ds", "qh2o", "k", "u", "np", "tsurf", "tp"):
        assert same_doubles(l2[f], l1[f]), f


# ---- 4. homogeneous track ---------------------------------------------------------------------------------------------------
def test_homogeneous_track_agrees_with_one_profile(hip):
    case = track_case()
    same = T.track_atmosphere(case.ctl, case.base, graded=False, thinned=None)
    one = T.track_atmosphere(case.ctl, case.base, lats=(0.0,), graded=False, thinned=None)
    out2 = run(hip, case, atm=same)
    out1 = run(hip, case, atm=one, ctl=with_ip(case, 1))
    assert_parity(out2, out1, "homogeneous track vs ip 1")


# ---- 5. the feature is live -------------------------------------------------------------------------------------------------
def profile_alone(atm, first, n):
    """Points [first, first + n) of atm as an atmosphere of their own."""
    out = abi.atm_t()
    for f in ("time", "z", "lon", "lat", "p", "t"):
        np.ctypeslib.as_array(getattr(out, f))[:n] = np.ctypeslib.as_array(getattr(atm, f))[first:first + n]
    np.ctypeslib.as_array(out.q)[:, :n] = np.ctypeslib.as_array(atm.q)[:, first:first + n]
    np.ctypeslib.as_array(out.k)[:, :n] = np.ctypeslib.as_array(atm.k)[:, first:first + n]
    out.np = n
    return out


def test_graded_track_differs_from_ip_1_and_the_end_takes_the_end_profile(hip):
    """Against ip 1 on the profile next to the tangent points (lat -1) alone the crossing limb rays move by more than
    1e-3; the nadir ray beyond the track's end is the ip 1 result on the end profile alone."""
    case = track_case()
    track = T.track_atmosphere(case.ctl, case.base, second_block=False)
    out2 = run(hip, case, atm=track, geom=case.geom[:12])
    out1 = run(hip, case, atm=profile_alone(track, 91, 91), geom=case.geom[:12], ctl=with_ip(case, 1))
    diff = common.rel_err(out2["rad"], out1["rad"])[T.LIMB_CROSSING]
    print("graded track, ip 2 against ip 1 on one profile, crossing limb rays: rel difference per ray", diff.max(axis=1))
    assert np.all(diff.max(axis=1) > 1e-3)
    g = case.geom[[T.NADIR_BEYOND]]
    beyond = run(hip, case, atm=track, geom=g)
    alone = run(hip, case, atm=profile_alone(track, track.np - 91, 91), geom=g, ctl=with_ip(case, 1))
    assert_parity(beyond, alone, "beyond the track's end vs the end profile under ip 1")


# ---- 6. order of the track --------------------------------------------------------------------------------------------------
def test_track_listed_north_to_south(hip):
    case = track_case()
    south_first = run(hip, case, atm=T.track_atmosphere(case.ctl, case.base, thinned=None, second_block=False), geom=case.geom[:12])
    north_first = run(hip, case, atm=T.track_atmosphere(case.ctl, case.base, thinned=None, second_block=False, order=(3, 2, 1, 0)),
                      geom=case.geom[:12])
    assert_parity(north_first, south_first, "north to south")


# ---- 7. dense Jacobian ------------------------------------------------------------------------------------------------------
def coarse(base, step):
    """Every step-th level of a one-profile atmosphere."""
    n = base.np
    keep = np.arange(0, n, step)
    out = abi.atm_t()
    for f in ("time", "z", "lon", "lat", "p", "t"):
        np.ctypeslib.as_array(getattr(out, f))[:len(keep)] = np.ctypeslib.as_array(getattr(base, f))[:n][keep]
    np.ctypeslib.as_array(out.q)[:, :len(keep)] = np.ctypeslib.as_array(base.q)[:, :n][:, keep]
    np.ctypeslib.as_array(out.k)[:, :len(keep)] = np.ctypeslib.as_array(base.k)[:, :n][:, keep]
    out.np = len(keep)
    return out


def test_dense_jacobian_on_two_profiles(hip):
    """T retrieved on all levels of two profiles A (lat -1) and B (lat 1).  A nadir ray south of A reads A alone: every
    column of B's levels is exactly zero.  A ray between them has non-zero columns in both.  Every column equals
    (F(x + h e) - F(x)) / h from two jur_formod_host calls with upstream's step for T, 1 K (jurassic.c:831-837), to
    1e-6 of the column's largest entry (the bound of tests/test_scene_jacobian_gpu.py for that comparison)."""
    case = track_case(rett_zmin=-100.0, rett_zmax=1000.0)
    atm = T.track_atmosphere(case.ctl, coarse(case.base, 3), lats=(-1.0, 1.0), thinned=None, second_block=False)
    nlev = atm.np // 2
    geom = np.array([[0.0, 700.0, 0.0, -1.8, 0.0, 0.0, -1.8], [0.0, 700.0, 0.0, 0.3, 0.0, 0.0, 0.3], T.limb_ray(15.0)])
    nd = case.ctl.nd
    obs = common.obs_from_geom(geom, nd)
    np.ctypeslib.as_array(obs.rad)[:] = 0.0
    m = hip.Model(case.ctl, case.lib_tables())
    try:
        k = m.kernel(atm, obs)
        el = hip.scene_elements(case.ctl, atm, 0, atm.np)
        iq, ip, cols = np.asarray(el["iq"]), np.asarray(el["ip"]), np.asarray(el["cols"])
        assert k.shape == (len(geom) * nd, atm.np) and np.all(iq == 1) and len(ip) == atm.np
        in_b = cols[ip >= nlev]
        in_a = cols[ip < nlev]
        assert np.all(k[0:nd][:, in_b] == 0) and np.any(k[0:nd][:, in_a] != 0)
        for r in (1, 2):
            assert np.any(k[r * nd:(r + 1) * nd][:, in_a] != 0) and np.any(k[r * nd:(r + 1) * nd][:, in_b] != 0), r
        m.set_atm(atm)
        y0 = m.formod_host(geom)["rad"]
        assert same_doubles(y0, np.ctypeslib.as_array(obs.rad)[:len(geom), :nd])
        worst_all = 0.0
        for e in range(len(ip)):
            pert = copy_atm(atm)
            np.ctypeslib.as_array(pert.t)[ip[e]] += 1.0
            m.set_atm(pert)
            quot = ((m.formod_host(geom)["rad"] - y0) / 1.0).ravel()
            scale = np.abs(quot).max()
            col = k[:, cols[e]]
            if scale == 0:
                assert np.all(col == 0), e
                continue
            worst_all = max(worst_all, np.abs(col - quot).max() / scale)
            assert np.abs(col - quot).max() < 1e-6 * scale, (e, ip[e], np.abs(col - quot).max() / scale)
        print("IP 2 dense Jacobian: worst column deviation %.3e of the column's largest entry over %d columns" % (worst_all, len(ip)))
    finally:
        m.close()


# ---- 8. routing -------------------------------------------------------------------------------------------------------------
def test_routing_leaves_the_bits_alone(hip, tmp_path):
    import torch
    case = track_case()
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
        pad = np.vstack([geom] + [geom[i % n][None] for i in range(5000 - n)])
        pad[n:, 4] += np.linspace(0.0, 0.5, 5000 - n)
        big = m.formod_host(pad)
        for f in FIELDS4:
            assert same_doubles(big[f][:n], base[f]), ("padded to 5000 rays", f)
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
        # two models side by side through the multi-device entry
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


def test_drop_in_formod_equals_the_model_entry(hip, tmp_path):
    case = track_case()
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
        # the switch is honoured per call: the same lane under ip 1 gives ip 1's answer, then ip 2's again
        c1 = with_ip(case, 1)
        c1.tblbase = case.ctl.tblbase
        obs1 = common.obs_from_geom(case.geom, nd)
        hip.formod(c1, case.atm, obs1)
        assert not same_doubles(np.ctypeslib.as_array(obs1.rad)[:n, :nd], want["rad"])
        obs2 = common.obs_from_geom(case.geom, nd)
        hip.formod(case.ctl, case.atm, obs2)
        assert same_doubles(np.ctypeslib.as_array(obs2.rad)[:n, :nd], want["rad"])
    finally:
        hip.dropin_finalize()
    # the command-line tool: IP from the control file, atmosphere and rays from text files written to 17 digits
    nd = case.ctl.nd
    ctl_text = "TBLBASE = ./tbl\nNG = %d\n" % case.ctl.ng + "".join("EMITTER[%d] = %s\n" % (g, e) for g, e in enumerate(common.LIMB_EMITTERS)) \
        + "ND = %d\n" % nd + "".join("NU[%d] = %.4f\n" % (d, v) for d, v in enumerate(common.LIMB_NU)) \
        + "USEGPU = -1\nWRITE_BINARY = 0\nREAD_BINARY = 0\nIP = 2\nRAYDS = 10\nRAYDZ = 1\n"
    (tmp_path / "track.ctl").write_text(ctl_text)
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
    tool = subprocess.run([exe, "track.ctl", "obs.tab", "atm.tab", "rad.tab"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert tool.returncode == 0, tool.stdout + tool.stderr
    got = [l.split() for l in open(tmp_path / "rad.tab") if l.strip() and not l.startswith("#")]
    assert len(got) == len(case.geom)
    for row, rad, tau in zip(got, want["rad"], want["tau"]):
        assert row[10:10 + 2 * nd] == ["%g" % v for v in list(rad) + list(tau)], (row, rad, tau)


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    case = track_case()
    with pytest.raises(hip.JurassicError, match="IP 3"):
        hip.Model(with_ip(case, 3), case.lib_tables())
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
            with pytest.raises(hip.JurassicError, match="error -1: .*ip = 2 .*two profiles"):
                call()
        again = m.formod_host(geom)                          # the refusals left the model's atmosphere alone
        for f in FIELDS4:
            assert same_doubles(again[f], good[f]), f
        lone = T.track_atmosphere(case.ctl, case.base)
        np.ctypeslib.as_array(lone.lat)[91] = -1.5
        far = T.track_atmosphere(case.ctl, case.base, lats=(-3.0, -1.0, 9.5, 12.0))
        for bad, words in ((lone, "Cannot identify profiles"), (far, "Distance of profiles is too large")):
            with pytest.raises(hip.JurassicError, match="error -1: " + words):
                m.set_atm(bad)
            with pytest.raises(hip.JurassicError, match="no atmosphere set"):
                m.formod_host(geom)
            with pytest.raises(hip.JurassicError, match="no atmosphere set"):
                m.kat_traceray(geom)
            m.set_atm(case.atm)
            after = m.formod_host(geom)
            for f in FIELDS4:
                assert same_doubles(after[f], good[f]), (words, f)
    finally:
        m.close()


# ---- 10. call sequence --------------------------------------------------------------------------------------------------------
def test_call_sequence_on_one_model_gives_fresh_model_bits(hip):
    """4 profiles, then 2, then 1, then 4 again on one long-lived model: a stale profile table would show."""
    case = track_case()
    geom = case.geom[:12]
    atms = [T.track_atmosphere(case.ctl, case.base, second_block=False),
            T.track_atmosphere(case.ctl, case.base, lats=(-1.0, 2.0), thinned=1, second_block=False),
            T.track_atmosphere(case.ctl, case.base, lats=(0.5,), thinned=None, second_block=False),
            T.track_atmosphere(case.ctl, case.base, second_block=False)]
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
