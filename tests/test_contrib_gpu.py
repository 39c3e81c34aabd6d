"""Contributions of the emitters (formod TASK contrib) on the GPU: jur_formod_contrib_host / _device, formod_contrib()
and the `formod ... TASK contrib` / `obs2spec` tools.

Variant g < ng is by definition the forward model on the atmosphere with every other gas's q and every window's k set
to 0, variant ng ("EXTINCT") the forward model with every q set to 0; the control block applies unchanged.  Each is
held to the oracle run on that edited atmosphere (1e-9 relative on radiances, common.tau_atol on transmittances), and
the total to the ordinary path bit for bit.  A contribution can lie ten orders of magnitude below the total (H2O at
48 km in the refspec shape: 1e-12 of a 0.02 total), where the look-up's absolute ~1e-13 on an emissivity (JUR_ARITH_FAST,
include/jurassic_hip.h) is no longer small relative to it: against the oracle a value may instead be within 1e-14 of
the ray's total radiance in that channel (ORACLE_FLOOR; measured 5.6e-16).  Against the library's own forward model on
the edited atmosphere the variants are bit-identical in that shape."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import common
from jurassic_hip import abi, synth, textio

pytestmark = pytest.mark.gpu
RTOL = 1e-9
ORACLE_FLOOR = 1e-14
PKG = os.path.join(common.ROOT, "jurassic-gpu_amd")
REFSPEC_EMITTERS = ["C2H2", "C2H6", "CCl4", "CH4", "ClO", "ClONO2", "CO", "CO2", "COF2", "F11", "F12", "F14", "F22", "H2O",
                    "H2O2", "HCN", "HNO3", "HNO4", "HOCl", "N2", "N2O", "N2O5", "NH3", "NO", "NO2", "O2", "O3", "OCS", "SF6",
                    "SO2"]


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def edited_atm(case, v):
    """Copy of case.atm for variant v (v < ng: gas v alone, no extinction; v == ng: no gas)."""
    a = abi.atm_t()
    C.memmove(C.byref(a), C.byref(case.atm), C.sizeof(abi.atm_t))
    ng = case.ctl.ng
    q, k = np.ctypeslib.as_array(a.q), np.ctypeslib.as_array(a.k)
    for g in range(ng):
        if g != v:
            q[g, :] = 0.0
    if v < ng:
        k[:, :] = 0.0
    return a


def model_for(hip, case, **kw):
    m = hip.Model(case.ctl, case.lib_tables())
    for name, val in kw.items():
        getattr(m, name)(*val) if isinstance(val, tuple) else getattr(m, name)(val)
    m.set_atm(case.atm)
    return m


def assert_close(rad, tau, ref, rtol=RTOL, total=None):
    fin = np.isfinite(ref["rad"])
    assert np.array_equal(fin, np.isfinite(rad))
    if fin.any():
        err = np.abs(rad[fin] - ref["rad"][fin])
        allow = rtol * np.abs(ref["rad"][fin]) + (0.0 if total is None else ORACLE_FLOOR * np.abs(total[fin]))
        k = np.argmax(err - allow)
        assert np.all(err <= allow), (k, rad[fin][k], ref["rad"][fin][k], common.rel_err(rad[fin], ref["rad"][fin]).max())
    terr = np.abs(tau - ref["tau"])
    assert np.all(terr <= rtol * np.abs(ref["tau"]) + common.tau_atol(ref["tau"])), terr.max()


def check_oracle(oracle, case, out, variants=None, rad_in=None, rays=None):
    tb = case.oracle_tables(oracle)
    sel = slice(None) if rays is None else rays
    geom = case.geom[sel]
    rin = None if rad_in is None else rad_in[sel]
    for v in range(case.ctl.ng + 1) if variants is None else variants:
        ref = oracle.formod_rays(case.ctl, edited_atm(case, v), tb, geom, rad_in=rin)
        assert np.array_equal(ref["np"], out["np"][sel]), v
        assert_close(out["rad_c"][v][sel], out["tau_c"][v][sel], ref, total=out["rad"][sel])


def assert_total_is_formod(m, case, out, rad_in=None):
    ref = m.formod_host(case.geom, rad_in=rad_in)
    for key in ("rad", "tau", "tp", "np"):
        assert np.array_equal(out[key], ref[key], equal_nan=key == "rad"), key


@pytest.mark.parametrize("name", ["limb", "limb_ctm4", "nadir_bbt", "limb_ext"])
def test_every_variant_against_the_oracle(hip, oracle, name):
    if name == "nadir_bbt":
        case = common.nadir_case()                   # WRITE_BBT, rays that end on the surface
    else:
        case = common.limb_case(nu=common.CTM4_NU) if name == "limb_ctm4" else common.limb_case()
    if name == "limb_ext":                           # an extinction that varies with altitude (the shipped profile has k = 0)
        common.extinction_profile(case.atm)
    m = model_for(hip, case)
    out = m.formod_contrib_host(case.geom)
    assert out["rad_c"].shape == (case.ctl.ng + 1, len(case.geom), case.ctl.nd)
    check_oracle(oracle, case, out)
    assert_total_is_formod(m, case, out)
    m.close()
    if name == "limb_ext":
        ng = case.ctl.ng
        assert out["tau_c"][ng].min() < 0.9          # the EXTINCT variant is not empty here ...
        tb = case.oracle_tables(oracle)
        for v in range(ng):                          # ... and a gas variant that kept k would show: gas v alone WITH k
            a = edited_atm(case, v)
            np.ctypeslib.as_array(a.k)[:] = np.ctypeslib.as_array(case.atm.k)
            with_k = oracle.formod_rays(case.ctl, a, tb, case.geom)
            assert np.abs(out["tau_c"][v] - with_k["tau"]).max() > 1e-3, v


@pytest.mark.parametrize("seed", [100, 103, 107, 111])
def test_random_configurations_against_the_oracle(hip, oracle, seed):
    from test_parity_gpu import _random_case
    case = _random_case(seed)
    m = model_for(hip, case)
    out = m.formod_contrib_host(case.geom)
    check_oracle(oracle, case, out)
    assert_total_is_formod(m, case, out)
    m.close()


def test_hydrostatic_with_h2o_traces_the_edited_atmospheres(hip, oracle):
    """HYDZ >= 0 with H2O an emitter: zeroing q_H2O moves every other variant's pressure profile -- the shared
    plane alone would be wrong here by ~1e-4.  The call leaves the caller's atmosphere on the device."""
    case = common.limb_case(hydz=10.0)
    assert "H2O" in common.LIMB_EMITTERS and case.ctl.ctm_h2o == 1
    m = model_for(hip, case)
    before = m.formod_host(case.geom)
    out = m.formod_contrib_host(case.geom)
    check_oracle(oracle, case, out)
    for key in ("rad", "tau", "tp", "np"):
        assert np.array_equal(out[key], before[key]), key
    after = m.formod_host(case.geom)
    assert np.array_equal(after["rad"], before["rad"]) and np.array_equal(after["tau"], before["tau"])
    m.close()


def test_single_emitter_variant_is_the_total_and_extinct_is_empty(hip):
    """One emitter, continua off, no extinction: variant 0 IS the forward model, bit for bit; the EXTINCT variant of
    limb rays is rad 0, tau 1."""
    off = dict(ctm_co2=0, ctm_h2o=0, ctm_n2=0, ctm_o2=0, ctm_auto=1)
    case = common.Case(["CO2"], common.LIMB_NU, os.path.join(common.GOLD, "limb", "atm.tab"), common.golden_geometry("limb"),
                       **off)
    np.ctypeslib.as_array(case.atm.k)[:] = 0.0
    m = model_for(hip, case)
    out = m.formod_contrib_host(case.geom)
    assert np.array_equal(out["rad_c"][0], out["rad"]) and np.array_equal(out["tau_c"][0], out["tau"])
    assert np.all(out["rad_c"][1] == 0.0) and np.all(out["tau_c"][1] == 1.0)
    m.close()
    case5 = common.limb_case(**off)                   # five emitters: EXTINCT is still empty
    m = model_for(hip, case5)
    out = m.formod_contrib_host(case5.geom)
    assert np.all(out["rad_c"][-1] == 0.0) and np.all(out["tau_c"][-1] == 1.0)
    m.close()


def test_nan_mask_reaches_every_variant(hip):
    case = common.limb_case()
    m = model_for(hip, case)
    clean = m.formod_contrib_host(case.geom)
    rad_in = np.zeros((len(case.geom), case.ctl.nd))
    rad_in[::7, 0] = np.nan
    rad_in[3::5, 1] = np.inf
    masked = ~np.isfinite(rad_in)
    out = m.formod_contrib_host(case.geom, rad_in=rad_in)
    for v in range(case.ctl.ng + 1):
        assert np.all(np.isnan(out["rad_c"][v][masked]))
        assert np.array_equal(out["rad_c"][v][~masked], clean["rad_c"][v][~masked])
        assert np.array_equal(out["tau_c"][v], clean["tau_c"][v])
    assert_total_is_formod(m, case, out, rad_in=rad_in)
    m.close()


def test_device_entry_equals_host_entry(hip):
    import torch
    case = common.limb_case(nu=common.CTM4_NU)
    m = model_for(hip, case)
    host = m.formod_contrib_host(case.geom)
    nr, nd, nv = len(case.geom), case.ctl.nd, case.ctl.ng + 1
    dev = torch.device("cuda:0")
    geom = torch.tensor(np.ascontiguousarray(case.geom.T), device=dev)
    rad = torch.zeros((nr, nd), dtype=torch.float64, device=dev)
    tau = torch.zeros_like(rad)
    tp = torch.zeros((3, nr), dtype=torch.float64, device=dev)
    npts = torch.zeros(nr, dtype=torch.int32, device=dev)
    rad_c = torch.zeros((nv, nr, nd), dtype=torch.float64, device=dev)
    tau_c = torch.zeros_like(rad_c)
    torch.cuda.synchronize()
    m.formod_contrib_device(nr, geom.data_ptr(), rad.data_ptr(), tau.data_ptr(), tp.data_ptr(), rad_c.data_ptr(),
                            tau_c.data_ptr(), npts.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(rad_c.cpu().numpy(), host["rad_c"]) and np.array_equal(tau_c.cpu().numpy(), host["tau_c"])
    assert np.array_equal(rad.cpu().numpy(), host["rad"]) and np.array_equal(npts.cpu().numpy(), host["np"])
    assert np.array_equal(tp.cpu().numpy().T, host["tp"])
    m.close()


def test_pencil_setting_does_not_matter(hip):
    """66 rays are below the fused kernel's threshold; contributions take the batched kernels either way."""
    case = common.limb_case()
    outs = []
    for pencil in (10000, 0):
        m = model_for(hip, case, set_pencil=pencil)
        outs.append(m.formod_contrib_host(case.geom))
        m.close()
    for key in ("rad", "tau", "tp", "np", "rad_c", "tau_c"):
        assert np.array_equal(outs[0][key], outs[1][key]), key


def test_many_rays_in_several_launches(hip, oracle):
    """20 000 rays through a 64 MiB workspace: several integration launches, compact tiles on and off."""
    case = common.limb_case(geom=synth.limb_geometry(20000, seed=21, nprofiles=4), nprofiles=4)
    outs = []
    for compact in (1, 0):
        m = model_for(hip, case, set_workspace_budget=64 << 20, set_compact_workspace=compact)
        outs.append(m.formod_contrib_host(case.geom))
        assert m.last_launches() > 1
        if compact:
            assert_total_is_formod(m, case, outs[-1])
        m.close()
    for key in ("rad", "tau", "tp", "np", "rad_c", "tau_c"):
        assert np.array_equal(outs[0][key], outs[1][key]), key
    check_oracle(oracle, case, outs[0], rays=slice(0, None, 397))


@pytest.mark.parametrize("nr", [0, 1])
def test_zero_and_one_ray(hip, oracle, nr):
    case = common.limb_case(geom=common.golden_geometry("limb")[30:30 + nr])
    m = model_for(hip, case)
    out = m.formod_contrib_host(case.geom)
    assert out["rad_c"].shape == (case.ctl.ng + 1, nr, case.ctl.nd)
    if nr:
        check_oracle(oracle, case, out)
    m.close()


def refspec_case(tmp_path, geom=None):
    """The refspec example's shape: 30 emitters, 100 channels from 1050 cm^-1, 66 limb rays at 3 .. 68 km."""
    nu = [1050.0 + i for i in range(100)]
    rows = np.loadtxt(os.path.join(common.GOLD, "limb", "atm.tab"), comments="#")      # time z lon lat p T q[5] k
    wide = np.hstack([rows[:, :6], np.tile(rows[:, 6:11], (1, 6)), rows[:, 11:12] + 1e-5])
    np.savetxt(tmp_path / "atm30.tab", wide, fmt="%.17g")
    g = common.golden_geometry("limb") if geom is None else geom
    return common.Case(REFSPEC_EMITTERS, nu, str(tmp_path / "atm30.tab"), g, table_kw=dict(nlev=3, ntemp=2))


def test_refspec_shape_against_separate_calls_and_the_oracle(hip, oracle, tmp_path):
    case = refspec_case(tmp_path)
    assert (case.ctl.ng, case.ctl.nd, len(case.geom)) == (30, 100, 66)
    m = model_for(hip, case)
    out = m.formod_contrib_host(case.geom)
    for v in range(case.ctl.ng + 1):
        m.set_atm(edited_atm(case, v))
        ref = m.formod_host(case.geom)
        assert_close(out["rad_c"][v], out["tau_c"][v], ref)
    m.close()
    check_oracle(oracle, case, out, variants=[REFSPEC_EMITTERS.index("CO2"), REFSPEC_EMITTERS.index("H2O"),
                                              REFSPEC_EMITTERS.index("O3"), case.ctl.ng])


LIMB_CTL = "TBLBASE = ./tbl\nNG = 5\nEMITTER[0] = CO2\nEMITTER[1] = H2O\nEMITTER[2] = O3\nEMITTER[3] = F11\n" \
           "EMITTER[4] = CCl4\nND = 2\nNU[0] = 792.0000\nNU[1] = 832.0000\nREAD_BINARY = 0\nWRITE_BINARY = 0\n"


def _run(args, cwd):
    out = subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_formod_task_contrib_writes_every_emitter(hip, tmp_path):
    """`formod ... TASK contrib` writes <rad>, <rad>.<EMITTER> and <rad>.EXTINCT; each agrees with a separate `formod`
    run on the edited atm.tab to the %g text."""
    case = common.limb_case()
    case.write_files(str(tmp_path), "tbl")
    (tmp_path / "limb.ctl").write_text(LIMB_CTL)
    exe = os.path.join(PKG, "formod")
    obs, atm = os.path.join(common.GOLD, "limb", "obs.tab"), os.path.join(common.GOLD, "limb", "atm.tab")
    _run([exe, "limb.ctl", obs, atm, "rad.tab", "TASK", "contrib"], tmp_path)
    names = ["rad.tab"] + ["rad.tab." + e for e in common.LIMB_EMITTERS] + ["rad.tab.EXTINCT"]
    assert sorted(p.name for p in tmp_path.glob("rad.tab*")) == sorted(names)
    rows = np.loadtxt(atm, comments="#")
    for v, name in enumerate(names[1:]):
        ed = rows.copy()
        for g in range(5):
            if g != v:
                ed[:, 6 + g] = 0.0
        if v < 5:
            ed[:, 11] = 0.0
        np.savetxt(tmp_path / "atm_ed.tab", ed, fmt="%.17g")
        _run([exe, "limb.ctl", obs, "atm_ed.tab", "ref.tab"], tmp_path)
        got, want = textio.read_obs_array(str(tmp_path / name), 2), textio.read_obs_array(str(tmp_path / "ref.tab"), 2)
        assert got.shape == want.shape == (66, 14)
        assert np.allclose(got, want, rtol=1e-5, atol=0), name
    plain = textio.read_obs_array(str(tmp_path / "rad.tab"), 2)
    _run([exe, "limb.ctl", obs, atm, "plain.tab"], tmp_path)
    assert np.array_equal(plain, textio.read_obs_array(str(tmp_path / "plain.tab"), 2))


def test_refspec_pipeline_end_to_end(hip, tmp_path):
    """climatology -> limb -> formod TASK contrib -> obs2spec, as the reference's example/refspec/run.sh runs it
    (30 emitters, 100 channels; synthetic tables)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "csrc")])
    case = refspec_case(tmp_path)
    case.write_files(str(tmp_path), "tbl")
    ctl = ["TBLBASE = ./tbl", "NG = 30"] + ["EMITTER[%d] = %s" % (g, e) for g, e in enumerate(REFSPEC_EMITTERS)]
    ctl += ["ND = 100"] + ["NU[%d] = %d" % (i, 1050 + i) for i in range(100)] + ["READ_BINARY = 0", "WRITE_BINARY = 0"]
    (tmp_path / "limb_1050.ctl").write_text("\n".join(ctl) + "\n")
    _run([os.path.join(PKG, "climatology"), "limb_1050.ctl", "atm.tab"], tmp_path)
    _run([os.path.join(PKG, "limb"), "limb_1050.ctl", "obs.tab", "Z0", "3", "Z1", "68", "DZ", "1.0"], tmp_path)
    _run([os.path.join(PKG, "formod"), "limb_1050.ctl", "obs.tab", "atm.tab", "rad_1050.tab", "TASK", "contrib"], tmp_path)
    outs = sorted(p.name for p in tmp_path.glob("rad_1050.tab*"))
    assert len(outs) == 32
    for f in outs:
        _run([os.path.join(PKG, "obs2spec"), "limb_1050.ctl", f, "spec." + f], tmp_path)
        lines = (tmp_path / ("spec." + f)).read_text().splitlines()
        assert len(lines) == 12 + 66 * 101
        vals = np.array([[float(x) for x in ln.split()] for ln in lines if ln and not ln.startswith("#")])
        assert vals.shape == (6600, 12) and np.isfinite(vals).all()
