"""GPU parity tests: the HIP path, called through the C-ABI of
libjurassic_hip.so, against the CPU oracle on the same seeded inputs.

Tolerance: north_star asks for 1e-6 relative on radiances; this suite asserts

  * radiance: 1e-9 relative (RTOL);
  * transmittance: 1e-9 relative plus common.tau_atol(tau) = 1e-13 + min(5e-14 / tau, 5e-12) absolute -- the
    algorithm's own (1 - eps) / tau is ill-conditioned for optically thick paths;
  * tangent point: altitude 1e-9 km, longitude / latitude 1e-9 deg;
  * LOS point counts and every other integer output: exact.

What the kernels compute with since round 3 -- the docstring of rounds 1-2 ("the
reference's fp64 operand order, no FMA contraction") holds for the ray tracer and for tables that are not strictly
increasing only:

  * ray tracing: the reference's operand order; where a division is replaced (shared reciprocals) the replacement
    returns the same double.  Differences from the oracle are last-bit differences of the device math library
    (exp, log, asin, atan2, sin, cos) amplified along <= 400 path segments;
  * emissivity-growth look-up on strictly increasing tables (the default arithmetic, JUR_ARITH_FAST): curve
    interpolations through bracket slopes formed once per model, blends through reciprocal bracket widths, the path
    transmittance carried as 1 - eps: ~1e-13 from the reference's divisions, NOT bit-identical to them;
    JUR_ARITH_EXACT (jur_model_set_arithmetic, or JUR_EGA_NO_RCP=1 for the process) and every table that is not
    strictly increasing keep the reference's divisions operand for operand;
  * radiance update: shared 1/T, exp through a 64-entry table, tanh through exp: ~1e-15 relative per segment.

The arrangements below (fused / batched / batched_grouped) share that arithmetic and are held to each other BIT FOR BIT in tests/test_pencil_gpu.py and in the
chunking / permutation invariance tests here.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import numpy as np
import pytest
import common
from jurassic_hip import abi, synth, textio

pytestmark = pytest.mark.gpu
RTOL = 1e-9


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert os.path.exists(lib.SO), "libjurassic_hip.so missing: the HIP path must be built"
    return lib


# How a call is arranged on the device.  Every test that goes through run_both runs once per arrangement, so that each
# edge case of the matrix meets the oracle DIRECTLY through the fused kernel and through the batched kernels (the ones
# bench.py times) -- not the latter only by way of "fused == batched":
#   fused            package-sized calls as ONE jur_pencil_kernel (the default for <= 10 000 rays)
#   batched          ray sort + jur_trace_kernel + jur_ega_kernel + jur_combine_kernel (one channel per workgroup)
#   batched_grouped  the same with jur_combine_group_kernel forced (up to four channels per workgroup, ragged groups too)
# Unsorted tables take ega_eps_exact in every arrangement, strict ones the reciprocal-width arithmetic.
ARRANGEMENTS = ("fused", "batched", "batched_grouped")
_state = {"arr": "fused", "key": None, "calls": 0}
_oracle_cache = {}


def pytest_generate_tests(metafunc):
    """Tests that go through run_both get one instance per arrangement; the others arrange their own calls."""
    if "arrangement" in metafunc.fixturenames:
        uses = "run_both" in metafunc.function.__code__.co_names
        metafunc.parametrize("arrangement", ARRANGEMENTS if uses else ("own",), indirect=True)


@pytest.fixture(autouse=True)
def arrangement(request, hip):
    rest = tuple(tok for tok in request.node.callspec.id.split("-") if tok != request.param)
    _state.update(arr=request.param, key=(request.node.originalname, rest), calls=0)
    if request.param == "batched_grouped":
        hip.tune_combine(4, 8, 0)
    yield request.param
    if request.param == "batched_grouped":
        hip.tune_combine(-1, 8, 1_000_000)
    _state["arr"] = "fused"


def run_both(hip, oracle, case, rad_in=None):
    model = hip.Model(case.ctl, case.lib_tables())
    if _state["arr"] in ("batched", "batched_grouped"):
        model.set_pencil(0)
    model.set_atm(case.atm)
    out = model.formod_host(case.geom, rad_in=rad_in)
    # the oracle's answer for the k-th call of a test is the same in every arrangement: computed once
    key = (_state["key"], _state["calls"])
    _state["calls"] += 1
    if key not in _oracle_cache:
        _oracle_cache[key] = oracle.formod_rays(case.ctl, case.atm, case.oracle_tables(oracle), case.geom, rad_in=rad_in)
    ref = _oracle_cache[key]
    model.close()
    return out, ref


def assert_parity(out, ref, rtol=RTOL, cartesian_tp=False):
    assert np.array_equal(out["np"], ref["np"])
    fin = np.isfinite(ref["rad"])
    assert np.array_equal(fin, np.isfinite(out["rad"]))
    assert common.rel_err(out["rad"][fin], ref["rad"][fin]).max() < rtol
    # transmittances: relative 1e-9 plus the absolute allowance of common.tau_atol -- 1.5e-13 for tau of order one, growing
    # as 5e-14 / tau to at most 5e-12 for optically thick paths, where the algorithm's own (1 - eps) / tau is
    # ill-conditioned (see there for the cases that set it; profiles/r03_batch_vs_oracle.log: 300 000 bench rays, worst
    # |dtau| by decade of tau, far inside this allowance)
    terr = np.abs(out["tau"] - ref["tau"])
    allow = rtol * np.abs(ref["tau"]) + common.tau_atol(ref["tau"])
    k = np.unravel_index(np.argmax(terr - allow), terr.shape)
    assert np.all(terr <= allow), (k, out["tau"][k], ref["tau"][k])
    assert np.abs(out["tp"][:, 0] - ref["tp"][:, 0]).max() < 1e-9      # km
    if cartesian_tp:       # rays over a pole or across the dateline (tests/test_scenes_gpu.py): positions 0.1 mm apart
        assert np.linalg.norm(synth._cart(*out["tp"].T) - synth._cart(*ref["tp"].T), axis=1).max() < 1e-7
        return
    # tangent-point longitude / latitude [deg]: 1e-9 (0.1 mm on the ground).  Rays that graze the surface put the parabola
    # through the three lowest points close to degenerate: seed 61660 of tools/fuzz_parity.py (tangent altitude -5.6 m)
    # reaches 2.4e-10 with every arrangement of the kernels; the ray tracer has been the same code since round 1
    assert np.abs(out["tp"][:, 1:] - ref["tp"][:, 1:]).max() < 1e-9


def test_limb_example_geometry(hip, oracle):
    """BASELINE configs[0] shape: the 66 rays of example/limb, 5 emitters, 2 channels."""
    out, ref = run_both(hip, oracle, common.limb_case())
    assert_parity(out, ref)
    gold = textio.read_obs_array(os.path.join(common.GOLD, "limb", "rad.org"), 2)
    for i, row in enumerate(gold):                      # and the reference's golden geometry columns
        assert "%g" % out["tp"][i, 0] == "%g" % row[7] and "%g" % out["tp"][i, 2] == "%g" % row[9]


def test_nadir_example_geometry_brightness_and_surface(hip, oracle):
    """example/nadir: ground-hitting rays (surface term) and WRITE_BBT=1."""
    out, ref = run_both(hip, oracle, common.nadir_case())
    assert_parity(out, ref)
    assert np.all((out["rad"] > 150) & (out["rad"] < 320))      # brightness temperatures [K]


def test_nadir_random_5000(hip, oracle):
    out, ref = run_both(hip, oracle, common.nadir_case(geom=synth.nadir_geometry(5000, seed=11)))
    assert_parity(out, ref)


def test_limb_four_continua_64_profiles(hip, oracle):
    """BASELINE configs[2] shape at a size the oracle does in seconds."""
    geom = synth.limb_geometry(3000, seed=5, nprofiles=64)
    out, ref = run_both(hip, oracle, common.limb_case(geom=geom, nu=common.CTM4_NU, nprofiles=64))
    assert_parity(out, ref)


@pytest.mark.parametrize("switches", [dict(ctm_co2=0), dict(ctm_h2o=0), dict(ctm_n2=0, ctm_o2=0),
                                      dict(ctm_co2=0, ctm_h2o=0, ctm_n2=0, ctm_o2=0), dict(refrac=0),
                                      dict(rayds=20.0, raydz=1.0), dict(hydz=10.0)])
def test_control_switches(hip, oracle, switches):
    geom = synth.limb_geometry(300, seed=2)
    out, ref = run_both(hip, oracle, common.limb_case(geom=geom, nu=common.CTM4_NU, ctm_auto=1, **switches))
    assert_parity(out, ref)


def test_edge_geometries(hip, oracle):
    """Ground-hitting limb rays, observer inside the atmosphere looking up and down,
    zenith view, view point above the atmosphere (no LOS), observer below it."""
    g = synth.limb_geometry(8, scan=True, zmin=-20.0, zmax=2.0)          # tangent below ground
    inside_down = np.array([[0, 30.0, 0, 0, 5.0, 0, 3.0]])
    inside_up = np.array([[0, 10.0, 0, 0, 60.0, 0, 2.0]])
    zenith = np.array([[0, 20.0, 0, 0, 80.0, 0, 0.0]])
    too_high = np.array([[0, 780.0, 0, 0, 95.0, 0, 20.0]])
    below = np.array([[0, -1.0, 0, 0, 10.0, 0, 1.0]])
    geom = np.vstack([g, inside_down, inside_up, zenith, too_high, below])
    out, ref = run_both(hip, oracle, common.limb_case(geom=geom))
    assert_parity(out, ref)
    assert list(out["np"][-2:]) == [0, 0]
    assert np.all(out["rad"][-2:] == 0) and np.all(out["tau"][-2:] == 1)


def test_nan_mask(hip, oracle):
    case = common.limb_case()
    rad_in = np.zeros((len(case.geom), 2))
    rad_in[0, 0] = np.nan
    rad_in[65, 1] = -np.inf
    out, ref = run_both(hip, oracle, case, rad_in=rad_in)
    assert_parity(out, ref)
    assert np.isnan(out["rad"][0, 0]) and np.isnan(out["rad"][65, 1])


@pytest.mark.parametrize("kw", [dict(table_kw=dict(descending=True)),            # locate_id is ascending-only upstream
                                dict(table_kw=dict(nlev=1)),                     # np < 2 -> transparent
                                dict(table_kw=dict(ntemp=1)),                    # nt < 2 -> transparent
                                dict(table_kw=dict(umax_eps=-1.0)),              # nu < 2 -> transparent
                                dict(table_kw=dict(nlev=40, ntemp=30, ratio=1.08)),   # maximum extents (TBLNU clips)
                                dict(table_kw=dict(dup_every=7)),                # sorted, not strict: zero-width fp32 brackets
                                dict(missing={(0, 1), (2, 0), (3, 0), (3, 1)})])
def test_table_shapes(hip, oracle, kw):
    out, ref = run_both(hip, oracle, common.limb_case(geom=synth.limb_geometry(200, seed=9), **kw))
    assert_parity(out, ref)


def test_strict_table_arithmetic_against_the_reference_divisions(hip, monkeypatch):
    """Strictly increasing tables let jur_ega_kernel use the cheaper arithmetic of DESIGN.md section 4 (quotients
    through one Newton step on v_rcp_f64, blends through reciprocal bracket widths, the path transmittance carried as
    1 - eps); JUR_EGA_NO_RCP=1 selects the reference's own divisions, operand for operand.  The two must agree far
    inside the suite's 1e-9 -- here 1e-12 on the radiances of 3000 rays x 4 channels (the budget of the contract is
    1e-6) -- and the point counts exactly."""
    case = common.limb_case(geom=synth.limb_geometry(3000, seed=4, nprofiles=8), nu=common.CTM4_NU, nprofiles=8)
    model = hip.Model(case.ctl, case.lib_tables())
    model.set_pencil(0)
    model.set_atm(case.atm)
    fast = model.formod_host(case.geom)
    monkeypatch.setenv("JUR_EGA_NO_RCP", "1")
    ieee = model.formod_host(case.geom)
    model.close()
    assert np.array_equal(fast["np"], ieee["np"])
    dev = common.rel_err(fast["rad"], ieee["rad"]).max()
    print("strict-table arithmetic vs reference divisions: worst relative radiance deviation %.2e" % dev)
    assert dev < 1e-12
    assert np.abs(fast["tau"] - ieee["tau"]).max() < 1e-13


def test_eight_emitters_with_generated_profiles(hip, oracle, tmp_path):
    """More emitters than the examples use (column densities of all of them are written per LOS point; the
    point before the exit has them redone when its segment is clipped), profiles from this tree's
    `climatology` tool."""
    import subprocess
    emitters = ["CO2", "H2O", "O3", "F11", "CCl4", "CH4", "N2O", "HNO3"]
    (tmp_path / "x.ctl").write_text("NG = 8\n" + "".join(f"EMITTER[{i}] = {e}\n" for i, e in enumerate(emitters))
                                    + "ND = 2\nNU[0] = 792.0\nNU[1] = 832.0\n")
    exe = os.path.join(common.ROOT, "jurassic-gpu_amd", "climatology")
    assert subprocess.run([exe, "x.ctl", "atm.tab"], cwd=tmp_path, capture_output=True, timeout=60).returncode == 0
    geom = np.vstack([synth.limb_geometry(150, seed=12), synth.nadir_geometry(40, seed=13)])
    case = common.Case(emitters, [792.0, 832.0], str(tmp_path / "atm.tab"), geom, table_kw=dict(nlev=12, ntemp=4))
    assert case.atm.np == 91
    out, ref = run_both(hip, oracle, case)
    assert_parity(out, ref)
    assert out["rad"].min() > 0


def test_degenerate_sizes(hip, oracle):
    """No emitters at all (extinction + N2/O2 continua only), a single ray with one channel and one emitter,
    rays that all miss the atmosphere, and one ray more than a workgroup holds."""
    geom = np.vstack([synth.limb_geometry(70, seed=3), synth.nadir_geometry(13, seed=4)])
    case = common.Case([], [792.0, 1450.0, 2150.0], os.path.join(common.GOLD, "limb", "atm.tab"), geom)
    np.ctypeslib.as_array(case.atm.k)[0, :case.atm.np] = 3e-4
    out, ref = run_both(hip, oracle, case)
    assert_parity(out, ref)
    assert out["rad"].min() > 0
    case = common.Case(["CO2"], [667.5], os.path.join(common.GOLD, "nadir", "atm.tab"), synth.nadir_geometry(1, seed=5),
                       write_bbt=1)
    out, ref = run_both(hip, oracle, case)
    assert_parity(out, ref)
    case = common.limb_case(geom=synth.limb_geometry(65, seed=6, zmin=200.0, zmax=400.0))
    out, ref = run_both(hip, oracle, case)
    assert_parity(out, ref)
    assert out["np"].max() == 0 and out["rad"].max() == 0.0 and out["tau"].min() == 1.0
    out, ref = run_both(hip, oracle, common.limb_case(geom=synth.limb_geometry(257, seed=7), nu=common.CTM4_NU))
    assert_parity(out, ref)


def test_extinction_that_varies_with_altitude(hip, oracle):
    """The shipped profiles carry k = 0 and every other case a constant, which the interpolation returns from any
    bracket; common.extinction_profile varies by a factor 1e6 over the profile.  The limb example's rays and nadir rays
    with all four continua on; the "ragged" scene (descending slices, a 2-level profile; synth.scene regrids k from the
    base); and extinction alone -- no emitter, no continuum -- where the transmittance of a ray is
    exp(-sum k_i ds_i) over its LOS record (jur_kat_traceray: k and the trapezoid weights ds as the tracer wrote them).
    The oracle meets that identity to 2.0e-15 on these rays (smallest tau 0.87); 1e-13 relative is 50 x that, for a device
    exp good to about one ulp per segment, and equals common.tau_atol at tau ~ 1."""
    import math
    limb_nadir = np.vstack([common.golden_geometry("limb"), synth.nadir_geometry(13, seed=4)])
    case = common.limb_case(geom=limb_nadir, nu=common.CTM4_NU)
    common.extinction_profile(case.atm)
    out, ref = run_both(hip, oracle, case)
    assert_parity(out, ref)
    assert ref["tau"].min() < 0.5 < ref["tau"].max()

    case = common.limb_case()
    common.extinction_profile(case.atm)
    case.atm, case.geom, _ = synth.scene("ragged", case.ctl, case.atm)
    out, ref = run_both(hip, oracle, case)
    assert_parity(out, ref, cartesian_tp=True)
    assert (ref["np"] > 1).sum() >= 150

    case = common.Case([], [792.0, 832.0], os.path.join(common.GOLD, "limb", "atm.tab"), limb_nadir,
                       ctm_co2=0, ctm_h2o=0, ctm_n2=0, ctm_o2=0, ctm_auto=1)
    common.extinction_profile(case.atm)
    out, ref = run_both(hip, oracle, case)
    assert_parity(out, ref)
    assert out["tau"].min() < 0.9                              # the identity below is not a trivial one
    model = hip.Model(case.ctl, case.lib_tables())
    model.set_atm(case.atm)
    los = model.kat_traceray(case.geom)
    model.close()
    assert np.array_equal(los["np"], out["np"])
    worst = 0.0
    for i, n in enumerate(los["np"]):
        want = math.exp(-math.fsum(los["k"][0, i, :n] * los["ds"][i, :n]))
        worst = max(worst, float(np.abs(out["tau"][i] / want - 1).max()))
    print("extinction only: largest |tau / exp(-sum k ds) - 1| = %.2e, smallest tau %.4f" % (worst, out["tau"].min()))
    assert worst <= 1e-13


def test_against_committed_example_results(hip):
    """HIP path against tests/golden/oracle_examples.json (no oracle run involved): the two reference examples
    and the four-continua limb case with the seeded synthetic tables."""
    for name, (case, gold) in common.oracle_goldens().items():
        model = hip.Model(case.ctl, case.lib_tables())
        model.set_atm(case.atm)
        out = model.formod_host(case.geom)
        model.close()
        assert_parity(out, gold)


def test_curtis_godson_columns(hip, oracle):
    """curtis_godson (jr_common.h:455-473): per gas the running column-weighted pressure and temperature
    and the cumulative column along the path.  The device forms the along-path prefix sums with a
    wavefront scan (different summation order than the sequential loop): 1e-12 relative."""
    geom = np.vstack([synth.limb_geometry(150, seed=41, nprofiles=3), synth.nadir_geometry(30, seed=42, nprofiles=3)])
    case = common.limb_case(geom=geom, nprofiles=3)
    model = hip.Model(case.ctl, case.lib_tables())
    model.set_atm(case.atm)
    got = model.curtis_godson(case.geom)
    for i in range(0, len(geom), 7):
        ref = oracle.curtis_godson(case.ctl, case.atm, case.geom[i])
        n = ref["np"]
        assert got["np"][i] == n and n > 100
        for key in ("cgp", "cgt", "cgu"):
            a, b = got[key][i, :case.ctl.ng, :n], ref[key][:case.ctl.ng, :n]
            # a gas that is absent at the top of the path has S(u) = 0 there: 0/0 in both implementations
            assert np.array_equal(np.isnan(a), np.isnan(b)), (i, key)
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=0, equal_nan=True)
            assert np.all(got[key][i, :, n:] == 0)
        assert np.all(np.diff(got["cgu"][i, 0, :n]) > 0)          # the column only grows
    model.close()


def test_heterogeneous_tables(hip, oracle):
    """Every (gas, channel) pair with its own pressure/temperature axes and grid ratio, and curves that
    degenerate to a single entry scattered through otherwise normal tables (the `nu < 2` early-out of
    ega_eps, jr_common.h:244-246, taken for some brackets only)."""
    shapes = [dict(nlev=33, ntemp=10), dict(nlev=7, ntemp=3, ratio=1.5), dict(nlev=12, ntemp=6, ratio=1.3),
              dict(nlev=40, ntemp=2, ratio=1.2), dict(nlev=5, ntemp=9, ratio=2.0, umax_eps=0.9)]
    case = common.limb_case(geom=synth.limb_geometry(300, seed=31), nu=common.CTM4_NU, nprofiles=3,
                            table_kw=lambda g, d: shapes[(2 * g + d) % len(shapes)])
    for (g, d), r in list(case.rows.items()):
        if (g + d) % 2:
            continue
        keep = np.ones(len(r), dtype=bool)                       # thin every 7th curve down to its first row
        start = np.flatnonzero(np.r_[True, (np.diff(r[:, 0]) != 0) | (np.diff(r[:, 1]) != 0)])
        for k, s0 in enumerate(start):
            s1 = start[k + 1] if k + 1 < len(start) else len(r)
            if k % 7 == 3:
                keep[s0 + 1:s1] = False
        case.rows[(g, d)] = r[keep]
    out, ref = run_both(hip, oracle, case)
    assert_parity(out, ref)


_random_case = common.random_case          # one generator for this file and tests/test_reference_*.py


@pytest.mark.parametrize("seed", range(24))
def test_random_configurations(hip, oracle, seed):
    out, ref = run_both(hip, oracle, _random_case(100 + seed))
    assert_parity(out, ref)


_obs_from_geom = common.obs_from_geom


def test_drop_in_formod_reads_reference_files(hip, oracle, tmp_path):
    """formod()/formod_pencil() on ctl_t/atm_t/obs_t with tables and filter
    functions read from reference-format files (missing files = transparent gas)."""
    case = common.limb_case(missing={(3, 0), (4, 1)}, filt=None)
    for nu in common.LIMB_NU:          # the shipped boxcar filter files
        src = os.path.join(common.GOLD, "limb", "boxcar_%.4f.filt" % nu)
        x, f = np.loadtxt(src, comments="#").T
        case.filters[common.LIMB_NU.index(nu)] = (x, f)
    case.write_files(str(tmp_path), base="boxcar")
    t_ref = oracle.Tables(case.ctl.ng, case.ctl.nd)
    assert t_ref.read_ascii(case.ctl) == 2
    assert t_ref.planck_filt(case.ctl) == 0
    obs_ref = _obs_from_geom(case.geom, 2)
    oracle.formod(case.ctl, case.atm, obs_ref, t_ref)

    case.ctl.useGPU = 1
    obs = _obs_from_geom(case.geom, 2)
    hip.formod(case.ctl, case.atm, obs)
    n = obs.nr
    for name in ("rad", "tau"):
        a = np.ctypeslib.as_array(getattr(obs, name))[:n]
        b = np.ctypeslib.as_array(getattr(obs_ref, name))[:n]
        assert common.rel_err(a[:, :2], b[:, :2]).max() < RTOL
        assert np.array_equal(a[:, 2:], b[:, 2:])              # upstream clears all ND channels
    for name in ("tpz", "tplon", "tplat"):
        assert np.abs(np.ctypeslib.as_array(getattr(obs, name))[:n] -
                      np.ctypeslib.as_array(getattr(obs_ref, name))[:n]).max() < 1e-9

    one = _obs_from_geom(case.geom, 2)
    hip.formod_pencil(case.ctl, case.atm, one, 17)
    assert np.array_equal(np.ctypeslib.as_array(one.rad)[17, :2], np.ctypeslib.as_array(obs.rad)[17, :2])
    assert np.ctypeslib.as_array(one.rad)[16, 0] == 7.0          # other rays untouched


def test_hundred_channels_three_gases(hip, oracle):
    """Many-channel shape (BASELINE configs[4] scaled to the compiled ND = 100): 100 channels
    650..2665 cm^-1 spanning all four continuum windows, CO2/H2O/O3 tables per channel (300
    tables, 20 M entries -- larger than L2), nadir and limb rays."""
    nu = list(np.round(np.linspace(650.0, 2665.0, 100), 4))
    geom = np.vstack([synth.nadir_geometry(300, seed=3), synth.limb_geometry(300, seed=4)])
    case = common.Case(["CO2", "H2O", "O3"], nu, os.path.join(common.GOLD, "limb", "atm.tab"), geom)
    out, ref = run_both(hip, oracle, case)
    assert_parity(out, ref)


WIDE = r"""
import os, sys
sys.path[:0] = [{root!r}, os.path.join({root!r}, 'jurassic-gpu_amd'), os.path.join({root!r}, 'tests')]
import numpy as np, common
from oracle import orc
from jurassic_hip import abi, lib, synth
assert (abi.ND, abi.NG) == (2378, 3)
out = (__import__('ctypes').c_size_t * 5)()
lib.lib().jur_abi_sizes(out)
assert list(out)[3:] == [2378, 3] and out[0] == __import__('ctypes').sizeof(abi.ctl_t) and out[2] == __import__('ctypes').sizeof(abi.obs_t)
nu = [650.0 + i * (2665.0 - 650.0) / 2377 for i in range(2378)]           # SURVEY 8d, C5
geom = np.vstack([synth.nadir_geometry(48, seed=5), synth.limb_geometry(16, seed=6)])
case = common.Case(["CO2", "H2O", "O3"], nu, os.path.join(common.GOLD, "limb", "atm.tab"), geom,
                   table_kw=dict(nlev=12, ntemp=4), write_bbt=0)
model = lib.Model(case.ctl, case.lib_tables())
model.set_atm(case.atm)
got = model.formod_host(case.geom)
ref = orc.formod_rays(case.ctl, case.atm, case.oracle_tables(orc), case.geom)
assert np.array_equal(got['np'], ref['np'])
assert np.max(np.abs(got['rad'] - ref['rad']) / np.abs(ref['rad'])) < 1e-9
assert np.all(np.abs(got['tau'] - ref['tau']) <= 1e-9 * np.abs(ref['tau']) + common.tau_atol(ref['tau']))
print('WIDE_OK', got['rad'].shape)
"""


def test_2378_channel_build(hip, oracle, tmp_path):
    """BASELINE configs[4] shape: library and oracle rebuilt with the reference's compile-time
    dimensions ND=2378, NG=3 (jurassic.h:138-145), 2378 channels x 3 emitters = 7134 tables,
    nadir and limb rays.  Runs in its own process because the dimensions are fixed at import."""
    script = tmp_path / "wide.py"
    script.write_text(WIDE.format(root=common.ROOT))
    env = dict(os.environ, JUR_ND="2378", JUR_NG="3", JUR_SUFFIX="_nd2378")
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=1200, env=env)
    assert out.returncode == 0 and "WIDE_OK (64, 2378)" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


DROPIN_NADIR = r"""
import os, sys
sys.path[:0] = [{root!r}, os.path.join({root!r}, 'jurassic-gpu_amd'), os.path.join({root!r}, 'tests')]
import numpy as np, common
from oracle import orc
from jurassic_hip import abi, lib, textio
case = common.nadir_case(useGPU=-1)
for d, nu in enumerate(common.NADIR_NU):
    case.filters[d] = tuple(np.loadtxt(os.path.join(common.GOLD, 'nadir', 'airs_%.4f.filt' % nu), comments='#').T)
case.write_files({tmp!r}, base='airs')
obs = textio.read_obs(os.path.join(common.GOLD, 'nadir', 'obs.tab'), case.ctl, max_rays=90)
ref = textio.read_obs(os.path.join(common.GOLD, 'nadir', 'obs.tab'), case.ctl, max_rays=90)
tb = orc.Tables(1, 3); assert tb.read_ascii(case.ctl) == 0 and tb.planck_filt(case.ctl) == 0
orc.formod(case.ctl, case.atm, ref, tb)
lib.formod(case.ctl, case.atm, obs)
a, b = np.ctypeslib.as_array(obs.rad)[:90, :3], np.ctypeslib.as_array(ref.rad)[:90, :3]
assert np.all((a > 150) & (a < 320)), a[:2]
assert np.max(np.abs(a - b) / b) < 1e-9
gold = textio.read_obs_array(os.path.join(common.GOLD, 'nadir', 'rad.org'), 3)
assert all('%g' % x == '%g' % y for x, y in zip(np.ctypeslib.as_array(obs.tplat)[:90], gold[:, 9]))
print('DROPIN_NADIR_OK')
"""


def test_drop_in_nadir_in_fresh_process(hip, oracle, tmp_path):
    """The drop-in entry caches its tables for the life of the process (as upstream), so the
    second configuration -- example/nadir: AIRS filters, WRITE_BBT=1, USEGPU=-1 -- runs in a
    process of its own."""
    script = tmp_path / "dropin_nadir.py"
    script.write_text(DROPIN_NADIR.format(root=common.ROOT, tmp=str(tmp_path)))
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "DROPIN_NADIR_OK" in out.stdout, out.stdout + out.stderr


DROPIN_TOGGLE = r"""
import os, sys
sys.path[:0] = [{root!r}, os.path.join({root!r}, 'jurassic-gpu_amd'), os.path.join({root!r}, 'tests')]
import numpy as np, common
from oracle import orc
from jurassic_hip import abi, lib, synth, textio
geom = synth.limb_geometry(200, seed=9)
case = common.limb_case(geom=geom, nu=common.CTM4_NU, ctm_auto=1, ctm_co2=0, ctm_h2o=0, ctm_n2=0, ctm_o2=0, useGPU=1)
case.write_files({tmp!r}, base='tog')
tb = orc.Tables(case.ctl.ng, case.ctl.nd); assert tb.read_ascii(case.ctl) == 0 and tb.planck_filt(case.ctl) == 0

def both():
    obs, ref = abi.obs_t(), abi.obs_t()
    for o in (obs, ref):
        o.nr = len(geom)
        for c, name in enumerate(textio.OBS_COLS[:7]):
            np.ctypeslib.as_array(getattr(o, name))[:o.nr] = geom[:, c]
    lib.formod(case.ctl, case.atm, obs)
    orc.formod(case.ctl, case.atm, ref, tb)
    a, b = np.ctypeslib.as_array(obs.rad)[:len(geom), :4].copy(), np.ctypeslib.as_array(ref.rad)[:len(geom), :4].copy()
    assert np.max(np.abs(a - b) / np.abs(b)) < 1e-9, np.max(np.abs(a - b) / np.abs(b))
    return a

off = both()                                    # first call of the process: every continuum switched off
case.ctl.ctm_h2o = 1                            # switched on later: looked up then (CPUdrivers.c:126-128)
h2o = both()
case.ctl.ctm_co2 = 1; case.ctl.ctm_n2 = 1; case.ctl.ctm_o2 = 1
allon = both()
assert np.any(np.abs(h2o - off) > 1e-6 * off)                         # the H2O continuum did arrive
assert np.any(np.abs(allon[:, 3] - h2o[:, 3]) > 1e-6 * h2o[:, 3])     # N2 window at 2150 cm^-1
case.ctl.ctm_h2o = 0; case.ctl.ctm_co2 = 0; case.ctl.ctm_n2 = 0; case.ctl.ctm_o2 = 0
assert np.array_equal(both(), off)                                     # and off again
print('TOGGLE_OK')
"""


def test_drop_in_continuum_switches_toggle_between_calls(hip, oracle, tmp_path):
    """Run-time switches are honoured on every drop-in call; a continuum that is off in the FIRST call of the
    process and on in a later one finds its emitter then, as upstream's latched statics do (CPUdrivers.c:126-134)."""
    script = tmp_path / "toggle.py"
    script.write_text(DROPIN_TOGGLE.format(root=common.ROOT, tmp=str(tmp_path)))
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "TOGGLE_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


DROPIN_FINALIZE = r"""
import os, sys, ctypes as C
sys.path[:0] = [{root!r}, os.path.join({root!r}, 'jurassic-gpu_amd'), os.path.join({root!r}, 'tests')]
import numpy as np, common, torch
from jurassic_hip import abi, lib, synth, textio
os.chdir({tmp!r})
geom = synth.limb_geometry(300, seed=8)
case = common.limb_case(geom=geom, useGPU=1)
case.write_files({tmp!r}, base='fin')

def run():
    obs = abi.obs_t()
    obs.nr = len(geom)
    for c, name in enumerate(textio.OBS_COLS[:7]):
        np.ctypeslib.as_array(getattr(obs, name))[:obs.nr] = geom[:, c]
    lib.formod(case.ctl, case.atm, obs)
    return np.ctypeslib.as_array(obs.rad)[:len(geom), :2].copy()

assert lib.dropin_finalize() == 0                      # nothing initialised yet: a no-op
torch.cuda.init()
a = run()                                              # first call: tables, lane, and the runtime's own one-off set-up
used = lambda: torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0]
running = used()
assert lib.dropin_finalize() == 1                      # one lane existed
after = used()
assert running - after > (1 << 20), (running, after)   # tables, atmosphere, staging buffers went back to the device
assert lib.dropin_finalize() == 0                      # twice is fine
level = []
for k in range(6):                                     # initialise / finalize again and again: same doubles, no growth
    b = run()
    assert np.array_equal(a, b)
    assert lib.dropin_finalize() == 1
    level.append(used())
# the HIP runtime's own pools settle within the first two cycles (tools/debug_finalize_cycles.py: +16 MB once, then flat
# to the byte over ten cycles); from then on nothing may stay behind
held, back = running - after, level[-1] - level[1]
assert back < (1 << 20), level
print('FINALIZE_OK', held, back)
"""


def test_drop_in_state_can_be_finalized(hip, tmp_path):
    """SURVEY 8b "explicit init/finalize": jur_dropin_finalize() frees the process-global lanes and tables behind
    formod(); the next call loads them again and returns the same doubles."""
    script = tmp_path / "finalize.py"
    script.write_text(DROPIN_FINALIZE.format(root=common.ROOT, tmp=str(tmp_path)))
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "FINALIZE_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_model_from_files_uses_the_binary_cache(hip, oracle, tmp_path, monkeypatch):
    """READ_BINARY=-1 / WRITE_BINARY=1 (upstream defaults, jurassic.c:1018-1019): the first model parses
    the ASCII tables and writes the cache into the working directory, the second one is built from the
    cache alone (ASCII files removed) and gives bit-identical results."""
    case = common.limb_case(read_binary=-1, write_binary=1)
    case.write_files(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    m1 = hip.Model(case.ctl)
    m1.set_atm(case.atm)
    a = m1.formod_host(case.geom)
    m1.close()
    assert os.path.exists(tmp_path / "bin.jurassic-hip-tables-g5-d2")
    for f in os.listdir(tmp_path):
        if f.endswith((".tab", ".filt")):
            os.remove(tmp_path / f)
    m2 = hip.Model(case.ctl)
    m2.set_atm(case.atm)
    b = m2.formod_host(case.geom)
    m2.close()
    assert np.array_equal(a["rad"], b["rad"]) and np.array_equal(a["tau"], b["tau"])
    ref = oracle.formod_rays(case.ctl, case.atm, case.oracle_tables(oracle), case.geom)
    assert common.rel_err(a["rad"], ref["rad"]).max() < 1e-6      # ASCII round trip: %.9g text, fp32 tables
    case.ctl.read_binary = 1
    os.remove(tmp_path / "bin.jurassic-hip-tables-g5-d2")
    with pytest.raises(hip.JurassicError, match="no table cache"):
        hip.Model(case.ctl)


CONCURRENT = r"""
import os, sys, time, threading
sys.path[:0] = [{root!r}, os.path.join({root!r}, 'jurassic-gpu_amd'), os.path.join({root!r}, 'tests')]
import numpy as np, common
from jurassic_hip import abi, lib, synth
case = common.limb_case(useGPU=1)
case.write_files({tmp!r}, base='boxcar')
def make_obs(seed):
    g = synth.limb_geometry(1088, seed=seed)
    o = abi.obs_t(); o.nr = len(g)
    for k, name in enumerate(('time', 'obsz', 'obslon', 'obslat', 'vpz', 'vplon', 'vplat')):
        np.ctypeslib.as_array(getattr(o, name))[:o.nr] = g[:, k]
    return o
nthr, ncall = 8, 4
serial = []
lib.formod(case.ctl, case.atm, make_obs(0))                    # loads the tables
t0 = time.perf_counter()
for t in range(nthr):
    for c in range(ncall):
        o = make_obs(100 * t + c); lib.formod(case.ctl, case.atm, o)
        serial.append(np.ctypeslib.as_array(o.rad)[:1088, :2].copy())
t_serial = time.perf_counter() - t0
def warm(t):
    lib.formod(case.ctl, case.atm, make_obs(7))
threads = [threading.Thread(target=warm, args=(t,)) for t in range(nthr)]     # creates the lanes: once per process
for th in threads: th.start()
for th in threads: th.join()
results = [None] * (nthr * ncall)
def work(t):
    for c in range(ncall):
        o = make_obs(100 * t + c); lib.formod(case.ctl, case.atm, o)
        results[t * ncall + c] = np.ctypeslib.as_array(o.rad)[:1088, :2].copy()
threads = [threading.Thread(target=work, args=(t,)) for t in range(nthr)]
t0 = time.perf_counter()
for th in threads: th.start()
for th in threads: th.join()
t_conc = time.perf_counter() - t0
assert all(np.array_equal(a, b) for a, b in zip(serial, results))
print('CONCURRENT_OK serial %.3f s concurrent %.3f s speedup %.2f' % (t_serial, t_conc, t_serial / t_conc))
"""


def test_concurrent_drop_in_callers_use_lanes(hip, tmp_path):
    """formod() is designed to be called from several threads at once (upstream: OpenMP callers and up
    to 4 lanes, GPUdrivers.cu:262-342).  Eight threads, 1088-ray packages: bit-identical to the serial
    results (the packages overlap on the GPU; the script prints the speed-up it saw)."""
    script = tmp_path / "concurrent.py"
    script.write_text(CONCURRENT.format(root=common.ROOT, tmp=str(tmp_path)))
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, JUR_LANES="8"))
    assert out.returncode == 0 and "CONCURRENT_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    print(out.stdout.strip().splitlines()[-1])   # the speed-up is reported (tools/run_lanes_bench.sh measures it from C),
                                                 # not asserted: wall-clock thresholds do not belong in a parity suite


LIMB_CTL = """# Forward model...
TBLBASE = ./boxcar
NG = 5
EMITTER[0] = CO2
EMITTER[1] = H2O
EMITTER[2] = O3
EMITTER[3] = F11
EMITTER[4] = CCl4
ND = 2
NU[0] = 792.0000
NU[1] = 832.0000
USEGPU = -1
WRITE_BINARY = 0
READ_BINARY = 0
"""


def test_formod_executable_end_to_end(hip, oracle, tmp_path):
    """`formod <ctl> <obs> <atm> <rad>` as example/limb/run.sh calls it (control file with
    the keys of example/limb/limb.ctl, the shipped obs.tab / atm.tab / .filt files, a command-line
    override).  The geometry columns of the written table equal the reference's rad.org as text."""
    case = common.limb_case()
    for d, nu in enumerate(common.LIMB_NU):
        case.filters[d] = tuple(np.loadtxt(os.path.join(common.GOLD, "limb", "boxcar_%.4f.filt" % nu), comments="#").T)
    case.write_files(str(tmp_path), base="boxcar")
    (tmp_path / "limb.ctl").write_text(LIMB_CTL)
    exe = os.path.join(common.ROOT, "jurassic-gpu_amd", "formod")
    out = subprocess.run([exe, "limb.ctl", os.path.join(common.GOLD, "limb", "obs.tab"),
                          os.path.join(common.GOLD, "limb", "atm.tab"), "rad.tab", "REFRAC", "1"],
                         cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    got = [l.split() for l in open(tmp_path / "rad.tab") if l.strip() and not l.startswith("#")]
    gold = [l.split() for l in open(os.path.join(common.GOLD, "limb", "rad.org")) if l.strip() and not l.startswith("#")]
    assert len(got) == len(gold) == 66
    for a, b in zip(got, gold):
        assert a[:8] == b[:8] and a[9] == b[9]                  # time .. tpz, tplat: text-identical
        assert abs(float(a[8]) - float(b[8])) < 1e-11           # tplon is atan2 noise
    header = [l for l in open(tmp_path / "rad.tab") if l.startswith("#")]
    assert header == [l for l in open(os.path.join(common.GOLD, "limb", "rad.org")) if l.startswith("#")]
    # radiance / transmittance columns against the oracle fed with the same files
    case.ctl.tblbase = os.path.join(str(tmp_path), "boxcar").encode()
    tb = oracle.Tables(5, 2)
    assert tb.read_ascii(case.ctl) == 0 and tb.planck_filt(case.ctl) == 0
    ref = oracle.formod_rays(case.ctl, case.atm, tb, case.geom)
    mine = np.array([[float(x) for x in row[10:14]] for row in got])
    want = np.hstack([ref["rad"], ref["tau"]])
    assert np.max(np.abs(mine - want) / np.abs(want)) < 1e-5    # %g keeps 6 significant digits


_retrieval_case = common.retrieval_case


@pytest.mark.parametrize("arith", ["fast", "exact"])
@pytest.mark.parametrize("kw", [dict(), dict(hydz=10.0), dict(extinction=True)]
                         + [pytest.param(dict(channels=c), id=c) for c in ("nd1", "nd3bbt", "nd7")])
def test_jacobian_matches_reference_kernel(hip, oracle, kw, arith):
    """jur_kernel (one batched call over n+1 stacked atmospheres) against the restated
    kernel() loop of n+1 formod calls (jurassic.c:812-857), under both arithmetics of the look-up
    (jur_model_set_arithmetic).  Columns are difference quotients (y1-y0)/h: compared relative to the largest entry of
    each column.  channels: one of common.CHANNELS instead of the example's two radiance channels."""
    kw = dict(kw)
    extinction = kw.pop("extinction", False)
    kw.update(common.CHANNELS[kw.pop("channels")] if "channels" in kw else {})
    case = _retrieval_case(**kw)
    if extinction:                                        # the retk columns (10 .. 20 km) perturb non-zero values
        common.extinction_profile(case.atm)
    nd = case.ctl.nd
    obs_ref = _obs_from_geom(case.geom, nd)
    obs = _obs_from_geom(case.geom, nd)
    for o in (obs_ref, obs):
        o.rad[5][min(1, nd - 1)] = float("nan")           # a masked measurement drops its row
    k_ref = oracle.kernel(case.ctl, case.atm, obs_ref, case.oracle_tables(oracle))
    model = hip.Model(case.ctl, case.lib_tables())
    model.set_arithmetic(hip.ARITH_EXACT if arith == "exact" else hip.ARITH_FAST)
    model.set_atm(case.atm)
    k = model.kernel(case.atm, obs)
    assert len(case.geom) == 66 and k.shape == k_ref.shape == (66 * nd - 1, 6 + 31 + 21 + 11)
    scale = np.abs(k_ref).max(axis=0)
    live = scale > 0          # with HYDZ >= 0 the pressure columns away from the reference level vanish
    assert live.sum() >= 31 + 21 + 11 and np.all(k[:, ~live] == 0)
    assert np.max(np.abs(k[:, live] - k_ref[:, live]) / scale[live]) < 1e-6
    if extinction:
        assert np.all(live[-11:]) and np.all(np.abs(k[:, -11:]).max(axis=0) > 0)      # the extinction columns are live
    n = obs.nr
    a, b = np.ctypeslib.as_array(obs.rad)[:n, :nd], np.ctypeslib.as_array(obs_ref.rad)[:n, :nd]
    fin = np.isfinite(b)
    assert np.array_equal(fin, np.isfinite(a)) and common.rel_err(a[fin], b[fin]).max() < RTOL
    # the model is left with the caller's atmosphere
    again = model.formod_host(case.geom)
    assert common.rel_err(again["rad"][fin], b[fin]).max() < RTOL
    model.close()


DROPIN_KERNEL = r"""
import os, sys
sys.path[:0] = [{root!r}, os.path.join({root!r}, 'jurassic-gpu_amd'), os.path.join({root!r}, 'tests')]
import numpy as np, common
from oracle import orc
from jurassic_hip import abi, lib, textio
case = common.limb_case(useGPU=1)
c = case.ctl
c.rett_zmin, c.rett_zmax = 10.0, 40.0
c.retq_zmin[2], c.retq_zmax[2] = 15.0, 35.0
case.write_files({tmp!r}, base='boxcar')
tb = orc.Tables(c.ng, c.nd); assert tb.read_ascii(c) == 0 and tb.planck_filt(c) == 0

def obs_of(geom):
    o = abi.obs_t()
    o.nr = len(geom)
    for k, name in enumerate(textio.OBS_COLS[:7]):
        np.ctypeslib.as_array(getattr(o, name))[:o.nr] = geom[:, k]
    return o
obs_ref, obs = obs_of(case.geom), obs_of(case.geom)
for o in (obs_ref, obs):
    o.rad[3][0] = float('nan')                         # a masked measurement drops its row
k_ref = orc.kernel(c, case.atm, obs_ref, tb)
m, n = k_ref.shape
assert (m, n) == (66 * 2 - 1, 31 + 21)
k = lib.kernel(c, case.atm, obs, m, n, tda=n + 5)      # the reference's symbol, a gsl_matrix with tda > size2
scale = np.abs(k_ref).max(axis=0)
assert np.max(np.abs(k - k_ref) / scale) < 1e-6
a, b = np.ctypeslib.as_array(obs.rad)[:66, :2], np.ctypeslib.as_array(obs_ref.rad)[:66, :2]
fin = np.isfinite(b)
assert np.array_equal(fin, np.isfinite(a)) and np.max(np.abs(a[fin] - b[fin]) / b[fin]) < 1e-9
again = obs_of(case.geom)
lib.formod(c, case.atm, again)                         # the lane is left with the caller's atmosphere
assert np.max(np.abs(np.ctypeslib.as_array(again.rad)[:66, :2][fin] - b[fin]) / b[fin]) < 1e-9
print('DROPIN_KERNEL_OK')
"""


def test_drop_in_kernel_symbol_takes_a_gsl_matrix(hip, oracle, tmp_path):
    """kernel(ctl, atm, obs, gsl_matrix *) under its own name (jurassic.c:812-857): tables from the files ctl names,
    the Jacobian written into a matrix whose row stride exceeds its width, a masked measurement dropped, obs left with
    the unperturbed forward model -- against the oracle's restatement of the reference loop."""
    script = tmp_path / "dropin_kernel.py"
    script.write_text(DROPIN_KERNEL.format(root=common.ROOT, tmp=str(tmp_path)))
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "DROPIN_KERNEL_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_jacobian_columns_are_as_near_the_derivative_as_the_reference_ones(hip, oracle):
    """Difference quotients divide the rounding noise of y by h.  For optically thin rays the ALGORITHM forms a segment's
    emissivity as 1 - (1 - 1e-9): y is good to ~1e-12 relative only, in the reference as here, and implementations that
    round differently disagree by that much per column whatever the look-up's arithmetic (tools/bench_jacobian.py:
    profiles/r04_jacobian_limb_example.json has all 728 columns of the limb example).  The yardstick is a central
    difference of the ORACLE with four times the reference's step (noise / 5.7, third-order truncation): per column, the
    GPU's forward differences -- both arithmetics -- must lie no further from it than the oracle's own forward
    differences do, up to 0.2 % of the column's norm.  Trace-gas columns at high altitude, where h is smallest, included."""
    import copy
    case = common.limb_case()
    c = case.ctl
    c.retp_zmin, c.retp_zmax, c.rett_zmin, c.rett_zmax = 30.0, 34.0, 30.0, 34.0
    for g in range(c.ng):
        c.retq_zmin[g], c.retq_zmax[g] = -999.0, -999.0
    c.retq_zmin[1], c.retq_zmax[1] = 60.0, 90.0          # H2O at the top: mixing ratios of 1e-6 .. 1e-7, h = 1 % of that
    c.retq_zmin[3], c.retq_zmax[3] = 20.0, 30.0          # F11
    tb = case.oracle_tables(oracle)
    obs_ref = _obs_from_geom(case.geom, 2)
    k_ref = oracle.kernel(c, case.atm, obs_ref, tb)
    n0 = case.atm.np
    z = np.ctypeslib.as_array(case.atm.z)[:n0]
    cols = ([("p", i) for i in range(n0) if 30 <= z[i] <= 34] + [("t", i) for i in range(n0) if 30 <= z[i] <= 34] +
            [(1, i) for i in range(n0) if 60 <= z[i] <= 90] + [(3, i) for i in range(n0) if 20 <= z[i] <= 30])
    assert len(cols) == k_ref.shape[1]

    def field(a, kind):
        return (np.ctypeslib.as_array(a.p) if kind == "p" else np.ctypeslib.as_array(a.t) if kind == "t"
                else np.ctypeslib.as_array(a.q)[kind])
    k_c = np.zeros_like(k_ref)
    for j, (kind, lev) in enumerate(cols):
        x0 = field(case.atm, kind)[lev]
        h = max(abs(0.01 * x0), 1e-7) if kind == "p" else 1.0 if kind == "t" else max(abs(0.01 * x0), 1e-15)   # jurassic.c:831-837
        y = []
        for sign in (+1, -1):
            a = copy.deepcopy(case.atm)
            field(a, kind)[lev] = x0 + sign * 4 * h
            y.append(oracle.formod_rays(c, a, tb, case.geom)["rad"].ravel())
        k_c[:, j] = (y[0] - y[1]) / (8 * h)
    scale = np.linalg.norm(k_c, axis=0)
    d_ref = np.linalg.norm(k_ref - k_c, axis=0)
    model = hip.Model(c, case.lib_tables())
    model.set_atm(case.atm)
    for mode in (hip.ARITH_FAST, hip.ARITH_EXACT):
        model.set_arithmetic(mode)
        k = model.kernel(case.atm, _obs_from_geom(case.geom, 2))
        excess = (np.linalg.norm(k - k_c, axis=0) - d_ref) / scale
        print("mode %d: columns further from the central differences than the oracle's %d of %d, worst excess %.2e of the "
              "column norm (oracle's own distance: up to %.2e)" % (mode, np.count_nonzero(excess > 0), len(cols), excess.max(), (d_ref / scale).max()))
        assert excess.max() < 2e-3
    model.close()


def test_large_batch_properties(hip, oracle):
    """One GPU's share of BASELINE configs[3] at full size: 1 250 000 of the 1e7 limb rays (rank 3 of 8 of the
    index-addressable set bench.py shards; 4 channels, 5 emitters, 64 profiles) -- more than configs[2]'s 1e6 rays, in
    ONE launch per kernel (120 GB workspace).  Properties that need no oracle run at that size, plus a sampled
    oracle comparison."""
    import bench
    from jurassic_hip import shard
    lo, hi = shard.ray_range(3, 8, 10_000_000)
    nr = hi - lo
    assert nr == 1_250_000
    geom = bench.workload_rays("limb_1e7_sharded", np.arange(lo, hi))
    case = common.limb_case(geom=geom[:8], nu=common.CTM4_NU, nprofiles=64)
    model = hip.Model(case.ctl, case.lib_tables())
    model.set_atm(case.atm)
    a = model.formod_host(geom)
    assert np.isfinite(a["rad"]).all() and np.all((a["tau"] >= 0) & (a["tau"] <= 1))
    assert a["np"].min() >= 100 and a["np"].max() < abi.NLOS
    # idempotence and independence of the chunking: bit-identical
    model.set_chunk_rays(40000)
    b = model.formod_host(geom)
    for k in ("rad", "tau", "tp", "np"):
        assert np.array_equal(a[k], b[k]), k
    # rays are independent: a permutation of the input permutes the output, bit for bit
    perm = np.random.default_rng(0).permutation(nr)[:200_000]
    c = model.formod_host(geom[perm])
    assert np.array_equal(c["rad"], a["rad"][perm]) and np.array_equal(c["tau"], a["tau"][perm])
    # sampled comparison with the oracle
    idx = np.random.default_rng(1).choice(nr, 3000, replace=False)
    ref = oracle.formod_rays(case.ctl, case.atm, case.oracle_tables(oracle), geom[idx])
    assert np.array_equal(a["np"][idx], ref["np"])
    worst = common.rel_err(a["rad"][idx], ref["rad"]).max()
    print("1.25e6 limb rays, 3000 sampled against the oracle: worst relative radiance deviation %.2e" % worst)
    assert worst < RTOL
    assert np.all(np.abs(a["tau"][idx] - ref["tau"]) <= RTOL * np.abs(ref["tau"]) + common.tau_atol(ref["tau"]))
    model.close()


def test_bench_dump_outputs_are_the_timed_path_results(hip, oracle, tmp_path):
    """A plain `bench.py --dump-outputs DIR` run: what its last timed step computed -- the batched kernels on the headline
    workload's rays, tables and profiles at 20 000 rays -- as the caller receives it, sampled against the oracle."""
    import bench
    nr = 20_000
    out = subprocess.run([sys.executable, os.path.join(common.ROOT, "bench.py"), "--rays", str(nr), "--steps", "2",
                          "--warmup", "1", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    doc = json.loads(out.stdout)
    assert doc["steps"] == 2 and doc["full"] is False and doc["config"]["rays_total"] == nr and doc["ms_per_step"] > 0
    a = {k: np.load(tmp_path / (k + ".npy")) for k in ("rad", "tau", "tp", "np")}
    assert [a[k].shape for k in ("rad", "tau", "tp", "np")] == [(nr, 4), (nr, 4), (nr, 3), (nr,)]
    assert all(v.dtype == np.float64 for v in a.values())
    idx = np.sort(np.random.default_rng(3).choice(nr, 400, replace=False))
    case = bench.build_case("limb_1e6", bench.workload_rays("limb_1e6", idx))
    ref = oracle.formod_rays(case.ctl, case.atm, case.oracle_tables(oracle), case.geom)
    assert np.array_equal(a["np"][idx], ref["np"])
    assert common.rel_err(a["rad"][idx], ref["rad"]).max() < RTOL
    assert np.all(np.abs(a["tau"][idx] - ref["tau"]) <= RTOL * np.abs(ref["tau"]) + common.tau_atol(ref["tau"]))
    assert np.abs(a["tp"][idx] - ref["tp"]).max() < 1e-9


def test_nadir_1e5_properties(hip, oracle):
    """BASELINE configs[1] at full size (1e5 nadir observations, CO2, the three AIRS channels of example/nadir,
    brightness temperatures, every ray ends on the ground): properties that need no oracle run at that size,
    plus a sampled oracle comparison."""
    nr = 100_000
    geom = synth.nadir_geometry(nr, seed=1000)
    case = common.nadir_case(geom=geom[:8])
    model = hip.Model(case.ctl, case.lib_tables())
    model.set_atm(case.atm)
    a = model.formod_host(geom)
    assert np.isfinite(a["rad"]).all() and np.all((a["tau"] >= 0) & (a["tau"] <= 1))
    assert np.all((a["rad"] > 150) & (a["rad"] < 320))                  # brightness temperatures [K]
    assert set(np.unique(a["np"])) <= {181, 182}                         # 181-182 points per nadir ray
    model.set_chunk_rays(7040)                                           # independence of the chunking: bit-identical
    b = model.formod_host(geom)
    for k in ("rad", "tau", "tp", "np"):
        assert np.array_equal(a[k], b[k]), k
    model.set_sort_rays(False)                                           # ... and of the processing order
    c = model.formod_host(geom)
    assert np.array_equal(a["rad"], c["rad"]) and np.array_equal(a["tau"], c["tau"])
    perm = np.random.default_rng(0).permutation(nr)[:30_000]             # rays are independent
    d = model.formod_host(geom[perm])
    assert np.array_equal(d["rad"], a["rad"][perm]) and np.array_equal(d["tau"], a["tau"][perm])
    idx = np.random.default_rng(1).choice(nr, 3000, replace=False)
    ref = oracle.formod_rays(case.ctl, case.atm, case.oracle_tables(oracle), geom[idx])
    assert np.array_equal(a["np"][idx], ref["np"])
    assert common.rel_err(a["rad"][idx], ref["rad"]).max() < RTOL
    assert np.all(np.abs(a["tau"][idx] - ref["tau"]) <= RTOL * np.abs(ref["tau"]) + common.tau_atol(ref["tau"]))
    model.close()


WIDE_FULL = r"""
import os, sys, time
sys.path[:0] = [{root!r}, os.path.join({root!r}, 'jurassic-gpu_amd'), os.path.join({root!r}, 'tests')]
import numpy as np, common
from oracle import orc
from jurassic_hip import abi, lib, shard
import bench
assert (abi.ND, abi.NG) == (2378, 3)
t0 = time.time()
lo, hi = shard.ray_range(5, 8, 1_000_000)                                  # rank 5 of 8 of configs[4]'s 1e6 observations
nr = hi - lo
assert nr == {nr}
geom = bench.workload_rays("airs_2378_sharded", np.arange(lo, hi))
case = bench.AirsCase(geom)         # full-size tables, 33 p x 10 T x ~203 u per pair: 7134 tables, 4.8e8 entries (3.8 GB on
tb = case.lib_tables()              # the device) -- the workload bench.py --workload airs_2378_sharded runs per GPU
assert tb.entries() > 4.5e8
model = lib.Model(case.ctl, tb)
model.set_atm(case.atm)
a = model.formod_host(geom)
assert np.isfinite(a["rad"]).all() and np.all(a["rad"] > 0) and np.all((a["tau"] >= 0) & (a["tau"] <= 1))
assert set(np.unique(a["np"])) <= {{181, 182}}
model.set_chunk_rays(448)                                                  # chunking: bit-identical
sub = slice(0, 20000)
b = model.formod_host(geom[sub])
for k in ("rad", "tau", "tp", "np"):
    assert np.array_equal(a[k][sub], b[k]), k
model.set_chunk_rays(1 << 21)
perm = np.random.default_rng(0).permutation(nr)[:4096]                     # rays are independent
c = model.formod_host(geom[perm])
assert np.array_equal(c["rad"], a["rad"][perm]) and np.array_equal(c["tau"], a["tau"][perm])
idx = np.random.default_rng(1).choice(nr, 64, replace=False)               # sampled rows against the oracle
orc.set_threads(bench.usable_cores())
ref = orc.formod_rays(case.ctl, case.atm, case.oracle_tables(orc), geom[idx])
assert np.array_equal(a["np"][idx], ref["np"])
worst = np.max(np.abs(a["rad"][idx] - ref["rad"]) / np.abs(ref["rad"]))
assert worst < 1e-9
assert np.all(np.abs(a["tau"][idx] - ref["tau"]) <= 1e-9 * np.abs(ref["tau"]) + common.tau_atol(ref["tau"]))
print('WIDE_FULL_OK', a["rad"].shape, tb.entries(), 'worst rel rad dev %.2e' % worst, '%.0f s' % (time.time() - t0))
"""


def test_2378_channels_full_size_tables(hip, oracle, tmp_path):
    """One GPU's share of BASELINE configs[4] at full size: 125 000 of the 1e6 nadir observations x 2378 channels x 3
    emitters with FULL-size tables (3.8 GB: beyond L2 and Infinity Cache) -- what `bench.py --workload
    airs_2378_sharded` runs per GPU.  The property checks of the other bench-size tests plus 64 sampled observations
    (152 000 radiances) against the oracle.  Own process: the ND=2378 build."""
    script = tmp_path / "wide_full.py"
    script.write_text(WIDE_FULL.format(root=common.ROOT, nr=125000))
    env = dict(os.environ, JUR_ND="2378", JUR_NG="3", JUR_SUFFIX="_nd2378")
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=1500, env=env)
    assert out.returncode == 0 and "WIDE_FULL_OK (125000, 2378)" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    print(out.stdout.strip().splitlines()[-1])


WIDE_BEYOND = r"""
import os, sys, time
sys.path[:0] = [{root!r}, os.path.join({root!r}, 'jurassic-gpu_amd'), os.path.join({root!r}, 'tests')]
import numpy as np, common
from oracle import orc
from jurassic_hip import abi, lib, synth, textio
import bench
assert (abi.ND, abi.NG) == (2378, 3)
t0 = time.time()
nu = [650.0 + i * (2665.0 - 650.0) / 2377 for i in range(2378)]
em = ["CO2", "H2O", "O3"]
ctl = abi.make_ctl(em, nu)
atm = textio.read_atm(os.path.join(common.GOLD, "limb", "atm.tab"), ctl)
# 40 pressure levels (the reference's TBLNP) x 10 T x ~203 u = 81 200 entries per pair; the same three tables for all
# 2378 channels -- what is tested is the addressing of 7134 x 81 200 = 5.8e8 entries (4.6 GB), not the spectroscopy
tb, ot = lib.Tables(3, 2378), orc.Tables(3, 2378)
for g, e in enumerate(em):
    rows = synth.table_rows(e, 1000.0, id_=g, nlev=40)
    for d, v in enumerate(nu):
        tb.feed_rows(g, d, rows)
        ot.feed_rows(g, d, rows)
        if g == 0:
            x, f = synth.boxcar_filter(v)
            tb.set_filter(d, x, f)
            ot.planck_shape(d, x, f)
n = tb.entries()
assert n > (1 << 29), n                                  # beyond what 32-bit byte offsets from ONE base could reach
model = lib.Model(ctl, tb)
model.set_atm(atm)
geom = np.vstack([bench.workload_rays("airs_2378_sharded", np.arange(448)), synth.limb_geometry(64, seed=3)])
a = model.formod_host(geom)
assert np.isfinite(a["rad"]).all() and np.all((a["tau"] >= 0) & (a["tau"] <= 1))
# the last channels' tables lie beyond entry 2^29: all of them against the oracle for a sample of rays
idx = np.r_[np.arange(0, 448, 56), 448 + np.arange(0, 64, 16)]
orc.set_threads(bench.usable_cores())
ref = orc.formod_rays(ctl, atm, ot, geom[idx])
assert np.array_equal(a["np"][idx], ref["np"])
worst = np.max(np.abs(a["rad"][idx] - ref["rad"]) / np.abs(ref["rad"]))
assert worst < 1e-9, worst
assert np.all(np.abs(a["tau"][idx] - ref["tau"]) <= 1e-9 * np.abs(ref["tau"]) + common.tau_atol(ref["tau"]))
# same tables for every channel of a gas and the same continuum-free physics? no: channels differ (continua, source
# function); but two models must agree bit for bit however the set is laid out: channels 0 .. 99 alone (well below 2^29)
sub = abi.make_ctl(em, nu[2278:])
tb2 = lib.Tables(3, 100)
for g, e in enumerate(em):
    rows = synth.table_rows(e, 1000.0, id_=g, nlev=40)
    for d in range(100):
        tb2.feed_rows(g, d, rows)
        if g == 0:
            tb2.set_filter(d, *synth.boxcar_filter(nu[2278 + d]))
m2 = lib.Model(sub, tb2)
m2.set_atm(textio.read_atm(os.path.join(common.GOLD, "limb", "atm.tab"), sub))
b = m2.formod_host(geom[idx])
assert np.array_equal(b["rad"], a["rad"][idx][:, 2278:]) and np.array_equal(b["tau"], a["tau"][idx][:, 2278:])
print('WIDE_BEYOND_OK', n, 'worst rel rad dev %.2e' % worst, '%.0f s' % (time.time() - t0))
"""


def test_table_set_beyond_two_to_the_29_entries(hip, oracle, tmp_path):
    """Full-extent many-channel sets (reference limits TBLNP/TBLNT/TBLNU = 40/30/304, jurassic.h:179-193: 2.6e9 entries
    for 2378 channels x 3 gases) do not fit 32-bit byte offsets from one base; the kernels address (gas, channel) pairs
    from a 64-bit wave-uniform base with 32-bit offsets inside the pair.  5.8e8 entries here (the round-2 library refused
    anything >= 2^29): 12 sampled rays x 2378 channels against the oracle, and the top 100 channels -- whose tables lie
    beyond entry 2^29 -- bit-identical to a 100-channel model of their own."""
    script = tmp_path / "wide_beyond.py"
    script.write_text(WIDE_BEYOND.format(root=common.ROOT))
    env = dict(os.environ, JUR_ND="2378", JUR_NG="3", JUR_SUFFIX="_nd2378")
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=1500, env=env)
    assert out.returncode == 0 and "WIDE_BEYOND_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    print(out.stdout.strip().splitlines()[-1])


def test_host_entry_with_pinned_and_pageable_arrays(hip):
    """jur_formod_host above the package size: arrays in pinned memory (jur_host_alloc) travel in place, pageable
    ones through the model's pinned image, copies overlapped with the kernels on a second stream -- same bits as
    the device-pointer entry either way, NaN mask included."""
    nr = 150_000
    case = common.limb_case(geom=synth.limb_geometry(nr, seed=31, nprofiles=4), nu=common.CTM4_NU, nprofiles=4)
    model = hip.Model(case.ctl, case.lib_tables())
    model.set_atm(case.atm)
    base = model.formod_host(case.geom[:60_000])                        # package-sized path (one staged transfer)
    res = {}
    for pinned in (True, False):
        b = model.host_buffers(nr, pinned=pinned)
        b.set_geometry(case.geom)
        b.rad[:] = 0.0
        b.rad[5, 1] = np.nan
        b.rad[nr - 1, 3] = np.inf
        model.formod_host_buffers(b)
        res[pinned] = dict(rad=b.rad.copy(), tau=b.tau.copy(), tp=b.tp.T.copy(), np=b.np.copy())
        b.rad[:] = 0.0
        model.formod_host_buffers(b)                                     # reuse of the staging buffers
        keep = np.ones(nr, bool); keep[[5, nr - 1]] = False
        assert np.array_equal(b.rad[keep], res[pinned]["rad"][keep]) and np.isfinite(b.rad).all()
        b.close()
    for k in ("rad", "tau", "tp", "np"):
        assert np.array_equal(res[True][k], res[False][k], equal_nan=(k == "rad")), k
    r = res[True]
    assert np.isnan(r["rad"][5, 1]) and np.isnan(r["rad"][nr - 1, 3]) and np.isnan(r["rad"]).sum() == 2
    for k in ("rad", "tau", "tp", "np"):
        x, y = r[k][:60_000], base[k]
        m = np.isfinite(x) if k == "rad" else np.ones(x.shape, bool)
        assert np.array_equal(x[m], y[m]), k
    model.close()


def test_isothermal_identity_on_device(hip):
    """rad = B(T) (1 - tau) when T is constant (telescoping of jr_common.h:296-298)."""
    case = common.limb_case(geom=synth.limb_geometry(20000, seed=4), nu=common.CTM4_NU)
    np.ctypeslib.as_array(case.atm.t)[:case.atm.np] = 240.0
    model = hip.Model(case.ctl, case.lib_tables())
    model.set_atm(case.atm)
    out = model.formod_host(case.geom)
    c1, c2 = 1.19104259e-8, 1.43877506
    for d, (x, f) in enumerate(case.filters):
        b = np.sum(f * c1 * x ** 3 / (np.exp(c2 * x / 240.0) - 1)) / f.sum()
        assert np.allclose(out["rad"][:, d], b * (1 - out["tau"][:, d]), rtol=1e-11, atol=0)
    model.close()


def test_device_pointer_entry_matches_host_entry(hip):
    """jur_formod_device on torch-owned HBM buffers and a torch stream."""
    import torch
    case = common.limb_case(geom=synth.limb_geometry(5000, seed=8))
    model = hip.Model(case.ctl, case.lib_tables())
    model.set_atm(case.atm)
    host = model.formod_host(case.geom)
    dev = torch.device("cuda", 0)
    nr, nd = len(case.geom), case.ctl.nd
    d_geom = torch.from_numpy(np.ascontiguousarray(case.geom.T)).to(dev)
    d_rad = torch.zeros((nr, nd), dtype=torch.float64, device=dev)
    d_tau = torch.empty((nr, nd), dtype=torch.float64, device=dev)
    d_tp = torch.empty((3, nr), dtype=torch.float64, device=dev)
    d_np = torch.empty(nr, dtype=torch.int32, device=dev)
    d_st = torch.zeros(1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.formod_device(nr, d_geom.data_ptr(), d_rad.data_ptr(), d_tau.data_ptr(), d_tp.data_ptr(),
                            d_np.data_ptr(), d_st.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert int(d_st.item()) == 0
    assert np.array_equal(d_rad.cpu().numpy(), host["rad"]) and np.array_equal(d_tau.cpu().numpy(), host["tau"])
    assert np.array_equal(d_tp.cpu().numpy().T, host["tp"]) and np.array_equal(d_np.cpu().numpy(), host["np"])
    model.close()


def test_device_entry_can_be_captured_in_a_graph(hip):
    """After jur_model_reserve the device entry only enqueues kernels: capture it into a HIP graph
    (through torch.cuda.graph on a side stream) and replay it on new inputs."""
    import torch
    case = common.limb_case(geom=synth.limb_geometry(1088, seed=12))
    model = hip.Model(case.ctl, case.lib_tables())
    model.set_atm(case.atm)
    dev = torch.device("cuda", 0)
    nr, nd = len(case.geom), case.ctl.nd
    d_geom = torch.from_numpy(np.ascontiguousarray(case.geom.T)).to(dev)
    d_rad = torch.zeros((nr, nd), dtype=torch.float64, device=dev)
    d_tau = torch.zeros((nr, nd), dtype=torch.float64, device=dev)
    d_tp = torch.zeros((3, nr), dtype=torch.float64, device=dev)
    d_st = torch.zeros(1, dtype=torch.int32, device=dev)
    model.reserve(nr)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d_rad.zero_()
        model.formod_device(nr, d_geom.data_ptr(), d_rad.data_ptr(), d_tau.data_ptr(), d_tp.data_ptr(), 0,
                            d_st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    graph.replay()
    torch.cuda.synchronize()
    first = model.formod_host(case.geom)
    assert np.array_equal(d_rad.cpu().numpy(), first["rad"]) and np.array_equal(d_tau.cpu().numpy(), first["tau"])
    other = synth.limb_geometry(nr, seed=13)                 # same buffers, new geometry, replay only
    d_geom.copy_(torch.from_numpy(np.ascontiguousarray(other.T)))
    graph.replay()
    torch.cuda.synchronize()
    second = model.formod_host(other)
    assert np.array_equal(d_rad.cpu().numpy(), second["rad"]) and int(d_st.item()) == 0
    model.close()


def test_nlos_overflow_is_reported(hip):
    """Upstream aborts with 'Too many LOS points!' (jr_common.h:693-695)."""
    case = common.limb_case(geom=synth.limb_geometry(64, scan=True), raydz=0.2)
    model = hip.Model(case.ctl, case.lib_tables())
    model.set_atm(case.atm)
    with pytest.raises(hip.JurassicError, match="Too many LOS points"):
        model.formod_host(case.geom)
    model.close()


def test_fov_convolution_on_device_arrays(hip, oracle):
    """formod_fov (jurassic.c:214-258) as a HIP kernel on results that stay in HBM: three limb scans through
    jur_formod_device, convolved in place by jur_fov_apply_device -- bit-identical to the oracle's restatement
    of formod_fov and to the library's host twin; a ray alone in its scan is refused as upstream aborts."""
    import torch
    scans, per = 3, 40
    geom = np.vstack([synth.limb_geometry(per, scan=True, zmin=5.0, zmax=44.0) for _ in range(scans)])
    geom[:, 0] = np.repeat(np.arange(scans, dtype=float), per)          # one time stamp per scan
    case = common.limb_case(geom=geom)
    base = textio.read_atm(os.path.join(common.GOLD, "limb", "atm.tab"), case.ctl)
    case.atm = synth.stack_profiles(base, case.ctl, scans, seed=3)       # a profile per time stamp
    model = hip.Model(case.ctl, case.lib_tables())
    model.set_atm(case.atm)
    dev = torch.device("cuda", 0)
    nr, nd = len(geom), case.ctl.nd
    d_geom = torch.from_numpy(np.ascontiguousarray(geom.T)).to(dev)
    d_rad = torch.zeros((nr, nd), dtype=torch.float64, device=dev)
    d_tau = torch.zeros((nr, nd), dtype=torch.float64, device=dev)
    d_tp = torch.zeros((3, nr), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    model.formod_device(nr, d_geom.data_ptr(), d_rad.data_ptr(), d_tau.data_ptr(), d_tp.data_ptr(), 0, 0, stream)
    torch.cuda.synchronize()
    rad0, tau0 = d_rad.cpu().numpy().copy(), d_tau.cpu().numpy().copy()
    dz = np.linspace(-1.5, 1.5, 21)
    w = np.exp(-0.5 * (dz / 0.6) ** 2)
    model.fov_apply_device(nr, d_geom[0].data_ptr(), d_geom[4].data_ptr(), d_rad.data_ptr(), d_tau.data_ptr(), dz, w, stream)
    got_r, got_t = d_rad.cpu().numpy(), d_tau.cpu().numpy()
    assert not np.array_equal(got_r, rad0)
    host_r, host_t = rad0.copy(), tau0.copy()                            # the library's host twin
    hip.fov_apply(geom[:, 0], geom[:, 4], host_r, host_t, dz, w)
    assert np.array_equal(got_r.view(np.uint64), host_r.view(np.uint64)) and np.array_equal(got_t.view(np.uint64), host_t.view(np.uint64))
    obs = _obs_from_geom(geom, nd)                                        # the oracle's restatement of formod_fov
    np.ctypeslib.as_array(obs.rad)[:nr, :nd] = rad0
    np.ctypeslib.as_array(obs.tau)[:nr, :nd] = tau0
    assert oracle.formod_fov(case.ctl, obs, dz, w) == 0
    assert np.array_equal(np.ctypeslib.as_array(obs.rad)[:nr, :nd].view(np.uint64), got_r.view(np.uint64))
    assert np.array_equal(np.ctypeslib.as_array(obs.tau)[:nr, :nd].view(np.uint64), got_t.view(np.uint64))
    lone = torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64, device=dev)            # first ray alone in its scan
    with pytest.raises(hip.JurassicError, match="Cannot apply FOV"):
        model.fov_apply_device(3, lone.data_ptr(), d_geom[4].data_ptr(), d_rad.data_ptr(), d_tau.data_ptr(), dz, w, stream)
    model.close()


@pytest.mark.parametrize("nchan", [2, 3, 4, 5, 7])
def test_grouped_radiance_update_kernel_equals_one_channel_per_workgroup(hip, nchan):
    """jur_combine_group_kernel (up to four channels of a ray block as the wavefronts of one workgroup, barriers between
    them; what large launches take) against jur_combine_kernel: the same lane program, so every output must agree BIT
    FOR BIT -- for every group shape (2, 3, 4 channels; a ragged last group for 5 and 7), ragged ray counts, rays
    that miss the atmosphere, masked inputs and every barrier interval."""
    nu = list(np.round(np.linspace(700.0, 2400.0, nchan), 4))
    g = synth.limb_geometry(1500 + 37 * nchan, seed=nchan, nprofiles=3)
    extra = np.array([[0, 780.0, 0, 0, 95.0, 0, 20.0], [1, 30.0, 0, 0, 5.0, 0, 3.0]])      # outside; observer inside
    geom = np.vstack([g[:700], extra, g[700:], synth.nadir_geometry(90, seed=2, nprofiles=3)])
    case = common.Case(["CO2", "H2O", "O3"], nu, os.path.join(common.GOLD, "limb", "atm.tab"), geom, nprofiles=3)
    rad_in = np.zeros((len(geom), nchan))
    rad_in[5, 0] = np.nan
    rad_in[701, nchan - 1] = np.inf
    m = hip.Model(case.ctl, case.lib_tables())
    m.set_atm(case.atm)
    m.set_pencil(0)                                  # the batched kernels
    try:
        hip.tune_combine(0, 8, 0)
        ref = m.formod_host(case.geom, rad_in=rad_in)
        assert np.isnan(ref["rad"][5, 0]) and np.isnan(ref["rad"][701, nchan - 1]) and ref["np"][700] == 0
        for group, sync in ((4, 8), (4, 1), (4, 0), (2, 2), (8, 4)):
            hip.tune_combine(group, sync, 0)
            out = m.formod_host(case.geom, rad_in=rad_in)
            for k in ("rad", "tau", "tp", "np"):
                x, y = np.asarray(out[k]), np.asarray(ref[k])
                assert np.array_equal(np.isnan(x), np.isnan(y)) if x.dtype.kind == "f" else True
                assert np.array_equal(np.nan_to_num(x, nan=-1.0).view(np.uint8), np.nan_to_num(y, nan=-1.0).view(np.uint8)), (k, group, sync)
        # several launches per call (chunks of 448 rays, tracing launches of two chunks) and unsorted rays
        hip.tune_combine(4, 8, 0)
        m.set_chunk_rays(448)
        m.set_trace_multiple(2)
        for sort in (1, 0):
            m.set_sort_rays(sort)
            out = m.formod_host(case.geom, rad_in=rad_in)
            for k in ("rad", "tau", "tp", "np"):
                x, y = np.asarray(out[k]), np.asarray(ref[k])
                assert np.array_equal(np.nan_to_num(x, nan=-1.0).view(np.uint8), np.nan_to_num(y, nan=-1.0).view(np.uint8)), (k, "chunks", sort)
    finally:
        hip.tune_combine(-1, 8, 1_000_000)              # back to the default rule
        m.close()
