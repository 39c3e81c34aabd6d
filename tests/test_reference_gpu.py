"""The HIP path against what the reference's own CPU forward model returned (tests/golden/reference_runs/, written by
tools/make_reference_goldens.py; tests/test_reference_cpu.py holds them against a live run and the inputs' hashes
against the manifest).  Nothing here loads the reference's library or reads its tree.

Every formod case of tests/refcases.py, through Model.formod_host in the three arrangements of
tests/test_scenes_gpu.py, under both arithmetics of the look-up, and through the drop-in formod(); the two
Jacobians through kernel().  The model's tables are READ FROM THE FILES the reference read (the %.9g text of the rows,
not the rows in memory: those differ by 2.7e-8 relative on radiances).

Bounds, the project's own: 1e-9 relative on radiances, 1e-9 relative + common.tau_atol on transmittances, 1e-9 km on the
tangent altitude, 0.1 mm between the tangent points as Cartesian positions, Jacobians within 1e-6 of each column's
largest entry.  On the rays refcases.departing names from the inputs (the reference reads los[-1] there,
DESIGN.md section 2) the kernels must give what the oracle gives: no LOS points, no radiance, unit transmittance, the
view point as tangent point.  Measured maxima per arrangement: tests/golden/README.md."""
import os
import subprocess
import sys
import numpy as np
import pytest
import common
import refcases as R
from jurassic_hip import abi, synth

pytestmark = pytest.mark.gpu
RTOL = 1e-9
ARRANGEMENTS = ("fused", "batched", "batched_grouped")
_cases = {}


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert os.path.exists(lib.SO), "libjurassic_hip.so missing: the HIP path must be built"
    return lib


def case_on_disk(name, tmp_path_factory):
    if name not in _cases:
        case, rad_in = R.FORMOD[name]()
        case.write_files(str(tmp_path_factory.mktemp(name)))
        _cases[name] = (case, rad_in, R.departing(case))
    return _cases[name]


def assert_against_reference(label, out, ref, case, dep):
    ok = ~dep
    fin = np.isfinite(ref["rad"])
    assert np.array_equal(fin[ok], np.isfinite(out["rad"])[ok])
    use = fin & ok[:, None]
    rerr = common.rel_err(out["rad"][use], ref["rad"][use]).max(initial=0.0)
    terr = np.abs(out["tau"] - ref["tau"])[ok]
    allow = (RTOL * np.abs(ref["tau"]) + common.tau_atol(ref["tau"]))[ok]
    zerr = np.abs(out["tp"][ok, 0] - ref["tp"][ok, 0]).max(initial=0.0)
    d = np.linalg.norm(synth._cart(*out["tp"][ok].T) - synth._cart(*ref["tp"][ok].T), axis=1).max(initial=0.0)
    print("REFGPU %s rad_rel %.3e tau_abs %.3e tau_over_allowance %.3e tpz_km %.3e tp_km %.3e"
          % (label, rerr, terr.max(initial=0.0), (terr / allow).max(initial=0.0), zerr, d))
    assert rerr < RTOL
    assert np.all(terr <= allow)
    assert zerr < 1e-9
    assert d < 1e-7                                          # km: 0.1 mm
    if "np" in out:
        assert np.all(out["np"][dep] == 0)
    assert np.all(out["rad"][dep] == 0) and np.all(out["tau"][dep] == 1)
    assert np.array_equal(out["tp"][dep], case.geom[dep][:, 4:7])


@pytest.mark.parametrize("arith", ["fast", "exact"])
@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
@pytest.mark.parametrize("name", list(R.FORMOD))
def test_formod_host_against_stored_reference(hip, tmp_path_factory, name, arrangement, arith):
    case, rad_in, dep = case_on_disk(name, tmp_path_factory)
    model = hip.Model(case.ctl)                              # tables and filters from the files
    if arrangement != "fused":
        model.set_pencil(0)
    if arrangement == "batched_grouped":
        hip.tune_combine(4, 8, 0)
    try:
        model.set_arithmetic(hip.ARITH_EXACT if arith == "exact" else hip.ARITH_FAST)
        model.set_atm(case.atm)
        out = model.formod_host(case.geom, rad_in=rad_in)
    finally:
        if arrangement == "batched_grouped":
            hip.tune_combine(-1, 8, 1_000_000)
        model.close()
    assert_against_reference("%s %s %s" % (name, arrangement, arith), out, R.stored(name), case, dep)


@pytest.fixture(scope="module")
def dropin_results(hip, tmp_path_factory):
    """One child process runs the drop-in formod() on every case (refcases._dropin_child)."""
    out = tmp_path_factory.mktemp("dropin")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([common.ROOT, os.path.join(common.ROOT, "jurassic-gpu_amd"),
                                                       os.path.join(common.ROOT, "tests")]))
    r = subprocess.run([sys.executable, os.path.join(common.ROOT, "tests", "refcases.py"), str(out)], capture_output=True,
                       text=True, timeout=900, env=env)
    return str(out), r


@pytest.mark.parametrize("name", list(R.FORMOD))
def test_drop_in_formod_against_stored_reference(dropin_results, tmp_path_factory, name):
    out, r = dropin_results
    path = os.path.join(out, name + ".npy")
    assert os.path.exists(path), "the child ended (status %d) before %s:\n%s" % (r.returncode, name, (r.stdout + r.stderr)[-3000:])
    a = np.load(path)
    nd = (a.shape[1] - 3) // 2
    res = dict(rad=a[:, :nd], tau=a[:, nd:2 * nd], tp=a[:, 2 * nd:])
    case, rad_in, dep = case_on_disk(name, tmp_path_factory)
    assert_against_reference("%s dropin fast" % name, res, R.stored(name), case, dep)


@pytest.mark.parametrize("arith", ["fast", "exact"])
@pytest.mark.parametrize("name", list(R.JACOBIANS))
def test_kernel_against_stored_reference(hip, tmp_path, name, arith):
    case, obs = R.jacobian_case(name)
    case.write_files(str(tmp_path))
    k_ref = R.stored(name)
    model = hip.Model(case.ctl)
    try:
        model.set_arithmetic(hip.ARITH_EXACT if arith == "exact" else hip.ARITH_FAST)
        model.set_atm(case.atm)
        k = model.kernel(case.atm, obs)
    finally:
        model.close()
    assert len(case.geom) == 66 and k.shape == k_ref.shape == (66 * case.ctl.nd - 1, 6 + 31 + 21 + 11)
    scale = np.abs(k_ref).max(axis=0)
    live = scale > 0
    assert live.sum() >= 31 + 21 + 11 and np.all(k[:, ~live] == 0)
    worst = np.max(np.abs(k[:, live] - k_ref[:, live]) / scale[live])
    print("REFGPU %s kernel %s jac_rel %.3e" % (name, arith, worst))
    assert worst < 1e-6
