"""No extinction work for an atmosphere without extinction (jur_view_t::atm_k_zero, jur_tune_k_elision): where every
extinction value of the atmosphere the caller set is +0.0, the ray tracer writes no extinction fields and their readers
take 0.0 instead of loading.  The interpolation of two zeros is +0.0, so the switch off against the default gives every
output bit for bit -- through the batched kernels, the fused kernel and the contributions (TASK contrib) -- and the flag
clears as soon as one value is anything else, -0.0 included.

130 limb rays (view points -5 .. 70 km: ground hits and short rays among them) over 2 stacked profiles, 2 channels,
2 emitters: two full tiles of 64 slots and a ragged third, and with two profiles one tile straddles two slices."""
import os
import numpy as np
import pytest
import common
from jurassic_hip import synth

pytestmark = pytest.mark.gpu

NR = 130
EMITTERS = ["CO2", "H2O"]


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def make_case(k_value=0.0, **ctl_kw):
    """The case with k = +0.0 everywhere but, where k_value is given, at level 20 of the SECOND profile."""
    g = synth.limb_geometry(NR, seed=11, zmin=-5.0, zmax=70.0, nprofiles=2)
    case = common.Case(EMITTERS, common.LIMB_NU, os.path.join(common.GOLD, "limb", "atm.tab"), g, nprofiles=2, **ctl_kw)
    n = case.atm.np
    k = np.ctypeslib.as_array(case.atm.k)
    k[:, :] = 0.0          # (with two emitters the file's third gas column was read as the extinction)
    k[0, n // 2 + 20] = k_value
    assert case.ctl.nw == 1 and n % 2 == 0 and 10.0 < np.ctypeslib.as_array(case.atm.z)[n // 2 + 20] < 40.0
    return case


@pytest.fixture(scope="module")
def zero_case():
    return make_case()


ENTRIES = ("batched", "fused", "contrib")


def run(hip, case, entry, elision, model=None):
    """-> (dict of output arrays, the model's flag) of one call; elision: what jur_tune_k_elision gets (-1: the default)."""
    m = model or hip.Model(case.ctl, case.lib_tables())
    try:
        hip.tune_k_elision(elision)
        if model is None:
            m.set_atm(case.atm)
        m.set_pencil(10000, 0) if entry == "fused" else m.set_pencil(0)
        flag = m.k_zero()
        out = m.formod_contrib_host(case.geom) if entry == "contrib" else m.formod_host(case.geom)
        return out, flag
    finally:
        hip.tune_k_elision(-1)
        if model is None:
            m.close()


def keys(entry):
    return ("rad", "tau", "tp", "np") + (("rad_c", "tau_c") if entry == "contrib" else ())


def assert_same(a, b, entry, what):
    for key in keys(entry):
        x, y = (a[key], b[key]) if key == "np" else (bits(a[key]), bits(b[key]))
        assert np.array_equal(x, y), (what, entry, key)


@pytest.fixture(scope="module")
def zero_results(hip, zero_case):
    """The all-zero case with the elision off, per entry point: computed once and left alone."""
    return {e: run(hip, zero_case, e, 0)[0] for e in ENTRIES}


@pytest.mark.parametrize("entry", ENTRIES)
def test_zero_extinction_elided_equals_full_work(hip, zero_case, zero_results, entry):
    on, flag_on = run(hip, zero_case, entry, -1)
    _, flag_off = run(hip, zero_case, entry, 0)
    assert flag_on and not flag_off
    assert np.isfinite(on["rad"]).all() and (on["np"] > 0).sum() > 100
    assert_same(on, zero_results[entry], entry, "k = 0")


@pytest.mark.parametrize("entry", ENTRIES)
def test_one_nonzero_value_clears_the_flag(hip, zero_results, entry):
    case = make_case(2e-3)
    on, flag_on = run(hip, case, entry, -1)
    off, _ = run(hip, case, entry, 0)
    assert not flag_on
    assert_same(on, off, entry, "one k > 0")
    # ... and the value is seen: rays of the second profile through its level change, the first profile's do not
    diff = np.any(bits(on["rad"]) != bits(zero_results[entry]["rad"]), axis=1)
    second = case.geom[:, 0] == 1
    assert diff[second].sum() > 10 and not diff[~second].any()
    if entry == "contrib":
        ng = len(EMITTERS)
        assert np.any(bits(on["tau_c"][ng]) != bits(zero_results[entry]["tau_c"][ng]))


@pytest.mark.parametrize("entry", ENTRIES)
def test_negative_zero_clears_the_flag(hip, zero_results, entry):
    case = make_case(-0.0)
    assert np.signbit(np.ctypeslib.as_array(case.atm.k)[0, case.atm.np // 2 + 20])
    on, flag_on = run(hip, case, entry, -1)
    off, _ = run(hip, case, entry, 0)
    assert not flag_on
    assert_same(on, off, entry, "k = -0.0")


def test_kernel_with_an_extinction_column(hip):
    """kernel() perturbs the extinction of a column: its stacked atmospheres never take the elision, whatever the switch
    says, and the caller's atmosphere is elided again afterwards."""
    case = make_case()
    c = case.ctl
    c.rett_zmin, c.rett_zmax = 20.0, 24.0
    c.retk_zmin[0], c.retk_zmax[0] = 10.0, 20.0
    jac = {}
    for elision in (-1, 0):
        m = hip.Model(c, case.lib_tables())
        try:
            hip.tune_k_elision(elision)
            m.set_atm(case.atm)
            obs = common.obs_from_geom(case.geom, c.nd)
            jac[elision] = (m.kernel(case.atm, obs), np.ctypeslib.as_array(obs.rad)[:NR, :c.nd].copy(), m.k_zero())
        finally:
            hip.tune_k_elision(-1)
            m.close()
    (k_on, rad_on, flag_on), (k_off, rad_off, flag_off) = jac[-1], jac[0]
    assert flag_on and not flag_off
    assert k_on.shape[1] > 4 and np.isfinite(k_on).all()
    assert np.array_equal(bits(k_on), bits(k_off)) and np.array_equal(bits(rad_on), bits(rad_off))
    nk = int(np.sum((np.ctypeslib.as_array(case.atm.z)[:case.atm.np] >= 10.0) & (np.ctypeslib.as_array(case.atm.z)[:case.atm.np] <= 20.0)))
    assert np.any(k_on[:, -nk:] != 0.0)                # the extinction columns are there and not empty


@pytest.mark.parametrize("entry", ("batched", "fused"))
def test_model_reused_across_atmospheres_follows_the_flag(hip, zero_case, zero_results, entry):
    some = make_case(2e-3)
    fresh_some, _ = run(hip, some, entry, 0)
    m = hip.Model(zero_case.ctl, zero_case.lib_tables())
    try:
        for case, want, expect in ((zero_case, True, zero_results[entry]), (some, False, fresh_some),
                                   (zero_case, True, zero_results[entry])):
            m.set_atm(case.atm)
            out, flag = run(hip, case, entry, -1, model=m)
            assert flag == want
            assert_same(out, expect, entry, "reused model")
    finally:
        m.close()
