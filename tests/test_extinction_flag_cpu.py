"""jur_atm_k_zero on host arrays: the decision whether the kernels may leave the extinction out (jur_view_t::atm_k_zero).
Only rows the caller has set qualify, on a sorted atmosphere, with every extinction value +0.0 bit for bit; the perturbed
atmospheres of kernel() and of the hydrostatic contribution variants and rows stacked on the device never do."""
import numpy as np
import common
from jurassic_hip import lib, synth


def test_all_positive_zeros_qualify():
    assert lib.atm_k_zero(np.zeros((2, 91)))
    assert lib.atm_k_zero(np.zeros(0))                 # no window at all: nothing to interpolate


def test_any_other_value_clears_it():
    for bad in (1e-300, 5e-324, -0.0, -1e-5, np.nan, np.inf):
        for at in (0, 57, 181):
            k = np.zeros((2, 91))
            k.flat[at] = bad
            assert not lib.atm_k_zero(k), (bad, at)


def test_unsorted_atmosphere_never_qualifies():
    assert not lib.atm_k_zero(np.zeros((1, 91)), atm_sorted=False)


def test_perturbed_and_device_rows_never_qualify():
    k = np.zeros((1, 182))
    assert lib.atm_k_zero(k, origin=lib.ATM_CALLER)
    assert not lib.atm_k_zero(k, origin=lib.ATM_PERTURBED)      # kernel(), hydrostatic contribution variants
    assert not lib.atm_k_zero(k, origin=lib.ATM_DEVICE)         # scene Jacobian, retrieval: rows written on the device
    assert not lib.atm_k_zero(k, origin=7)


def test_stacked_example_profiles_carry_no_extinction():
    """The shipped limb profile and its perturbed copies (synth.stack_profiles, the benchmark's atmosphere) hold k = +0.0."""
    case = common.limb_case(nu=common.CTM4_NU, nprofiles=64)
    n, nw = case.atm.np, case.ctl.nw
    assert nw >= 1 and lib.atm_k_zero(np.ctypeslib.as_array(case.atm.k)[:nw, :n])
    common.extinction_profile(case.atm)
    assert not lib.atm_k_zero(np.ctypeslib.as_array(case.atm.k)[:nw, :n])
