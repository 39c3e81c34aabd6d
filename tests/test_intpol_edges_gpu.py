"""jur_intpol_kernel (behind jur_intpol_atm) at the constructed edges of tests/edgecases.py: the cases of
tests/test_intpol_edges_cpu.py on the device, against the oracle and against the extended-precision model.

NaN positions are the oracle's.  T, q and k are pure IEEE arithmetic in the reference's order and equal the oracle bit for
bit; so does p under IP 3 and wherever a level without pressure makes it linear.  Elsewhere p passes through the
device's exp and log: the project's allowance for that is a relative 1e-13 (test_hip_regridding_matches_the_oracle), and
as the condition number of exp grows with its exponent E, 1e-13 (1 + |E|) here, E from the model (under IP 2 the blend of
the two profiles' allowances); the cases keep |E| <= 10.  Every finite value lies within twice the model's derived bound
(edgecases' docstring), p with the device's allowance on top."""
import ctypes as C
import numpy as np
import pytest
import edgecases as E
from jurassic_hip import abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


@pytest.mark.parametrize("name", E.intpol_case_names())
def test_kernel_regridding_at_constructed_edges(hip, oracle, name):
    case, val, bnd, pexp, hits = E.intpol_ref(name)
    for j, (hit, expect) in enumerate(zip(hits, case["expect"])):
        assert hit == expect, (name, j, sorted(hit), sorted(expect))
    ctl, src = E.intpol_ctl(case["ip"], case["cx"], case["cz"]), E.to_atm(case["src"])
    dest, ref = E.dest_atm(case["z"], case["lon"], case["lat"]), abi.atm_t()
    C.memmove(C.byref(ref), C.byref(dest), C.sizeof(abi.atm_t))
    assert oracle.intpol_atm(ctl, ref, src) == 0
    hip.intpol_atm(ctl, dest, src)
    a, b = E.rows_of(dest), E.rows_of(ref)
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan)
    assert np.all(nan.all(axis=0) | ~nan.any(axis=0))                       # p, T, q and k together or not at all
    ok = ~nan
    same = ok.copy()
    same[0] &= (pexp[0] == 0)                                               # p: where no exp and log enter
    assert np.array_equal(E.bits(a[same]), E.bits(b[same])), name
    dev = 1e-13 * pexp                                                      # 1e-13 |p| (1 + |E|)
    through = ok[0] & (pexp[0] > 0)
    assert case["ip"] == 3 or through.any()
    worst = float(np.max(np.abs(a[0, through] - b[0, through]) / dev[0, through].astype(np.float64))) if through.any() else 0.0
    print("intpol %-50s kernel p against the oracle: worst difference / allowed = %.3f" % (name, worst))
    assert worst <= 1
    ratio = E.intpol_check(a, val, bnd, extra=dev)
    print("intpol %-50s kernel against the model: worst error / allowed = %.3f" % (name, ratio))
    assert ratio <= 1
