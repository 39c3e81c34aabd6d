"""What Model.set_scene_overflow rests on without a GPU: the rule jur_np_overflows, the constants of the header and of
lib.py, and the policy jur_retrieve_decide on a failed slice and on trials whose costs are all NaN (the policy itself
is unchanged: these cases were its contract before)."""
import os
import re
import numpy as np
from jurassic_hip import abi, lib as hip

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jurassic_hip.h")


def header_constant(name):
    text = open(HEADER).read()
    m = re.search(r"\b%s\s*=\s*(-?\d+)" % name, text)
    assert m, name
    return int(m.group(1))


def test_the_rule_counts_a_ray_that_fills_the_array():
    """the tracer clamps to NLOS - 1 points and keeps no flag per ray: a ray that fills the array counts, clamped or not"""
    assert not hip.np_overflows(abi.NLOS - 2)
    assert hip.np_overflows(abi.NLOS - 1)
    assert hip.np_overflows(abi.NLOS)
    assert not hip.np_overflows(0) and not hip.np_overflows(2)


def test_the_constants_are_the_headers():
    for py, c in (("OVERFLOW_ERROR", "JUR_OVERFLOW_ERROR"), ("OVERFLOW_ISOLATE", "JUR_OVERFLOW_ISOLATE"), ("RET_FAILED", "JUR_RET_FAILED"),
                  ("TRIAL_OVERFLOW", "JUR_TRIAL_OVERFLOW"), ("RET_ACTIVE", "JUR_RET_ACTIVE"), ("RET_CONVERGED", "JUR_RET_CONVERGED"),
                  ("RET_STALLED", "JUR_RET_STALLED"), ("RET_MAXITER", "JUR_RET_MAXITER")):
        assert getattr(hip, py) == header_constant(c), py
    assert (hip.OVERFLOW_ERROR, hip.OVERFLOW_ISOLATE, hip.RET_FAILED, hip.TRIAL_OVERFLOW) == (0, 1, 4, -2)
    assert len({hip.RET_ACTIVE, hip.RET_CONVERGED, hip.RET_STALLED, hip.RET_MAXITER, hip.RET_FAILED}) == 5


def test_the_policy_leaves_a_failed_slice_alone():
    J = np.array([10.0, np.nan, 10.0])
    Jt = np.array([[5.0, 1.0, 12.0], [6.0, 2.0, 11.0]])
    lamt = np.array([[0.1, 0.1, 0.1], [10.0, 10.0, 10.0]])
    status = np.zeros((2, 3), dtype=np.int32)
    lam = np.array([1.0, 3.0, 1.0])
    state = np.array([hip.RET_ACTIVE, hip.RET_FAILED, hip.RET_ACTIVE], dtype=np.int32)
    d = hip.retrieve_decide(J, Jt, lamt, status, lam, state, 0.0, 1e6, 10.0)
    assert d["state"][1] == hip.RET_FAILED and d["best"][1] == -1 and d["accept"][1] == -1
    assert d["lam"][1] == 3.0
    assert (d["best"][0], d["accept"][0], d["lam"][0]) == (0, 1, 0.1)
    assert (d["best"][2], d["accept"][2], d["lam"][2]) == (1, 0, 10.0)


def test_the_policy_rejects_a_slice_whose_every_trial_is_nan():
    """what a trial pass in which every damping overflowed hands to the policy: no candidate, a rejection, lam * fac_max
    -- and JUR_RET_STALLED once lam stands at lam_max"""
    nan = np.nan
    J = np.array([10.0, 10.0, 10.0])
    Jt = np.array([[nan, nan, nan], [nan, 4.0, nan]])
    lamt = np.array([[0.1, 0.1, 100.0], [10.0, 10.0, 100.0]])
    status = np.zeros((2, 3), dtype=np.int32)
    lam = np.array([1.0, 1.0, 100.0])
    state = np.zeros(3, dtype=np.int32)
    d = hip.retrieve_decide(J, Jt, lamt, status, lam, state, 0.0, 100.0, 10.0)
    assert (d["best"][0], d["accept"][0], d["lam"][0], d["state"][0]) == (-1, 0, 10.0, hip.RET_ACTIVE)
    assert (d["best"][1], d["accept"][1], d["lam"][1], d["state"][1]) == (1, 1, 10.0, hip.RET_ACTIVE)
    assert (d["best"][2], d["accept"][2], d["lam"][2], d["state"][2]) == (-1, 0, 100.0, hip.RET_STALLED)
