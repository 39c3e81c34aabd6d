"""retrieve_decide (jur_retrieve_decide): the accept/reject policy of one iteration of Model.retrieve_scene, host
arithmetic without a GPU, against a restatement in numpy scalars on seeded batches.  Everything is compared exactly: the
policy only compares, copies, and forms lam * fac_max, J - Jt and tol * J, one IEEE operation each."""
import numpy as np
import pytest
from jurassic_hip import lib as hip

NLAM = 4


def restated(J, Jt, lamt, status, lam, state, tol, lam_max, fac_max):
    lam, state = lam.copy(), state.copy()
    ns = len(J)
    best, accept = np.full(ns, -1, dtype=np.int32), np.full(ns, -1, dtype=np.int32)
    for s in range(ns):
        if state[s] != hip.RET_ACTIVE:
            continue
        b = -1
        for l in range(Jt.shape[0]):
            if status[l, s] != 0 or np.isnan(Jt[l, s]):
                continue
            if b < 0 or Jt[l, s] < Jt[b, s]:
                b = l
        best[s] = b
        accept[s] = 1 if (b >= 0 and Jt[b, s] < J[s]) else 0
        if accept[s]:
            lam[s] = lamt[b, s]
            if np.float64(J[s]) - np.float64(Jt[b, s]) <= np.float64(tol) * np.float64(J[s]):
                state[s] = hip.RET_CONVERGED
        elif lam[s] == lam_max:
            state[s] = hip.RET_STALLED
        else:
            lam[s] = min(np.float64(lam[s]) * np.float64(fac_max), np.float64(lam_max))
    return dict(lam=lam, state=state, best=best, accept=accept)


def batch(seed, ns=257):
    """a seeded batch in which every case of the policy occurs many times"""
    rng = np.random.default_rng(seed)
    lam_max = 100.0
    J = 10.0 ** rng.uniform(-3.0, 3.0, ns)
    Jt = J * 10.0 ** rng.uniform(-1.0, 1.0, (NLAM, ns))
    kind = rng.integers(0, 10, (NLAM, ns))
    Jt[kind == 0] = np.nan
    Jt[kind == 1] = np.inf
    Jt[kind == 2] = np.broadcast_to(J, Jt.shape)[kind == 2]              # equal to J: never accepted
    tie = rng.integers(0, 3, ns) == 0
    Jt[2, tie] = Jt[0, tie]                                              # ties between candidates
    status = np.where(rng.integers(0, 5, (NLAM, ns)) == 0, rng.integers(1, 40, (NLAM, ns)), 0).astype(np.int32)
    none = rng.integers(0, 8, ns) == 0                                   # no candidate at all: all broken down or NaN
    status[:, none & (rng.integers(0, 2, ns) == 0)] = 3
    Jt[:, none] = np.where(status[:, none] == 0, np.nan, Jt[:, none])
    lamt = 10.0 ** rng.uniform(-6.0, 2.0, (NLAM, ns))
    lam = 10.0 ** rng.uniform(-3.0, 2.0, ns)
    lam[rng.integers(0, 4, ns) == 0] = lam_max                           # at the upper bound: a rejection stalls
    lam[rng.integers(0, 6, ns) == 0] = lam_max / 2.0                     # grows beyond it: clamped
    state = np.where(rng.integers(0, 4, ns) == 0, rng.integers(1, 4, ns), 0).astype(np.int32)
    return J, Jt, lamt, status, lam, state, lam_max


@pytest.mark.parametrize("tol", [0.0, 0.5, 0.25])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_policy_against_numpy(seed, tol):
    J, Jt, lamt, status, lam, state, lam_max = batch(seed)
    fac_max = 10.0
    got = hip.retrieve_decide(J, Jt, lamt, status, lam, state, tol, lam_max, fac_max)
    want = restated(J, Jt, lamt, status, lam, state, tol, lam_max, fac_max)
    for f in ("lam", "state", "best", "accept"):
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f].view(np.uint8), want[f].view(np.uint8)), f
    done = state != hip.RET_ACTIVE
    assert done.any() and np.all(got["best"][done] == -1) and np.all(got["accept"][done] == -1)
    assert np.array_equal(got["lam"][done], lam[done]) and np.array_equal(got["state"][done], state[done])
    active = ~done
    # every case occurs: accepted and converged, accepted and not, rejected and grown, clamped, stalled, no candidate
    acc = active & (got["accept"] == 1)
    rej = active & (got["accept"] == 0)
    assert acc.any() and rej.any() and np.any(got["best"][active] == -1) and np.any(rej & (got["best"] >= 0))
    assert np.any(got["state"][rej] == hip.RET_STALLED) and np.any(got["lam"][rej & (lam < lam_max)] == lam_max)
    assert np.any(got["lam"][rej] < lam_max)
    if tol > 0:
        assert np.any(got["state"][acc] == hip.RET_CONVERGED) and np.any(got["state"][acc] == hip.RET_ACTIVE)
    else:
        assert np.all(got["state"][acc] == hip.RET_ACTIVE)              # J - Jt > 0 = tol * J for every accepted step
    assert np.all(got["state"][active & (got["state"] != hip.RET_ACTIVE)] != hip.RET_MAXITER)


def test_the_rules_one_by_one():
    nan, inf = np.nan, np.inf
    J = np.array([10.0, 10.0, 10.0, 10.0, 10.0, 10.0, 10.0])
    #              tie   NaN   +inf  broken  none  equal  finished
    Jt = np.array([[5.0, nan, inf, 1.0, nan, 10.0, 1.0],
                   [5.0, 9.0, inf, 9.5, nan, 10.0, 1.0],
                   [7.0, nan, inf, 9.0, 2.0, 11.0, 1.0]])
    status = np.array([[0, 0, 0, 4, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0]], dtype=np.int32)
    lamt = np.array([[0.1] * 7, [1.0] * 7, [10.0] * 7])
    lam = np.array([1.0, 1.0, 100.0, 1.0, 50.0, 1.0, 3.0])
    state = np.array([0, 0, 0, 0, 0, 0, hip.RET_STALLED], dtype=np.int32)
    got = hip.retrieve_decide(J, Jt, lamt, status, lam, state, 0.06, 100.0, 10.0)
    assert list(got["best"]) == [0, 1, 0, 2, -1, 0, -1]                  # ties: the smallest l; +inf is a candidate
    assert list(got["accept"]) == [1, 1, 0, 1, 0, 0, -1]                 # strict: Jt == J is rejected
    assert list(got["lam"]) == [0.1, 1.0, 100.0, 10.0, 100.0, 10.0, 3.0]
    C, S = hip.RET_CONVERGED, hip.RET_STALLED
    assert list(got["state"]) == [0, 0, S, 0, 0, 0, S]                   # 10 - 9 > 0.6; lam == lam_max on entry stalls
    got = hip.retrieve_decide(J, Jt, lamt, status, lam, state, 0.1, 100.0, 10.0)
    assert list(got["state"]) == [0, C, S, C, 0, 0, S]                   # 10 - 9 <= 1.0: converged; 10 - 5 is not
    with pytest.raises(hip.JurassicError, match="jur_retrieve_decide: bad arguments"):
        hip.retrieve_decide(J, Jt[:0], lamt[:0], status[:0], lam, state, 0.1, 100.0, 10.0)
