"""The full a-priori precision of the slices (jur_model_set_prior_precision, jur_model_prior_precision,
jur_prior_corr_host): what needs no GPU.  The symbols and their argument types, the layout the Python wrapper hands on,
and the closed form of the exponential prior's inverse that tests/test_prior_full_gpu.py holds the device to.

Closed form (a first-order Markov chain): for one quantity on ascending altitudes z with correlation length c and
rho_k = exp(-(z_{k+1} - z_k) / c), the correlation matrix C_ij = exp(-|z_i - z_j| / c) has the tridiagonal inverse
  C^-1_kk = 1 + rho_{k-1}^2 / (1 - rho_{k-1}^2) + rho_k^2 / (1 - rho_k^2)   (a missing neighbour drops its term)
  C^-1_{k,k+1} = -rho_k / (1 - rho_k^2)
and R = Sa^-1 = C^-1 / (sigma sigma^T).  The helper is held here to the inverse in np.longdouble within 2e-14 of
sqrt(R_ii R_jj), for 17 ... 300 uneven levels and c = 0.5 ... 20 km (worst seen: 1.3e-16 at 300 levels and 20 km).
np.linalg.inv has no longdouble kernel, so that inverse is the longdouble Cholesky one of tests/test_scene_diagnose_gpu.py."""
import ctypes as C
import inspect
import numpy as np
import pytest
from jurassic_hip import lib
from test_scene_diagnose_gpu import cholesky_ld, inverse_lower_ld

LD = np.longdouble


def exp_prior_inverse(z, sigma, c):
    """R = Sa^-1 of Sa_ij = sigma_i sigma_j exp(-|z_i - z_j| / c) on strictly ascending z, in np.longdouble"""
    z, sigma = np.asarray(z, LD), np.asarray(sigma, LD)
    n = len(z)
    assert np.all(np.diff(z) > 0) and c > 0
    rho = np.exp(-np.diff(z) / LD(c))
    t = rho * rho / (1 - rho * rho)
    Ci = np.zeros((n, n), LD)
    d = np.ones(n, LD)
    d[1:] += t
    d[:-1] += t
    Ci[np.diag_indices(n)] = d
    off = -rho / (1 - rho * rho)
    k = np.arange(n - 1)
    Ci[k, k + 1] = off
    Ci[k + 1, k] = off
    return Ci / np.outer(sigma, sigma)


def exp_prior(z, sigma, c):
    """Sa itself, in np.longdouble"""
    z, sigma = np.asarray(z, LD), np.asarray(sigma, LD)
    return np.outer(sigma, sigma) * np.exp(-np.abs(z[:, None] - z[None, :]) / LD(c))


def uneven_levels(rng, n, top=60.0):
    """n strictly ascending altitudes in km with spacings that vary by a factor of ten"""
    dz = 10.0 ** rng.uniform(-0.5, 0.5, n)
    return np.cumsum(dz) * (top / dz.sum())


@pytest.mark.parametrize("n", [17, 64, 300])
@pytest.mark.parametrize("c", [0.5, 5.0, 20.0])
def test_closed_form_against_the_longdouble_inverse(n, c):
    rng = np.random.default_rng(1000 * n + int(10 * c))
    z = uneven_levels(rng, n)
    sigma = 10.0 ** rng.uniform(-1.0, 1.0, n)
    R = exp_prior_inverse(z, sigma, c)
    # (np.linalg.inv has no longdouble kernel: the inverse in longdouble is the Cholesky one of the diagnose tests)
    Y = inverse_lower_ld(cholesky_ld(exp_prior(z, sigma, c)))
    want = Y.T @ Y
    scale = np.sqrt(np.outer(np.diag(want), np.diag(want)))
    worst = float(np.max(np.abs(R - want) / scale))
    print("PRIOR closed form, n = %d, c = %g: worst error / sqrt(R_ii R_jj) %.2e" % (n, c, worst))
    assert worst <= 2e-14
    assert np.array_equal(R, R.T)
    k = np.arange(n)
    assert np.all(R[np.abs(k[:, None] - k[None, :]) > 1] == 0)


def test_symbols_and_argument_types():
    L = lib.lib()
    lp_, ip_, dp = C.POINTER(C.c_long), C.POINTER(C.c_int), lib.dp
    assert L.jur_model_set_prior_precision.argtypes == [C.c_void_p, C.c_long, lp_, dp]
    assert L.jur_model_prior_precision.argtypes == [C.c_void_p, lp_, dp] and L.jur_model_prior_precision.restype is C.c_long
    assert L.jur_prior_corr_host.argtypes == [C.c_void_p, C.c_long, lp_, ip_, dp, dp, C.c_int, dp, dp, dp, ip_]
    for name in ("set_prior_precision", "prior_precision"):
        assert callable(getattr(lib.Model, name))
    assert list(inspect.signature(lib.prior_corr).parameters) == ["model", "ctl", "atm", "time", "sigma_q", "cz_q"]
    # the existing methods keep their signatures: the precision is held by the model
    assert "R" not in inspect.signature(lib.Model.solve_slices).parameters
    assert "R" not in inspect.signature(lib.Model.retrieve_scene).parameters


def test_null_model_is_refused_without_a_device():
    L = lib.lib()
    assert L.jur_model_set_prior_precision(None, 0, None, None) < 0
    assert L.jur_model_prior_precision(None, None, None) < 0
    assert L.jur_prior_corr_host(None, 1, None, None, None, None, 0, None, None, None, None) < 0


class _Handle:
    """stands in for a Model in the wrapper: records what reaches the library"""
    h = None


def test_wrapper_lays_out_like_scene_slices(monkeypatch):
    """Model.set_prior_precision hands on wptr as int64 and R flat at the running sum of the squared widths, as
    scene_slices lays out A; a size that does not fit is refused before the library is called."""
    seen = {}

    class Fake:
        def jur_model_set_prior_precision(self, h, ns, wp, R):
            seen["ns"] = ns
            seen["wptr"] = None if not wp else np.ctypeslib.as_array(wp, shape=(ns + 1,)).copy()
            seen["R"] = None if not R else np.ctypeslib.as_array(R, shape=(int((np.diff(seen["wptr"]) ** 2).sum()),)).copy()
            return 0

    monkeypatch.setattr(lib, "lib", lambda: Fake())
    widths = [3, 0, 2]
    wptr = np.concatenate([[0], np.cumsum(widths)]).astype(np.int32)          # (another dtype: the wrapper converts)
    mats = [np.arange(w * w, dtype=np.float64).reshape(w, w) + 10 * i for i, w in enumerate(widths)]
    R = np.concatenate([m.ravel() for m in mats])
    lib.Model.set_prior_precision(_Handle(), wptr, R)
    assert seen["ns"] == 3 and seen["wptr"].dtype == np.int64 and np.array_equal(seen["wptr"], [0, 3, 3, 5])
    aptr = np.concatenate([[0], np.cumsum(np.array(widths) ** 2)])
    for i, w in enumerate(widths):
        assert np.array_equal(seen["R"][aptr[i]:aptr[i + 1]].reshape(w, w), mats[i])
    with pytest.raises(ValueError):
        lib.Model.set_prior_precision(_Handle(), wptr, R[:-1])
    lib.Model.set_prior_precision(_Handle(), None)
    assert seen["ns"] == 0 and seen["wptr"] is None and seen["R"] is None
