"""error_components (jur_error_components): upstream's set_cov_meas, host arithmetic with no GPU.  The two variances of
every measurement -- noise err_noise[id]^2 and forward model (err_formod[id] / 100 * y)^2 -- and the weight 1 / (their sum),
against the same IEEE operations in numpy, bit for bit; the edge cases of the rule; the refusals by their words."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    return lib


def bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), what


def is_plus_zero(a):
    return bool(np.all(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) == 0))


def rule(y, en, ef):
    """the rule of include/jurassic_hip.h in numpy, operation for operation"""
    with np.errstate(all="ignore"):
        vn = np.broadcast_to(en * en, y.shape)
        f = ef / 100 * y
        vf = f * f
        total = vn + vf
        ok = (total > 0) & np.isfinite(total)
        weight = np.where(ok, 1 / np.where(ok, total, 1.0), 0.0)
    return np.stack([np.where(ok, vn, 0.0), np.where(ok, vf, 0.0)]), weight


def test_against_numpy(hip):
    rng = np.random.default_rng(11)
    for nr, nd in ((1, 1), (7, 3), (64, 5), (130, 2)):
        y = rng.uniform(-2.0, 5.0, (nr, nd)) * 10.0 ** rng.integers(-6, 3, (nr, nd))
        en = 10.0 ** rng.uniform(-5.0, 0.0, nd)
        ef = rng.uniform(0.0, 5.0, nd)
        var, weight = hip.error_components(y, en, ef)
        assert var.shape == (2, nr, nd) and weight.shape == (nr, nd)
        wvar, wweight = rule(y, en, ef)
        bits(var, wvar, "var of %d x %d" % (nr, nd))
        bits(weight, wweight, "weight of %d x %d" % (nr, nd))
        assert np.all(weight > 0)
        assert np.all(np.abs(weight * (var[0] + var[1]) - 1) < 1e-15)


def test_edge_cases(hip):
    y = np.array([[1.0, np.nan, 3.0], [np.inf, 2.0, -np.inf], [0.0, -4.0, 1e200]])
    en, ef = np.array([0.1, 0.2, 0.0]), np.array([1.0, 0.0, 2.0])
    var, weight = hip.error_components(y, en, ef)
    wvar, wweight = rule(y, en, ef)
    bits(var, wvar, "var")
    bits(weight, wweight, "weight")
    # a y that is not finite under a forward-model term: weight 0 and both variances +0.0
    for r, c in ((1, 0), (1, 2)):
        assert is_plus_zero(weight[r, c]) and is_plus_zero(var[:, r, c])
    # ... and without one (err_formod == 0) the product 0 * nan or 0 * inf is NaN all the same
    assert is_plus_zero(weight[0, 1]) and is_plus_zero(var[:, 0, 1])
    # (1e200 * 0.02)^2 overflows: the sum is not finite
    assert is_plus_zero(weight[2, 2]) and is_plus_zero(var[:, 2, 2])
    assert weight[0, 0] > 0 and weight[1, 1] == 1 / (0.2 * 0.2) and weight[2, 1] == 1 / (0.2 * 0.2)

    # err_noise == 0 with err_formod == 0: nothing is known of the error, the measurement takes no part
    var, weight = hip.error_components(np.ones((4, 2)), np.zeros(2), np.zeros(2))
    assert is_plus_zero(var) and is_plus_zero(weight)

    # err_formod alone: the weight is 1 / (e / 100 * y)^2; y == 0 has no error at all and takes no part
    y = np.array([[2.0, 0.0], [-3.0, 5e-3]])
    var, weight = hip.error_components(y, np.zeros(2), np.array([1.0, 10.0]))
    assert is_plus_zero(var[0])
    bits(var[1], np.where(y == 0, 0.0, (np.array([1.0, 10.0]) / 100 * y) ** 2), "forward-model variance alone")
    assert is_plus_zero(weight[0, 1]) and is_plus_zero(var[:, 0, 1])
    bits(weight, rule(y, np.zeros(2), np.array([1.0, 10.0]))[1], "weight under the forward-model term alone")

    # nr == 0
    var, weight = hip.error_components(np.zeros((0, 3)), np.ones(3), np.ones(3))
    assert var.shape == (2, 0, 3) and weight.shape == (0, 3)


def test_refusals(hip):
    y = np.ones((2, 3))
    good = np.ones(3)
    for bad, word in ((-1.0, "-1"), (np.nan, "nan"), (np.inf, "inf")):
        e = good.copy()
        e[1] = bad
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_error_components: err_noise of channel 1 is %s: negative or not finite"
                           % (hip.EINVAL, word)):
            hip.error_components(y, e, good)
        with pytest.raises(hip.JurassicError, match=r"error %d: jur_error_components: err_formod of channel 1 is %s: negative or not finite"
                           % (hip.EINVAL, word)):
            hip.error_components(y, good, e)
    with pytest.raises(ValueError):
        hip.error_components(y, np.ones(2), good)
    rc = hip.lib().jur_error_components(3, 2, None, hip._p(good), hip._p(good), None, None)
    assert rc == hip.EINVAL and "jur_error_components: null argument" in hip.lib().jur_last_error().decode()
