"""The box on the state of the scene retrieval, host arithmetic (no GPU): jur_state_bound (the rule the device kernels
share as one text), jur_state_bounds_upstream (upstream's physical range per quantity) and jur_state_on_bounds (which
elements a box holds).  The yardstick of the rule is its own two lines, written out here in float64 scalars; everything
is compared bit for bit."""
import numpy as np
import pytest
import common
from jurassic_hip import abi, lib

INF, NAN = np.inf, np.nan


def rule(x, lo, hi):
    """c = x > lo ? x : lo;  c = c < hi ? c : hi"""
    x, lo, hi = np.float64(x), np.float64(lo), np.float64(hi)
    c = x if x > lo else lo
    return c if c < hi else hi


def same_bits(a, b):
    return np.array_equal(np.atleast_1d(np.asarray(a, dtype=np.float64)).view(np.uint64),
                          np.atleast_1d(np.asarray(b, dtype=np.float64)).view(np.uint64))


def test_the_rule_on_named_values():
    named = [
        (NAN, 1.0, 2.0, 1.0),                   # a NaN x gives lo
        (NAN, -INF, 2.0, -INF),
        (INF, 1.0, 2.0, 2.0), (-INF, 1.0, 2.0, 1.0),
        (INF, 1.0, INF, INF), (-INF, -INF, 2.0, -INF),
        (1.5, -INF, INF, 1.5), (-7e300, -INF, INF, -7e300),
        (1.0, 1.0, 2.0, 1.0), (2.0, 1.0, 2.0, 2.0),        # x == lo, x == hi
        (0.5, 3.0, 3.0, 3.0), (3.0, 3.0, 3.0, 3.0), (9.0, 3.0, 3.0, 3.0), (NAN, 3.0, 3.0, 3.0),   # lo == hi
        (0.0, -0.0, 1.0, -0.0), (-0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 1.0, 0.0), (-0.0, -0.0, 1.0, -0.0),   # x > lo is false for equal zeros: lo
        (-0.0, -1.0, 0.0, 0.0), (0.0, -1.0, -0.0, -0.0),                                           # c < hi is false for equal zeros: hi
        (-1e-320, 0.0, 1.0, 0.0), (1e-320, 0.0, 1.0, 1e-320),
    ]
    for x, lo, hi, want in named:
        got = lib.state_bound(x, lo, hi)
        assert same_bits(got, want), (x, lo, hi, got, want)
        assert same_bits(got, rule(x, lo, hi)), (x, lo, hi)


def test_the_rule_on_seeded_values():
    rng = np.random.default_rng(11)
    pool = np.r_[rng.standard_normal(40) * 10.0 ** rng.integers(-3, 4, 40), [NAN, INF, -INF, 0.0, -0.0, 5e-7, 5e4, 100.0, 400.0, 1.0]]
    edges = np.r_[pool[~np.isnan(pool)]]
    n = 0
    for _ in range(3000):
        lo, hi = np.sort(rng.choice(edges, 2))
        if rng.random() < 0.1:
            hi = lo
        x = rng.choice(np.r_[pool, lo, hi, np.nextafter(lo, -INF), np.nextafter(hi, INF)])
        assert same_bits(lib.state_bound(x, lo, hi), rule(x, lo, hi)), (x, lo, hi)
        n += 1
    xs = rng.standard_normal((7, 5))
    got = lib.state_bound(xs, -0.5, np.linspace(0.0, 1.0, 5))
    want = np.array([[rule(xs[i, j], -0.5, np.linspace(0.0, 1.0, 5)[j]) for j in range(5)] for i in range(7)])
    assert got.shape == (7, 5) and same_bits(got, want) and np.any(got != xs) and np.any(got == xs)


def test_upstreams_box_for_a_control_with_several_emitters_and_windows():
    case = common.limb_case()
    c = case.ctl
    assert c.ng >= 2 and c.nw >= 1
    lo, hi = lib.state_bounds_upstream(c)
    nq = 2 + c.ng + c.nw
    assert len(lo) == nq and len(hi) == nq
    assert same_bits(lo, [5e-7, 100.0] + [0.0] * (c.ng + c.nw))
    assert same_bits(hi, [5e4, 400.0] + [1.0] * c.ng + [INF] * c.nw)
    one = abi.ctl_t.from_buffer_copy(bytes(c))
    one.ng, one.nw = 1, 0
    lo1, hi1 = lib.state_bounds_upstream(one)
    assert same_bits(lo1, [5e-7, 100.0, 0.0]) and same_bits(hi1, [5e4, 400.0, 1.0])
    bad = abi.ctl_t.from_buffer_copy(bytes(c))
    bad.ng = -1
    with pytest.raises(lib.JurassicError, match="jur_state_bounds_upstream"):
        lib.state_bounds_upstream(bad)


def test_on_bounds_against_numpy():
    rng = np.random.default_rng(12)
    for trial in range(50):
        nq = int(rng.integers(1, 9))
        lo = np.where(rng.random(nq) < 0.2, -INF, rng.standard_normal(nq))
        hi = np.where(rng.random(nq) < 0.2, INF, lo + np.where(rng.random(nq) < 0.2, 0.0, rng.random(nq)))
        hi = np.where(np.isinf(lo) & (rng.random(nq) < 0.5), INF, hi)
        n = int(rng.integers(0, 200))
        iq = rng.integers(0, nq, n).astype(np.int32)
        x = rng.standard_normal(n)
        pick = rng.random(n)
        x = np.where(pick < 0.25, lo[iq], np.where(pick < 0.5, hi[iq], np.where(pick < 0.55, NAN, x)))
        got = lib.state_on_bounds(lo, hi, iq, x)
        want = np.where(x == lo[iq], -1, np.where(x == hi[iq], 1, 0)).astype(np.int8)
        assert got["side"].dtype == np.int8 and np.array_equal(got["side"], want), trial
        assert got["count"] == int(np.count_nonzero(want))
    both = lib.state_on_bounds([2.0], [2.0], [0, 0], [2.0, 3.0])
    assert list(both["side"]) == [-1, 0] and both["count"] == 1          # lo == hi and x equal to both: the lower side
    with pytest.raises(lib.JurassicError, match=r"jur_state_on_bounds: element 1 is of quantity 3, the box has 2"):
        lib.state_on_bounds([0.0, 0.0], [1.0, 1.0], [0, 3], [0.5, 0.5])
