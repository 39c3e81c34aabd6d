"""jur_avk_summary (host arithmetic of the library, no GPU): what is read off one slice's averaging kernel -- the trace
per quantity, the row sums within the element's quantity, and dz / AVK_ii -- against a restatement in numpy built on
scene_elements.  The restatement sums in the library's order (ascending j, one addition per term, from 0.0), so dofs_q and
area are compared bit for bit; the resolution is one subtraction, one halving (exact) and one division, bit for bit."""
import numpy as np
import pytest
import common
from jurassic_hip import abi, lib


def windows(c):
    """T and one gas, over different windows"""
    c.retp_zmin, c.retp_zmax = -999.0, -999.0
    c.rett_zmin, c.rett_zmax = 10.0, 40.0
    for g in range(c.ng):
        c.retq_zmin[g], c.retq_zmax[g] = -999.0, -999.0
    c.retq_zmin[2], c.retq_zmax[2] = 15.0, 35.0
    for w in range(c.nw):
        c.retk_zmin[w], c.retk_zmax[w] = -999.0, -999.0


@pytest.fixture(scope="module")
def case():
    c = common.limb_case()
    windows(c.ctl)
    atm = abi.atm_t.from_buffer_copy(c.atm)
    z = np.ctypeslib.as_array(atm.z)
    n = atm.np
    z[:n] += 0.3 * np.sin(np.arange(n))                              # uneven levels, still ascending: dz differs by element
    assert np.all(np.diff(z[:n]) > 0)
    c.atm = atm
    return c


def restated(case, first, length, avk):
    el = lib.scene_elements(case.ctl, case.atm, first, length)
    iq, ip = el["iq"], el["ip"]
    w = len(iq)
    z = np.ctypeslib.as_array(case.atm.z)
    dofs_q = np.zeros(2 + case.ctl.ng + case.ctl.nw)
    area, res = np.zeros(w), np.zeros(w)
    for i in range(w):
        dofs_q[iq[i]] = dofs_q[iq[i]] + avk[i, i]
        acc = 0.0
        for j in range(w):
            if iq[j] == iq[i]:
                acc = acc + avk[i, j]
        area[i] = acc
        same = np.flatnonzero(iq == iq[i])
        at = int(np.flatnonzero(same == i)[0])
        if len(same) == 1:
            dz = 0.0
        elif at == 0:
            dz = abs(z[ip[same[1]]] - z[ip[i]])
        elif at == len(same) - 1:
            dz = abs(z[ip[i]] - z[ip[same[-2]]])
        else:
            dz = abs(z[ip[same[at + 1]]] - z[ip[same[at - 1]]]) / 2
        res[i] = dz / avk[i, i] if avk[i, i] > 0 else np.inf
    return dofs_q, area, res, iq, ip


def bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, a, b)


SLICES = ("full", "lone_gas_end", "lone_T")


def slice_of(case, name):
    """(first, len): the whole profile; up to the first level of the gas window (a lone gas element at the slice's end,
    several of T); from the last level of the T window on (a lone T element, no gas)"""
    z = np.ctypeslib.as_array(case.atm.z)[:case.atm.np]
    if name == "lone_gas_end":
        return 0, int(np.flatnonzero(z >= 15.0)[0]) + 1
    if name == "lone_T":
        first = int(np.flatnonzero(z <= 40.0)[-1])
        return first, case.atm.np - first
    return 0, case.atm.np


@pytest.mark.parametrize("name", SLICES)
def test_against_numpy(case, name):
    first, length = slice_of(case, name)
    w = len(lib.scene_elements(case.ctl, case.atm, first, length)["iq"])
    rng = np.random.default_rng(11)
    avk = rng.standard_normal((w, w)) * 0.1
    avk[np.diag_indices(w)] = rng.uniform(0.05, 1.0, w)
    got = lib.avk_summary(case.ctl, case.atm, first, length, avk)
    dofs_q, area, res, iq, ip = restated(case, first, length, avk)
    counts = np.bincount(iq, minlength=len(dofs_q))
    if name == "full":
        assert counts[1] >= 3 and counts[4] >= 3 and counts.sum() == w == counts[1] + counts[4]
    elif name == "lone_gas_end":
        assert counts[4] == 1 and counts[1] >= 3
    else:
        assert counts[1] == 1 and counts[4] == 0 and w == 1
    assert np.array_equal(got["iq"], iq) and np.array_equal(got["ip"], ip)
    bits(got["dofs_q"], dofs_q, "dofs_q")
    bits(got["area"], area, "area")
    bits(got["resolution"], res, "resolution")
    assert np.all(np.isfinite(got["resolution"])) and np.all(got["resolution"][counts[iq] > 1] > 0)
    lone = np.flatnonzero(counts[iq] == 1)
    assert np.all(got["resolution"][lone] == 0)                      # a lone element: dz = 0
    assert got["dofs_q"].sum() == pytest.approx(np.trace(avk), rel=1e-12)


def test_resolution_is_infinite_where_the_diagonal_is_not_positive(case):
    first, length = slice_of(case, "lone_gas_end")
    w = len(lib.scene_elements(case.ctl, case.atm, first, length)["iq"])
    rng = np.random.default_rng(12)
    avk = rng.standard_normal((w, w)) * 0.1 + np.eye(w)
    avk[0, 0], avk[2, 2], avk[w - 1, w - 1] = 0.0, -0.25, np.nan     # (the last one is the lone gas element)
    got = lib.avk_summary(case.ctl, case.atm, first, length, avk)
    for i in (0, 2, w - 1):
        assert got["resolution"][i] == np.inf
    others = np.setdiff1d(np.arange(w), [0, 2, w - 1])
    assert np.all(np.isfinite(got["resolution"][others])) and np.all(got["resolution"][others] > 0)
    bits(got["resolution"], restated(case, first, length, avk)[2], "resolution")


def test_empty_slice_and_refusals(case):
    got = lib.avk_summary(case.ctl, case.atm, 0, 5, np.zeros((0, 0)))   # 0 .. 4 km: no element
    assert len(got["area"]) == 0 and len(got["resolution"]) == 0 and np.all(got["dofs_q"] == 0)
    with pytest.raises(ValueError, match=r"avk must be"):
        lib.avk_summary(case.ctl, case.atm, 0, case.atm.np, np.zeros((3, 3)))
    with pytest.raises(lib.JurassicError, match=r"outside the atmosphere"):
        lib.avk_summary(case.ctl, case.atm, 0, case.atm.np + 1, np.zeros((0, 0)))
