"""jur_scene_layout / jur_scene_columns (host arithmetic of the library, no GPU): the slice of the atmosphere every ray
of a scene is traced through and the block of state elements that lies in it, against restatements in numpy of
locate_atm's two bisections (jr_common.h:127-154, tests/refcases.locate_atm) and of atm2x (jurassic.c:1491-1513)."""
import numpy as np
import pytest
import common
import refcases
from jurassic_hip import lib, synth

NAMES = ["ragged", "lone_ends", "lone_up", "short_last"]


def scene(name, windows=True):
    case = common.limb_case()
    case.atm, case.geom, _ = synth.scene(name, case.ctl, case.atm)
    c = case.ctl
    if windows:                                   # as common.retrieval_case: p, T, one gas and the extinction
        c.retp_zmin, c.retp_zmax = 20.0, 25.0
        c.rett_zmin, c.rett_zmax = 10.0, 40.0
        c.retq_zmin[2], c.retq_zmax[2] = 15.0, 35.0
        c.retk_zmin[0], c.retk_zmax[0] = 10.0, 20.0
    return case


def state_elements(ctl, atm):
    """atm2x in numpy: (quantity, point) of every state element, quantity-major with the point index inside."""
    n = atm.np
    z = np.ctypeslib.as_array(atm.z)[:n]
    win = [(ctl.retp_zmin, ctl.retp_zmax), (ctl.rett_zmin, ctl.rett_zmax)]
    win += [(ctl.retq_zmin[g], ctl.retq_zmax[g]) for g in range(ctl.ng)]
    win += [(ctl.retk_zmin[w], ctl.retk_zmax[w]) for w in range(ctl.nw)]
    return [(iq, ip) for iq, (lo, hi) in enumerate(win) for ip in range(n) if lo <= z[ip] <= hi]


@pytest.mark.parametrize("name", NAMES)
def test_layout_against_locate_atm(name):
    case = scene(name)
    atm, ctl = case.atm, case.ctl
    time = np.ctypeslib.as_array(atm.time)[:atm.np]
    t = case.geom[:, 0]
    assert set(synth.SCENES[name][1]) <= set(t)                    # the extra time stamps are among the rays'
    lay = lib.scene_layout(ctl, atm, t)
    want = np.array([refcases.locate_atm(time, x) for x in t])
    assert np.array_equal(lay["first"], want[:, 0]) and np.array_equal(lay["len"], want[:, 1])
    elements = state_elements(ctl, atm)
    width = np.array([sum(f <= ip < f + n for _, ip in elements) if n >= 2 else 0 for f, n in want])
    assert np.array_equal(np.diff(lay["rowptr"]), width) and lay["rowptr"][0] == 0
    assert np.array_equal(lay["rowptr"], np.concatenate([[0], np.cumsum(width)]))
    assert width.max() >= 25
    one = lay["len"] < 2
    if name != "short_last":                                       # (there every time stamp meets two points or more)
        assert one.any()
    assert np.all(width[one] == 0)


@pytest.mark.parametrize("name", NAMES)
def test_columns_follow_the_state_vector(name):
    case = scene(name)
    atm, ctl = case.atm, case.ctl
    elements = state_elements(ctl, atm)
    assert np.array_equal(lib.scene_columns(ctl, atm, 0, atm.np), np.arange(len(elements)))
    lay = lib.scene_layout(ctl, atm, case.geom[:, 0])
    for f, n in sorted({(int(a), int(b)) for a, b in zip(lay["first"], lay["len"])}):
        cols = lib.scene_columns(ctl, atm, f, n)
        assert np.all(np.diff(cols) > 0)
        assert list(cols) == [j for j, (_, ip) in enumerate(elements) if f <= ip < f + n]
    w = np.diff(lay["rowptr"])
    for r in range(len(w)):
        if lay["len"][r] >= 2:
            assert w[r] == len(lib.scene_columns(ctl, atm, lay["first"][r], lay["len"][r]))


def test_lone_end_points_join_their_neighbours_block():
    """lone_ends: the one-point first profile (5 km) and last profile (75 km) have no slice of their own.  With T
    retrieved at all altitudes the first one's element appears in the columns of the slice after it, the last one's in
    those of the slice before it; their own time stamps meet one point and have no block."""
    case = scene("lone_ends", windows=False)
    atm, ctl = case.atm, case.ctl
    ctl.rett_zmin, ctl.rett_zmax = 0.0, 100.0
    n = atm.np
    lay = lib.scene_layout(ctl, atm, np.array([1.0, 4.0, 0.0, 5.0]))
    assert list(lay["first"][:2]) == [0, n - 46] and list(lay["len"][:2]) == [51, 46]
    assert lib.scene_columns(ctl, atm, 0, 51)[0] == 0              # T of point 0, the foreign point
    assert lib.scene_columns(ctl, atm, n - 46, 46)[-1] == n - 1    # T of the last point
    assert np.array_equal(np.diff(lay["rowptr"]), [51, 46, 0, 0])  # the lone profiles' own time stamps: one point, no block


def test_no_rays_and_no_windows():
    case = scene("ragged", windows=False)
    lay = lib.scene_layout(case.ctl, case.atm, np.zeros(0))
    assert len(lay["first"]) == 0 and list(lay["rowptr"]) == [0]
    lay = lib.scene_layout(case.ctl, case.atm, case.geom[:, 0])    # all windows at -999
    assert np.all(lay["rowptr"] == 0) and (lay["len"] >= 2).any()
    assert len(lib.scene_columns(case.ctl, case.atm, 0, case.atm.np)) == 0


def test_blocks_to_dense_scatters_by_column():
    case = scene("short_last")
    atm, ctl = case.atm, case.ctl
    t = case.geom[::7, 0]
    lay = lib.scene_layout(ctl, atm, t)
    nd = 2
    out = dict(lay, rad=np.zeros((len(t), nd)), k=np.arange(1.0, 1.0 + lay["rowptr"][-1] * nd))
    dense = lib.scene_blocks_to_dense(ctl, atm, out)
    assert dense.shape == (len(t) * nd, len(state_elements(ctl, atm)))
    assert np.count_nonzero(dense) == len(out["k"])
    r = int(np.argmax(np.diff(lay["rowptr"])))
    cols = lib.scene_columns(ctl, atm, lay["first"][r], lay["len"][r])
    w = len(cols)
    assert np.array_equal(dense[r * nd + 1, cols], out["k"][lay["rowptr"][r] * nd + w:lay["rowptr"][r] * nd + 2 * w])
