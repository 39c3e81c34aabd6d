"""jur_scene_slices / jur_scene_elements (host arithmetic of the library, no GPU): the distinct slices of a scene that
carry state elements, in the order the rays first meet them -- the layout of jur_normal_scene_host's sums -- and the
quantity and point of every element of a slice, against restatements in numpy built on jur_scene_layout (itself held to
locate_atm by tests/test_scene_layout_cpu.py) and on the retrieval windows."""
import ctypes as C
import numpy as np
import pytest
import common
from jurassic_hip import abi, lib, synth
from test_scene_jacobian_gpu import retrieval_windows
from test_scene_layout_cpu import state_elements


def scene(name, windows=retrieval_windows):
    case = common.limb_case()
    case.atm, case.geom, _ = synth.scene(name, case.ctl, case.atm)
    if windows:
        windows(case.ctl)
    return case


def layout_or_refusal(case, time):
    try:
        return lib.scene_layout(case.ctl, case.atm, time), None
    except lib.JurassicError as e:
        return None, str(e)


def slices_in_numpy(lay):
    """The unique (first, len) pairs of the layout with width > 0 in first-appearance order, and every ray's index."""
    width = np.diff(lay["rowptr"])
    order, sid = {}, np.full(len(width), -1, dtype=np.int32)
    for r in range(len(width)):
        if width[r] > 0:
            sid[r] = order.setdefault((int(lay["first"][r]), int(lay["len"][r])), len(order))
    w = np.array([width[np.flatnonzero(sid == s)[0]] for s in range(len(order))], dtype=np.int64)
    return list(order), sid, w


@pytest.mark.parametrize("name", sorted(synth.SCENES))
def test_slices_against_the_layout(name):
    case = scene(name)
    rng = np.random.default_rng(3)
    t = case.geom[rng.permutation(len(case.geom)), 0]              # (the slices come in the order of THESE rays)
    lay, refused = layout_or_refusal(case, t)
    if refused:
        with pytest.raises(lib.JurassicError) as e:
            lib.scene_slices(case.ctl, case.atm, t)
        assert str(e.value).split(":")[0] == refused.split(":")[0]
        return
    pairs, sid, w = slices_in_numpy(lay)
    out = lib.scene_slices(case.ctl, case.atm, t)
    assert len(pairs) >= (1 if name == "unsorted" else 2)          # (unsorted: locate_atm hands every ray all points)
    assert [(int(a), int(b)) for a, b in zip(out["sfirst"], out["slen"])] == pairs
    assert np.array_equal(out["sid"], sid)
    assert np.array_equal(out["wptr"], np.concatenate([[0], np.cumsum(w)]))
    assert np.array_equal(out["aptr"], np.concatenate([[0], np.cumsum(w * w)]))
    assert out["wptr"].dtype == out["aptr"].dtype == np.int64
    # the counting call: every array NULL
    n = lib.lib().jur_scene_slices(C.byref(case.ctl), C.byref(case.atm), len(t), t.ctypes.data_as(lib.dp), None, None, None, None, None)
    assert n == len(pairs)
    # the same rays in another order: the same slices, renumbered
    rev = lib.scene_slices(case.ctl, case.atm, t[::-1])
    assert sorted(zip(rev["sfirst"], rev["slen"])) == sorted(pairs)
    back = rev["sid"][::-1]
    assert np.array_equal(back < 0, sid < 0)
    assert all((rev["sfirst"][back[r]], rev["slen"][back[r]]) == pairs[sid[r]] for r in np.flatnonzero(sid >= 0))


def all_temperatures(c):
    c.rett_zmin, c.rett_zmax = -10.0, 100.0


def test_time_stamps_that_share_a_slice_and_rays_of_width_zero():
    """short_last with T retrieved at all altitudes: the ray time stamp 1.5 matches no profile and is traced, as the rays
    of the time stamp 2.0 are, through the last profile of two levels -- rays with different time stamps in one slice
    of width 2.  (With the windows of the Jacobian tests that profile, at 0 and 80 km, holds no element, and ragged's
    extra time stamps all meet a single point: no scene shares a slice of width > 0 there.)  The time stamps 0.5 and
    3.0 meet one point: width 0, slice -1."""
    case = scene("short_last", windows=all_temperatures)
    t = case.geom[:, 0]
    assert {1.5, 2.0} <= set(t) and 1.5 in synth.SCENES["short_last"][1]
    lay = lib.scene_layout(case.ctl, case.atm, t)
    out = lib.scene_slices(case.ctl, case.atm, t)
    width = np.diff(lay["rowptr"])
    assert (width == 0).any() and np.array_equal(out["sid"] < 0, width == 0)
    assert np.all(out["sid"][(t == 0.5) | (t == 3.0)] == -1)
    shared = [s for s in range(len(out["sfirst"])) if len(np.unique(t[out["sid"] == s])) > 1]
    assert len(shared) == 1 and set(t[out["sid"] == shared[0]]) == {1.5, 2.0}
    assert out["slen"][shared[0]] == 2 and out["wptr"][shared[0] + 1] - out["wptr"][shared[0]] == 2
    assert len(out["sfirst"]) == 3
    for s in range(len(out["sfirst"])):
        rays = out["sid"] == s
        assert np.all(lay["first"][rays] == out["sfirst"][s]) and np.all(lay["len"][rays] == out["slen"][s])
        assert np.all(width[rays] == out["wptr"][s + 1] - out["wptr"][s])
    # first appearance: the first ray of slice s comes before the first ray of slice s + 1
    firsts = [np.flatnonzero(out["sid"] == s)[0] for s in range(len(out["sfirst"]))]
    assert firsts == sorted(firsts)
    # ragged, the windows of the Jacobian tests: every extra time stamp meets one point and gets -1
    case = scene("ragged")
    t = case.geom[:, 0]
    out = lib.scene_slices(case.ctl, case.atm, t)
    assert np.all(out["sid"][np.isin(t, synth.SCENES["ragged"][1])] == -1) and len(out["sfirst"]) == 4


def test_no_rays_and_no_windows():
    case = scene("ragged", windows=None)
    for t in (np.zeros(0), case.geom[:, 0]):
        out = lib.scene_slices(case.ctl, case.atm, t)
        assert len(out["sfirst"]) == 0 and list(out["wptr"]) == [0] and list(out["aptr"]) == [0]
        assert np.all(out["sid"] == -1) and len(out["sid"]) == len(t)


@pytest.mark.parametrize("name", ["ragged", "lone_ends", "lone_up", "short_last"])
def test_elements_against_the_windows(name):
    case = scene(name)
    ctl, atm = case.ctl, case.atm
    elements = state_elements(ctl, atm)                            # (iq, ip) of the whole state, in its order
    assert {iq for iq, _ in elements} == {0, 1, 2 + 2, 2 + ctl.ng}  # p, T, the third gas, the first window
    out = lib.scene_slices(ctl, atm, case.geom[:, 0])
    for f, n in list(zip(out["sfirst"], out["slen"])) + [(0, atm.np), (3, 0)]:
        el = lib.scene_elements(ctl, atm, f, n)
        assert np.array_equal(el["cols"], lib.scene_columns(ctl, atm, f, n))
        want = [(j, iq, ip) for j, (iq, ip) in enumerate(elements) if f <= ip < f + n]
        assert [tuple(int(x) for x in row) for row in zip(el["cols"], el["iq"], el["ip"])] == want
    for s in range(len(out["sfirst"])):
        assert len(lib.scene_elements(ctl, atm, out["sfirst"][s], out["slen"][s])["cols"]) == out["wptr"][s + 1] - out["wptr"][s]


def test_refusals_are_the_layouts():
    case = scene("short_last")
    t = case.geom[:, 0]
    short = abi.atm_t()
    C.memmove(C.byref(short), C.byref(case.atm), C.sizeof(abi.atm_t))
    for np_bad in (1, 0, abi.NP + 1):
        short.np = np_bad
        with pytest.raises(lib.JurassicError) as a:
            lib.scene_layout(case.ctl, short, t)
        with pytest.raises(lib.JurassicError) as b:
            lib.scene_slices(case.ctl, short, t)
        assert str(a.value) == str(b.value) and "error %d" % lib.EINVAL in str(b.value)
    for bad in ((-1, 2), (0, case.atm.np + 1), (case.atm.np, 1), (2, -1)):
        with pytest.raises(lib.JurassicError) as a:
            lib.scene_columns(case.ctl, case.atm, *bad)
        with pytest.raises(lib.JurassicError) as b:
            lib.scene_elements(case.ctl, case.atm, *bad)
        assert "error %d" % lib.EINVAL in str(a.value) and "error %d" % lib.EINVAL in str(b.value)
    # a negative ray count is refused by both (the binding cannot make one: the C entry directly)
    L = lib.lib()
    lp = C.POINTER(C.c_long)
    rp = np.zeros(1, dtype=np.int64)
    assert L.jur_scene_layout(C.byref(case.ctl), C.byref(case.atm), -1, None, None, None, rp.ctypes.data_as(lp)) == lib.EINVAL
    assert L.jur_scene_slices(C.byref(case.ctl), C.byref(case.atm), -1, None, None, None, None, None, None) == lib.EINVAL
