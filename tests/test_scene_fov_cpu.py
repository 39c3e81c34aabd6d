"""jur_scene_fov_live (host arithmetic of the library, no GPU): scans, windows and the effective mask that the scene
entries apply while a field of view is set, against restatements in numpy of formod_fov's window (jurassic.c:223-230:
the rays within JUR_NFOV positions that carry the ray's time stamp)."""
import numpy as np
import pytest
from jurassic_hip import abi, lib

NFOV = abi.NFOV


def window(time, ir):
    return [j for j in range(max(ir - NFOV, 0), min(ir + NFOV + 1, len(time))) if time[j] == time[ir]]


def live_in_numpy(time, rad):
    return np.array([[all(np.isfinite(rad[j, d]) for j in window(time, i)) for d in range(rad.shape[1])] for i in range(len(time))])


def test_a_window_slides_along_a_scan_of_13():
    assert 13 > 2 * NFOV + 1
    time = np.full(13, 3.5)
    rad = np.zeros((13, 2))
    assert lib.scene_fov_live(time, rad).all()
    for at in range(13):                              # a NaN on ray `at`, channel 1, masks the rays whose window holds it
        rad[:] = 0.0
        rad[at, 1] = np.nan
        live = lib.scene_fov_live(time, rad)
        assert live[:, 0].all()
        assert np.array_equal(~live[:, 1], np.abs(np.arange(13) - at) <= NFOV), at
        assert np.array_equal(live, live_in_numpy(time, rad))
    assert live[0, 1] and not live[12 - NFOV, 1], "ray 0 is beyond the last ray's window"


def test_a_scan_of_two():
    time = np.array([1.0, 1.0])
    rad = np.zeros((2, 3))
    assert lib.scene_fov_live(time, rad).all()
    rad[1, 2] = np.inf
    live = lib.scene_fov_live(time, rad)
    assert np.array_equal(live, [[True, True, False]] * 2)


def test_a_nan_stays_inside_its_scan():
    """three scans of 8, 13 and 2 rays; a NaN on ray 6 of the second masks that scan's rays within 5 positions and no ray
    of the scans before and after it, although rays of both lie within 5 positions of it or of a masked ray"""
    time = np.concatenate([np.full(8, 0.25), np.full(13, 0.5), np.full(2, 7.0)])
    rad = np.random.default_rng(0).uniform(1.0, 2.0, (23, 2))
    at = 8 + 1
    rad[at, 0] = np.nan
    live = lib.scene_fov_live(time, rad)
    want = np.ones((23, 2), bool)
    want[8:8 + 1 + NFOV + 1, 0] = False               # rays 8 .. 14: positions 0 .. 6 of the scan, within 5 of position 1
    assert np.array_equal(live, want)
    assert live[:8].all() and live[21:].all()
    assert np.array_equal(live, live_in_numpy(time, rad))
    rad[at, 0], rad[20, 1] = 1.0, -np.inf            # the last ray of the second scan: ray 21 is next to it, in another scan
    live = lib.scene_fov_live(time, rad)
    want = np.ones((23, 2), bool)
    want[15:21, 1] = False
    assert np.array_equal(live, want)


def test_seeded_scans_against_numpy():
    rng = np.random.default_rng(5)
    lengths = rng.integers(2, 30, 12)
    time = np.repeat(rng.permutation(12) * 0.75, lengths)
    rad = rng.uniform(0.0, 1.0, (len(time), 3))
    rad[rng.uniform(size=rad.shape) < 0.03] = np.nan
    assert np.array_equal(lib.scene_fov_live(time, rad), live_in_numpy(time, rad))


def test_refusals_name_the_ray():
    rad = np.zeros((9, 2))
    with pytest.raises(lib.JurassicError, match=r"error %d: jur_scene_fov_live: ray 4 is alone in its window" % lib.EINVAL):
        lib.scene_fov_live(np.array([0.0, 0.0, 1.0, 1.0, 2.0, 3.0, 3.0, 3.0, 3.0]), rad)
    with pytest.raises(lib.JurassicError, match=r"error %d: jur_scene_fov_live: ray 8 is alone in its window" % lib.EINVAL):
        lib.scene_fov_live(np.array([0.0, 0.0, 1.0, 1.0, 2.0, 2.0, 3.0, 3.0, 4.0]), rad)
    with pytest.raises(lib.JurassicError, match=r"error %d: jur_scene_fov_live: ray 6 starts a second run of rays with the time stamp 1\b" % lib.EINVAL):
        lib.scene_fov_live(np.array([0.0, 0.0, 1.0, 1.0, 2.0, 2.0, 1.0, 1.0, 1.0]), rad)
    far = np.concatenate([np.full(20, 1.0), np.full(20, 2.0), np.full(20, 1.0)])   # windows apart, the same time stamp
    with pytest.raises(lib.JurassicError, match=r"ray 40 starts a second run"):
        lib.scene_fov_live(far, np.zeros((60, 1)))
    with pytest.raises(lib.JurassicError, match=r"ray 2 is alone in its window"):
        lib.scene_fov_live(np.array([0.0, 0.0, np.nan, 1.0, 1.0]), np.zeros((5, 1)))
    assert lib.scene_fov_live(np.zeros(0), np.zeros((0, 2))).shape == (0, 2)
