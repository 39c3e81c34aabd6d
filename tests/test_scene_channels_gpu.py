"""The Jacobian and the scene entries at channel counts other than two, and in brightness temperatures.

Every other test of Model.kernel_scene, normal_scene, gradient_scene, trial_scene, retrieve_scene, diagnose_scene,
gain_scene, param_error_scene and of the field of view inside them runs on the limb example's two radiance channels.  Two
divides every chunk these kernels cut the measurements into -- groups of 8 and of 64, tiles of 64, 256 values at a time --
so no chunk ever holds part of a ray's channels, and the address arithmetic with nd (m / nd, r * nd + id,
(rowptr[r] - base) * nd + id * w + col) has run at one value only.  The configurations of common.CHANNELS:

  nd1      one channel: every loop over the channels of a ray is degenerate, a block is one row
  nd3      the smallest odd count: every chunk straddles rays
  nd3bbt   the same in brightness temperatures: the conversion's log1p inside every difference quotient, Jacobian entries
           of the order of 1 K per unit of state instead of 1e-5
  nd7      coprime to every chunk size: a group of 8 never holds whole rays
  nd65     one ray's channels exceed a chunk of 64 and a tile row of the gain kernels (small tables, five rays per time
           stamp, narrow windows: test_scene_jacobian_gpu.REDUCED)

A scene's name carries its configuration ('ragged@nd3', test_scene_jacobian_gpu.scene_case), so the checks are the
neighbouring files' own, called with such a name: no bound is stated here.  Bit identity against Model.kernel,
Model.formod_host and the replays on the host; the derived gamma bounds against np.longdouble; the chains in float64
scalars -- each as its own file states it.  What this file adds is what makes a check mean something at the
configuration at hand (the channel count in use, the unit of the radiances, measurements per slice beyond a chunk).
A field-of-view shape is not combined with brightness temperatures: the reference converts inside formod and convolves
nowhere after it, so nothing defines the order of the two."""
import numpy as np
import pytest
import common
import test_scene_diagnose_gpu as D
import test_scene_fov_gpu as F
import test_scene_gain_gpu as G
import test_scene_jacobian_gpu as J
import test_scene_normal_gpu as N
import test_scene_param_gpu as PA
import test_scene_recomp_gpu as RC
import test_scene_retrieve_gpu as T

pytestmark = pytest.mark.gpu
ALL = ("nd1", "nd3", "nd3bbt", "nd7", "nd65")


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def on(scene, channels):
    return [scene + "@" + c for c in channels]


def configured(case, name):
    """the case runs on the channels its name states, and in the unit it states"""
    channels = common.CHANNELS[J.channels_of(name)[1]]
    nd = len(channels["nu"])
    assert case.ctl.nd == nd and [case.ctl.nu[d] for d in range(nd)] == channels["nu"]
    assert case.ctl.write_bbt == channels.get("write_bbt", 0)
    return nd


def unit_of(case, rad):
    """radiances of the synthetic limb spectra stay below 1 W / (m^2 sr cm^-1); brightness temperatures of rays that
    met any air lie between 1 K and 400 K -- the two cannot be mistaken for one another"""
    seen = rad[np.isfinite(rad) & (rad != 0)]
    assert len(seen) > 0
    if case.ctl.write_bbt:
        assert seen.min() > 1.0 and seen.max() < 400.0
    else:
        assert 0 < seen.min() and seen.max() < 1.0


def layout_is_not_trivial(hip, name, out=None):
    """more than one slice, the widest of more than 32 elements (more than 16 in the reduced scene of nd65); with nd65
    a ray's channels alone exceed a chunk of 64 measurements"""
    case, geom, y, weight = N.inputs(hip, name)
    nd = configured(case, name)
    lay = T.layout(hip, name)[0]
    widths = np.diff(lay["wptr"])
    assert len(widths) >= 2 and widths.max() > (16 if J.channels_of(name)[1] == "nd65" else 32)
    assert y.shape == (len(geom), nd)
    unit_of(case, y)
    return case, lay, nd


# ---- 1. kernel_scene ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,arith", [(n, a) for c in ALL for n in on("ragged", [c]) + on("lone_ends", [c])
                                        for a in (("fast", "exact") if c == "nd3bbt" else ("fast",))])
def test_kernel_scene_blocks_are_the_dense_jacobian(hip, name, arith):
    """test_same_doubles_as_the_dense_jacobian: the blocks against Model.kernel bit for bit, zeros outside, rad, tau and
    the tangent points against formod_host."""
    J.test_same_doubles_as_the_dense_jacobian(hip, name, arith)
    case, geom, k, obs, out = J.dense_and_blocks(hip, name, arith)
    nd = configured(case, name)
    assert out["rad"].shape == (len(geom), nd) and k.shape[0] == len(geom) * nd
    unit_of(case, out["rad"])
    widths = np.diff(out["rowptr"])
    assert (widths > 0).sum() >= 10 and len(out["k"]) == widths.sum() * nd
    rows = np.repeat(widths > 0, nd)
    per_channel = np.abs(k[rows]).reshape(-1, nd, k.shape[1]).max(axis=(0, 2))
    assert np.all(per_channel > 0), "every channel has entries that are not zero"
    print("CHANNELS kernel_scene %s %s: %d rays, %d block entries, largest |k| %.3g" % (name, arith, len(geom), len(out["k"]), np.abs(k).max()))


@pytest.mark.parametrize("name", [n for c in ALL for n in on("ragged", [c]) + on("lone_ends", [c])])
def test_kernel_scene_passes(hip, name):
    J.test_passes(hip, name)


@pytest.mark.parametrize("name", on("ragged", ("nd3", "nd7", "nd65")))
def test_kernel_scene_nan_mask(hip, name):
    """a masked measurement in the first and in the last channel: NaN rows of the blocks where Model.kernel drops rows"""
    J.test_nan_mask(hip, name)


@pytest.mark.parametrize("arith", ["fast", "exact"])
def test_kernel_scene_against_the_stored_reference_in_brightness_temperatures(hip, tmp_path, arith):
    J.test_blocks_against_stored_reference(hip, tmp_path, "jacobian_nd3_bbt", arith)


# ---- 2. normal_scene ---------------------------------------------------------------------------------------------------
SUMS_ON = on("ragged", ("nd1", "nd3bbt", "nd7", "nd65"))


@pytest.mark.parametrize("name", SUMS_ON)
def test_normal_scene_against_the_blocks(hip, name):
    case, lay, nd = layout_is_not_trivial(hip, name)
    N.test_against_the_blocks(hip, name, "fast")
    out = N.blocks_and_sums(hip, name)[1]
    per_slice = np.bincount(out["sid"][out["sid"] >= 0]) * nd
    assert np.array_equal(out["nlive"], per_slice)
    if nd != 65:
        assert np.all(per_slice % 8 != 0), "no slice's measurements fill its groups of 8"


@pytest.mark.parametrize("name", SUMS_ON)
def test_normal_scene_arrangements(hip, name):
    N.test_arrangements(hip, name)


@pytest.mark.parametrize("name", on("ragged", ("nd3", "nd7")))
def test_normal_scene_live_rule(hip, name):
    """masked measurements on every channel index, the last included"""
    layout_is_not_trivial(hip, name)
    N.test_live_rule(hip, name)


# ---- 3. gradient_scene -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SUMS_ON)
def test_gradient_scene(hip, name):
    case, lay, nd = layout_is_not_trivial(hip, name)
    per_slice = np.bincount(lay["sid"][lay["sid"] >= 0]) * nd
    assert (per_slice.max() > 64) == (nd >= 65), "only with nd65 does a slice have more than a chunk of 64 measurements"
    RC.test_gradient_against_the_normal_equations(hip, name)


# ---- 4. trial_scene ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", on("ragged", ("nd3bbt", "nd7")))
def test_trial_scene(hip, name):
    layout_is_not_trivial(hip, name)
    T.test_trial_costs_are_normal_scene_on_the_written_back_atmosphere(hip, name)


# ---- 5. retrieve_scene -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", on("ragged", ("nd3", "nd7")))
def test_retrieve_scene_replay(hip, name, mode):
    """(not on nd1: six measurements per slice leave the systems rank-deficient without a prior, and the first
    iteration's solves need not succeed)"""
    layout_is_not_trivial(hip, name)
    T.test_replay_on_the_host(hip, name, mode)
    got = T.retrieved(hip, name, mode)
    assert np.any(got["h_accept"] == 1) and np.any(got["x"] != T.layout(hip, name)[3])


def test_retrieve_scene_replay_with_a_reused_jacobian(hip):
    RC.test_replay_on_the_host(hip, "ragged@nd3", 0, 2)


# ---- 6. the field of view ----------------------------------------------------------------------------------------------
FOV_ON = on("ragged", ("nd3", "nd7"))


def fov_scene_is_not_trivial(hip, name):
    case, geom, y, weight, lay = F.scene(hip, name)[:5]
    nd = configured(case, name)
    assert not case.ctl.write_bbt and y.shape == (len(geom), nd)
    assert len(lay["sfirst"]) >= 3 and np.diff(lay["wptr"]).max() > 32
    values = (np.diff(lay["rowptr"]) + 1) * nd                           # of a ray: the base and its columns, every channel
    assert np.any(values[values > nd] % 8 != 0)
    return values


@pytest.mark.parametrize("name", FOV_ON)
def test_fov_kernel_scene(hip, name):
    fov_scene_is_not_trivial(hip, name)
    F.test_kernel_scene_against_the_host_replay(hip, name)


@pytest.mark.parametrize("name", FOV_ON)
def test_fov_normal_scene(hip, name):
    fov_scene_is_not_trivial(hip, name)
    F.test_normal_scene_against_its_blocks(hip, name)


@pytest.mark.parametrize("name", FOV_ON)
def test_fov_trial_scene(hip, name):
    fov_scene_is_not_trivial(hip, name)
    F.test_trial_costs_are_normal_scene_on_the_written_back_atmosphere(hip, name)


def test_fov_long_shape_with_seven_channels(hip):
    """a ray's (w + 1) * 7 values are taken 256 at a time and the shape of 150 points is staged again for each: the
    widest slice's count is neither a multiple of 256 nor below it"""
    name = "ragged@nd7"
    case = J.scene_case(name, windows=F.wide_windows)
    nd = configured(case, name)
    geom = F.scan_geometry(case)
    values = (np.diff(hip.scene_layout(case.ctl, case.atm, geom[:, 0])["rowptr"]) + 1) * nd
    assert values.max() > 2 * 256 and values.max() % 256 != 0
    F.test_a_long_shape_and_wide_slices(hip, name)


# ---- 7. diagnose_scene and gain_scene ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", on("ragged", ("nd3bbt", "nd7")))
def test_diagnose_scene(hip, name):
    layout_is_not_trivial(hip, name)
    D.test_scene_entry_equals_its_halves(hip, name, "all")


@pytest.mark.parametrize("name", on("ragged", ("nd3bbt", "nd7", "nd65")))
def test_gain_scene(hip, name):
    """with nd65 one ray's rows alone exceed a tile of 64 measurements"""
    layout_is_not_trivial(hip, name)
    G.test_scene_entry_against_its_pieces(hip, name)


# ---- 8. param_error_scene ----------------------------------------------------------------------------------------------
def test_param_error_scene(hip):
    configured(J.scene_case("ragged@nd3"), "ragged@nd3")
    PA.test_a_real_parameter(hip, False, "ragged@nd3")
