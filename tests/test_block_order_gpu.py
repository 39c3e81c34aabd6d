"""The block order of a sorted launch (jur_tune_block_order, jur_chunk_t::blk_order): the one-lane-per-ray tracers and
the radiance update start the blocks of 256 sorted slots longest paths first instead of in slot order.  Placement only:
every workgroup computes what it computed before, from the same slots into the same slots, so order on against order
off gives rad, tau, tp and np bit for bit -- through both tracers (the slice kernel, one workgroup to the block, and the
64-lane kernel, four), both update kernels (one channel per workgroup; grouped with two, one and four super-blocks to
the block, and with super-blocks of 512 slots, which stay in order) and the partial last block.

The base case is 5 * 256 + 37 = 1317 limb rays on 3 profiles whose view points lie between -5 and 70 km: rays that hit
the ground and short ones among them.  One run per arrangement is also held to the oracle with the suite's tolerances
(radiances 1e-9 relative, transmittances 1e-9 relative + common.tau_atol, tangent points 1e-9)."""
import numpy as np
import pytest
import common
from jurassic_hip import synth

pytestmark = pytest.mark.gpu

NR = 5 * 256 + 37
NBLK = (NR + 255) // 256


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def base_case(nu=common.CTM4_NU, nr=NR, nprofiles=3, seed=3):
    g = synth.limb_geometry(nr, seed=seed, zmin=-5.0, zmax=70.0, nprofiles=nprofiles)
    return common.limb_case(geom=g, nu=nu, nprofiles=nprofiles)


def by_profile_case(nu=common.CTM4_NU):
    """1171 + 1170 = 2341 rays on two profiles: enough per profile for the sort to group the rays by profile (key =
    profile, tangent altitude).  The slots are then two ascending runs, -5 .. 70 km and -5 .. 30 km; the order interleaves
    their blocks; block 4 straddles both profiles -- it begins at 60 km in the first and holds the lowest rays of the
    second, so it is started second --; and the partial tenth block is started eighth, so the launches must cover whole
    blocks.  The base case's slots ascend through the whole launch: its order is 0 1 2 ..., under which a wrong mapping
    would not show."""
    g0 = synth.limb_geometry(1171, seed=5, zmin=-5.0, zmax=70.0)
    g1 = synth.limb_geometry(1170, seed=6, zmin=-5.0, zmax=30.0)
    g1[:, 0] = 1
    g = np.vstack([g0, g1])[np.random.default_rng(7).permutation(2341)]
    return common.limb_case(geom=g, nu=nu, nprofiles=2)


BY_PROFILE_ORDER = [0, 4, 5, 6, 1, 7, 8, 2, 9, 3]


@pytest.fixture(scope="module")
def case():
    return base_case()


@pytest.fixture(scope="module")
def case2():
    return by_profile_case()


@pytest.fixture(scope="module")
def ref(oracle, case):
    """The oracle's answer for the base case, computed once and left alone."""
    return oracle.formod_rays(case.ctl, case.atm, case.oracle_tables(oracle), case.geom)


# tracer: tune_trace_slice mode (2: slice kernel, 1: 64-lane kernel); update: tune_combine's channels per group
# (0: one channel per workgroup; g: grouped, 8 / min(nd, g) tiles of 64 slots to the super-block)
ARRANGEMENTS = {"slice+grouped4": (2, 4), "lanes64+plain": (1, 0), "slice+grouped2": (2, 2), "lanes64+grouped1": (1, 1)}


def run(hip, case, mode, slice_mode=2, group=4, prepare=None):
    """-> (forward results, block order read back) of one call on the batched kernels under jur_tune_block_order(mode)."""
    m = hip.Model(case.ctl, case.lib_tables())
    try:
        m.set_atm(case.atm)
        m.set_pencil(0)
        if prepare:
            prepare(m)
        hip.tune_trace(1)
        hip.tune_trace_slice(slice_mode)
        hip.tune_combine(group, 8, 0)
        hip.tune_block_order(mode)
        out = m.formod_host(case.geom)
        return out, m.block_order()
    finally:
        hip.tune_block_order(0)
        hip.tune_combine(-1, 8, 1_000_000)
        hip.tune_trace_slice(0)
        hip.tune_trace(0)
        m.close()


def assert_same(on, off, what):
    for key in ("rad", "tau", "tp"):
        assert np.array_equal(bits(on[key]), bits(off[key])), (what, key)
    assert np.array_equal(on["np"], off["np"]), (what, "np")


def assert_permutation(order, nblk, what=""):
    assert order.shape == (nblk,) and np.array_equal(np.sort(order), np.arange(nblk)), (what, order)


def assert_oracle(out, ref):
    assert np.array_equal(out["np"], ref["np"])
    fin = np.isfinite(ref["rad"])
    assert np.array_equal(fin, np.isfinite(out["rad"]))
    assert common.rel_err(out["rad"][fin], ref["rad"][fin]).max() < 1e-9
    terr = np.abs(out["tau"] - ref["tau"])
    assert np.all(terr <= 1e-9 * np.abs(ref["tau"]) + common.tau_atol(ref["tau"]))
    assert np.abs(out["tp"] - ref["tp"]).max() < 1e-9


@pytest.mark.parametrize("name", sorted(ARRANGEMENTS))
def test_order_on_equals_order_off_and_the_oracle(hip, case, ref, name):
    slice_mode, group = ARRANGEMENTS[name]
    on, order = run(hip, case, 2, slice_mode, group)
    off, none = run(hip, case, 1, slice_mode, group)
    assert_permutation(order, NBLK, name)
    assert len(none) == 0
    assert_same(on, off, name)
    assert_oracle(on, ref)


@pytest.mark.parametrize("name", sorted(ARRANGEMENTS))
def test_order_that_moves_blocks(hip, case2, name):
    slice_mode, group = ARRANGEMENTS[name]
    on, order = run(hip, case2, 2, slice_mode, group)
    off, _ = run(hip, case2, 1, slice_mode, group)
    assert_permutation(order, 10, name)
    assert_lowest_rays_ascend(case2, order, by_profile=True)
    assert list(order) == BY_PROFILE_ORDER
    assert_same(on, off, name)


def test_grouped_update_with_four_super_blocks_to_the_block(hip):
    """Six channels in one group: super-blocks of one tile, four to the block of 256 slots."""
    case = by_profile_case(nu=common.CTM4_NU + [667.782, 950.0])
    on, order = run(hip, case, 2, 2, 6)
    off, _ = run(hip, case, 1, 2, 6)
    assert list(order) == BY_PROFILE_ORDER
    assert_same(on, off, "grouped6")


def assert_lowest_rays_ascend(case, order, by_profile):
    """The tangent altitudes of the blocks' lowest rays do not decrease along the order.  The rays look at their tangent
    point, so the geometric tangent altitude the sort key holds is the view point's altitude up to rounding: the key is
    that altitude in float32 (spacing 8e-6 km at 70 km), so two slots, and two blocks, may change places when they are
    closer than that.  Allowance 2e-5 km.  -> the altitudes of the blocks' FIRST rays along the order"""
    vpz, prof = case.geom[:, 4], case.geom[:, 0]
    slots = np.lexsort((vpz, prof)) if by_profile else np.argsort(vpz, kind="stable")
    lowest = np.array([vpz[slots[b * 256:(b + 1) * 256]].min() for b in order])
    assert np.all(np.diff(lowest) >= -2e-5), lowest
    return vpz[slots[order.astype(np.int64) * 256]]


def test_read_back_is_a_permutation_in_tangent_altitude_order(hip, case):
    _, order = run(hip, case, 2)
    assert_permutation(order, NBLK)
    # 1317 rays on 3 profiles are sorted by tangent altitude alone: a block's first ray is its lowest
    first = assert_lowest_rays_ascend(case, order, by_profile=False)
    assert np.all(np.diff(first) >= -2e-5), first
    # and here, where the slots ascend through the whole launch, the blocks stay in order: longest paths first already
    assert np.array_equal(order, np.arange(NBLK))


def test_equal_keys_leave_a_permutation(hip):
    """3 x 256 rays of one geometry: every block key is the same."""
    g = np.repeat(synth.limb_geometry(1, scan=True, zmin=20.0, zmax=20.0), 3 * 256, axis=0)
    case = common.limb_case(geom=g, nu=common.CTM4_NU)
    on, order = run(hip, case, 2)
    off, _ = run(hip, case, 1)
    assert_permutation(order, 3)
    assert_same(on, off, "ties")
    assert np.array_equal(bits(on["rad"]), bits(np.broadcast_to(on["rad"][0], on["rad"].shape)))


def test_several_integration_launches_per_trace_launch(hip, case):
    """Chunks of 256 rays: one trace launch (ordered), several integration launches, which run in order -- laid out by
    path length (the default) and at JUR_NLOS points per ray."""
    def compact(m):
        m.set_chunk_rays(256)

    def plain(m):
        m.set_chunk_rays(256)
        m.set_compact_workspace(False)
        m.set_trace_multiple(6)

    for name, prepare in (("compact", compact), ("plain", plain)):
        on, order = run(hip, case, 2, prepare=prepare)
        off, _ = run(hip, case, 1, prepare=prepare)
        assert_permutation(order, NBLK, name)
        assert_same(on, off, name)


def test_call_larger_than_a_trace_launch_builds_no_order(hip, case):
    def prepare(m):
        m.set_chunk_rays(256)
        m.set_compact_workspace(False)
        m.set_trace_multiple(1)

    on, order = run(hip, case, 2, prepare=prepare)
    off, _ = run(hip, case, 1, prepare=prepare)
    assert len(order) == 0
    assert_same(on, off, "nr > Rt")


def test_unsorted_call_builds_no_order(hip, case):
    on, order = run(hip, case, 2, prepare=lambda m: m.set_sort_rays(False))
    off, _ = run(hip, case, 1, prepare=lambda m: m.set_sort_rays(False))
    assert len(order) == 0
    assert_same(on, off, "unsorted")


def test_default_rule_builds_no_order_for_a_small_call(hip, case):
    _, order = run(hip, case, 0)
    assert len(order) == 0
