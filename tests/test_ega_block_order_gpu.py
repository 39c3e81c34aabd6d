"""The look-up kernel takes the launch's block order (jur_tune_block_order_ega): jur_ega_kernel feeds the ray block that
xcd_block_item hands it through the order jur_combine_kernel already uses, so its longest ray blocks start first.
Placement only: with the order against without, every output is the same bit for bit.

4096 * 64 + 70 rays of the benchmark's generator on 2 profiles: the smallest call for which the default rule builds an
order (262 144 rays), one trace launch and one integration launch over the same slots, 1025 blocks of which the last
holds 70 rays.  The transmittance plane the look-up writes has no read-back of its own (34 GB here); it is read through
the contributions (jur_formod_contrib_host), whose kernel turns every plane entry of every (ray, channel, emitter) into
that emitter's own radiance and transmittance, next to rad and tau of the forward model itself.  Before each measured
call the model runs the same rays on the other profile each, so that a plane entry the ordered launch failed to write
would hold another ray set's value, not the one an earlier run left there."""
import numpy as np
import pytest
import common
from jurassic_hip import synth

pytestmark = pytest.mark.gpu

NR = 4096 * 64 + 70
NBLK = (NR + 255) // 256


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


@pytest.fixture(scope="module")
def case():
    return common.limb_case(geom=synth.limb_rays(np.arange(NR), nprofiles=2), nu=common.CTM4_NU, nprofiles=2)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run(hip, case, ega_order):
    m = hip.Model(case.ctl, case.lib_tables())
    try:
        m.set_atm(case.atm)
        m.set_pencil(0)
        hip.tune_block_order_ega(ega_order)
        other = case.geom.copy()
        other[:, 0] = 1.0 - other[:, 0]
        m.formod_host(other)                               # leaves another ray set's values in the workspaces
        out = m.formod_contrib_host(case.geom)
        return out, m.block_order(), m.last_launches()
    finally:
        hip.tune_block_order_ega(-1)
        m.close()


def test_look_up_with_the_order_equals_the_look_up_in_slot_order(hip, case):
    on, order, launches = run(hip, case, 1)
    off, order_off, launches_off = run(hip, case, 0)
    # the default rule built the order, and the one integration launch covers the slots of the trace launch
    assert order.shape == (NBLK,) and np.array_equal(np.sort(order), np.arange(NBLK))
    assert np.array_equal(order, order_off) and launches == 1 and launches_off == 1
    assert not np.array_equal(order, np.arange(NBLK))      # two profiles: the order moves blocks
    assert np.isfinite(on["rad"]).all() and on["np"].min() > 0
    for key in ("rad", "tau", "rad_c", "tau_c", "tp"):
        assert np.array_equal(bits(on[key]), bits(off[key])), key
    assert np.array_equal(on["np"], off["np"])
    # the plane was read: every emitter with a table leaves a transmittance below one somewhere
    ng = case.ctl.ng
    assert all(on["tau_c"][g].min() < 1.0 for g in range(ng))
