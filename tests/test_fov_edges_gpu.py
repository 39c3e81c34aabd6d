"""jur_fov_kernel (behind jur_fov_apply_device) at the constructed edges of tests/edgecases.py: the cases of
tests/test_fov_edges_cpu.py on device arrays, convolved in place.  The kernel equals the host twin and the oracle bit for
bit -- both computed from saved inputs, so a lane that read an already convolved neighbour would differ -- and lies
within the derived bound of the extended-precision model (twice the bound is allowed; edgecases' docstring counts the
operations).  nr nd of 255, 256 and 257 puts the launch's last lanes on both sides of a 256-lane block edge."""
import os
import numpy as np
import pytest
import common
import edgecases as E
from test_fov_edges_cpu import EXPECT, host_and_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


@pytest.fixture(scope="module")
def models(hip):
    """a model per channel count: jur_fov_apply_device takes nd from the model"""
    made = {}
    for nd in sorted({nd for nd, _ in E.FOV_SIZES}):
        case = common.Case(["CO2"], E.common_nu(nd), os.path.join(common.GOLD, "limb", "atm.tab"), np.zeros((1, 7)),
                           table_kw=dict(nlev=3, ntemp=2))
        made[nd] = hip.Model(case.ctl, case.lib_tables())
    yield made
    for m in made.values():
        m.close()


def on_device(model, batch, dz, w):
    """the in-place device call on copies of a batch's arrays -> rad, tau on the host"""
    import torch
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(np.ascontiguousarray(batch[k])).to(dev) for k in ("time", "vpz", "rad", "tau")}
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    model.fov_apply_device(len(batch["time"]), d["time"].data_ptr(), d["vpz"].data_ptr(), d["rad"].data_ptr(), d["tau"].data_ptr(),
                           dz, w, stream)
    return d["rad"].cpu().numpy(), d["tau"].cpu().numpy()


@pytest.mark.parametrize("nd,nr", E.FOV_SIZES)
def test_kernel_at_constructed_edges(hip, oracle, models, nd, nr):
    for shape in E.fov_shapes_of(nd, nr):
        batch, dz, w, ref = E.fov_case(nd, nr, shape)
        assert E.fov_edges(batch, ref, dz) == EXPECT[shape], shape
        saved = {k: batch[k].copy() for k in ("time", "vpz", "rad", "tau")}
        got_r, got_t = on_device(models[nd], batch, dz, w)
        assert all(np.array_equal(E.bits(batch[k]), E.bits(saved[k])) for k in saved)
        r, t, o_r, o_t = host_and_oracle(hip, oracle, batch, nd, dz, w)          # out of place, from the saved inputs
        assert np.array_equal(E.bits(got_r), E.bits(r)) and np.array_equal(E.bits(got_t), E.bits(t)), (shape, "host twin")
        assert np.array_equal(E.bits(got_r), E.bits(o_r)) and np.array_equal(E.bits(got_t), E.bits(o_t)), (shape, "oracle")
        ratio = E.fov_ratio(got_r, got_t, ref)
        print("fov nd=%d nr=%d %-5s kernel: worst error / allowed = %.3f" % (nd, nr, shape, ratio))
        assert ratio <= 1, shape


@pytest.mark.parametrize("lone", ["first", "middle", "last"])
def test_kernel_refuses_a_lone_ray(hip, models, lone):
    """As on the host: the call raises, and the entry promises nothing about d_rad and d_tau after it (the lanes of the
    other rays have written theirs), so nothing is asserted about them.  The next call on the model is served."""
    batch = E.fov_batch(E.NR_BASE, 2, lone=lone)
    dz, w = E.SHAPES["zeros"]
    with pytest.raises(hip.JurassicError, match="Cannot apply FOV"):
        on_device(models[2], batch, dz, w)
    good, _, _, ref = E.fov_case(2, E.NR_BASE, "zeros")
    got_r, got_t = on_device(models[2], good, dz, w)
    assert E.fov_ratio(got_r, got_t, ref) <= 1
