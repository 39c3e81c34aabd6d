"""The field-of-view convolution at constructed edges, on the CPU: the library's host twin (jur_fov_apply) and the oracle's
restatement of formod_fov against each other, bit for bit, and against the extended-precision model of
tests/edgecases.py within its derived bound (gamma_{n+7} S / |wsum| and the term of wsum's own roundings; the docstring
there counts the operations).  Twice the bound is allowed.

Every input is constructed (edgecases.fov_batch): scans of 2, 3, 11, 12 and 13 rays around the window of 11, a 2-ray scan
first and one last, ascending, descending and unequally spaced scans, two interleaved time stamps, shapes of 1, 2 and 2048
weights, exact zeros among the weights, an asymmetric shape with a negative lobe, offsets that reach beyond both ends of
every scan and land on neighbours' altitudes, and 1, 2, 3 and 7 channels with nr nd at 255, 256 and 257.  The model's
trace says which of these a case reaches, and the tests assert that list."""
import numpy as np
import pytest
import edgecases as E

EDGES = {"zfov exact", "2-ray scans clipped at lo = 0 and hi = nr", "scan shorter than the window", "full window",
         "interleaved: src is not lo + k", "ascending and descending scans", "unequal spacing",
         "dz beyond both ends of every scan", "end rays extrapolated by more than one spacing", "zfov on a neighbour's vpz"}
# one offset of a quarter kilometre reaches neither a neighbour nor both ends
EXPECT = {s: EDGES - ({"dz beyond both ends of every scan", "end rays extrapolated by more than one spacing",
                       "zfov on a neighbour's vpz"} if s == "n1" else set()) for s in E.SHAPES}


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    return lib


def host_and_oracle(hip, oracle, batch, nd, dz, w):
    nr = len(batch["time"])
    r, t = batch["rad"].copy(), batch["tau"].copy()
    hip.fov_apply(batch["time"], batch["vpz"], r, t, dz, w)
    obs = E.fov_obs(batch, nd)
    assert oracle.formod_fov(E.fov_ctl(nd), obs, dz, w) == 0
    return r, t, np.ctypeslib.as_array(obs.rad)[:nr, :nd].copy(), np.ctypeslib.as_array(obs.tau)[:nr, :nd].copy()


@pytest.mark.parametrize("nd,nr", E.FOV_SIZES)
def test_host_twin_and_oracle_at_constructed_edges(hip, oracle, nd, nr):
    worst = 0.0
    for shape in E.fov_shapes_of(nd, nr):
        batch, dz, w, ref = E.fov_case(nd, nr, shape)
        assert len(batch["time"]) == nr and batch["rad"].shape == (nr, nd)
        assert E.fov_edges(batch, ref, dz) == EXPECT[shape], shape           # the case reaches what it was built for
        r, t, o_r, o_t = host_and_oracle(hip, oracle, batch, nd, dz, w)
        assert np.array_equal(E.bits(r), E.bits(o_r)) and np.array_equal(E.bits(t), E.bits(o_t)), shape
        ratio = E.fov_ratio(r, t, ref)
        print("fov nd=%d nr=%d %-5s host twin / oracle: worst error / allowed = %.3f" % (nd, nr, shape, ratio))
        assert ratio <= 1, shape
        assert not np.array_equal(r, batch["rad"])
        worst = max(worst, ratio)
    print("fov nd=%d nr=%d: worst error / allowed = %.3f" % (nd, nr, worst))


@pytest.mark.parametrize("nd,nr", [(2, E.NR_BASE), (7, E.NR_BASE)])
def test_a_ray_reads_only_unconvolved_neighbours(hip, nd, nr):
    """The call is in place.  Every ray of the batch equals the same ray of a call on the rays of its window alone, from
    saved inputs: a ray that read a neighbour the loop had already convolved would differ."""
    for shape in ("zeros", "asym"):
        batch, dz, w, _ = E.fov_case(nd, nr, shape)
        r, t = batch["rad"].copy(), batch["tau"].copy()
        hip.fov_apply(batch["time"], batch["vpz"], r, t, dz, w)
        for ir in range(nr):
            src = E.fov_window(batch["time"], ir)[2]
            k = int(np.flatnonzero(src == ir)[0])
            r1, t1 = batch["rad"][src].copy(), batch["tau"][src].copy()
            hip.fov_apply(batch["time"][src], batch["vpz"][src], r1, t1, dz, w)
            assert np.array_equal(E.bits(r1[k]), E.bits(r[ir])) and np.array_equal(E.bits(t1[k]), E.bits(t[ir])), (shape, ir)


@pytest.mark.parametrize("lone", ["first", "middle", "last"])
def test_a_lone_ray_is_refused(hip, oracle, lone):
    """A ray without a second ray of its time stamp within +-5 positions -- first in the batch, in the middle (its time
    stamp returns 15 positions away) and last.  Host twin, oracle and model refuse the batch.  The entry documents the
    refusal and nothing about rad and tau after it (the host loop has convolved the rays in front of the lone one), so
    nothing is asserted about them."""
    nd = 2
    batch = E.fov_batch(E.NR_BASE, nd, lone=lone)
    dz, w = E.SHAPES["zeros"]
    at = {"first": 0, "middle": sum(E.BASE_SCANS[:3]), "last": E.NR_BASE}[lone]
    with pytest.raises(E.LoneRay) as err:
        E.fov_model(batch["time"], batch["vpz"], batch["rad"], batch["tau"], dz, w)
    assert err.value.args[0] == at
    r, t = batch["rad"].copy(), batch["tau"].copy()
    with pytest.raises(hip.JurassicError, match="Cannot apply FOV"):
        hip.fov_apply(batch["time"], batch["vpz"], r, t, dz, w)
    assert oracle.formod_fov(E.fov_ctl(nd), E.fov_obs(batch, nd), dz, w) == -1
