"""The strict-table look-up with its [0, 1] clamps as output modifiers (fma_c01 / add_c01 in jur_kernels.hip) against
what the library computed BEFORE that change, bit for bit: the modifier clamps the rounded result of the very
operation a v_min_f64 / v_max_f64 pair used to follow, so no output may move by a single bit.

The expected values under tests/golden/ega_clamp/ were recorded ONCE on an MI355X from the library built from the
commit before the change (the inputs are made by the functions below, from fixed seeds, and stored beside them):

    git worktree add ../parent <parent commit> && make -C ../parent/jurassic-gpu_amd/csrc
    JURASSIC_HIP_SO=../parent/jurassic-gpu_amd/libjurassic_hip.so python3 tests/test_ega_clamp_gpu.py --record [directory]

  lookup_in.npy   (2, 4, N)  tau, t, u, p for the pairs PAIRS of the limb case, N = 4096 + 8
  lookup_out.npy  (2, N)     Model.kat_ega_eps(ig, id_, tau, t, u, p, mode=3) of the parent
  formod_geom.npy (150, 7)   150 limb rays over three profiles (two full tiles of 64 rays and a partial one)
  formod_rad.npy, formod_tau.npy  (3, 150, 4)  jur_formod_device of the parent, one plane per arrangement of ARRANGEMENTS

The look-up inputs drive each clamp to both rails (lookup_inputs): columns far beyond a curve's last entry (emissivity
past 1), columns below its first entry on a nearly transparent path (extrapolation below 0), temperatures and
pressures outside the table axes on either side (blends outside [0, 1]), pressures so far below the axis that the
pressure blend of two positive emissivities is negative, an interior control group, and eight inputs
with a NaN in one of the four arguments.  That the recorded outputs DO sit on both rails and in between is asserted on
the fixture itself, so the comparison cannot pass on inputs that never reach a clamp."""
import os
import sys
import numpy as np
import pytest

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "jurassic-gpu_amd"), os.path.join(_root, "tests")]
import common
from jurassic_hip import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(common.GOLD, "ega_clamp")
PAIRS = ((0, 0), (2, 1))
N_LOOKUP, N_NAN = 4096, 8
ARRANGEMENTS = ("fused", "batched", "batched_grouped")


def lookup_inputs(rows, seed):
    """(4, N_LOOKUP + N_NAN): tau, t, u, p for one table (rows of p, T, u, eps), six groups of N_LOOKUP / 6 + the NaNs."""
    rng = np.random.default_rng(seed)
    plev, tlo, thi = np.unique(rows[:, 0]), rows[:, 1].min(), rows[:, 1].max()
    ulo, uhi = rows[:, 2].min(), rows[:, 2].max()
    n = N_LOOKUP // 6
    logu = lambda a, b, k: 10.0 ** rng.uniform(np.log10(a), np.log10(b), k)
    inside_t = lambda k: rng.uniform(tlo + 10, thi - 10, k)
    inside_p = lambda k: logu(plev[1], plev[-2], k)
    groups = [
        # emissivity past 1 on every curve: columns far beyond the last entry
        (logu(1e-6, 1.0, n), inside_t(n), uhi * logu(1e3, 1e9, n), inside_p(n)),
        # extrapolation below 0: column far below the first entry on a nearly transparent path -- tau within 1e-8 below 1
        # (the curve's line through its first bracket, followed down and back up: an emissivity of +-1e-20 .. 1e-8), and
        # tau up to 1e-6 ABOVE 1 (path emissivity below 0: every curve clamps at 0 for certain)
        (np.where(rng.random(n) < 0.5, 1.0 - logu(1e-12, 1e-8, n), 1.0 + logu(1e-9, 1e-6, n)), inside_t(n),
         ulo * logu(1e-9, 1e-4, n), inside_p(n)),
        # temperature outside the axis on both sides (up to 60 K), emissivities of order one: the T blends leave [0, 1]
        (logu(1e-3, 0.999, n), np.where(rng.random(n) < 0.5, tlo - rng.uniform(0.5, 60, n), thi + rng.uniform(0.5, 60, n)),
         logu(ulo * 1e3, uhi * 1e-2, n), inside_p(n)),
        # pressure outside the axis on both sides: the p blend leaves [0, 1]
        (logu(1e-3, 0.999, n), inside_t(n), logu(ulo * 1e3, uhi * 1e-2, n),
         np.where(rng.random(n) < 0.5, plev[0] * rng.uniform(0.01, 0.95, n), plev[-1] * rng.uniform(1.05, 30, n))),
        # the p blend itself BELOW 0 on a path with tau < 1: a nearly transparent path (every curve is read at about the
        # segment's column, so the two levels' emissivities differ by their tables' ~13 %) and a pressure 3 .. 30 axis
        # origins below the axis (negative: nothing nearer extrapolates these tables past 0) -- the final add_c01 clamps a
        # negative sum of two positive blends, and the look-up answers 1 / tau
        (1.0 - logu(1e-6, 1e-4, n), inside_t(n), logu(ulo * 1e3, uhi * 1e-3, n), -plev[0] * rng.uniform(3, 30, n)),
    ]
    m = N_LOOKUP - 5 * n        # interior control group
    groups.append((logu(1e-6, 0.999999, m), inside_t(m), logu(ulo * 10, uhi * 0.1, m), inside_p(m)))
    x = np.concatenate([np.stack(g) for g in groups], axis=1)
    x = x[:, rng.permutation(x.shape[1])]           # mixed wavefronts: lanes on both rails and in between
    nan = np.tile(np.array([[0.5], [250.0], [np.sqrt(ulo * uhi)], [100.0]]), (1, N_NAN))
    nan[2, 4:] = uhi * 1e6                           # the second four next to a clamp at 1
    for k in range(N_NAN):
        nan[k % 4, k] = np.nan                       # tau, t, u, p in turn
    return np.concatenate([x, nan], axis=1)


def formod_case(geom=None):
    g = synth.limb_geometry(150, seed=5, nprofiles=3) if geom is None else geom
    return common.limb_case(geom=g, nu=common.CTM4_NU, nprofiles=3)


def run_lookup(hip, x):
    case = common.limb_case()
    m = hip.Model(case.ctl, case.lib_tables())
    out = np.stack([m.kat_ega_eps(ig, id_, *x[k], mode=3) for k, (ig, id_) in enumerate(PAIRS)])
    m.close()
    return out


def run_formod(hip, case, arrangement):
    """jur_formod_device on torch-owned buffers, arranged with the switches of tests/test_parity_gpu.py."""
    import torch
    model = hip.Model(case.ctl, case.lib_tables())
    if arrangement != "fused":
        model.set_pencil(0)
    model.enable_timing()
    if arrangement == "batched_grouped":
        hip.tune_combine(4, 8, 0)
    try:
        model.set_atm(case.atm)
        dev = torch.device("cuda", 0)
        nr, nd = len(case.geom), case.ctl.nd
        d_geom = torch.from_numpy(np.ascontiguousarray(case.geom.T)).to(dev)
        d_rad = torch.zeros((nr, nd), dtype=torch.float64, device=dev)
        d_tau = torch.empty((nr, nd), dtype=torch.float64, device=dev)
        d_tp = torch.empty((3, nr), dtype=torch.float64, device=dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        model.formod_device(nr, d_geom.data_ptr(), d_rad.data_ptr(), d_tau.data_ptr(), d_tp.data_ptr(), 0, d_st.data_ptr(), 0)
        torch.cuda.synchronize()
        assert int(d_st.item()) == 0
        ms = model.kernel_ms()                      # the arrangement asked for is the one that ran
        if arrangement == "fused":
            assert ms["pencil_launches"] > 0 and ms["ega_launches"] == 0, ms
        else:
            assert ms["pencil_launches"] == 0 and ms["ega_launches"] > 0 and ms["combine_launches"] > 0, ms
        return d_rad.cpu().numpy(), d_tau.cpu().numpy()
    finally:
        if arrangement == "batched_grouped":
            hip.tune_combine(-1, 8, 1_000_000)
        model.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert os.path.exists(lib.SO), "libjurassic_hip.so missing: the HIP path must be built"
    return lib


def test_recorded_lookup_outputs_sit_on_both_rails_and_between():
    """A condition on the fixture (no device code runs): the parent's outputs hold look-ups that ended in the final
    clamp at 1 (path transmittance 0 -> 0), in the final clamp at 0 (1 - 0 over tau -> 1 / tau) and strictly between."""
    x, ref = np.load(os.path.join(GOLD, "lookup_in.npy")), np.load(os.path.join(GOLD, "lookup_out.npy"))
    assert x.shape == (len(PAIRS), 4, N_LOOKUP + N_NAN) and ref.shape == (len(PAIRS), N_LOOKUP + N_NAN)
    for k, (ig, id_) in enumerate(PAIRS):
        tau, out = x[k, 0, :N_LOOKUP], ref[k, :N_LOOKUP]
        assert np.all(tau >= 1e-9) and np.all(np.isfinite(out))       # none answered by the tau < 1e-9 gate
        zeros, ones, between = out == 0.0, out == 1.0 / tau, (out > 0.0) & (out < 1.0 / tau)
        print("pair (%d, %d): %d exact zeros, %d equal to 1 / tau, %d strictly between" % (ig, id_, zeros.sum(), ones.sum(), between.sum()))
        assert zeros.sum() >= 64 and ones.sum() >= 64 and between.sum() >= 1024
        # ... and the final clamp at 0 is reached from a NEGATIVE p blend too (tau < 1), not only from four curves at 0
        print("   equal to 1 / tau with tau < 1: %d" % (ones & (tau < 1)).sum())
        assert (ones & (tau < 1)).sum() >= 64
        assert zeros.sum() + ones.sum() + between.sum() == N_LOOKUP
        assert np.all(np.isnan(ref[k, N_LOOKUP:]))                    # one NaN argument each


def test_lookup_is_bit_equal_to_the_recorded_parent(hip):
    x, ref = np.load(os.path.join(GOLD, "lookup_in.npy")), np.load(os.path.join(GOLD, "lookup_out.npy"))
    got = run_lookup(hip, x)
    for k, pair in enumerate(PAIRS):
        bad = np.nonzero(bits(got[k, :N_LOOKUP]) != bits(ref[k, :N_LOOKUP]))[0]
        assert len(bad) == 0, (pair, len(bad), x[k][:, bad[:3]], got[k, bad[:3]], ref[k, bad[:3]])
        # a NaN in tau, t, u or p: what the parent answered, bit for bit
        assert np.array_equal(bits(got[k, N_LOOKUP:]), bits(ref[k, N_LOOKUP:])), (pair, got[k, N_LOOKUP:], ref[k, N_LOOKUP:])


@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
def test_forward_model_is_bit_equal_to_the_recorded_parent(hip, arrangement):
    geom = np.load(os.path.join(GOLD, "formod_geom.npy"))
    assert geom.shape == (150, 7)
    k = ARRANGEMENTS.index(arrangement)
    ref_rad, ref_tau = np.load(os.path.join(GOLD, "formod_rad.npy"))[k], np.load(os.path.join(GOLD, "formod_tau.npy"))[k]
    assert np.all(np.isfinite(ref_rad)) and np.all(ref_rad > 0) and np.all((ref_tau >= 0) & (ref_tau <= 1))
    rad, tau = run_formod(hip, formod_case(geom), arrangement)
    assert rad.shape == ref_rad.shape == (150, len(common.CTM4_NU))
    assert np.array_equal(bits(rad), bits(ref_rad)), int(np.count_nonzero(bits(rad) != bits(ref_rad)))
    assert np.array_equal(bits(tau), bits(ref_tau)), int(np.count_nonzero(bits(tau) != bits(ref_tau)))


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"] and len(sys.argv) <= 3, __doc__
    if len(sys.argv) == 3:
        GOLD = sys.argv[2]                          # (another directory than tests/golden/ega_clamp)
    import torch
    torch.cuda.is_available()                       # torch's HIP runtime first (tests/conftest.py)
    from jurassic_hip import lib
    print("recording from", lib.SO)
    os.makedirs(GOLD, exist_ok=True)
    rows = common.limb_case().rows
    x = np.stack([lookup_inputs(rows[pair], seed=100 + k) for k, pair in enumerate(PAIRS)])
    np.save(os.path.join(GOLD, "lookup_in.npy"), x)
    np.save(os.path.join(GOLD, "lookup_out.npy"), run_lookup(lib, x))
    case = formod_case()
    np.save(os.path.join(GOLD, "formod_geom.npy"), case.geom)
    res = [run_formod(lib, case, a) for a in ARRANGEMENTS]
    np.save(os.path.join(GOLD, "formod_rad.npy"), np.stack([r[0] for r in res]))
    np.save(os.path.join(GOLD, "formod_tau.npy"), np.stack([r[1] for r in res]))
