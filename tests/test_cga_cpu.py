"""Curtis-Godson forward model (FORMOD 1), the part that needs no GPU.

  * the look-up blocks of tests/cga_model.py, put together as ega_eps, equal the oracle's ega_eps bit for bit -- this
    pins the blocks the CGA rule is built from to the reference;
  * on tables whose curve is the same at every level and temperature the model's path transmittance is
    1 - c01(get_eps(curve, column so far)) along real rays: the prefix bookkeeping, independent of the means;
  * resource usage of the compiled kernels: no jur_cga_kernel instance uses scratch or more VGPRs than the
    jur_ega_kernel instance with the same switches, and no kernel that existed before changed;
  * the known-answer hook is exported.
"""
import json
import os
import re
import subprocess
import numpy as np
import pytest
import common
import cga_model as M
from jurassic_hip import lib, synth

ROOT = common.ROOT


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_doubles(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a)[~np.isnan(a)], bits(b)[~np.isnan(b)])


def around(x, k=2):
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


def lookup_inputs(rows, seed, n_random=1500):
    """(tau, t, u, p) of the kind tests/test_kat_gpu.py::ega_inputs builds: the tau gate, both ends of the p and T axes,
    both ends of a curve and beyond, u = 0, and random draws."""
    rng = np.random.default_rng(seed)
    plev, tlev = np.unique(rows[:, 0]), np.unique(rows[:, 1])
    plev = np.concatenate([plev, np.repeat(plev[-1:], max(0, 6 - len(plev)))])
    tlev = np.concatenate([tlev, np.repeat(tlev[-1:], max(0, 5 - len(tlev)))])
    ulo, uhi = rows[:, 2].min(), rows[:, 2].max()
    taus = around(1e-9, 1) + [1.0, np.nextafter(1.0, 0), 0.999, 0.5, 1e-3, 1e-8, 0.0, 1e-300]
    ps = [plev[0] * 0.1, np.nextafter(plev[0], 0), plev[0], plev[1], np.sqrt(plev[3] * plev[4]), np.nextafter(plev[-1], 0),
          plev[-1], plev[-1] * 1.2]
    ts = [100.0, tlev[0] - 1e-9, tlev[0], 0.5 * (tlev[2] + tlev[3]), tlev[-1], tlev[-1] + 1e-9, 399.99]
    us = [0.0, ulo * 1e-6, ulo, np.sqrt(ulo * uhi), uhi, uhi * 1e6, 1e30]
    g = np.array(np.meshgrid(taus, ts, us, ps, indexing="ij")).reshape(4, -1)
    r = np.stack([10.0 ** rng.uniform(-9.3, 0, n_random), rng.uniform(150, 360, n_random),
                  10.0 ** rng.uniform(np.log10(ulo) - 3, np.log10(uhi) + 3, n_random),
                  10.0 ** rng.uniform(np.log10(plev[0]) - 1, np.log10(plev[-1]) + 0.3, n_random)])
    x = np.concatenate([g, r], axis=1)
    return x[0], x[1], x[2], x[3]


@pytest.mark.parametrize("kw,pairs", [(dict(), ((0, 0), (2, 1), (4, 0))),
                                      (dict(table_kw=dict(dup_every=7)), ((1, 1),)),
                                      (dict(table_kw=dict(descending=True)), ((1, 1),)),
                                      (dict(table_kw=dict(nlev=2, ntemp=2)), ((1, 1),))])
def test_lookup_blocks_restate_ega_eps_bit_for_bit(oracle, kw, pairs):
    case = common.limb_case(**kw)
    ot = case.oracle_tables(oracle)
    for ig, id_ in pairs:
        pair = M.Pair(case.rows[(ig, id_)])
        tau, t, u, p = lookup_inputs(case.rows[(ig, id_)], seed=10 * ig + id_)
        ref = oracle.ega_eps(ot, ig, id_, tau, t, u, p)
        got = np.array([M.ega_eps(pair, *x) for x in zip(tau.tolist(), t.tolist(), u.tolist(), p.tolist())])
        assert np.any(tau < 1e-9) and np.all(ref[tau < 1e-9] == 0) and np.any(ref[tau >= 1e-9] > 0)
        bad = np.nonzero(~((bits(got) == bits(ref)) | (np.isnan(got) & np.isnan(ref))))[0]
        assert len(bad) == 0, (ig, id_, len(bad), tau[bad[:3]], t[bad[:3]], u[bad[:3]], p[bad[:3]], got[bad[:3]], ref[bad[:3]])


def test_lookup_blocks_without_a_table_and_on_nan(oracle):
    case = common.limb_case(missing={(1, 0)}, table_kw=dict(nlev=3, ntemp=3))
    ot = case.oracle_tables(oracle)
    tau = np.array([0.5, 1e-10, 1.0]); t = np.full(3, 250.0); u = np.full(3, 1e18); p = np.full(3, 100.0)
    assert list(oracle.ega_eps(ot, 1, 0, tau, t, u, p)) == [M.ega_eps(None, *x) for x in zip(tau, t, u, p)] == [1.0, 0.0, 1.0]
    assert [M.cga_lookup(None, *x) for x in zip(tau, t, u, p)] == [0.5, 0.0, 1.0]
    pair = M.Pair(case.rows[(0, 0)])
    nan = float("nan")
    for x in ((nan, 250.0, 1e18, 100.0), (0.5, nan, 1e18, 100.0), (0.5, 250.0, nan, 100.0), (0.5, 250.0, 1e18, nan)):
        ref = oracle.ega_eps(ot, 0, 0, *[np.array([v]) for v in x])[0]
        assert np.isnan(ref) and np.isnan(M.ega_eps(pair, *x)), x
        # past the gate the CGA rule does not use tau: a NaN there (no gate: the comparison is false) changes nothing
        got = M.cga_lookup(pair, *x)
        assert got == M.cga_lookup(pair, 0.5, *x[1:]) if x[0] != x[0] else np.isnan(got), x


def one_curve_rows(k, nlev=5, ntemp=4):
    """A table whose curve is the same at every level and temperature."""
    u = 1e14 * 1.3 ** np.arange(120)
    eps = 1.0 - np.exp(-(k * u) ** 0.7)
    blocks = []
    for p in np.exp(np.linspace(np.log(0.016), np.log(1000.0), nlev)):
        for t in 180.0 + 40.0 * np.arange(ntemp):
            blk = np.empty((len(u), 4))
            blk[:, 0], blk[:, 1], blk[:, 2], blk[:, 3] = p, t, u, eps
            blocks.append(blk)
    return np.vstack(blocks)


@pytest.mark.parametrize("which", ["limb", "nadir"])
def test_prefix_bookkeeping_on_one_curve_tables(oracle, which):
    case = common.limb_case() if which == "limb" else common.nadir_case()
    ctl2 = M.ega_ctl(case.ctl)
    geom = case.geom[::6] if which == "limb" else case.geom[:12]
    rising = total = 0
    for ig in range(case.ctl.ng):
        # (per gas a strength that takes the path from transparent well into the curve)
        rows = one_curve_rows(k=[3e-22, 2e-21, 1e-18, 1e-15, 1e-15][ig])
        pair = M.Pair(rows)
        cu, ce = pair.u[0][0], pair.eps[0][0]
        inside = 0
        for g in geom:
            tr = oracle.traceray(ctl2, case.atm, g)
            assert tr["np"] > 1
            got = M.path_tau(pair, tr["p"].tolist(), tr["t"].tolist(), tr["u"][ig].tolist())
            w, want = 0.0, []
            for ui in tr["u"][ig].tolist():
                w = w + ui
                i = M.locate_tbl_id(cu, len(cu), w)
                want.append(1.0 - M.c01(M.lip(cu[i], ce[i], cu[i + 1], ce[i + 1], w)))
            assert same_doubles(got, want), (which, ig, g)
            assert max(got) <= 1.0 and min(got) >= 0.0
            inside += int(np.sum((np.array(got) > 0) & (np.array(got) < 0.999)))
            rising += int(np.sum(np.diff(got) > 0)); total += len(got)
        assert inside > 20, (which, ig, inside)      # the gas's paths reach well into the curve
    assert rising == 0, (rising, total)          # one curve, a growing column: nothing can rise here


def test_w_zero_leaves_the_path_transmittance_alone():
    pair = M.Pair(one_curve_rows(1e-18))
    p, t = [100.0, 90.0, 80.0, 70.0], [250.0, 240.0, 230.0, 220.0]
    assert M.path_tau(pair, p, t, [0.0, 0.0, 0.0, 0.0]) == [1.0] * 4
    got = M.path_tau(pair, p, t, [0.0, 0.0, 1e18, 0.0])
    assert got[:2] == [1.0, 1.0] and 0 < got[2] < 1 and got[3] == got[2]
    cgp, cgt, cgu = M.means(p, t, [0.0, 2e18, 0.0, 2e18])
    assert np.isnan(cgp[0]) and np.isnan(cgt[0]) and cgu[0] == 0.0
    assert cgp[1:] == [90.0, 90.0, 80.0] and cgt[1:] == [240.0, 240.0, 230.0]


def compiled_resources(tmp_path):
    """name -> (VGPRs, scratch bytes) from the metadata of the kernels compiled as tests/test_contrib_cpu.py compiles
    them (test_contrib_kernel_register_budget)."""
    csrc = os.path.join(ROOT, "jurassic-gpu_amd", "csrc")
    asm = tmp_path / "k.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-ffp-contract=off", "-std=c++17",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-DJUR_ND=100", "-DJUR_NG=30", "-S",
                           "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "jur_kernels.hip")],
                          stderr=subprocess.DEVNULL)
    text = asm.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    seen = {}
    for block in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        seen[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)),
                      int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)))
    return seen


def test_cga_kernel_resources_and_untouched_kernels(tmp_path):
    """Every jur_cga_kernel instance: no scratch, VGPRs not above the jur_ega_kernel instance with the same template
    switches from the same compile (the CGA look-up is a subset of the EGA one plus three running sums).  Every kernel
    that existed before: VGPRs and scratch of the parent commit's source compiled the same way, recorded in
    tests/golden/kernel_resources_parent.json with the commit they came from."""
    seen = compiled_resources(tmp_path)
    cga = sorted(n for n in seen if "14jur_cga_kernel" in n)
    assert len(cga) == 5, cga
    for name in cga:
        vgprs, scratch = seen[name]
        ega_vgprs, _ = seen[name.replace("14jur_cga_kernel", "14jur_ega_kernel")]
        print("%s: %d VGPRs, scratch %d (jur_ega_kernel: %d)" % (name, vgprs, scratch, ega_vgprs))
        assert scratch == 0 and vgprs <= ega_vgprs, (name, vgprs, scratch, ega_vgprs)
    for name in (n for n in seen if "jur_kat_cga_kernel" in n):
        assert seen[name][1] == 0, (name, seen[name])
    parent = json.load(open(os.path.join(common.GOLD, "kernel_resources_parent.json")))
    assert len(parent["kernels"]) >= 60
    for name, (vgprs, scratch) in parent["kernels"].items():
        assert name in seen, (name, "gone")
        assert seen[name] == (vgprs, scratch), (name, seen[name], (vgprs, scratch), parent["commit"])


def test_cga_hook_is_exported_and_bound():
    L = lib.lib()
    assert hasattr(L, "jur_kat_cga_eps") and len(L.jur_kat_cga_eps.argtypes) == 11
    assert hasattr(lib.Model, "kat_cga_eps")
