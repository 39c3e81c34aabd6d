"""bench.py on the CPU: which counter summaries its roofline block accepts, and that what it prints is a fraction
of a stated peak, recomputable from the same inputs; what a plain run measures and what --dump-outputs writes."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest
import bench

KMS = dict(trace_ms=44.0, ega_ms=281.0, combine_ms=91.0, trace_launches=5, ega_launches=5, combine_launches=5)
SHAPE = (5, 4, 1, 20, 5)          # ng, nd, nw, pairs with a table, gases with a table
AB = dict(ega=3.03e6 * 4096, total=3.2e6 * 4096, rays=4096)
SUM_NP = 253e6                     # LOS points of the 1e6-ray batch


def _summary(path, sha):
    doc = {"kernel_source_sha256": sha, "workloads": {"limb_1e6": {"rays_per_launch": 1e6, "kernels": {
        "trace": {"SQ_INSTS_VALU": 2.38e9, "FETCH_SIZE": 5.0e5, "WRITE_SIZE": 2.0e7},
        "ega": {"SQ_INSTS_VALU": 2.649e10, "FETCH_SIZE": 4.12e7, "WRITE_SIZE": 3.95e7},
        "combine": {"SQ_INSTS_VALU": 5.49e9, "FETCH_SIZE": 4.2e7, "WRITE_SIZE": 3.4e5}}}}}
    path.write_text(json.dumps(doc))


def test_counters_of_other_kernel_sources_are_refused(tmp_path, monkeypatch):
    f = tmp_path / "pmc.json"
    monkeypatch.setattr(bench, "PMC_SUMMARY", str(f))
    assert bench.load_pmc("limb_1e6") == (None, "no profiles/pmc_current.json")
    _summary(f, "0" * 64)
    pmc, why = bench.load_pmc("limb_1e6")
    assert pmc is None and "sha mismatch" in why
    r = bench.roofline_block("limb_1e6", KMS, 1_000_000, 5, SUM_NP, SHAPE, AB)
    assert r["bound"] == "hbm" and r["pmc_source"] is None and r["traffic"] is None and "sha mismatch" in r["pmc_missing"]
    assert 0 < r["frac"] < 1 and r["frac"] == r["hbm_compulsory_frac"]      # the fraction a run can measure by itself
    _summary(f, bench.kernel_source_sha())
    pmc, why = bench.load_pmc("limb_1e6")
    assert why is None and pmc["rays_per_launch"] == 1e6
    assert bench.load_pmc("nadir_1e5")[0] is None                            # no pass for that workload in this file


def test_roofline_fraction_is_recomputable_and_below_one(tmp_path, monkeypatch):
    f = tmp_path / "pmc.json"
    monkeypatch.setattr(bench, "PMC_SUMMARY", str(f))
    _summary(f, bench.kernel_source_sha())
    r = bench.roofline_block("limb_1e6", KMS, 1_000_000, 5, SUM_NP, SHAPE, AB)
    assert r["bound"] == "valu_fp64_issue" and r["kernel"] == "jur_ega_kernel" and r["unit"].startswith("G wavefront")
    avg_s = 281.0 / 5 * 1e-3
    assert r["frac"] == pytest.approx(2.649e10 / avg_s / (256 * 4 * 2.4e9 / 4))
    assert r["achieved"] == pytest.approx(r["frac"] * r["peak"]) and r["peak"] == pytest.approx(614.4)
    assert r["traffic"] == pytest.approx((2 * 4.12e7 + 3.95e7) * 1024)        # gfx950: FETCH_SIZE counts half
    assert r["hbm_frac"] == pytest.approx(r["traffic"] / avg_s / 8e12)
    for k in ("trace", "ega", "combine"):
        e = r["kernels"][k]
        assert 0 < e["valu_issue_frac"] < 1 and 0 < e["hbm_frac"] < 1 and 0 < e["hbm_compulsory_frac"] < 1
    assert r["algorithmic_frac"] > 1                                          # kept, labelled: not a fraction of peak
    # half the rays per launch: half the instructions, same fraction at half the time
    kms = dict(KMS, ega_ms=281.0, ega_launches=10)
    r2 = bench.roofline_block("limb_1e7_sharded", kms, 1_000_000, 5, SUM_NP, SHAPE, AB)
    assert r2["bound"] == "valu_fp64_issue" and r2["frac"] == pytest.approx(r["frac"])


def _run_bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    return subprocess.run([sys.executable, bench.__file__, *argv], capture_output=True, text=True,
                          env=dict(env, OMP_NUM_THREADS="2"), timeout=600)


def test_plain_run_times_its_steps_and_dumps_what_the_last_one_computed(tmp_path):
    """A plain run prints the headline and nothing --full adds; --dump-outputs writes the last timed step's radiances,
    the same for the same arguments (--dry-run: the forward model replaced by a function of each ray's geometry)."""
    for d in ("a", "b"):
        out = _run_bench("--dry-run", "--rays", "3000", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / d))
        assert out.returncode == 0, out.stdout + out.stderr
        doc = json.loads(out.stdout)
        assert doc["steps"] == 3 and doc["warmup"] == 1 and doc["full"] is False
        assert doc["value"] == pytest.approx(3000 * 1e3 / doc["ms_per_step"])
        assert not {"rerun_mismatches", "gather_check", "cpu_baseline", "roofline", "extra"} & set(doc)
    a, b = (np.load(tmp_path / d / "rad.npy") for d in ("a", "b"))
    assert a.dtype == np.float64 and a.shape == (3000, 4) and np.array_equal(a, b)
    g = bench.workload_rays("limb_1e6", np.arange(3000))
    assert np.allclose(a, np.stack([(g * (d + 1.0)).sum(axis=1) for d in range(4)], axis=1), rtol=1e-14, atol=0)
    assert _run_bench("--dry-run", "--steps", "0").returncode != 0


def test_dump_outputs_samples_the_same_rows_of_every_array_within_the_budget(tmp_path, monkeypatch):
    import torch
    assert bench.DUMP_BYTES + 4 * 128 <= 64e6           # data and one .npy header per array of a single-GPU run
    n = 10_000
    rad = torch.arange(4 * n, dtype=torch.float64).reshape(n, 4)
    rows = torch.arange(n, dtype=torch.int32)
    monkeypatch.setattr(bench, "DUMP_BYTES", 8 * 5 * 1000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"rad": rad, "np": rows})
    r, i = np.load(tmp_path / "a" / "rad.npy"), np.load(tmp_path / "a" / "np.npy")
    assert r.shape == (1000, 4) and i.shape == (1000,) and r.dtype == i.dtype == np.float64
    assert np.all(np.diff(i) > 0) and np.array_equal(r, rad.numpy()[i.astype(int)])
    assert all(np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)) for f in ("rad.npy", "np.npy"))
    bench.dump_outputs(str(tmp_path / "c"), {"rad": rad[:900]})                  # fits: every row, in order
    assert np.array_equal(np.load(tmp_path / "c" / "rad.npy"), rad[:900].numpy())
