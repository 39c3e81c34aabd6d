"""The radiance pin that is one file-drop away, and the pins of the packed data blobs.

(1) example/{limb,nadir}/rad.org columns 11+ (radiance, transmittance) were produced by the reference with
    emissivity tables that are NOT in the reference tree (.MISSING_LARGE_BLOBS lines 1-11), so no radiance of
    this repository is pinned to THOSE numbers yet (tests/test_reference_cpu.py and test_reference_gpu.py pin oracle
    and HIP path to the reference's own CPU program on synthetic tables).  Point JUR_REF_TABLES at a directory that holds

        boxcar_792.0000_{CO2,H2O,O3,CCl4}.tab  boxcar_832.0000_{CO2,H2O,O3,F11}.tab     (limb)
        airs_{667.7820,668.5410,669.8110}_CO2.tab                                       (nadir)

    and these tests run the example exactly as example/*/run.sh does (`formod <ctl> obs.tab atm.tab rad.tab`,
    run.sh:17, checked by `diff rad.tab rad.org`, :70-72): the oracle on the CPU, the HIP path through the
    drop-in formod() on the GPU, each compared with rad.org column by column -- equal as %g text, or within
    1e-6 relative (north_star's bar) of the six digits rad.org holds where the last digit flips.  Without the directory they skip and say why.

(2) jurassic-gpu_amd/data/ctm.bin (continuum coefficients, reference src/ctm*.tbl, read at jr_common.h:317,
    335, 366, 380) and clim.bin (src/climatology.tbl) are numeric data packed once by tools/extract_*.py: their
    sha256 is pinned here, and they are re-derived from the numbers of those files (tests/golden/reference_data)
    and compared byte for byte.
"""
import ctypes as C
import hashlib
import os
import shutil
import struct
import subprocess
import sys
import numpy as np
import pytest
import common
from jurassic_hip import abi, textio

REF_TABLES = os.environ.get("JUR_REF_TABLES", "")
EXAMPLES = {
    "limb": dict(base="boxcar", emitters=common.LIMB_EMITTERS, nu=common.LIMB_NU, ctl={},
                 need=["boxcar_792.0000_CO2.tab", "boxcar_792.0000_H2O.tab", "boxcar_792.0000_O3.tab", "boxcar_792.0000_CCl4.tab",
                       "boxcar_832.0000_CO2.tab", "boxcar_832.0000_H2O.tab", "boxcar_832.0000_O3.tab", "boxcar_832.0000_F11.tab"]),
    "nadir": dict(base="airs", emitters=common.NADIR_EMITTERS, nu=common.NADIR_NU, ctl=dict(write_bbt=1),
                  need=["airs_667.7820_CO2.tab", "airs_668.5410_CO2.tab", "airs_669.8110_CO2.tab"]),
}
CTM_SHA256 = "26c77666d1f1f819e29ea15f4235a75549b495ae9af89ddf249c461d115721ad"
CLIM_SHA256 = "6bf43a30fcfe4bcd56ed67bf7136b397fc0d456f5f87d365d4f29fa1c5b70f2c"


def _need_tables(example):
    if not REF_TABLES:
        pytest.skip("JUR_REF_TABLES is not set: the emissivity tables behind example/%s/rad.org columns 11+ are missing "
                    "blobs of the reference tree (.MISSING_LARGE_BLOBS), so there is no reference-produced radiance to "
                    "compare with -- radiances stay pinned to the reference's CPU program on synthetic tables only "
                    "(tests/test_reference_cpu.py)" % example)
    missing = [f for f in EXAMPLES[example]["need"] if not os.path.exists(os.path.join(REF_TABLES, f))]
    if missing:
        pytest.skip("JUR_REF_TABLES=%s lacks %s" % (REF_TABLES, ", ".join(missing)))


def _stage(example, tmp_path):
    """A directory laid out like example/<name>/: the user's tables, the shipped filters, atm.tab, obs.tab."""
    ex = EXAMPLES[example]
    for f in os.listdir(REF_TABLES):
        if f.startswith(ex["base"] + "_") and f.endswith(".tab"):
            os.symlink(os.path.abspath(os.path.join(REF_TABLES, f)), tmp_path / f)
    gold = os.path.join(common.GOLD, example)
    for f in os.listdir(gold):
        if f.endswith(".filt") or f in ("atm.tab", "obs.tab", "rad.org"):
            shutil.copy(os.path.join(gold, f), tmp_path / f)
    ctl = abi.make_ctl(ex["emitters"], ex["nu"], **ex["ctl"])
    ctl.tblbase = os.path.join(str(tmp_path), ex["base"]).encode()
    ctl.read_binary, ctl.write_binary = 0, 0
    nd = len(ex["nu"])
    gold_rows = textio.read_obs_array(os.path.join(gold, "rad.org"), nd)
    atm = textio.read_atm(os.path.join(gold, "atm.tab"), ctl)
    return ctl, atm, gold_rows, nd


def _assert_matches_rad_org(rad, tau, gold_rows, nd, what):
    """Columns 11.. of rad.org: nd radiances then nd transmittances per ray, printed with %g."""
    want = np.concatenate([gold_rows[:, 10:10 + nd], gold_rows[:, 10 + nd:10 + 2 * nd]], axis=1)
    got = np.concatenate([rad, tau], axis=1)
    worst = 0.0
    for i in range(len(want)):
        for j in range(2 * nd):
            if "%g" % got[i, j] == "%g" % want[i, j]:
                continue
            # rad.org holds 6 significant digits, i.e. the reference's value to within 5e-6 relative (half a unit of
            # the sixth digit); on top of that north_star's 1e-6
            err = abs(got[i, j] - want[i, j]) / max(abs(want[i, j]), 1e-300)
            worst = max(worst, err)
            assert err < 6e-6, (what, "ray", i, "column", 11 + j, got[i, j], want[i, j])
    return worst


@pytest.mark.parametrize("example", ["limb", "nadir"])
def test_oracle_reproduces_rad_org_radiances(example, oracle, tmp_path):
    _need_tables(example)
    ctl, atm, gold_rows, nd = _stage(example, tmp_path)
    tb = oracle.Tables(ctl.ng, ctl.nd)
    tb.read_ascii(ctl)
    tb.planck_filt(ctl)
    res = oracle.formod_rays(ctl, atm, tb, gold_rows[:, :7])
    _assert_matches_rad_org(res["rad"], res["tau"], gold_rows, nd, "oracle, example/" + example)


@pytest.mark.gpu
@pytest.mark.parametrize("example", ["limb", "nadir"])
def test_hip_formod_reproduces_rad_org_radiances(example, tmp_path):
    """The drop-in formod() reading the reference's own files, in a fresh process (tables are latched per process)."""
    _need_tables(example)
    ctl, atm, gold_rows, nd = _stage(example, tmp_path)
    script = tmp_path / "run.py"
    script.write_text("""
import sys, numpy as np
sys.path[:0] = [%r, %r, %r]
import os
os.chdir(%r)
import common
from jurassic_hip import abi, lib, textio
ex = %r
ctl = abi.make_ctl(ex['emitters'], ex['nu'], **ex['ctl'])
ctl.tblbase = ('./' + ex['base']).encode()
ctl.read_binary, ctl.write_binary = 0, 0
atm = textio.read_atm('atm.tab', ctl)
obs = textio.read_obs('rad.org', ctl)
lib.formod(ctl, atm, obs)
n, nd = obs.nr, ctl.nd
np.save('rad.npy', np.ctypeslib.as_array(obs.rad)[:n, :nd])
np.save('tau.npy', np.ctypeslib.as_array(obs.tau)[:n, :nd])
""" % (common.ROOT, os.path.join(common.ROOT, "jurassic-gpu_amd"), os.path.join(common.ROOT, "tests"), str(tmp_path),
       dict(emitters=EXAMPLES[example]["emitters"], nu=EXAMPLES[example]["nu"], ctl=EXAMPLES[example]["ctl"],
            base=EXAMPLES[example]["base"])))
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    rad, tau = np.load(tmp_path / "rad.npy"), np.load(tmp_path / "tau.npy")
    _assert_matches_rad_org(rad, tau, gold_rows, nd, "HIP formod(), example/" + example)


def test_the_skip_reason_names_the_missing_blobs():
    """Without the tables the two tests above must skip (not pass, not fail) and say what is missing."""
    if REF_TABLES:
        pytest.skip("JUR_REF_TABLES is set")
    with pytest.raises(pytest.skip.Exception) as e:
        _need_tables("limb")
    assert "MISSING_LARGE_BLOBS" in str(e.value) and "rad.org" in str(e.value)


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def test_packed_data_blobs_are_the_pinned_ones():
    data = os.path.join(common.ROOT, "jurassic-gpu_amd", "data")
    assert _sha(os.path.join(data, "ctm.bin")) == CTM_SHA256
    assert _sha(os.path.join(data, "clim.bin")) == CLIM_SHA256
    assert os.path.getsize(os.path.join(data, "ctm.bin")) == 8 * (6 * 2001 + 2 * 98 + 2 * 90)
    assert os.path.getsize(os.path.join(data, "clim.bin")) == 30 * (8 + 8 * 121)


def _reference_arrays(stem):
    """{name: values} of tests/golden/reference_data/<stem>.txt: the numbers of the reference's src/<stem>.tbl as
    written there, each array as a line `[name] count` and then its values."""
    arrays, counts = {}, {}
    for line in open(os.path.join(common.GOLD, "reference_data", stem + ".txt")):
        if line.startswith("#"):
            continue
        if line.startswith("["):
            name, n = line[1:].split("]")
            arrays[name], counts[name] = [], int(n)
        else:
            arrays[name] += [float(v) for v in line.split()]
    assert {k: len(v) for k, v in arrays.items()} == counts, stem
    return arrays


def test_packed_data_blobs_rederive_from_the_reference_tree():
    """Pack the numbers of the reference's ctm*.tbl / climatology.tbl (tests/golden/reference_data) again, in the
    order tools/extract_ctm.py and tools/extract_clim.py write them, and compare with the blobs byte for byte."""
    data = os.path.join(common.ROOT, "jurassic-gpu_amd", "data")
    co2, h2o, n2, o2 = (_reference_arrays(f) for f in ("ctmco2", "ctmh2o", "ctmn2", "ctmo2"))
    seq = [co2["co2296"], co2["co2260"], co2["co2230"], h2o["h2o296"], h2o["h2o260"], h2o["h2ofrn"],
           n2["ba"], n2["betaa"], o2["ba"], o2["betaa"]]
    assert [len(v) for v in seq] == [2001] * 6 + [98, 98, 90, 90]
    ctm_blob = b"".join(struct.pack("<%dd" % len(v), *v) for v in seq)
    assert ctm_blob == open(os.path.join(data, "ctm.bin"), "rb").read(), "ctm.bin"
    clim = _reference_arrays("climatology")
    assert list(clim)[:3] == ["z", "pre", "tem"] and all(len(v) == 121 for v in clim.values())
    clim_blob = b"".join(k.lower().encode().ljust(8, b"\0") + struct.pack("<121d", *v) for k, v in clim.items())
    assert clim_blob == open(os.path.join(data, "clim.bin"), "rb").read(), "clim.bin"
    # spot values against the text of the reference's initialisers (first CO2 296 K coefficient, last O2 beta)
    ctm = np.fromfile(os.path.join(data, "ctm.bin"), dtype="<f8")
    assert ctm[0] == 9.3388e-5 and ctm[-1] == 504.0
