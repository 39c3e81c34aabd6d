"""CPU side of the contributions (formod TASK contrib): the obs2spec converter's text, the contribution kernel's
register budget, the exported entry points and the CLI's task switch (in CHECKMODE, no GPU)."""
import os
import re
import subprocess
import numpy as np
import common
from jurassic_hip import lib, textio

ROOT = common.ROOT
PKG = os.path.join(ROOT, "jurassic-gpu_amd")
LIMB_CTL = "TBLBASE = ./boxcar\nNG = 5\nEMITTER[0] = CO2\nEMITTER[1] = H2O\nEMITTER[2] = O3\nEMITTER[3] = F11\n" \
           "EMITTER[4] = CCl4\nND = 2\nNU[0] = 792.0000\nNU[1] = 832.0000\n"
SPEC_HEADER = ["# $1 = time (seconds since 2000-01-01T00:00Z)", "# $2 = observer altitude [km]",
               "# $3 = observer longitude [deg]", "# $4 = observer latitude [deg]", "# $5 = view point altitude [km]",
               "# $6 = view point longitude [deg]", "# $7 = view point latitude [deg]",
               "# $8 = tangent point altitude [km]", "# $9 = tangent point longitude [deg]",
               "# $10 = tangent point latitude [deg]", "# $11 = channel wavenumber [cm^-1]",
               "# $12 = channel radiance [W/(m^2 sr cm^-1)]"]


def _obs2spec():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "csrc")])    # (the session build lists other tools)
    exe = os.path.join(PKG, "obs2spec")
    assert os.path.exists(exe)
    return exe


def test_obs2spec_writes_the_spectrum_layout(tmp_path):
    """One line per (ray, channel): geometry, tangent point, wavenumber, radiance -- `%.2f %g x9 %.4f %g` -- after a
    blank line per ray and the twelve `$n` header lines."""
    exe = _obs2spec()
    (tmp_path / "limb.ctl").write_text(LIMB_CTL)
    src = os.path.join(common.GOLD, "limb", "rad.org")
    out = subprocess.run([exe, "limb.ctl", src, "spec.tab"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = textio.read_obs_array(src, 2)
    want = list(SPEC_HEADER)
    for r in rows:
        want.append("")
        for id_, nu in enumerate((792.0, 832.0)):
            want.append("%.2f %g %g %g %g %g %g %g %g %g %.4f %g" % (tuple(r[:10]) + (nu, r[10 + id_])))
    got = (tmp_path / "spec.tab").read_text().split("\n")
    assert got[-1] == "" and got[:-1] == want
    assert len(rows) == 66


def test_obs2spec_needs_its_arguments(tmp_path):
    exe = _obs2spec()
    (tmp_path / "limb.ctl").write_text(LIMB_CTL)
    for args in ([], ["limb.ctl"], ["limb.ctl", os.path.join(common.GOLD, "limb", "rad.org")]):
        out = subprocess.run([exe] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "Give parameters" in out.stdout
    assert not (tmp_path / "spec.tab").exists()


def test_formod_task_contrib_names_its_outputs_in_checkmode(tmp_path):
    """TASK contrib is read from the command line (or the control file) and names <rad>.<EMITTER> and <rad>.EXTINCT;
    CHECKMODE keeps the GPU out of it and writes nothing."""
    exe = os.path.join(PKG, "formod")
    (tmp_path / "limb.ctl").write_text(LIMB_CTL)
    args = [exe, "limb.ctl", os.path.join(common.GOLD, "limb", "obs.tab"), os.path.join(common.GOLD, "limb", "atm.tab"),
            "rad.tab", "CHECKMODE", "1"]
    out = subprocess.run(args + ["TASK", "contrib"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "TASK = contrib" in out.stdout and "formod_contrib: no operation in checkmode" in out.stdout
    for name in ["rad.tab"] + ["rad.tab." + e for e in common.LIMB_EMITTERS] + ["rad.tab.EXTINCT"]:
        assert "skip writing target file name for observation data: %s\n" % name in out.stdout, name
    plain = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert plain.returncode == 0 and "TASK = -" in plain.stdout and "rad.tab.CO2" not in plain.stdout
    assert not list(tmp_path.glob("rad.tab*"))


def test_contrib_kernel_register_budget(tmp_path):
    """jur_contrib_kernel, compiled as test_abi_cpu.test_kernel_register_budgets_and_cache_policy compiles the kernels:
    within 64 VGPRs (8 wavefronts per SIMD) and no scratch, like the other radiance-update kernels; the transmittance plane is read with
    non-temporal loads."""
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
    (name,) = [n for n in seen if "jur_contrib_kernel" in n]
    vgprs, scratch = seen[name]
    assert vgprs <= 64 and scratch == 0, (vgprs, scratch)
    start = text.index("\n" + name + ":")
    body = text[start:text.index("s_endpgm", start)]
    assert len(re.findall(r"^\s*global_load\S*\s.*\bnt\b", body, re.M)) >= 1


def test_contrib_symbols_are_exported():
    L = lib.lib()
    for n in ("formod_contrib", "jur_formod_contrib_host", "jur_formod_contrib_device", "jur_model_last_contrib_ms"):
        assert hasattr(L, n), n
