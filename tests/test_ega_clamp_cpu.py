"""The strict-table look-up clamps its seven results to [0, 1] with the VOP3 `clamp` output modifier of the instruction
that produces them (fma_c01 / add_c01 in jur_kernels.hip), not with a v_min_f64 / v_max_f64 pair behind it.  Read off
the ISA of jur_ega_kernel<true, true, true>, cross-compiled as tests/test_abi_cpu.py does for the register budgets:

  instructions carrying `clamp`     >= 4   (static: the level loop is rolled, so 2 curve clamps + 1 temperature blend
                                            in its body, and the pressure blend behind it; 7 per look-up when run)
  v_min_f64 / v_max_f64 left        <= 3   (the temperature-bracket test's, none of them a clamp of a result)

With the compiler these were read from: 4 and 3, 61 VGPRs, no scratch (11 v_min_f64 / v_max_f64 and no `clamp`
before the change)."""
import os
import re
import subprocess
import common


def test_strict_lookup_clamps_are_output_modifiers(tmp_path):
    csrc = os.path.join(common.ROOT, "jurassic-gpu_amd", "csrc")
    asm = tmp_path / "k.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-ffp-contract=off", "-std=c++17",
                           "-I" + os.path.join(common.ROOT, "include"), "-I" + csrc, "-DJUR_ND=100", "-DJUR_NG=30", "-S",
                           "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "jur_kernels.hip")],
                          stderr=subprocess.DEVNULL)
    text = asm.read_text()
    names = [n for n in re.findall(r"^(\S*jur_ega_kernelILb1ELb1ELb1EE\S*):", text, re.M) if "kat" not in n]
    assert len(names) == 1, names
    start = text.index("\n" + names[0] + ":")
    body = text[start:text.index("s_endpgm", start)]
    clamped = re.findall(r"^\s*v_\w+\s.*\bclamp\b", body, re.M)
    minmax = re.findall(r"^\s*v_(?:min|max)_f64\b", body, re.M)
    print("jur_ega_kernel<true,true,true>: %d instructions with clamp, %d v_min_f64 / v_max_f64" % (len(clamped), len(minmax)))
    assert len(clamped) >= 4, clamped
    assert all(re.match(r"\s*v_(fma|add)_f64\b", c) for c in clamped), clamped
    assert len(minmax) <= 3, len(minmax)
