"""The ray tracer kernels as the compiler builds them for gfx950 (cross-compiled, no GPU): register and scratch budgets of
every tracer kernel, and how the profile rows are read.  jur_trace_slice_kernel keeps the slice of its workgroup's rays
in LDS; the point of it is that the stepping loop's gathers are ds_read instructions (counted on lgkmcnt alone) -- a
read of LDS through a generic pointer would be a flat_load, which also waits behind the LOS stores in vmcnt."""
import os
import re
import subprocess
import common


def test_tracer_kernels_budgets_and_lds_reads(tmp_path):
    csrc = os.path.join(common.ROOT, "jurassic-gpu_amd", "csrc")
    asm = tmp_path / "k.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-ffp-contract=off", "-std=c++17",
                           "-I" + os.path.join(common.ROOT, "include"), "-I" + csrc, "-DJUR_ND=100", "-DJUR_NG=30", "-S",
                           "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "jur_kernels.hip")],
                          stderr=subprocess.DEVNULL)
    text = asm.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    seen = {}
    for block in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        seen[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)),
                      int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)))
    tracers = [n for n in seen if "jur_trace_" in n]
    for key in ("jur_trace_kernel", "jur_trace_lanes_kernel", "jur_trace_slice_kernel"):
        assert len([n for n in tracers if key in n]) == 1, (key, tracers)
    assert len(tracers) == 3, tracers

    def body(name):
        start = text.index("\n" + name + ":")
        return text[start:text.index("s_endpgm", start)]
    count = lambda code, op: len(re.findall(r"^\s*%s" % op, code, re.M))
    for name in tracers:
        vgprs, scratch = seen[name]
        print(name, "VGPRs", vgprs, "scratch", scratch, "flat_load", count(body(name), "flat_load"),
              "global_load", count(body(name), "global_load"), "ds_read", count(body(name), "ds_read"))
        assert vgprs <= 128 and scratch <= 32, (name, vgprs, scratch)
        assert count(body(name), "flat_load") == 0, name
    (lds,) = [n for n in tracers if "jur_trace_slice_kernel" in n]
    (plain,) = [n for n in tracers if "jur_trace_kernel" in n]
    # the tangent-point columns are in LDS in both (13 reads); the staged path adds the profile gathers: bracket walk
    # both ways, bracket values of two probes, p / T / slope, columns and extinction -- far more than the columns alone
    assert count(body(lds), "ds_read") >= count(body(plain), "ds_read") + 30
    nt = len(re.findall(r"^\s*global_store\S*\s.*\bnt\b", body(lds), re.M))
    assert nt >= 10, nt                                   # both paths write the LOS rows past the L2
