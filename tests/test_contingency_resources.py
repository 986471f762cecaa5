"""The LDS path of the contingency table (ldsCountKernel, csrc/em2_contingency.hip) is a loop of loads and LDS atomics around
a 64 KiB table: scratch memory or spilled registers in it would put memory traffic where the kernel has none to spare.  The
compiler's own resource usage remarks of a cross-compile for gfx950 (no GPU needed) say whether it has any; the assembly is
not searched."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "expressionmatrix2_amd", "csrc")


def test_the_lds_kernel_has_no_scratch_and_no_spills(tmp_path):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "unit.o"), os.path.join(CSRC, "em2_contingency.hip")]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-3000:]
    # remark: Function Name: <mangled>, then one remark per figure until the next function
    usage = {}
    name = None
    for line in done.stderr.split("\n"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            usage[name][m.group(1).strip()] = int(m.group(2))
    kernels = {n: u for n, u in usage.items() if "ldsCountKernel" in n}
    assert len(kernels) == 2, sorted(usage)                    # the 16-byte and the 4-byte loads
    for n, u in kernels.items():
        assert u["ScratchSize"] == 0 and u["SGPRs Spill"] == 0 and u["VGPRs Spill"] == 0, (n, u)
        assert u["VGPRs"] <= 64, (n, u)                         # eight waves per SIMD stay possible: the LDS decides the occupancy
