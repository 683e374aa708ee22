"""CPU: the two kernels of the uv-fused step -- k_predict_march<.., true> (rhs
only) and k_finish_march (the corrector finish on the march, which
holds the p' / p rows and the step maxima beside the u / v rings) -- use no
scratch in any instantiation; the first-order finish and the rhs-only march
keep three waves per SIMD, the second-order finish stays within 176 VGPRs.
Read from the gfx950 code object by tools/kernel_resources.py."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cfd-demo_amd", "lib", "libcfd_amd.so")
TOOL = os.path.join(ROOT, "tools", "kernel_resources.py")


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_uv_fused_kernels_use_no_scratch():
    out = subprocess.run([sys.executable, TOOL, LIB, "k_predict_march|k_finish_march"],
                         capture_output=True, text=True, check=True).stdout
    seen = {"k_predict_march": 0, "k_finish_march": 0}
    for line in out.splitlines():
        m = re.match(r"vgpr\s+(\d+).*?scratch\s+(\d+)\s+code\s+(\d+)\s+.*"
                     r"(k_predict_march|k_finish_march)<(\d), \d, \w+, \d+(, true)?>", line)
        if not m or (m.group(4) == "k_predict_march" and not m.group(6)):
            continue
        vg, scratch, name, scheme = int(m.group(1)), int(m.group(2)), m.group(4), int(m.group(5))
        seen[name] += 1
        print(line)
        assert scratch == 0, line
        # 3 waves per SIMD at <= 168 VGPRs; the second-order finish is built for
        # two and takes 169-176 today (profiles/r11/kernel_resources_new.txt): 176 pins that
        assert vg <= (176 if name == "k_finish_march" and scheme == 1 else 168), line
    # scheme x spacing form x mask x segment rows (the second-order finish: 4 rows only)
    assert seen == {"k_predict_march": 16, "k_finish_march": 12}, seen
