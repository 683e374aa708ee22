"""CPU: the default 8-sweep launches carry two complete marches (the
reference's form and the guarded fma form, one wave-uniform branch at the top)
and still do not spill; the two kernels that publish the guard's maxima stay
at scratch 0.  Read from the gfx950 code object by tools/kernel_resources.py.

Measured (tools/kernel_resources.py, VGPRs / scratch B / code B):
  before the fma form   k_jacobi_lds<8, 1, 0>  104 / 0 /  87156
                        k_jacobi_lds<8, 1, 1>  103 / 0 /  91872
  with both bodies      k_jacobi_lds<8, 1, 0>  105 / 0   (code about twice)
                        k_jacobi_lds<8, 1, 1>  105 / 0
The ceiling is the earlier figure plus the 2 VGPRs the branch was seen to
need at most; 4 waves per SIMD need <= 128 either way."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cfd-demo_amd", "lib", "libcfd_amd.so")
TOOL = os.path.join(ROOT, "tools", "kernel_resources.py")

MARCH = {r"k_jacobi_lds<8, 1, 0>$": 104 + 2, r"k_jacobi_lds<8, 1, 1>$": 103 + 2}
PUBLISHERS = (r"k_predict_march<", r"k_correct_finish4m<")


def _resources():
    out = subprocess.run([sys.executable, TOOL, LIB], capture_output=True, text=True, check=True).stdout
    rows = []
    for line in out.splitlines():
        m = re.match(r"vgpr\s+(\d+).*?scratch\s+(\d+)\s+code\s+(\d+)\s+(.*)$", line)
        if m:
            rows.append((int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4).strip()))
    return rows


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_dual_body_march_does_not_spill():
    rows = _resources()
    for pat, vmax in MARCH.items():
        hits = [r for r in rows if re.search(pat, r[3])]
        assert hits, pat
        for vg, scratch, code, name in hits:
            print(f"{name}: vgpr {vg} scratch {scratch} code {code}")
            assert scratch == 0, f"{name}: {scratch} B of scratch"
            assert vg <= vmax, f"{name}: {vg} VGPRs > {vmax}"


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_maxima_publishers_do_not_spill():
    rows = _resources()
    for pat in PUBLISHERS:
        hits = [r for r in rows if re.search(pat, r[3])]
        assert hits, pat
        for vg, scratch, code, name in hits:
            assert scratch == 0, f"{name}: {scratch} B of scratch"
