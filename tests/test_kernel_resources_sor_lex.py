"""CPU: the script-order SOR kernel (k_sor_lex, cfd_sor_lex.hip) keeps its
chunk of old values, right-hand sides and neighbour rows in registers: no
scratch in either division form.  Read from the gfx950 code object by
tools/kernel_resources.py.

Measured (VGPRs / scratch B): k_sor_lex<1> 117 / 0, k_sor_lex<0> 123 / 0."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cfd-demo_amd", "lib", "libcfd_amd.so")
TOOL = os.path.join(ROOT, "tools", "kernel_resources.py")


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_sor_lex_kernels_do_not_spill():
    out = subprocess.run([sys.executable, TOOL, LIB], capture_output=True, text=True, check=True).stdout
    hits = []
    for line in out.splitlines():
        m = re.match(r"vgpr\s+(\d+).*?scratch\s+(\d+)\s+code\s+(\d+)\s+(.*)$", line)
        if m and re.search(r"k_sor_lex<[01]>", m.group(4)):
            hits.append((int(m.group(1)), int(m.group(2)), m.group(4).strip()))
    assert len(hits) == 2, hits
    for vg, scratch, name in hits:
        print(f"{name}: vgpr {vg} scratch {scratch}")
        assert scratch == 0, f"{name}: {scratch} B of scratch"
        assert vg <= 128, f"{name}: {vg} VGPRs (4 waves per SIMD need <= 128)"
