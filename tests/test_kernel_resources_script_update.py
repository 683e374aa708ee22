"""CPU: the kernels of the script's Jacobi solve (cfd_jacobi_script.hip) and of
the script's time step (cfd_script_update.hip) compile for gfx950 and stay out
of scratch.  Read from the gfx950 code object by tools/kernel_resources.py."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cfd-demo_amd", "lib", "libcfd_amd.so")
TOOL = os.path.join(ROOT, "tools", "kernel_resources.py")
# the solve's two division forms; the step's begin, end and pressure-maximum passes
WANT = {"k_jacobi_script<0>", "k_jacobi_script<1>", "k_script_begin", "k_script_end", "k_script_pmax"}


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_script_update_kernels_use_no_scratch():
    out = subprocess.run([sys.executable, TOOL, LIB], capture_output=True, text=True, check=True).stdout
    hits = {}
    for line in out.splitlines():
        m = re.match(r"vgpr\s+(\d+).*?scratch\s+(\d+)\s+code\s+(\d+)\s+(.*)$", line)
        if not m:
            continue
        k = re.search(r"k_jacobi_script<\d>|k_script_(?:begin|end|pmax)\b", m.group(4))
        if k:
            hits[k.group(0)] = (int(m.group(1)), int(m.group(2)))
    assert set(hits) == WANT, sorted(hits)
    for name, (vg, scratch) in sorted(hits.items()):
        print(f"{name}: vgpr {vg} scratch {scratch}")
        assert scratch == 0, f"{name}: {scratch} B of scratch"
