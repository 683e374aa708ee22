"""CPU: the tracer kernels (cfd_tracers.hip) select their buffer with a
device-side word; that must stay a register select, not an array in scratch.
Read from the gfx950 code object by tools/kernel_resources.py."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cfd-demo_amd", "lib", "libcfd_amd.so")
TOOL = os.path.join(ROOT, "tools", "kernel_resources.py")
KERNELS = ("k_trc_advect", "k_trc_scatter", "k_trc_inject", "k_trc_density")


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_tracer_kernels_use_no_scratch():
    out = subprocess.run([sys.executable, TOOL, LIB], capture_output=True, text=True, check=True).stdout
    hits = {}
    for line in out.splitlines():
        m = re.match(r"vgpr\s+(\d+).*?scratch\s+(\d+)\s+code\s+(\d+)\s+(.*)$", line)
        if not m:
            continue
        for k in KERNELS:
            if re.search(rf"\b{k}\b", m.group(4)):
                hits[k] = (int(m.group(1)), int(m.group(2)))
    assert sorted(hits) == sorted(KERNELS), hits
    for name, (vg, scratch) in hits.items():
        print(f"{name}: vgpr {vg} scratch {scratch}")
        assert scratch == 0, f"{name}: {scratch} B of scratch"
