"""CPU: the script substep's kernels (cfd_script_step.hip) hold their u / v
windows in registers; every instantiation must stay out of scratch.  Read
from the gfx950 code object by tools/kernel_resources.py."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cfd-demo_amd", "lib", "libcfd_amd.so")
TOOL = os.path.join(ROOT, "tools", "kernel_resources.py")
# scheme x division form x rows per segment, and the corrector's two division forms
WANT = {f"k_script_predict<{s}, {f}, {r}>" for s in (0, 1, 2) for f in (0, 1) for r in (4, 8)} | \
       {"k_script_correct<0>", "k_script_correct<1>"}


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_script_step_kernels_use_no_scratch():
    out = subprocess.run([sys.executable, TOOL, LIB], capture_output=True, text=True, check=True).stdout
    hits = {}
    for line in out.splitlines():
        m = re.match(r"vgpr\s+(\d+).*?scratch\s+(\d+)\s+code\s+(\d+)\s+(.*)$", line)
        if not m:
            continue
        k = re.search(r"k_script_(?:predict|correct)<[\d, ]+>", m.group(4))
        if k:
            hits[k.group(0)] = (int(m.group(1)), int(m.group(2)))
    assert set(hits) == WANT, sorted(hits)
    for name, (vg, scratch) in sorted(hits.items()):
        print(f"{name}: vgpr {vg} scratch {scratch}")
        assert scratch == 0, f"{name}: {scratch} B of scratch"
