"""For the tests that read device assembly: one clipa_amd/csrc source cross-compiled to gfx950 with the compiler and the
flags the library itself is built with (clipa_amd/build.py), so that an audit in the tests audits the code that ships."""
import os
import shutil
import subprocess
import sys

import pytest

from clipa_amd.build import CSRC, FLAGS, HERE, HIPCC

needs_hipcc = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")


def device_asm(src, out_dir):
    """Path of the gfx950 assembly of clipa_amd/csrc/<src>, written into out_dir."""
    asm = out_dir / (src + ".s")
    r = subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-o", str(asm), os.path.join(CSRC, src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return asm


def audited_asm(src, out_dir):
    """device_asm() that clipa_amd/isa_audit.py has passed."""
    asm = device_asm(src, out_dir)
    a = subprocess.run([sys.executable, os.path.join(HERE, "isa_audit.py"), str(asm)], capture_output=True, text=True)
    assert a.returncode == 0, a.stdout[-3000:]
    return asm
