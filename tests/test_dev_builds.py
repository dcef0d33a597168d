"""The measurement builds of the fused kernels (tools/README.md: fused_probe.sh, ablate.sh, mkvariant.sh) are not part of the
default build, so nothing else notices when an edit of fdoct_kernels.hip breaks one.  Each is parsed here for gfx950 with the
Makefile's flags (device side only, no code generated): the one-instantiation tuning build on its own and with every
instrument's switch.  Nothing is run and no assembly is read."""
import os
import re
import shlex
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fdoct_amd", "csrc")


def makefile_cxxflags():
    with open(os.path.join(CSRC, "Makefile")) as f:
        m = re.search(r"^CXXFLAGS \?= (.*)$", f.read(), re.M)
    assert m, "the Makefile's CXXFLAGS line"
    return shlex.split(m.group(1))


@pytest.mark.parametrize("flag", [None, "-DFDOCT_FUSED_PROBE", "-DFDOCT_CLOCKPROBE", "-DFDOCT_RUNTIME_ABLATE", "-DFDOCT_CT_ABLATE=1"])
def test_instrument_build_compiles(flag):
    hipcc = shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-fsyntax-only", "-DFDOCT_DEV_ONE=5"] + ([flag] if flag else []) + makefile_cxxflags() + ["fdoct_kernels.hip"]
    run = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, " ".join(cmd) + "\n" + run.stderr
