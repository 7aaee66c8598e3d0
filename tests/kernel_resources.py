"""What the test_*_resources_cpu.py modules share: the compiler's resource report of a csrc file for gfx950 with the Makefile's own CXXFLAGS
(the build that ships), as {mangled kernel name: {key: value}}.  A module makes its fixture with  resources = fixture("file.hip")  and keeps
its instance lists and assertions."""
import os
import re
import shlex
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mesh-reconstruction_amd")
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


def makefile_flags():
    """CXXFLAGS as mesh-reconstruction_amd/Makefile sets them"""
    text = open(os.path.join(PKG, "Makefile")).read()
    m = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", text, re.M)
    assert m, "no CXXFLAGS line in the Makefile"
    return shlex.split(m.group(1).replace("$(ARCH)", "gfx950"))


def report(tmp, source):
    """-Rpass-analysis=kernel-resource-usage of csrc/<source>, device code only; the object file goes to the directory `tmp`"""
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert hipcc, "hipcc is needed to build the library"
    r = subprocess.run([hipcc] + makefile_flags() + ["--cuda-device-only", "-c", os.path.join("csrc", source), "-o", str(tmp / (source + ".o")),
                                                     "-Rpass-analysis=kernel-resource-usage"], cwd=PKG, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        if "remark:" not in line or "[-Rpass-analysis" not in line:
            continue
        key, _, val = line.split("remark:", 1)[1].rsplit("[-Rpass-analysis", 1)[0].strip().rpartition(":")
        if key.strip() == "Function Name":
            cur = kernels.setdefault(val.strip(), {})
        elif cur is not None:
            cur[key.strip()] = val.strip()
    return kernels


def fixture(*sources):
    """the module-scoped fixture of a test module: the kernels of the listed csrc files, each compiled once per module"""
    @pytest.fixture(scope="module")
    def resources(tmp_path_factory):
        tmp = tmp_path_factory.mktemp("resources")
        kernels = {}
        for source in sources:
            kernels.update(report(tmp, source))
        return kernels
    return resources
