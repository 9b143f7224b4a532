"""CPU: lib/dg_compose.hsaco, the stand-alone gfx950 code object of the delta
composition, exists and holds exactly the kernels dg_compose_plan_run launches
(csrc/dg_compose_host.cpp looks them up by these names).  Only the symbol table
is read, as in test_update_kernel_set_cpu.py: every kernel has one kernel
descriptor symbol, `<name>.kd`.
"""
from __future__ import annotations

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HSACO = os.path.join(ROOT, "delta-compression_amd", "lib", "dg_compose.hsaco")
HOST = os.path.join(ROOT, "delta-compression_amd", "csrc", "dg_compose_host.cpp")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

EXPECTED = {"dg_compose_map_kernel", "dg_compose_emit_kernel"}


def test_code_object_is_built():
    assert os.path.exists(HSACO), "lib/dg_compose.hsaco is missing: the Makefile's `all` builds it"


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump missing")
def test_code_object_holds_exactly_the_launched_kernels():
    r = subprocess.run([OBJDUMP, "-t", HSACO], check=True, capture_output=True, text=True)
    got = {line.split()[-1][:-3] for line in r.stdout.splitlines() if line.split() and line.split()[-1].endswith(".kd")}
    assert got == EXPECTED, {"unexpected": sorted(got - EXPECTED), "missing": sorted(EXPECTED - got)}


def test_host_code_looks_up_the_same_names():
    names = set(re.findall(r'hipModuleGetFunction\([^,]+,[^,]+,\s*"([a-z_]+)"\)', open(HOST).read()))
    assert names == EXPECTED
