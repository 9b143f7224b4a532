"""CPU: the stand-alone gfx950 code object of the lineage reads
(lib/dg_lineage.hsaco) exists and holds exactly the kernels the host code
launches: csrc/dg_lineage_host.cpp names them once, in its k..Kernels[] table,
which load_kernels (dg_hostutil.h) looks up.  Only the symbol table is read, as
in test_read_kernel_set_cpu.py: every kernel has one kernel descriptor symbol,
`<name>.kd`.
"""
from __future__ import annotations

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "delta-compression_amd")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
HSACO = os.path.join(PKG, "lib", "dg_lineage.hsaco")

EXPECTED = {"dg_lineage_read_kernel"}


def test_code_object_is_built():
    assert os.path.exists(HSACO), "lib/dg_lineage.hsaco is missing: the Makefile's `all` builds it"


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump missing")
def test_code_object_holds_exactly_the_launched_kernels():
    r = subprocess.run([OBJDUMP, "-t", HSACO], check=True, capture_output=True, text=True)
    got = {line.split()[-1][:-3] for line in r.stdout.splitlines() if line.split() and line.split()[-1].endswith(".kd")}
    assert got == EXPECTED, {"unexpected": sorted(got - EXPECTED), "missing": sorted(EXPECTED - got)}


def test_host_code_looks_up_the_same_names():
    src = open(os.path.join(PKG, "csrc", "dg_lineage_host.cpp")).read()
    tables = re.findall(r"static const char\* const k\w+Kernels\[\] = \{([^}]*)\};", src)
    assert len(tables) == 1, "one kernel-name table per host file"
    names = re.findall(r'"([a-z_0-9]+)"', tables[0])
    assert len(names) == len(set(names))
    assert set(names) == EXPECTED
    # the table is what is looked up: the loader is called with it, and nothing else asks the module for a function
    assert re.search(r"load_kernels\([^;]*\bk\w+Kernels\b", src)
    assert "hipModuleGetFunction" not in src
    assert '"dg_lineage.hsaco"' in src


def test_exported_capacity_makes_progress(dg):
    assert dg.lineage_work_items() >= dg.LINEAGE_MAX_DEPTH == 64
    assert dg.LINEAGE_BASE == 0xFFFFFFFF
