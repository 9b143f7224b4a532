"""CPU: the stand-alone gfx950 code objects of the transform plans
(lib/dg_inplace.hsaco, lib/dg_update.hsaco, lib/dg_compose.hsaco) exist and each
holds exactly the kernels its plan launches: csrc/dg_<module>_host.cpp names
them once, in its k..Kernels[] table, which load_kernels (dg_hostutil.h) looks
up.  Only the symbol table is read, as in test_kernel_set_cpu.py: every kernel
has one kernel descriptor symbol, `<name>.kd`.
"""
from __future__ import annotations

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "delta-compression_amd")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

EXPECTED = {
    "inplace": {"dg_inplace_order_kernel", "dg_inplace_emit_kernel"},
    "update": {"dg_update_kernel"},
    "compose": {"dg_compose_map_kernel", "dg_compose_emit_kernel"},
}
MODULES = sorted(EXPECTED)


def _hsaco(module):
    return os.path.join(PKG, "lib", f"dg_{module}.hsaco")


@pytest.mark.parametrize("module", MODULES)
def test_code_object_is_built(module):
    assert os.path.exists(_hsaco(module)), f"lib/dg_{module}.hsaco is missing: the Makefile's `all` builds it"


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump missing")
@pytest.mark.parametrize("module", MODULES)
def test_code_object_holds_exactly_the_launched_kernels(module):
    want = EXPECTED[module]
    r = subprocess.run([OBJDUMP, "-t", _hsaco(module)], check=True, capture_output=True, text=True)
    got = {line.split()[-1][:-3] for line in r.stdout.splitlines() if line.split() and line.split()[-1].endswith(".kd")}
    assert got == want, {"unexpected": sorted(got - want), "missing": sorted(want - got)}


@pytest.mark.parametrize("module", MODULES)
def test_host_code_looks_up_the_same_names(module):
    src = open(os.path.join(PKG, "csrc", f"dg_{module}_host.cpp")).read()
    tables = re.findall(r"static const char\* const k\w+Kernels\[\] = \{([^}]*)\};", src)
    assert len(tables) == 1, "one kernel-name table per host file"
    names = re.findall(r'"([a-z_0-9]+)"', tables[0])
    assert len(names) == len(set(names))
    assert set(names) == EXPECTED[module]
    # the table is what is looked up: the loader is called with it, and nothing else asks the module for a function
    assert re.search(r"load_kernels\([^;]*\bk\w+Kernels\b", src)
    assert "hipModuleGetFunction" not in src
