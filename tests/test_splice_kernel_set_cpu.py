"""CPU: the stand-alone gfx950 code object of the splice (lib/dg_splice.hsaco)
exists and holds exactly the kernels the host code launches:
csrc/dg_splice_host.cpp names them once, in its k..Kernels[] table, which
load_kernels (dg_hostutil.h) looks up.  Only the symbol table is read, as in
test_transform_kernel_set_cpu.py: every kernel has one kernel descriptor symbol,
`<name>.kd`.  And the plan's geometry function is reachable without HIP: it is
compiled with g++ alone and called.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "delta-compression_amd")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
HSACO = os.path.join(PKG, "lib", "dg_splice.hsaco")

EXPECTED = {"dg_splice_map_kernel", "dg_splice_resolve_kernel", "dg_splice_emit_kernel"}

GEOMETRY_MAIN = r"""
#include <cstdio>
#include "dg_plan.h"
int main() {
	const dg_pair_t whole{16, 1000, 32, 600};
	const dg_pair_t segs[3] = {{16, 500, 32, 256}, {16, 1000, 288, 256}, {516, 500, 544, 88}};
	const uint32_t first[2] = {0, 3};
	const uint64_t caps[3] = {100, 200, 300};
	dg::SpliceGeometry g;
	std::string err;
	int rc = dg::splice_plan_geometry(segs, 3, &whole, first, 1, caps, g, err);
	printf("%d %llu %u %u %u %d\n", rc, (unsigned long long)g.bound, g.descs[2].rebase, g.descs[2].v_rel, g.groups[0].count,
	       g.descs[2].shift == (1ull << 63) && g.descs[1].shift == dg::gf2_xpow(8 * 88));
	const dg_pair_t gap[3] = {{16, 500, 32, 256}, {16, 1000, 289, 255}, {516, 500, 544, 88}};
	rc = dg::splice_plan_geometry(gap, 3, &whole, first, 1, caps, g, err);
	printf("%d %s\n", rc, err.c_str());
	return 0;
}
"""


def test_code_object_is_built():
    assert os.path.exists(HSACO), "lib/dg_splice.hsaco is missing: the Makefile's `all` builds it"


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump missing")
def test_code_object_holds_exactly_the_launched_kernels():
    r = subprocess.run([OBJDUMP, "-t", HSACO], check=True, capture_output=True, text=True)
    got = {line.split()[-1][:-3] for line in r.stdout.splitlines() if line.split() and line.split()[-1].endswith(".kd")}
    assert got == EXPECTED, {"unexpected": sorted(got - EXPECTED), "missing": sorted(EXPECTED - got)}


def test_host_code_looks_up_the_same_names():
    src = open(os.path.join(PKG, "csrc", "dg_splice_host.cpp")).read()
    tables = re.findall(r"static const char\* const k\w+Kernels\[\] = \{([^}]*)\};", src)
    assert len(tables) == 1, "one kernel-name table per host file"
    names = re.findall(r'"([a-z_0-9]+)"', tables[0])
    assert len(names) == len(set(names))
    assert set(names) == EXPECTED
    # the table is what is looked up: the loader is called with it, and nothing else asks the module for a function
    assert re.search(r"load_kernels\([^;]*\bk\w+Kernels\b", src)
    assert "hipModuleGetFunction" not in src


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_geometry_is_reachable_without_hip(tmp_path):
    main = tmp_path / "geom_main.cpp"
    main.write_text(GEOMETRY_MAIN)
    exe = tmp_path / "geom"
    csrc = os.path.join(PKG, "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", csrc, str(main), os.path.join(csrc, "dg_plan.cpp"),
                    os.path.join(csrc, "dg_format.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    assert lines[0] == "0 601 500 512 3 1"   # bound: the capacities and one byte for the group
    assert lines[1].startswith("1 ") and "segment 1" in lines[1]
