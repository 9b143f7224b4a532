"""CPU: dg_update_plan_create's descriptor checks under ASan + UBSan.

update_check_descs (dg_plan.cpp, no HIP) is what dg_update_plan_create runs
before it touches the device.  tests/sanitize/update_check.cpp calls it with
empty, touching, overlapping, oversized and wrapping descriptors; it is
compiled here with g++ -fsanitize=address,undefined and run as its own program.
"""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "delta-compression_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

OK, INVALID_ARG, TOO_LARGE = 0, 1, 3
WANT = {
    "empty": OK, "one": OK, "zero_cap": OK, "touching": OK, "touching_unsorted": OK,
    "overlap_one_byte": INVALID_ARG, "overlap_inside": INVALID_ARG, "overlap_same": INVALID_ARG,
    "cap_4g": TOO_LARGE, "ref_4g": TOO_LARGE, "delta_4g": TOO_LARGE, "cap_below_4g": OK, "far_offset": OK,
    "wraps": INVALID_ARG, "many_touching": OK, "many_one_overlap": INVALID_ARG,
}


def test_descriptor_checks_under_sanitizers(tmp_path):
    exe = tmp_path / "update_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "sanitize", "update_check.cpp"),
           os.path.join(CSRC, "dg_plan.cpp"), os.path.join(CSRC, "dg_format.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-500:] + p.stderr[-4000:]
    got = {}
    for line in p.stdout.splitlines():
        name, rc, msg = line.split(" ", 2)
        got[name] = int(rc)
        assert (msg == "-") == (int(rc) == OK), line
    assert got == WANT
