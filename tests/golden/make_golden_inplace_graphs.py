#!/usr/bin/env python3
"""Regenerate the in-place conversion goldens from the REFERENCE itself.

For every named graph of tests/inplace_graphs.py and both cycle policies, the
crafted standard delta is converted by the reference's own CLI
(`oracle/_ref/delta inplace`, compiled from the reference's src/c by
oracle/Makefile).  Stored per case: the recipe parameters, the sha256 of R and
of the standard delta, and the length and sha256 of the reference's output,
plus its hex when under 4 KiB.  Three files:

    golden_inplace_graphs.json   named_graphs()
    golden_inplace_seams.json    seam_graphs(): the larger ones, no hex
    golden_inplace_high.json     the "inplace" row of tests/high_offset_cases.py,
                                 every accepted case of each policy's list: names,
                                 lengths and digests only.  The reference file is
                                 written sparse (its length, then the corpus's few
                                 windows) into a temporary directory.

Run in the dev container:

    make -C oracle ref && python tests/golden/make_golden_inplace_graphs.py
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, TESTS)

import oracle as O  # noqa: E402
from conftest import load_product  # noqa: E402
from inplace_graphs import POLICIES, build, named_graphs, seam_graphs  # noqa: E402

REF_CLI = os.path.join(ROOT, "oracle", "_ref", "delta")
INLINE_MAX = 4096
GENERATOR = "reference src/c via oracle/_ref/delta inplace"


def sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def ref_inplace_file(fr: str, std: bytes, policy: str, tmp: str) -> bytes:
    fd, fo = (os.path.join(tmp, x) for x in ("d", "o"))
    open(fd, "wb").write(std)
    subprocess.run([REF_CLI, "inplace", fr, fd, fo, "--policy", policy], check=True, capture_output=True)
    return open(fo, "rb").read()


def ref_inplace(R: bytes, std: bytes, policy: str, tmp: str) -> bytes:
    fr = os.path.join(tmp, "r")
    open(fr, "wb").write(R)
    return ref_inplace_file(fr, std, policy, tmp)


def write_sparse(path: str, buf, length: int):
    """The first `length` bytes of a sparse_model.SparseBytes as a sparse file."""
    with open(path, "wb") as f:
        f.truncate(length)
        for o, b in buf.head(length).windows():
            f.seek(o)
            f.write(b)


def graph_cases(dg, orc, graphs, tmp, inline):
    cases = []
    for name, params, R, cmds in graphs:
        std, V = build(dg, orc, R, cmds)
        for policy in POLICIES:
            out = ref_inplace(R, std, policy, tmp)
            e = {"name": name, "policy": policy, "params": params, "r_sha256": sha(R),
                 "std_sha256": sha(std), "v_len": len(V), "len": len(out), "sha256": sha(out)}
            if inline and len(out) < INLINE_MAX:
                e["hex"] = out.hex()
            cases.append(e)
    return cases


def high_cases(tmp):
    import high_offset_cases as hc
    cases, files = [], {}
    for name, ref_len, d, st in hc.corpus()["inplace"]:
        for policy in POLICIES:
            if st.get(policy) != hc.OK:
                continue
            if ref_len not in files:
                files[ref_len] = os.path.join(tmp, f"r_{ref_len:x}")
                write_sparse(files[ref_len], hc.R, ref_len)
            out = ref_inplace_file(files[ref_len], d, policy, tmp)
            cases.append({"name": name, "policy": policy, "std_sha256": sha(d), "len": len(out), "sha256": sha(out)})
    return cases


def dump(name, cases):
    doc = {"generator": GENERATOR, "cases": cases}
    path = os.path.join(HERE, name)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{len(cases)} cases -> {path} ({os.path.getsize(path)} bytes)")


def main():
    dg = load_product()
    orc = O.Oracle()
    with tempfile.TemporaryDirectory() as tmp:
        dump("golden_inplace_graphs.json", graph_cases(dg, orc, named_graphs(), tmp, True))
        dump("golden_inplace_seams.json", graph_cases(dg, orc, seam_graphs(), tmp, False))
        dump("golden_inplace_high.json", high_cases(tmp))


if __name__ == "__main__":
    main()
