#!/usr/bin/env python3
"""Regenerate tests/golden/golden_greedy.json from the REFERENCE itself.

Greedy deltas of the shared test inputs (tests/greedy_cases.py, tests/cases.py
and the synthetic generators), minted by the reference's own src/c as
oracle/Makefile compiles it: the default tie-break through
oracle/_ref/libdelta_ref.so (`ref_encode_pair`, algorithm 0), --splay through
the reference CLI oracle/_ref/delta (`encode greedy ... --splay`), in-place
deltas through `ref_encode_pair_inplace`.  Run in the dev container:

    make -C oracle ref && python tests/golden/make_golden_greedy.py

Entry format as golden.json: inputs as a generator spec + sha256, the delta
bytes inline (hex) up to 2048 bytes, else sha256 + length.
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(HERE))

import oracle as O  # noqa: E402
import greedy_cases as G  # noqa: E402
from cases import small_cases  # noqa: E402

GREEDY = 0
INLINE_MAX = 2048


def sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def cli_splay(tmp: str, R: bytes, V: bytes, p: int) -> bytes:
    rp, vp, dp = (os.path.join(tmp, n) for n in "rvd")
    with open(rp, "wb") as f:
        f.write(R)
    with open(vp, "wb") as f:
        f.write(V)
    subprocess.run([O.REF_CLI, "encode", "greedy", rp, vp, dp, "--splay", "--seed-len", str(p)],
                   check=True, capture_output=True)
    with open(dp, "rb") as f:
        return f.read()


def entry(d: bytes, R: bytes, V: bytes, p: int, splay: bool, **extra) -> dict:
    e = {"algo": GREEDY, "p": p, "splay": splay, "r_sha256": sha(R), "v_sha256": sha(V),
         "r_len": len(R), "v_len": len(V), "delta_len": len(d), "delta_sha256": sha(d),
         "src_crc": d[9:17].hex(), "dst_crc": d[17:25].hex()}
    if len(d) <= INLINE_MAX:
        e["delta_hex"] = d.hex()
    e.update(extra)
    return e


def main():
    ref = O.Reference()
    orc = O.Oracle()
    out = {"generator": "reference src/c via oracle/_ref (ref_encode_pair; --splay: the delta CLI)", "cases": []}
    items = []   # (spec, R, V, p)
    seen = set()
    for name, R, V, p, _ in small_cases():   # (greedy ignores --table-size: one entry per input and p)
        if (R, V, p) not in seen:
            seen.add((R, V, p))
            items.append((dict(name=name, kind="small"), R, V, p))
    for name, R, V, p in G.named_cases():
        items.append((dict(name=name, kind="greedy_named"), R, V, p))
    for p in (1, 2, 3, 4, 5, 8, 16):
        for i, (R, V) in enumerate(G.random_pairs(0x6EED0 + p, 6)):
            items.append((dict(name=f"rand_p{p}_{i}", kind="greedy_random", seed=0x6EED0 + p, index=i), R, V, p))
    for spec in G.midsize_specs():
        R, V = G.spec_inputs(orc, spec)
        items.append((spec, R, V, 16))
    with tempfile.TemporaryDirectory() as tmp:
        for spec, R, V, p in items:
            out["cases"].append(entry(ref.encode(GREEDY, R, V, p=p), R, V, p, False, **spec))
            out["cases"].append(entry(cli_splay(tmp, R, V, p), R, V, p, True, **spec))
    # in-place conversion of greedy's commands (main.c encode greedy --inplace)
    for spec, R, V, p in items:
        if spec["name"] in ("transposition_p4", "rotation", "blocks130", "c4_0", "gap5"):
            for policy in (0, 1):
                d = ref.encode_inplace(GREEDY, R, V, p=p, policy=policy)
                out["cases"].append(dict(entry(d, R, V, p, False, **spec), inplace=True, policy=policy))
    path = os.path.join(HERE, "golden_greedy.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print(f"wrote {len(out['cases'])} cases to {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
