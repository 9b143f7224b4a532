"""CPU: range reads on the host (dg_read, `delta read`) against the Python model
of tests/read_cases.py, and the model against the oracle's decode.

No GPU: dg_read is pure host code, and `delta read` calls nothing else.
"""
from __future__ import annotations

import os
import subprocess

import pytest

import read_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "delta-compression_amd", "bin", "delta")


def test_model_is_the_oracles_decode_sliced(dg, orc):
    n = 0
    for name, R, d, st, V, rs in rc.with_ranges(dg, orc):
        if st:
            continue
        code, out = orc.decode(R, d, ignore_hash=True)
        assert code == 0 and out == V, name
        for off, ln in rs:
            assert rc.model_read(V, off, ln) == out[off:off + ln], (name, off, ln)
        assert b"".join(rc.model_read(V, o, ln) for o, ln in rc.tiling(len(V))) == V, name
        n += 1
    assert n > 100


def test_corpus_reaches_what_it_is_for(dg, orc):
    by = {c[0]: c for c in rc.with_ranges(dg, orc)}
    assert 12000 < len(by["onepass_1pct"][2]) < 16000             # 4 windows
    assert len(by["onepass_dense24"][2]) > 5 * rc.WINDOW          # several windows and index entries
    assert len(by["long_add"][2]) > 19 * rc.STRIDE                # the payload skips index strides
    assert len(by["many_descending"][2]) > 2 * rc.WINDOW
    assert sum(1 for c in by.values() if c[0].startswith("w")) == 88
    assert sum(1 for c in by.values() if c[3]) == 10


def test_dg_read_equals_the_model(dg, orc):
    for name, R, d, st, V, rs in rc.with_ranges(dg, orc):
        for off, ln in rs:
            if st:
                with pytest.raises(dg.DeltaError) as e:
                    dg.read_range(R, d, off, ln)
                assert e.value.code == st, name
            else:
                assert dg.read_range(R, d, off, ln) == rc.model_read(V, off, ln), (name, off, ln)
        if not st:
            assert b"".join(dg.read_range(R, d, o, ln) for o, ln in rc.tiling(len(V))) == V, name


def test_dg_read_offsets_past_32_bits(dg, orc):
    name, R, d, st, V, _ = rc.with_ranges(dg, orc)[0]
    assert not st
    assert dg.read_range(R, d, 1 << 40, 1 << 40) == b""
    assert dg.read_range(R, d, 5, (1 << 64) - 1) == V[5:]
    assert dg.read_range(R, d, (1 << 64) - 1, (1 << 64) - 1) == b""


def _cli_read(tmp_path, R, d, off, ln):
    (tmp_path / "r").write_bytes(R)
    (tmp_path / "d").write_bytes(d)
    out = tmp_path / "o"
    if out.exists():
        out.unlink()
    p = subprocess.run([CLI, "read", str(tmp_path / "r"), str(tmp_path / "d"), str(off), str(ln), str(out)],
                       capture_output=True, text=True)
    return p, (out.read_bytes() if out.exists() else None)


def test_cli_read(dg, orc, tmp_path):
    cases = rc.with_ranges(dg, orc)
    picked = [c for c in cases if c[3]] + [c for c in cases if not c[3]][:24]
    for name, R, d, st, V, rs in picked:
        off, ln = rs[len(rs) // 3]
        p, got = _cli_read(tmp_path, R, d, off, ln)
        if st:
            assert p.returncode == 1 and got is None, name
            assert dg.status_string(st) in p.stderr, (name, p.stderr)
        else:
            assert p.returncode == 0, (name, p.stderr)
            assert got == rc.model_read(V, off, ln), (name, off, ln)
    p = subprocess.run([CLI, "read", "a", "b"], capture_output=True, text=True)
    assert p.returncode == 1 and "delta read <ref> <delta> <offset> <length> <output>" in p.stderr


def test_cli_read_agrees_with_the_reference_decode(dg, orc, tmp_path):
    import oracle as O
    if not os.path.exists(O.REF_CLI):
        pytest.skip("oracle/_ref/delta is not built")
    good = [c for c in rc.with_ranges(dg, orc) if not c[3]]
    for name, R, d, st, V, rs in good[:20]:
        (tmp_path / "r").write_bytes(R)
        (tmp_path / "d").write_bytes(d)
        p = subprocess.run([O.REF_CLI, "decode", str(tmp_path / "r"), str(tmp_path / "d"), str(tmp_path / "v"),
                            "--ignore-hash"], capture_output=True, text=True)
        assert p.returncode == 0, (name, p.stderr)
        whole = (tmp_path / "v").read_bytes()
        for off, ln in (rs[1], rs[len(rs) // 2], (0, len(whole))):
            p, got = _cli_read(tmp_path, R, d, off, ln)
            assert p.returncode == 0 and got == whole[off:off + ln], (name, off, ln)
