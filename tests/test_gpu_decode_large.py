"""GPU: dg_decode_large (a chunked index of the delta, then the version read as
tiles) gives the status and the output bytes dg_decode gives, for valid,
non-sequential, in-place, malformed and CRC-failing inputs, through the C ABI,
the Python wrapper and the command line.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import pytest

import index_cases as ic
import read_cases as rc

pytestmark = pytest.mark.gpu

OK, MALFORMED, SRC_CRC, DST_CRC = 0, 8, 9, 10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "delta-compression_amd", "bin", "delta")


def _call(dg, ctx, fn, R, d, ignore, *extra):
    """(status, output or None) of dg_decode / dg_decode_large through the C ABI."""
    out = dg._lib.Buffer()
    rc_ = fn(ctx.handle, dg._lib._u8(R), len(R), dg._lib._u8(d), len(d), int(ignore), *extra, C.byref(out))
    got = None
    if out.data:
        got = C.string_at(out.data, out.len) if out.len else b""
    dg.lib.dg_buffer_free(C.byref(out))
    return rc_, got


def _both(dg, ctx, R, d, ignore=False, chunk=4096, tile=4096):
    a = _call(dg, ctx, dg.lib.dg_decode, R, d, ignore)
    b = _call(dg, ctx, dg.lib.dg_decode_large, R, d, ignore, chunk, tile)
    return a, b


# 1. every stream of index_cases, valid, non-sequential and malformed: the same status and bytes
def test_every_stream_of_index_cases(dg, ctx, orc):
    seen = {}
    for name, R, d, st in ic.all_cases(dg, orc):
        a, b = _both(dg, ctx, R, d)
        assert a == b, (name, a[0], b[0])
        seen[a[0]] = seen.get(a[0], 0) + 1
        if st == OK:
            assert a == (OK, rc.model_version(R, d)[1]), name
        elif st == MALFORMED:
            assert a == (MALFORMED, None), name
    assert seen[OK] > 60 and seen[MALFORMED] >= 20


# 2. the CRC checks and their precedence; the output is returned on a bad output CRC
def test_crc_failures(dg, ctx, orc):
    cases = {c[0]: c for c in ic.new_cases(orc)}
    for name in ("command_at_chunk_edge", "many_descending_x", "bad_type_middle"):
        _, R, d, st = cases[name]
        V = rc.model_version(R, d)[1]
        wrong_r = bytes([R[0] ^ 1]) + R[1:]
        bad_dst = d[:17] + bytes([d[17] ^ 0x80]) + d[18:]
        both_bad = bad_dst
        for ignore in (False, True):
            a, b = _both(dg, ctx, wrong_r, d, ignore)
            assert a == b, (name, ignore, a[0], b[0])
            if st == OK:
                assert a[0] == (OK if ignore else SRC_CRC) and (a[1] is None) == (not ignore)
            a, b = _both(dg, ctx, R, bad_dst, ignore)
            assert a == b, (name, ignore, a[0], b[0])
            if st == OK:
                assert a == ((OK if ignore else DST_CRC), V)   # the output is returned either way
            a, b = _both(dg, ctx, wrong_r, both_bad, ignore)   # the source check comes first
            assert a == b and (st != OK or ignore or a == (SRC_CRC, None))
        if st:
            assert _both(dg, ctx, wrong_r, d)[1] == (MALFORMED, None)   # malformed comes before the source check


# 3. an in-place delta takes the ordinary decode
def test_inplace_delta(dg, ctx, orc):
    import oracle as O
    R, V = orc.synth_transpose(0x1A2B, 24, 600)
    d = dg.make_inplace(R, orc.encode(O.CORRECTING, R, V, p=16, q=1))
    assert d[4] & 1
    a, b = _both(dg, ctx, R, d)
    assert a == b == (OK, V)
    a, b = _both(dg, ctx, R[:-1] + b"\0", d)
    assert a == b and a[0] == SRC_CRC


# 4. what the header checks refuse, and odd tile and chunk sizes
def test_headers_and_sizes(dg, ctx, orc):
    name, R, d, _ = next(c for c in ic.new_cases(orc) if c[0] == "payload_all_01")
    V = rc.model_version(R, d)[1]
    for bad in (b"", d[:24], b"X" + d[1:]):
        a, b = _both(dg, ctx, R, bad)
        assert a == b == (MALFORMED, None)
    for chunk, tile in ((0, 0), (8192, 1), (4096, 1000), (65536, 1 << 30)):
        if tile == 1 and len(V) > 20000:
            continue
        assert _call(dg, ctx, dg.lib.dg_decode_large, R, d, False, chunk, tile) == (OK, V), (chunk, tile)
    assert _call(dg, ctx, dg.lib.dg_decode_large, R, d, False, 100, 0)[0] == 1   # chunk_bytes is a multiple of 4096
    assert dg.decode_large(R, d, ctx=ctx) == dg.decode(R, d, ctx=ctx) == V
    with pytest.raises(dg.DeltaError) as e:
        dg.decode_large(R, d[:-3], ctx=ctx)   # the last command is cut
    assert e.value.code == MALFORMED
    # version_size 0: no tiles
    z = rc.stream(orc, R, [], version_size=0)
    assert _both(dg, ctx, R, z) == ((OK, b""), (OK, b""))


# 5. what encode_large emits for a 4 MiB pair in 256 KiB segments, default chunk and tile sizes
@pytest.mark.parametrize("algorithm", ["onepass", "correcting"])
def test_encode_large_result(dg, ctx, orc, algorithm):
    R, V = orc.synth_pair(0x4D1B0000 + len(algorithm), 4 << 20, 41943)   # 1 % edits
    d = dg.encode_large(R, V, algorithm, seg_bytes=256 << 10, window_bytes=0 if algorithm == "onepass" else 256 << 10,
                        ctx=ctx)
    a, b = _both(dg, ctx, R, d, chunk=0, tile=0)
    assert a == b and a[0] == OK and a[1] == V


# 6. the command line: decode --tile-size against decode: the file, the exit code and stderr
def test_cli_tiled_decode_equals_decode(dg, orc, tmp_path):
    cases = {c[0]: c for c in ic.new_cases(orc)}
    picks = [("fake_end_then_copy_out_of_bounds", None), ("many_exchanged_x", None), ("command_at_chunk_edge", "dst")]
    for k, (name, damage) in enumerate(picks):
        _, R, d, st = cases[name]
        if damage == "dst":
            d = d[:20] + bytes([d[20] ^ 1]) + d[21:]
        (tmp_path / f"r{k}").write_bytes(R)
        (tmp_path / f"d{k}").write_bytes(d)
        res = []
        for tag, extra in (("a", []), ("b", ["--tile-size", "4096", "--chunk-size", "4096"])):
            out = tmp_path / f"o{k}{tag}"
            p = subprocess.run([CLI, "decode", str(tmp_path / f"r{k}"), str(tmp_path / f"d{k}"), str(out)] + extra,
                               capture_output=True, text=True, timeout=120)
            res.append((p.returncode, p.stderr, out.read_bytes() if out.exists() else None))
        assert res[0] == res[1], (name, res[0][:2], res[1][:2])
        if damage == "dst":
            assert res[0][0] == 1 and res[0][1] == "output integrity check failed\n" and res[0][2] is not None
        elif st:
            assert res[0][0] == 1 and res[0][2] is None
        else:
            assert res[0][0] == 0 and res[0][2] == rc.model_version(R, d)[1]
