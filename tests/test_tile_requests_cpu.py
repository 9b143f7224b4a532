"""CPU: dg_tile_requests (include/delta_gpu.h) through ctypes: host arithmetic,
no GPU.  The requests cover [0, version_size) in order without gaps, their
slots are contiguous (out_off == off), every tile but the last is full, and a
cap that is too small is DG_ERR_CAPACITY with the count still reported.
"""
from __future__ import annotations

import ctypes as C

import pytest

OK, INVALID_ARG, CAPACITY = 0, 1, 7
TILE = 65536


def _tiles(dg, vs, tile, cap=None):
    n = C.c_uint32(0xDEAD)
    rc = dg.lib.dg_tile_requests(vs, tile, None, 0, C.byref(n))
    assert rc == (CAPACITY if n.value else OK)
    cap = n.value if cap is None else cap
    arr = (dg.ReadReq * max(cap, 1))()
    m = C.c_uint32(0)
    rc = dg.lib.dg_tile_requests(vs, tile, arr, cap, C.byref(m))
    assert m.value == n.value
    return rc, [(a.stream, a.off, a.len, a.reserved, a.out_off) for a in arr[:min(cap, m.value)]], m.value


@pytest.mark.parametrize("vs", [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE, 0xFFFFFFFF])
@pytest.mark.parametrize("tile", [TILE, 0])
def test_tiles_cover_the_version(dg, vs, tile):
    rc, reqs, n = _tiles(dg, vs, tile)
    t = tile or 65536   # DG_TILE_BYTES_DEFAULT
    assert rc == OK and n == -(-vs // t) and len(reqs) == n
    at = 0
    for k, (stream, off, ln, reserved, out_off) in enumerate(reqs):
        assert (stream, reserved) == (0, 0) and off == at and out_off == off
        assert ln == (t if k + 1 < n else vs - at) and 1 <= ln <= t
        at += ln
    assert at == vs


def test_odd_tile_sizes(dg):
    rc, reqs, n = _tiles(dg, 10000, 4096)
    assert rc == OK and [(r[1], r[2]) for r in reqs] == [(0, 4096), (4096, 4096), (8192, 1808)]
    rc, reqs, n = _tiles(dg, 10, 3)
    assert [(r[1], r[2]) for r in reqs] == [(0, 3), (3, 3), (6, 3), (9, 1)]
    rc, reqs, n = _tiles(dg, 0xFFFFFFFF, 0xFFFFFFFF)
    assert rc == OK and [(r[1], r[2], r[4]) for r in reqs] == [(0, 0xFFFFFFFF, 0)]


def test_cap_too_small_reports_the_count(dg):
    rc, reqs, n = _tiles(dg, 5 * TILE + 1, TILE, cap=5)
    assert rc == CAPACITY and n == 6
    assert all(r == (0, 0, 0, 0, 0) for r in reqs)   # nothing was written
    rc, reqs, n = _tiles(dg, 5 * TILE + 1, TILE, cap=6)
    assert rc == OK and n == 6
    assert dg.lib.dg_tile_requests(10, 4, None, 0, None) == INVALID_ARG


def test_python_wrapper(dg):
    assert dg.tile_requests(0) == []
    assert dg.tile_requests(10, 4) == [(0, 4, 0), (4, 4, 4), (8, 2, 8)]
