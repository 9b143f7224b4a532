"""CPU: the streams of tests/window_cases.py are what they claim to be.

Every stream decodes on the host to the commands it was built from; its second
command starts k bytes before the end of the first parse window, measured on
the parsed stream; and every kind and every k is present for both window
sizes.  The oracle replays each stream to its V.
"""
from __future__ import annotations

import pytest

import compose_cases as cc
import update_cases as uc
import window_cases as wc


@pytest.mark.parametrize("form", ["standard", "inplace"])
def test_streams_decode_to_their_commands(dg, orc, form):
    cases = wc.standard_cases(dg, orc) if form == "standard" else wc.inplace_cases(dg, orc)
    for name, R, V, d, m in cases:
        assert len(R) == 600 and len(d) <= 4300, name
        cmds, inplace, vs, src_crc, _ = dg.decode_delta(d)
        placed, size = cc.place(dg, m["cmds"])
        assert cmds == placed and vs == size == len(V) and inplace == (form == "inplace"), name
        assert src_crc == orc.crc64_xz(R), name
        rc, out = orc.decode(R, d)
        assert rc == 0 and out == V, name


@pytest.mark.parametrize("form", ["standard", "inplace"])
def test_second_command_sits_k_bytes_before_the_window_end(dg, orc, form):
    cases = wc.standard_cases(dg, orc) if form == "standard" else wc.inplace_cases(dg, orc)
    seen = set()
    for name, _, _, d, m in cases:
        W, k, kind = m["W"], m["k"], m["kind"]
        at = uc.commands_at(d)
        assert at[0][:2] == (wc.FIRST, 2), name
        if kind.startswith("noend"):
            assert len(at) == 1, name   # the ADD alone: no END byte follows it
            assert at[0][0] + at[0][2] + at[0][3] == len(d) == wc.FIRST + W + int(kind[5:]), name
            seen.add((W, kind))
            continue
        x, t = at[1][0], at[1][1]
        assert x - wc.FIRST == W - k, name
        assert t == {"copy": 1, "add": 2, "end": 0}[kind], name
        assert at[-1][1] == 0 and at[-1][0] == len(d) - 1, name   # END is the last byte
        assert len(at) == (2 if kind == "end" else 6), name
        if kind == "add":
            assert at[1][3] == 20, name
        seen.add((W, kind, k))
    assert seen == ({(W, kind, k) for W in wc.WINDOWS for kind in wc.KINDS for k in wc.KS} |
                    {(W, kind) for W in wc.WINDOWS for kind in ("noend0", "noend1")})
    assert len(cases) == 88
