"""Streams that pin the command-chain parser's window rules (csrc/dg_parse_chain.h)
for every kernel that reads a stream: inputs of tests/test_window_cases_cpu.py
and of one GPU test each in test_gpu_decode_order.py, test_gpu_invert.py,
test_gpu_inplace_device.py, test_gpu_compose.py and test_gpu_update.py.

The parser takes a stream in windows of W bytes, the first one starting at
stream byte 25: W = 1024 in the one-wave kernels (in-place, compose, invert),
W = 4096 in decode and update.  Every stream here begins with an ADD whose
payload length puts the start of the second command k bytes before the end of
that first window, for k = 0..13:

  copy   a COPY (13-byte header): k = 13 fits exactly, k = 1..12 is cut by the
         window, k = 0 starts the next window (the ADD ends at the window's end)
  add    an ADD of 20 bytes: its 9-byte header is cut for k = 1..8, its payload
         crosses the boundary for k = 9..13
  end    the END byte: the window's last byte for k = 1, the next window's first
         for k = 0

and is followed (copy, add) by three short commands, so that the window the
parser restarts is parsed too.  noend0 / noend1 are the end stream without its
END byte, ending exactly at the window's end and one byte after it (a stream
may end without END, encoding.c:111-178).

A case is (name, R, V, delta, meta); meta holds W, k, kind and the command list
in compose_cases' form.  inplace_cases builds the same streams with flag byte 1
for the update kernel: the commands then act on the buffer that holds R, and V
is the oracle's sequential replay.  Nothing here needs a GPU.
"""
from __future__ import annotations

import random

import compose_cases as cc
import update_cases as uc

WINDOWS = [1024, 4096]
KS = list(range(14))
KINDS = ["copy", "add", "end"]
FIRST = 25   # stream offset of the first window

_R = random.Random(21).randbytes(600)


def _cmds(W, k, kind):
    rng = random.Random(1000 * W + 10 * (k or 0) + len(kind))
    lit = rng.randbytes
    if kind.startswith("noend"):          # the ADD ends int(kind[5:]) bytes after the window's end
        return [("A", lit(W - 9 + int(kind[5:])))]
    cmds = [("A", lit(W - k - 9))]        # header 9 + payload: the next command at window offset W - k
    if kind == "end":
        return cmds
    cmds.append(("C", 37, 100) if kind == "copy" else ("A", lit(20)))
    return cmds + [("C", 5, 7), ("A", lit(3)), ("C", 100, 9)]


def _specs():
    for W in WINDOWS:
        for kind in KINDS:
            for k in KS:
                yield W, k, kind
        for kind in ("noend0", "noend1"):
            yield W, None, kind


def _finish(d, kind):
    assert d[-1] == 0
    return d[:-1] if kind.startswith("noend") else d


_cache = {}


def standard_cases(dg, orc):
    """Standard deltas of R -> V, built once per session."""
    if "std" not in _cache:
        out = []
        for W, k, kind in _specs():
            cmds = _cmds(W, k, kind)
            d = _finish(cc.make_delta(dg, orc, cmds, _R), kind)
            out.append((f"w{W}_{kind}" + ("" if k is None else f"_k{k}"), _R, cc.apply(cmds, _R), d,
                        dict(W=W, k=k, kind=kind, cmds=cmds)))
        _cache["std"] = out
    return _cache["std"]


def inplace_cases(dg, orc):
    """The same command lists as in-place deltas (flag byte 1), with the oracle's replay as V."""
    if "inp" not in _cache:
        out = []
        for W, k, kind in _specs():
            cmds = _cmds(W, k, kind)
            placed, size = cc.place(dg, cmds)
            d, V = uc.make_delta(dg, orc, _R, placed, size)
            assert d[4] == 1
            out.append((f"w{W}_{kind}" + ("" if k is None else f"_k{k}"), _R, V, _finish(d, kind),
                        dict(W=W, k=k, kind=kind, cmds=cmds)))
        _cache["inp"] = out
    return _cache["inp"]
