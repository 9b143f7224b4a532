"""CPU: the Python model of the chunked index pass (tests/index_cases.py) leaves
the index the one-block pass's model leaves, on every stream of index_cases at
three chunk sizes; the fake-command streams are the adversarial ones they claim
to be; and a version is the concatenation of its tiles.
"""
from __future__ import annotations

import pytest

import index_cases as ic
import read_cases as rc


@pytest.mark.parametrize("chunk_bytes", [4096, 8192, 65536])
def test_chunked_model_equals_serial_model(dg, orc, chunk_bytes):
    seen = set()
    for name, R, d, st, want in ic.models(dg, orc):
        got = ic.chunked_index(len(R), d, chunk_bytes)
        assert got == want, (name, chunk_bytes, got[0], want[0],
                             [(k, a, b) for k, (a, b) in enumerate(zip(got[1], want[1])) if a != b][:4])
        assert want[0]["status"] == st, name
        seen.add(want[0]["status"])
    assert seen == {ic.OK, ic.UNSUPPORTED, ic.MALFORMED}


def test_the_streams_have_the_shapes_they_claim(orc):
    cases = {c[0]: c for c in ic.new_cases(orc)}
    for name, R, d, st in cases.values():
        if name not in ("stream_of_25_bytes", "exactly_one_chunk"):
            assert 3 <= -(-len(d) // ic.CHUNK) <= 10 or name.startswith("one_byte"), (name, len(d))
    assert len(cases["exactly_one_chunk"][2]) == ic.CHUNK and len(cases["stream_of_25_bytes"][2]) == 25
    # sequential and not: the break on the chunk edge clears the flag, the shifted streams keep it
    assert ic.serial_index(2000, cases["break_on_chunk_edge"][2])[0]["seq"] == 0
    assert ic.serial_index(3000, cases["command_at_chunk_edge"][2])[0]["seq"] == 1
    for name in ("many_exchanged_x", "many_exchanged_late_x", "many_descending_x", "many_overlapping_x",
                 "short_of_version_x"):
        h = ic.serial_index(2000, cases[name][2])[0]
        assert (h["status"], h["seq"]) == (ic.OK, 0), name
    # END in chunk 1: valid, with malformed bytes in the chunks after it
    d = cases["end_in_chunk_1_then_garbage"][2]
    assert rc.parse(3000, d)[0] == ic.OK and d[4 * ic.CHUNK] == 7
    # every malformed stream sits between valid neighbours
    order = [c[3] for c in ic.new_cases(orc)]
    for k, st in enumerate(order):
        if st:
            assert order[k - 1] == ic.OK and order[k + 1] == ic.OK


def test_fake_commands_mislead_a_false_entry_only(orc):
    """At each chunk edge inside the long payload the exit table sends the false
    entry (the edge itself) to END or to malformed, or along a fake chain, while
    the walk from the true entry passes: the stream is valid."""
    fakes = [c for c in ic.new_cases(orc) if c[0].startswith("fake_")]
    assert len(fakes) == 4
    kinds = set()
    for name, R, d, st in fakes:
        assert st == ic.OK and rc.parse(len(R), d)[0] == ic.OK
        ex = ic.exit_table(d, ic.CHUNK)
        true_offsets = {c[0] for c in rc.parse(len(R), d)[2]}
        for edge in (ic.CHUNK, 2 * ic.CHUNK):
            assert edge not in true_offsets
            kinds.add("end" if ex[edge] == ic.END else "bad" if ex[edge] == ic.BAD else "chain")
        chunks, walk_bad = ic.walk(d, ex, ic.CHUNK)
        assert not walk_bad
        # the chain jumps over the chunk between the edges: it inherits chunk 2's entry, a true command
        assert chunks[1][0] == chunks[2][0] and chunks[1][0] in true_offsets and chunks[1][0] > 2 * ic.CHUNK
        assert ex[25] == chunks[1][0]
    assert {"end", "bad"} <= kinds


def test_version_is_the_concatenation_of_its_tiles(dg, orc):
    for name, R, d, st in ic.all_cases(dg, orc):
        if st:
            continue
        _, V, _ = rc.model_version(R, d)
        tiles = dg.tile_requests(len(V), 4096)
        assert b"".join(rc.model_read(V, off, n) for off, n, _ in tiles) == V, name
        assert [t[2] for t in tiles] == [t[0] for t in tiles]
