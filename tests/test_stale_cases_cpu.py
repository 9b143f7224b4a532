"""CPU: the preconditions of tests/test_gpu_stale_index.py, on the batches of
tests/stale_cases.py.  A run under a stale index proves something only where
the index really is stale, so every case is held against the index model
(index_cases.serial_index) here, before any of them reaches a GPU.
"""
from __future__ import annotations

import index_cases as ic
import read_cases as rc
import stale_cases as sc


def test_read_families(orc):
    fams = sc.read_families(orc)
    assert set(fams) == {"payload", "framing", "smaller", "larger", "unordered", "fills"}
    for fam, cases in fams.items():
        assert len(cases) >= sc.MIN_STREAMS, (fam, len(cases))
        for name, R, a, b in cases:
            ia = sc.index_of(len(R), a)
            assert ia[0]["status"] == rc.OK and ia[0]["seq"] == 1, name   # A is served through the index
            if fam == "fills":
                for f in sc.FILLS:
                    assert sc.index_of(len(R), bytes([f]) * len(a)) != ia, (name, f)
                continue
            assert len(a) == len(b) and a != b, name
            ib = sc.index_of(len(R), b)
            assert ib[0]["status"] == rc.OK, name                        # B holds valid streams only
            assert (ia == ib) == (fam == "payload"), name
            va, vb = rc.model_version(R, a)[1], rc.model_version(R, b)[1]
            if fam == "payload":
                assert va != vb and len(va) == len(vb), name
            if fam == "framing":
                assert va == vb, name
            if fam in ("smaller", "larger"):
                assert (len(vb) < len(va)) == (fam == "smaller") and len(va) != len(vb), name
            if fam == "unordered":
                assert ib[0]["seq"] == 0, name
    # both index models agree that the payload family is not stale and the others are
    for fam in ("payload", "framing"):
        name, R, a, b = fams[fam][1]
        assert (ic.chunked_index(len(R), a, 4096) == ic.chunked_index(len(R), b, 4096)) == (fam == "payload")
    # streams of one window and of more than ten
    assert min(len(c[2]) for c in fams["payload"]) < 4096 and max(len(c[2]) for c in fams["payload"]) > 40960


def test_lineage_families(dg, orc):
    fams = sc.lineage_families(dg, orc)
    for fam, cases in fams.items():
        names = [c[0] for c in cases]
        for fname in sc.FORESTS:   # every forest with its top, middle and base level replaced
            levels = {n.split("_level")[1].split("_")[0] for n in names if n.startswith(fname)}
            depth = int(fname[len("history_depth"):])
            want = {str(j) for j in (depth - 1, depth // 2, 0)}
            # (a level whose delta has no ADD has no other payload)
            assert levels == want or (fam == "payload" and levels and levels <= want), (fam, fname)
        if fam == "fills":
            continue
        streams = sc.lineage_streams(cases)
        assert len(streams) == len(cases)   # one level at a time
        assert len(streams) >= sc.MIN_STREAMS, (fam, len(streams))
        for (name, na, nb), (ref_len, a, b) in zip(cases, streams):
            assert len(a) == len(b), name
            ia, ib = sc.index_of(ref_len, a), sc.index_of(ref_len, b)
            assert ia[0]["status"] == rc.OK and ia[0]["seq"] == 1, name
            assert ib[0]["status"] == rc.OK, name                        # B holds valid streams only, under the stated ref_len
            assert (ia == ib) == (fam == "payload"), name
            assert fam != "unordered" or ib[0]["seq"] == 0, name
