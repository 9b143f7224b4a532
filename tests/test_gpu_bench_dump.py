"""GPU: a plain `bench.py` run and its --dump-outputs (one small run, shared).

A plain run measures the printed line alone (no `also`, no CPU baseline, no
stage-profile pass), times exactly --steps steps and reports ms_per_step;
--dump-outputs writes what the last timed step computed, which for the C2
generator's pairs must be the oracle's deltas byte for byte."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS, STEPS, WARMUP = 24, 3, 1


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory, torch_cuda):
    out = tmp_path_factory.mktemp("bench_dump")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DG_")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--pairs", str(PAIRS), "--dump-outputs", str(out / "dump")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    return lines[0], out / "dump"


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone(plain_run):
    line, _ = plain_run
    assert line["steps"] == STEPS and line["warmup"] == WARMUP
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    # value = job bytes x steps / time of the timed steps, ms_per_step = that time / steps
    job = 2 * 65536 * PAIRS
    assert line["value"] == pytest.approx(job / (line["ms_per_step"] / 1e3) / 2**30, rel=1e-2)
    assert "also" not in line and line["cpu_baseline"] is None
    assert line["full"] is None   # and no detail file unless --full-out names one


@pytest.mark.gpu
def test_dump_outputs_are_the_oracles_deltas(plain_run, orc):
    import oracle as O
    _, dump = plain_run
    arrays = {f[:-4]: np.load(dump / f) for f in sorted(os.listdir(dump))}
    assert set(arrays) == {"delta_bytes", "delta_bytes_streams", "offsets", "status"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 10**6
    offs, status = arrays["offsets"], arrays["status"]
    assert offs.shape == (PAIRS + 1,) and status.shape == (PAIRS,) and not status.any()
    streams = arrays["delta_bytes_streams"].astype(int).tolist()
    assert sorted(streams) == list(range(PAIRS))          # 24 C2 deltas fit the sample whole
    want, sizes = [], []
    for i in range(PAIRS):
        R, V = orc.synth_pair(0xC2000000 + i, 65536, 655)
        want.append(orc.encode(O.ONEPASS, R, V, p=16, q=1))
        sizes.append(len(want[-1]))
    assert offs.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    got = arrays["delta_bytes"].astype(np.uint8).tobytes()
    assert got == b"".join(want[i] for i in streams)
