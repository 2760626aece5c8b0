"""bench.py as the driver runs it: a plain run prints the headline line and
nothing that takes runs of its own, --dump-outputs writes what the timed path
computed (checked against the oracle), --full adds the roofline figures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import misaka_net_amd as mk
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x4D49534B41
LANES = 70001  # odd, several blocks
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY = {"roofline", "roofline_issue", "roofline_hbm", "roofline_lds", "executed", "cpu_baseline"}


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--lanes", str(LANES), *args],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout  # one JSON result line
    return json.loads(lines[0])


def test_plain_run_and_dump_outputs(gpu, tmp_path):
    rec = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert HEADLINE <= set(rec) and not FULL_ONLY & set(rec), sorted(rec)
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0
    got = {n: np.load(tmp_path / f"{n}.npy") for n in ("out", "status", "lanes", "stats")}
    assert np.array_equal(got["lanes"], np.arange(LANES))  # below bench.DUMP_LANES: every lane
    out, st, sp = po.OracleNet(mk.networks.example_network()).compute_batch(po.gen_inputs(SEED, LANES))
    assert np.array_equal(got["out"], out) and np.array_equal(got["status"], st)
    # the device counters of the 3 timed steps: retired, lanes with an output, lanes finished
    assert got["stats"][:3].tolist() == [3 * int(sp.sum()), 3 * int(((st & po.ST_HAS_OUTPUT) != 0).sum()), 3 * LANES]


def test_full_run_adds_the_roofline(gpu):
    rec = _bench("--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert HEADLINE | FULL_ONLY <= set(rec), sorted(rec)
    assert rec["cpu_baseline"] is None and rec["roofline"]["bound"] in ("hbm", "valu", "lds")
    assert rec["roofline_hbm"]["launch_us"] > 0 and rec["roofline_issue"]["peak_measured"] > 0
