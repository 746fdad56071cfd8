"""bench.py as every later change runs it: a plain run is the headline alone (no other leg, check
or baseline: those need --full), --steps sets the timed steps, the line carries ms_per_step, and
--dump-outputs writes the last timed step's verdicts, identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_is_the_headline_alone_and_dumps_its_verdicts(tmp_path):
    n = 70001   # not a multiple of 64: the last verdict word is partial
    lines, dumps = [], []
    for d, steps in (("a", 3), ("b", 2)):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
               "--triples", str(n), "--dump-outputs", str(tmp_path / d)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [x for x in r.stdout.splitlines() if x.strip()]
        assert len(out) == 1, out
        lines.append(json.loads(out[0]))
        assert os.listdir(tmp_path / d) == ["verdicts.npy"]
        dumps.append(np.load(tmp_path / d / "verdicts.npy"))
    for line, steps in zip(lines, (3, 2)):
        assert line["steps"] == steps and line["warmup"] == 1 and line["n_gpus"] == 1
        assert line["unit"] == "verifies/s" and line["higher_is_better"] is True and line["dtype"] == "int64"
        assert line["ms_per_step"] > 0
        assert abs(line["value"] - n / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
        assert line["config"]["verdicts_ok"] is True
        # what --full adds is absent
        assert not {"configs", "digest", "cpu_baseline", "roofline"} & set(line)
    a, b = dumps
    assert a.dtype == np.float32 and a.shape == (n,) and (a == 1).all()   # the workload's triples are all valid
    assert (a == b).all()
