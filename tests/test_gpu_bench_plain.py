"""bench.py's plain run and --dump-outputs on the GPU: `bench.py --gpus 1
--steps K --warmup W` prints the contract's keys for the K timed steps and
nothing that belongs behind --full (no parity, no variants, no detail file);
--dump-outputs DIR holds what the last timed step returned -- the selected
set of the workload's golden, the n scores and the mean within the §8(d)
bound -- as float64 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as GU

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_outputs(tmp_path):
    name = "B_mnist"
    out_dir = tmp_path / "outs"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--workload", name, "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    p = GU.C.case_params(name)
    want = p["n"] * p["d"] * 8 / (line["ms_per_step"] * 1e-3) / 1e9
    assert abs(line["value"] - want) <= 1e-3 * want  # value = n d 8 bytes / step time
    for k in ("parity", "variants", "cpu_baseline", "detail_file", "rccl"):
        assert k not in line, k
    assert set(line["summary"]) == {name}

    g, rec = GU.load(name), GU.manifest()[name]
    assert sorted(os.listdir(out_dir)) == ["mean.npy", "scores.npy", "sel.npy"]
    sel, sc, mean = (np.load(out_dir / (k + ".npy")) for k in ("sel", "scores", "mean"))
    assert sel.dtype == sc.dtype == mean.dtype == np.float64
    assert sc.shape == (p["n"],) and mean.shape == (p["d"],)
    assert np.array_equal(sel, g["sel"].astype(np.float64))
    GU.check_scores(sc, g, rel=1e-9)
    GU.check_mean(mean, g, rec)
