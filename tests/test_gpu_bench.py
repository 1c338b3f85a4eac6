"""GPU: the plain benchmark line and `--dump-outputs` (bench.py run as a child process, as the driver runs it)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A run without `--full` times exactly `--steps` cycles, reports the headline keys and none of the `--full`
    measurements; `--dump-outputs` writes the whole level-0 field (32^3: below the sample size) and the norms of the timed
    cycles, and two runs with the same arguments write the same arrays bit for bit."""
    import bench
    import emg3d_amd as em
    runs = []
    for d in ("a", "b"):
        line = _bench("--workload", "32F", "--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path / d))
        assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0
        assert line["metric"] == "Mcells/s per multigrid cycle" and line["unit"] == "Mcells/s"
        assert line["higher_is_better"] is True and line["dtype"] == "c128"
        assert line["value"] == pytest.approx(line["config"]["cells"] / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-6)
        for k in ("roofline", "residual_kernel", "config_256V", "batched_sources", "hbm_stream", "time_to_tol", "parity",
                  "cpu_baseline"):
            assert k not in line, k
        runs.append((line, {f: np.load(tmp_path / d / (f + ".npy")) for f in ("efield_re", "efield_im", "residual_norms")}))
    grid = bench.build_problem(em, "32F", 1.0)[0]
    (line, a), (_, b) = runs
    assert a["efield_re"].dtype == a["efield_im"].dtype == a["residual_norms"].dtype == np.float64
    assert a["efield_re"].shape == a["efield_im"].shape == (grid.nE,) and np.isfinite(a["efield_re"]).all()
    assert np.abs(a["efield_re"]).max() > 0 and np.abs(a["efield_im"]).max() > 0 and a["residual_norms"].shape == (3,)
    # the norms of the three timed cycles: the last three entries of the line's history (relative to the source norm)
    rel = np.asarray(line["rel_error_after"][-3:])
    np.testing.assert_allclose(a["residual_norms"] / a["residual_norms"][0], rel / rel[0], rtol=1e-12)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
