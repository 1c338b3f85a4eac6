"""The exact cubic receiver adjoint against the per-receiver source loop it replaces, at 128^3 (BASELINE.json configs[1] model).

  (a) DeviceMG.set_receiver_adjoint(rec, w, method='cubic'): host-built table, k_spline_eval_adjoint, the transposed prefilter
      (nine field-sized filter passes), k_trim_add -- per active component
  (b) the reference's rule as optimize.gradient() / Jacobian(adjoint='reference') apply it: one set_source (1 m dipole) per
      receiver, accumulated

for 16 and 256 receivers spread over the core of the grid.  Host clock around calls that end in a device synchronise, one warm-up
call each, median and range of five, one process.  Prints one JSON line.

    python tools/receiver_adjoint_timing.py [workload=128F] [repeats=5]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import emg3d_amd as em  # noqa: E402
from emg3d_amd import fields, solver  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "128F"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
FREQ = 1.0
grid, model, _, _ = bench.build_problem(em, wl, FREQ)
spec = fields.FrequencySpec(FREQ)
parts = solver._exact_parts(grid, model, spec.smu0)
smu0 = spec.smu0


def receivers(n, rng):
    return (rng.uniform(-900., 900., n), rng.uniform(-900., 900., n), rng.uniform(-900., -100., n), rng.uniform(0., 360., n),
            rng.uniform(-30., 30., n))


def timed(fn):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return {"ms_median": 1e3 * float(np.median(times)), "ms_min": 1e3 * min(times), "ms_max": 1e3 * max(times)}


out = {"workload": wl, "repeats": reps}
with solver.DeviceMG.from_model(grid, parts, spec) as dev:
    for n in (16, 256):
        rng = np.random.default_rng(n)
        rec = receivers(n, rng)
        w = rng.standard_normal(n) + 1j * rng.standard_normal(n)

        def exact():
            dev.set_receiver_adjoint(rec, w, method='cubic')

        def loop():
            for i in range(n):
                dev.set_source([c[i] for c in rec], smu0, strength=w[i] / smu0, accumulate=i > 0)
        out[f"n{n}"] = {"exact_cubic": timed(exact), "source_loop": timed(loop)}
print(json.dumps(out))
