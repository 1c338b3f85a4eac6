"""Batched Krylov solves against one solve per source: the bench's 128^3 workload (BASELINE.json configs[1] model: F-cycle,
semicoarsening + line relaxation, tol = 1e-6, colour order) with BiCGSTAB around the cycle, 8 distinct dipole sources.

  (a) one solve(..., handle=dev, sslsolver='bicgstab') per source in sequence on one handle
  (b) solve_sources(..., sslsolver='bicgstab') on one batched handle

Host clock around calls that end in a device synchronisation, one warm-up call each, median and range of five, one
process; download=False in both (solve() with a Krylov solver returns its iterate from a workspace vector whatever
``download`` says: (a) includes that copy, as the per-source path does).  A further, instrumented run of each gives the time inside
the multigrid cycles (``DeviceMG.cycle``; every call ends with the norms on the host): time per preconditioner cycle and
system, and the share of the solve spent outside the cycles (vector kernels, reductions, host).  Prints one JSON line.

    python tools/batched_krylov_timing.py [workload=128F] [sources=8] [repeats=5]
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
nsrc = int(sys.argv[2]) if len(sys.argv) > 2 else 8
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
FREQ = 1.0
grid, model, _, cycle = bench.build_problem(em, wl, FREQ)
opts = dict(cycle=cycle, semicoarsening=True, linerelaxation=True, sslsolver='bicgstab', tol=1e-6, ordering='colour', verb=0)
sources = [[-700. + 200. * k, 100. * (k % 3 - 1), -100. * (k % 2), 30. + 10. * k, 10.] for k in range(nsrc)]
spec = fields.FrequencySpec(FREQ)
parts = solver._exact_parts(grid, model, spec.smu0)


class CycleClock:
    """Host time inside ``dev.cycle`` (the call returns with the norms: the device has finished the cycle)."""

    def __init__(self, dev):
        self.s, self.calls, self._cycle = 0.0, 0, dev.cycle
        dev.cycle = self

    def __call__(self, *a, **kw):
        t0 = time.perf_counter()
        out = self._cycle(*a, **kw)
        self.s += time.perf_counter() - t0
        self.calls += 1
        return out


def per_source(dev):
    infos = []
    for src in sources:
        _, info = solver.solve(grid, None, fields.SourceField(grid, freq=FREQ), handle=dev, source=(src, 0), download=False,
                               return_info=True, **opts)
        infos.append(info)
    return infos


def batched(dev):
    return solver.solve_sources(grid, None, sources, FREQ, handle=dev, download=False, **opts)[1]


def measure(run, dev):
    run(dev)                                    # warm-up: set-up, launch graphs, workspace
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        infos = run(dev)
        times.append(time.perf_counter() - t0)
    clock = CycleClock(dev)
    t0 = time.perf_counter()
    run(dev)
    total = time.perf_counter() - t0
    cyc = sum(i['it_mg'] for i in infos)
    return {"s_median": float(np.median(times)), "s_min": min(times), "s_max": max(times), "s_all": times,
            "it_ssl": [i['it_ssl'] for i in infos], "it_mg": [i['it_mg'] for i in infos],
            "exit": [i['exit'] for i in infos], "cycle_calls": clock.calls, "s_in_cycles": clock.s, "s_instrumented": total,
            "ms_per_cycle_and_system": 1e3 * clock.s / cyc if cyc else None,
            "share_outside_cycles": 1.0 - clock.s / total}


out = {"workload": wl, "sources": nsrc, "repeats": reps, "options": {k: v for k, v in opts.items() if k != 'verb'}}
with solver.DeviceMG.from_model(grid, parts, spec) as dev:
    out["per_source"] = measure(per_source, dev)
with solver.DeviceMG.from_model(grid, parts, spec) as dev:
    out["batched"] = measure(batched, dev)
    out["batched"]["device_bytes"] = dev.device_bytes
a, b = out["per_source"], out["batched"]
out["speedup_median"] = a["s_median"] / b["s_median"]
out["ms_per_source"] = {"per_source": 1e3 * a["s_median"] / nsrc, "batched": 1e3 * b["s_median"] / nsrc}
out["same_iterations"] = a["it_ssl"] == b["it_ssl"] and a["it_mg"] == b["it_mg"]
print(json.dumps(out))
