"""Survey gradient against the loop of optimize.gradient() per source: the bench's 128^3 workload (BASELINE.json configs[1]: the
grid and the x-resistivities of its model -- the gradient takes isotropic models --, F-cycle, semicoarsening + line relaxation,
tol = 1e-6, colour order), 8 point dipoles, 1 frequency, 16 receivers; observed data = 0.8 x the synthetic data.

  (a) optimize.gradient() per source, gradients added on the host: a handle, a hierarchy and an nC-sized download per pair
  (b) optimize.survey_gradient(batch=8): one handle, batched solves, the sum over the sources formed on the device
  (c) optimize.survey_gradient(batch=1): one handle, one system at a time

Host clock around calls that end in a device synchronisation, one warm-up call, median and range of five, one process per
measurement: without arguments the tool runs the three measurements one after the other as child processes, each under a
`timeout` of its own, stops at the first non-zero status, and prints one JSON line with the three results, the phases of (b)
(``info['phases']``: forward, data, adjoint sources, backward, accumulate -- medians over the five runs) and whether a speed-up
may be claimed: only if the median of (b) lies below the minimum of (a)'s five runs.

    python tools/survey_gradient_timing.py [workload=128F] [sources=8] [repeats=5]
    python tools/survey_gradient_timing.py --step a|b|c [workload] [sources] [repeats]      (one measurement, one JSON line)
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 420             # per measurement: warm-up + five runs of at most a few seconds each at 128^3


def step(which, wl, nsrc, reps):
    import bench
    import emg3d_amd as em
    FREQ = 1.0
    grid, tri, _, cycle = bench.build_problem(em, wl, FREQ)
    model = em.Model(grid, tri.property_x)
    opts = dict(cycle=cycle, semicoarsening=True, linerelaxation=True, tol=1e-6, ordering='colour', verb=0)
    sources = [[-700. + 200. * k, 100. * (k % 3 - 1), -100. * (k % 2), 30. + 10. * k, 10.] for k in range(nsrc)]
    k = np.arange(16)
    rec = (-750. + 100. * k, 60. * (k % 4) - 90., np.full(16, -50.), 15. * (k % 5), 5. * (k % 3))
    syn, _ = em.shard.solve_survey(grid, model, sources, [FREQ], rec, **opts)
    observed = 0.8 * syn
    weights = 1.0 / (0.05 * np.abs(observed)) ** 2

    def loop():
        phi, grad = 0.0, np.zeros(grid.vnC, order='F')
        its = []
        for i, src in enumerate(sources):
            p, g, info = em.optimize.gradient(grid, model, src, FREQ, rec, observed[i, 0], weights[i, 0], **opts)
            phi, grad = phi + p, grad + g
            its.append((info['forward']['it_mg'], info['backward']['it_mg']))
        return phi, grad, its, None

    def survey(batch):
        phi, grad, info = em.optimize.survey_gradient(grid, model, sources, [FREQ], rec, observed, weights, batch=batch, **opts)
        its = [(info['forward'][i][0]['it_mg'], info['backward'][i][0]['it_mg']) for i in range(nsrc)]
        return phi, grad, its, info['phases']

    run = {'a': loop, 'b': lambda: survey(8), 'c': lambda: survey(1)}[which]
    run()                                       # warm-up: library, device pool, first set-up
    times, phases = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        phi, grad, its, ph = run()
        times.append(time.perf_counter() - t0)
        phases.append(ph)
    out = {"step": which, "s_median": float(np.median(times)), "s_min": min(times), "s_max": max(times), "s_all": times,
           "phi": phi, "grad_norm": float(np.linalg.norm(grad)), "it_mg": its}
    if phases[0] is not None:
        out["phases_s_median"] = {key: float(np.median([p[key] for p in phases])) for key in phases[0]}
    print(json.dumps(out))


def main(argv):
    if argv and argv[0] == '--step':
        which, rest = argv[1], argv[2:]
    else:
        which, rest = None, argv
    wl = rest[0] if len(rest) > 0 else "128F"
    nsrc = int(rest[1]) if len(rest) > 1 else 8
    reps = int(rest[2]) if len(rest) > 2 else 5
    if which is not None:
        step(which, wl, nsrc, reps)
        return 0
    out = {"workload": wl, "sources": nsrc, "frequencies": 1, "receivers": 16, "repeats": reps}
    for name, key in (('a', 'gradient_per_source'), ('b', 'survey_gradient_batch8'), ('c', 'survey_gradient_batch1')):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", name, wl, str(nsrc),
               str(reps)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:
            print(f"step ({name}) ended with status {res.returncode}: stopping here", file=sys.stderr)
            print(json.dumps(out))
            return res.returncode
        out[key] = json.loads(res.stdout.strip().splitlines()[-1])
    a, b, c = out["gradient_per_source"], out["survey_gradient_batch8"], out["survey_gradient_batch1"]
    out["ms_per_pair"] = {"a": 1e3 * a["s_median"] / nsrc, "b": 1e3 * b["s_median"] / nsrc, "c": 1e3 * c["s_median"] / nsrc}
    out["same_iterations"] = a["it_mg"] == b["it_mg"] == c["it_mg"]
    out["grad_rel_dev_b_vs_a"] = abs(b["grad_norm"] / a["grad_norm"] - 1)
    out["speedup_may_be_claimed"] = b["s_median"] < a["s_min"]
    out["ratio_median_a_over_b"] = a["s_median"] / b["s_median"]
    if not out["speedup_may_be_claimed"]:
        out["note"] = "median of (b) is not below the minimum of (a): no speed-up claimed, both are printed"
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
