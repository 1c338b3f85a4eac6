"""What reading the gradient back on the model grid costs per frequency: the bench's 128^3 grid (BASELINE.json configs[1]: F-cycle,
semicoarsening + line relaxation, tol = 1e-6, colour order) as the computational grid, an isotropic layered resistivity model on a
64 x 64 x 48 model grid over the same extent (uniform cells: no interior edge is shared with the stretched grid), 8 point dipoles,
1 frequency, 16 receivers, batch = 8.  A ``SurveyJacobian(model_grid=)`` is opened and one ``jtvec`` run, so that the accumulator
of the handle holds the sum over the 8 sources; then, on that handle,

  (a) ``grad_acc_get()`` plus the host's map to the model grid -- what there was before: ``nC`` doubles cross PCIe, then
      ``optimize.model_gradient(grid, model, grad, model_grid)`` (the reference's cubic interpolation, which uploads them again);
  (a') the same download plus ``model_gradient(..., method='transpose')`` (the exact operator through the stateless call);
  (b) ``grad_acc_get_model()``: k_regrid_scale + k_volume_average_adjoint on the resident tables and factors, ``nM`` doubles back.

(a) and (b) do not compute the same thing ((a) is not the derivative with respect to the model cells; (a') and (b) agree to
rounding, which the tool checks): the tool compares what a user pays per frequency for a gradient on the model grid.  No threshold
is attached.  Host clock around calls that end in a device synchronisation, one warm-up repetition, median and range of five; the
measurement runs as a child process under a `timeout` of its own, and the tool prints one JSON line.

    python tools/model_grid_timing.py [workload=128F] [sources=8] [repeats=5]
    python tools/model_grid_timing.py --step [workload] [sources] [repeats]           (the measurement itself, one JSON line)
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 420             # open (8 forward solves) + one jtvec (8 more) at 128^3, then 3 x 6 read-backs
MODEL_CELLS = (64, 64, 48)


def step(wl, nsrc, reps):
    import bench
    import emg3d_amd as em
    FREQ = 1.0
    grid, _, _, cycle = bench.build_problem(em, wl, FREQ)
    edges = [np.linspace(e[0], e[-1], n + 1) for e, n in zip((grid.nodes_x, grid.nodes_y, grid.nodes_z), MODEL_CELLS)]
    model_grid = em.TensorMesh([np.diff(e) for e in edges], origin=[e[0] for e in edges])
    _, _, Z = np.meshgrid(model_grid.cell_centers_x, model_grid.cell_centers_y, model_grid.cell_centers_z, indexing='ij')
    rho = np.full(model_grid.vnC, 10.0)
    rho[Z > -1000.] = 1.0
    rho[Z > 0.] = 0.3
    model = em.Model(model_grid, rho.ravel(order='F'))
    opts = dict(cycle=cycle, semicoarsening=True, linerelaxation=True, tol=1e-6, ordering='colour', verb=0)
    sources = [[-700. + 200. * k, 100. * (k % 3 - 1), -100. * (k % 2), 30. + 10. * k, 10.] for k in range(nsrc)]
    k = np.arange(16)
    rec = (-750. + 100. * k, 60. * (k % 4) - 90., np.full(16, -50.), 15. * (k % 5), 5. * (k % 3))
    rng = np.random.default_rng(0)
    t = {'get_plus_cubic': [], 'get_plus_transpose': [], 'get_model': []}
    with em.optimize.SurveyJacobian(grid, model, sources, [FREQ], rec, batch=nsrc, model_grid=model_grid, **opts) as sj:
        w = (rng.standard_normal(sj.synthetic.shape) + 1j * rng.standard_normal(sj.synthetic.shape)) / np.abs(sj.synthetic)
        sj.jtvec(w, mapped=True)
        its = [sj.info[i][0]['it_mg'] for i in range(nsrc)]
        dev = next(iter(sj._held))
        for r in range(reps + 1):
            t0 = time.perf_counter()
            g = dev.grad_acc_get().reshape(grid.vnC, order='F')
            cubic = em.optimize.model_gradient(grid, model, g, model_grid)
            t1 = time.perf_counter()
            g = dev.grad_acc_get().reshape(grid.vnC, order='F')
            exact = em.optimize.model_gradient(grid, model, g, model_grid, method='transpose')
            t2 = time.perf_counter()
            gm = dev.grad_acc_get_model().reshape(model_grid.vnC, order='F')
            t3 = time.perf_counter()
            t['get_plus_cubic'].append(t1 - t0); t['get_plus_transpose'].append(t2 - t1); t['get_model'].append(t3 - t2)
        # model_gradient works on -grad, the handle on the accumulator as it is
        agree = float(np.abs(exact + gm).max() / np.abs(gm).max())
        far = float(np.abs(cubic + gm).max() / np.abs(gm).max())
        bytes_ = sj.device_bytes
    out = {"it_mg": its, "nC": int(grid.nC), "nM": int(model_grid.nC), "device_bytes": int(bytes_),
           "transpose_vs_get_model_rel": agree, "cubic_vs_get_model_rel": far}
    for key, v in t.items():
        v = v[1:]                               # (the first repetition is the warm-up)
        out[key] = {"s_median": float(np.median(v)), "s_min": min(v), "s_max": max(v), "s_all": v}
    print(json.dumps(out))


def main(argv):
    child = bool(argv) and argv[0] == '--step'
    rest = argv[1:] if child else argv
    wl = rest[0] if len(rest) > 0 else "128F"
    nsrc = int(rest[1]) if len(rest) > 1 else 8
    reps = int(rest[2]) if len(rest) > 2 else 5
    if child:
        step(wl, nsrc, reps)
        return 0
    out = {"workload": wl, "model_cells": list(MODEL_CELLS), "sources": nsrc, "frequencies": 1, "receivers": 16, "repeats": reps}
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", wl, str(nsrc), str(reps)]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if res.returncode != 0:
        print(f"the measurement ended with status {res.returncode}", file=sys.stderr)
        print(json.dumps(out))
        return res.returncode
    out.update(json.loads(res.stdout.strip().splitlines()[-1]))
    out["readback_ms"] = {k: 1e3 * out[k]["s_median"] for k in ("get_plus_cubic", "get_plus_transpose", "get_model")}
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
