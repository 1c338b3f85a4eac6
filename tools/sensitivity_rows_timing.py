"""Explicit rows of J: optimize.SurveyJacobian.sensitivity_rows against the only exact way the interface offered before it -- one
jtvec per datum and per real / imaginary part --, on the bench's 128^3 workload (BASELINE.json configs[1]: grid and tri-axial
model, F-cycle, semicoarsening + line relaxation, tol = 1e-6, colour order), 8 point dipoles, 1 frequency, 16 receivers, cubic
receivers with the exact adjoint, batch = 8.

  (m) the model on a 64 x 64 x 48 model grid over the same extent (the bench's model restated there):
      SurveyJacobian(model_grid=).sensitivity_rows(0, mapped=True) -- 32 receiver solves (e_d and i e_d per receiver) in four
      batched solves, after each per chunk of forward fields one sens_rows launch and one regrid launch pair per plane,
      model-grid-sized planes read back: 128 rows
  (c) the bench's model on the computational grid: sensitivity_rows(0) -- the same solves, one sens_rows per chunk, 128 rows of
      nC complex values on the host (4.3 GB; twice that is read back, the imaginary planes of either solve are dropped)
  (l) the jtvec loop of (m)'s object on a SUBSET of the data (`subset` of the 128: every 128 / subset-th datum), two
      jtvec(mapped=True) calls per datum; `s_per_datum` is its time per datum and `s_all_data_extrapolated` that times 128 -- an
      extrapolation, marked as such, not a measurement of the full loop

Every measurement on one open SurveyJacobian (the forward solves are not timed).  Host clock around calls that end in a device
synchronisation, one warm-up repetition, median and range of `repeats`; one process per measurement: without arguments the tool
runs the three measurements one after the other as child processes, each under a `timeout` of its own, stops at the first
non-zero status, and prints one JSON line.  (l) also compares its rows with sensitivity_rows' rows of the same data on its own
object, row against row (`rows_max_rel_dev`: largest deviation relative to the row's largest magnitude; `rows_bit_for_bit`);
`rel_dev_subset` compares the norms of (l)'s and (m)'s subsets across the two processes.

    python tools/sensitivity_rows_timing.py [workload=128F] [sources=8] [repeats=3] [subset=4]
    python tools/sensitivity_rows_timing.py --step m|c|l [workload] [sources] [repeats] [subset]     (one measurement, one JSON line)
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 420             # per measurement: open + warm-up + a few repetitions of seconds each at 128^3
NREC = 16
MODEL_GRID = (64, 64, 48)


def bench_model_on(em, grid, model_grid):
    """bench.build_problem's model, restated on ``model_grid`` (uniform cells over the extent of ``grid``)."""
    X, Y, Z = np.meshgrid(model_grid.cell_centers_x, model_grid.cell_centers_y, model_grid.cell_centers_z, indexing='ij')
    rho = np.full(model_grid.vnC, 10.0)
    rho[Z > -1000.] = 1.0
    rho[Z > 0.] = 0.3
    rho[(abs(X) < 500) & (abs(Y) < 500) & (Z > -800) & (Z < -600)] = 100.0
    rho = rho.ravel(order='F')
    return em.Model(model_grid, rho, 2 * rho, 3 * rho)


def step(which, wl, nsrc, reps, subset):
    import bench
    import emg3d_amd as em
    FREQ = 1.0
    grid, model, _, cycle = bench.build_problem(em, wl, FREQ)
    opts = dict(cycle=cycle, semicoarsening=True, linerelaxation=True, tol=1e-6, ordering='colour', verb=0,
                receiver_interpolation='cubic', adjoint='exact')
    sources = [[-700. + 200. * k, 100. * (k % 3 - 1), -100. * (k % 2), 30. + 10. * k, 10.] for k in range(nsrc)]
    k = np.arange(NREC)
    rec = (-750. + 100. * k, 60. * (k % 4) - 90., np.full(NREC, -50.), 15. * (k % 5), 5. * (k % 3))
    ndata = nsrc * NREC
    picked = np.zeros(ndata, dtype=bool)
    picked[::max(1, ndata // subset)] = True
    picked = picked.reshape(nsrc, NREC)
    out = {"step": which, "data": ndata}
    on_model = which in ('m', 'l')
    if on_model:
        ext = [(float(n[0]), float(n[-1])) for n in (grid.nodes_x, grid.nodes_y, grid.nodes_z)]
        model_grid = em.TensorMesh([np.full(n, (hi - lo) / n) for n, (lo, hi) in zip(MODEL_GRID, ext)], origin=[lo for lo, _ in ext])
        model = bench_model_on(em, grid, model_grid)
        opts['model_grid'] = model_grid
        out["model_grid"] = list(MODEL_GRID)
    with em.optimize.SurveyJacobian(grid, model, sources, [FREQ], rec, batch=8, **opts) as sj:
        def rows():
            t0 = time.perf_counter()
            r = sj.sensitivity_rows(0, mapped=on_model)
            return time.perf_counter() - t0, r

        def loop():
            t0 = time.perf_counter()
            got = []
            for i, r in zip(*np.nonzero(picked)):
                parts = []
                for unit in (1.0, 1j):
                    w = np.zeros((nsrc, 1, NREC), dtype=np.complex128)
                    w[i, 0, r] = unit
                    parts.append(sj.jtvec(w, mapped=True))
                got.append(parts[0] + 1j * parts[1])
            return time.perf_counter() - t0, np.stack(got)
        run = loop if which == 'l' else rows
        run()                                   # warm-up
        ts = []
        for _ in range(reps):
            t, r = run()
            ts.append(t)
        out.update({"s_median": float(np.median(ts)), "s_min": min(ts), "s_max": max(ts), "s_all": ts})
        if which == 'l':
            n = int(picked.sum())
            same = sj.sensitivity_rows(0, mapped=True)[picked]          # (not timed) the rows of the same data, row against row
            dev = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(same, r))
            out.update({"subset": n, "jtvec_calls": 2 * n, "s_per_datum": out["s_median"] / n,
                        "s_all_data_extrapolated": out["s_median"] / n * ndata, "norm_subset": float(np.linalg.norm(r)),
                        "rows_max_rel_dev": dev, "rows_bit_for_bit": bool(np.array_equal(same, r))})
        else:
            out.update({"rows": int(r.shape[0] * r.shape[1]), "bytes_returned": int(r.size * r.itemsize),
                        "device_bytes": int(sj.device_bytes), "it_mg": [x['it_mg'] for x in sj.rows_info],
                        "it_mg_imag": [x['it_mg'] for x in sj.rows_info_imag],
                        "norm_subset": float(np.linalg.norm(r[picked]))})
    print(json.dumps(out))


def main(argv):
    if argv and argv[0] == '--step':
        which, rest = argv[1], argv[2:]
    else:
        which, rest = None, argv
    wl = rest[0] if len(rest) > 0 else "128F"
    nsrc = int(rest[1]) if len(rest) > 1 else 8
    reps = int(rest[2]) if len(rest) > 2 else 3
    subset = int(rest[3]) if len(rest) > 3 else 4
    if which is not None:
        step(which, wl, nsrc, reps, subset)
        return 0
    out = {"workload": wl, "sources": nsrc, "frequencies": 1, "receivers": NREC, "repeats": reps}
    for name, key in (('m', 'rows_model_grid'), ('c', 'rows_computational_grid'), ('l', 'jtvec_loop_subset')):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", name, wl, str(nsrc),
               str(reps), str(subset)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:
            print(f"step ({name}) ended with status {res.returncode}: stopping here", file=sys.stderr)
            print(json.dumps(out))
            return res.returncode
        out[key] = json.loads(res.stdout.strip().splitlines()[-1])
    m, c, lp = out["rows_model_grid"], out["rows_computational_grid"], out["jtvec_loop_subset"]
    out["rel_dev_subset"] = abs(lp["norm_subset"] / m["norm_subset"] - 1)
    out["ratio_extrapolated_loop_over_rows_model_grid"] = lp["s_all_data_extrapolated"] / m["s_median"]
    out["note"] = "the loop's time for all data is extrapolated from the subset; only the subset was run"
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
