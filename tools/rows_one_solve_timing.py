"""Rows of J from one adjoint solve per receiver: optimize.SurveyJacobian.park_rows and sensitivity_rows with solves=1 against the
default solves=2 (the parent's path, unchanged), on the workload of tools/row_store_timing.py: the bench's 128^3 grid and tri-axial
model (BASELINE.json configs[1]; F-cycle, semicoarsening + line relaxation, tol = 1e-6, colour order), 8 point dipoles, 1 frequency,
16 receivers = 256 real rows, cubic receivers with the exact adjoint, batch = 8.

  (c) the bench's model on the computational grid: rows of 2097152 columns; solves=1 fills the store from the fields in one launch
      per chunk (k_sens_rows_fill), solves=2 goes through the handle's row buffer (k_sens_rows, then k_rows_park)
  (m) the model on a 64 x 64 x 48 model grid: rows of 196608 columns; both forms regrid plane by plane and park

Each step runs on one open SurveyJacobian (the forward solves are not timed): host clock around calls that end in a device
synchronisation, one warm-up of each form, then the two forms ALTERNATING in the same process, median and range of `repeats`.
`solves_s` is the time of the adjoint solves by the solver's own clocks (per batched solve the largest 'time' of its infos), reported
apart.  `handles_bytes` is SurveyJacobian.device_bytes after the first park of each form -- solves=1 first, on the fresh object, so
that its figure is free of the row buffer solves=2 then allocates.  `gap` is the largest |Im rows(solves=1) - Im rows(solves=2)|
relative to the row's largest magnitude, `trunc` the same between solves=2 at tol and solves=2 at tol / 1000 on a second object: what
the one-solve form changes, against what the default's own second solve leaves undetermined.

A speed-up is CLAIMED only where the median of solves=1 lies below the minimum of solves=2's runs (`faster`); the tool prints both
and says so otherwise.  One process per step, each under a `timeout` of its own; the tool stops at the first non-zero status.

    python tools/rows_one_solve_timing.py [workload=128F] [sources=8] [repeats=3]
    python tools/rows_one_solve_timing.py --step c|m [workload] [sources] [repeats]         (one measurement, one JSON line)
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
STEP_LIMIT_S = 540
NREC = 16
BATCH = 8
MODEL_GRID = (64, 64, 48)


def stats(ts):
    return {"s_median": float(np.median(ts)), "s_min": float(min(ts)), "s_max": float(max(ts))}


def alternating(fns, reps):
    """One warm-up of every fn, then `reps` rounds in which each runs once, in turn (every fn ends in a device synchronisation) ->
    ({name: stats}, {name: last result})."""
    last = {name: fn() for name, fn in fns.items()}
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            last[name] = fn()
            ts[name].append(time.perf_counter() - t0)
    return {name: stats(t) for name, t in ts.items()}, last


def verdict(out, what):
    """Claim a speed-up only if the median of solves=1 lies below the minimum of solves=2's runs."""
    one, two = out[what + "_solves1"], out[what + "_solves2"]
    faster = one["s_median"] < two["s_min"]
    out[what + "_faster"] = bool(faster)
    out[what + "_ratio_of_medians"] = two["s_median"] / one["s_median"]
    msg = (f"{what}: solves=1 median {one['s_median']:.3f} s (range {one['s_min']:.3f} .. {one['s_max']:.3f}), solves=2 median "
           f"{two['s_median']:.3f} s (range {two['s_min']:.3f} .. {two['s_max']:.3f}): ")
    msg += (f"solves=1 is faster, {out[what + '_ratio_of_medians']:.2f} x by the medians" if faster else
            "NO speed-up is claimed (the median of solves=1 is not below the minimum of solves=2)")
    print(msg, file=sys.stderr)


def solves_time(info, parts):
    return float(sum(max(info[r][part]['time'] for r in range(k0, min(k0 + BATCH, NREC)))
                     for k0 in range(0, NREC, BATCH) for part in parts))


def imag_gap(a, b):
    size = np.abs(b).reshape(b.shape[:2] + (-1,)).max(axis=2)
    return float((np.abs(a.imag - b.imag).reshape(b.shape[:2] + (-1,)).max(axis=2) / size).max())


def step(which, wl, nsrc, reps):
    import bench
    import emg3d_amd as em
    from sensitivity_rows_timing import bench_model_on
    FREQ, TOL = 1.0, 1e-6
    grid, model, _, cycle = bench.build_problem(em, wl, FREQ)
    opts = dict(cycle=cycle, semicoarsening=True, linerelaxation=True, ordering='colour', verb=0, receiver_interpolation='cubic',
                adjoint='exact')
    sources = [[-700. + 200. * k, 100. * (k % 3 - 1), -100. * (k % 2), 30. + 10. * k, 10.] for k in range(nsrc)]
    k = np.arange(NREC)
    rec = (-750. + 100. * k, 60. * (k % 4) - 90., np.full(NREC, -50.), 15. * (k % 5), 5. * (k % 3))
    out = {"step": which, "tol": TOL}
    on_model = which == 'm'
    if on_model:
        ext = [(float(n[0]), float(n[-1])) for n in (grid.nodes_x, grid.nodes_y, grid.nodes_z)]
        model_grid = em.TensorMesh([np.full(n, (hi - lo) / n) for n, (lo, hi) in zip(MODEL_GRID, ext)], origin=[lo for lo, _ in ext])
        model = bench_model_on(em, grid, model_grid)
        opts['model_grid'] = model_grid
        out["model_grid"] = list(MODEL_GRID)
    with em.optimize.SurveyJacobian(grid, model, sources, [FREQ], rec, batch=BATCH, tol=TOL, **opts) as sj:
        held = []

        def park(solves):
            while held:                         # one store at a time
                held.pop().close()
            held.append(sj.park_rows(mapped=on_model, solves=solves))
            return held[0]
        out["handles_bytes_fresh"] = int(sj.device_bytes)
        park(1)
        out["handles_bytes_solves1"] = int(sj.device_bytes)
        park(2)
        out["handles_bytes_solves2"] = int(sj.device_bytes)
        solves_s = {1: [], 2: []}

        def timed_park(solves):
            store = park(solves)
            solves_s[solves].append(solves_time(store.info[0], (0,) if solves == 1 else (0, 1)))
            return store
        t, last = alternating({"park_rows_solves2": lambda: timed_park(2), "park_rows_solves1": lambda: timed_park(1)}, reps)
        out.update(t)
        for s in (1, 2):
            out[f"solves_s_solves{s}"] = stats(solves_s[s][1:])            # (without the warm-up)
        store = last["park_rows_solves1"]
        out.update({"rows": store.n_rows, "cols": store.rows.n_cols, "store_bytes": store.device_bytes})
        verdict(out, "park_rows")
        t, rows = alternating({"sensitivity_rows_solves2": lambda: sj.sensitivity_rows(0, mapped=on_model, solves=2),
                               "sensitivity_rows_solves1": lambda: sj.sensitivity_rows(0, mapped=on_model, solves=1)}, reps)
        out.update(t)
        verdict(out, "sensitivity_rows")
        one, two = rows["sensitivity_rows_solves1"], rows["sensitivity_rows_solves2"]
        out["real_parts_bit_for_bit"] = bool(np.array_equal(one.real, two.real))
        R = one.transpose(0, 1, 4, 3, 2).reshape(nsrc * NREC, -1)       # (every row is F-ordered: this is its memory order, no copy)
        out["parked_bit_for_bit"] = bool(all(np.array_equal(store.rows.get_row(i), (R[i // 2].real, R[i // 2].imag)[i % 2])
                                             for i in range(0, store.n_rows, 37)))
        out["gap"] = imag_gap(one, two)
        del one, R, rows
        while held:
            held.pop().close()
    with em.optimize.SurveyJacobian(grid, model, sources, [FREQ], rec, batch=BATCH, tol=TOL / 1000, **opts) as sj:
        tight = sj.sensitivity_rows(0, mapped=on_model, solves=2)
        out["tight_exits"] = sorted({int(x['exit']) for x in sj.rows_info + sj.rows_info_imag})
        out["trunc"] = imag_gap(two, tight)
    out["gap_within_trunc"] = bool(out["gap"] <= out["trunc"])
    print(json.dumps(out))


def main(argv):
    if argv and argv[0] == '--step':
        which, rest = argv[1], argv[2:]
        step(which, rest[0] if rest else "128F", int(rest[1]) if len(rest) > 1 else 8, int(rest[2]) if len(rest) > 2 else 3)
        return 0
    wl = argv[0] if len(argv) > 0 else "128F"
    nsrc = int(argv[1]) if len(argv) > 1 else 8
    reps = int(argv[2]) if len(argv) > 2 else 3
    out = {"workload": wl, "sources": nsrc, "frequencies": 1, "receivers": NREC, "batch": BATCH, "repeats": reps}
    for name, key in (('c', 'computational_grid'), ('m', 'model_grid')):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", name, wl, str(nsrc), str(reps)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:
            print(f"step ({name}) ended with status {res.returncode}: stopping here", file=sys.stderr)
            print(json.dumps(out))
            return res.returncode
        out[key] = json.loads(res.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
