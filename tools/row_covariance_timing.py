"""Smoothing covariance of a row store: optimize.RowStore.with_covariance(inplace=True) and the gram() after it, against the host
route the interface offered before (get_row, the numpy reference of maps.SmoothingCovariance, set_row) and against a device-to-device
copy of the store times the number of active axes (the floor: per axis the store is read once and written once), all in one run.
The sizes are those of tools/row_store_timing.py: 256 rows

  (c) on the computational grid of the bench's 128^3 workload (BASELINE.json configs[1]): rows of 2097152 columns, 4.3 GB
  (m) on a uniform 64 x 64 x 48 model grid over the same extent: rows of 196608 columns
  (k) no timing table: a store of `rows` rows on grid (c) or (m), each call `repeats` times -- the step to run under a profiler for
      kernel times (rocprofv3 --kernel-trace --stats -- python tools/row_covariance_timing.py --step k c ...)

The stores are filled from the host (row i = a random row times 1 + i / n: no solve; the kernels' time does not depend on the
values), correlation lengths 400 m per axis, a standard deviation per cell.  Host clock around calls that end in a device
synchronisation, one warm-up, median and range of `repeats`.  Per axis: DeviceRows.smooth with the factors of that axis alone, so
that `share_of_copy` = (time of one copy of the store) / (time of the axis) says how near the axis is to reading and writing the store
once.  The host route is timed on `host_rows` rows and scaled to the store.  One process per step, each under a `timeout` of its
own; the tool stops at the first non-zero status.

    python tools/row_covariance_timing.py [rows=256] [repeats=3] [host_rows=8]
    python tools/row_covariance_timing.py --step c|m [rows] [repeats] [host_rows]       (one measurement, one JSON line)
    python tools/row_covariance_timing.py --step k c|m [rows] [repeats]
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
MODEL_GRID = (64, 64, 48)
LENGTHS = (400., 400., 400.)


def timed(fn, reps):
    """One warm-up, then `reps` host-clock times of fn() (every fn ends in a device synchronisation) -> (stats, last result)."""
    fn()
    ts, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        ts.append(time.perf_counter() - t0)
    return {"s_median": float(np.median(ts)), "s_min": min(ts), "s_max": max(ts)}, res


def grid_of(em, which):
    import bench
    grid = bench.build_problem(em, "128F", 1.0)[0]
    if which == 'c':
        return grid
    ext = [(float(n[0]), float(n[-1])) for n in (grid.nodes_x, grid.nodes_y, grid.nodes_z)]
    return em.TensorMesh([np.full(n, (hi - lo) / n) for n, (lo, hi) in zip(MODEL_GRID, ext)], origin=[lo for lo, _ in ext])


def filled_store(em, grid, n_rows, rng):
    """A RowStore of n_rows rows on `grid`, filled from the host; -> (store, the first row as it was set)."""
    vnC = tuple(int(n) for n in grid.vnC)
    base = rng.standard_normal(grid.nC)
    rows = em.solver.DeviceRows(n_rows, grid.nC)
    for i in range(n_rows):
        rows.set_row(i, base * (1 + i / n_rows))
    index = np.array([(0, 0, i, 0) for i in range(n_rows)], dtype=np.int64)
    return em.optimize.RowStore(rows, index, (1, 1, n_rows), vnC, False, [True]), base


def fresh(em, store):
    """The same device rows under a new RowStore (a converted store refuses a second covariance; the times do not depend on the values)."""
    return em.optimize.RowStore(store.rows, store.index, store._shape, store._vnM, store.components, store._real)


def step(which, n_rows, reps, host_rows):
    import torch
    import emg3d_amd as em
    rng = np.random.default_rng(3)
    grid = grid_of(em, which)
    vnC = tuple(int(n) for n in grid.vnC)
    std = np.asfortranarray(rng.uniform(0.5, 2., vnC))
    out = {"step": which, "grid": list(vnC), "rows": n_rows, "cols": grid.nC, "lengths_m": list(LENGTHS), "repeats": reps,
           "plan": {"xyz"[ax]: em._lib.rows_smooth_plan(vnC, ax) for ax in range(3)}}
    store, base = filled_store(em, grid, n_rows, rng)
    with store:
        nbytes = n_rows * grid.nC * 8
        out["store_bytes"] = nbytes
        # the floor: one device-to-device copy of as many bytes (read once, written once), in this run
        dev = torch.device("cuda", 0)
        a = torch.zeros(n_rows * grid.nC, dtype=torch.float64, device=dev)
        b = torch.empty_like(a)

        def copy():
            b.copy_(a)
            torch.cuda.synchronize()
        out["copy"], _ = timed(copy, reps)
        del a, b
        torch.cuda.empty_cache()
        t_copy = out["copy"]["s_median"]
        out["copy_bytes_per_s"] = 2 * nbytes / t_copy
        for passes in (1, 3):
            cov = em.maps.SmoothingCovariance(grid, LENGTHS, std=std, passes=passes)
            active = sum(f is not None for f in cov.factors)
            key = f"passes_{passes}"
            out[key] = {"active_axes": active}
            out[key]["with_covariance_inplace"], conv = timed(lambda: fresh(em, store).with_covariance(cov, inplace=True), reps)
            t = out[key]["with_covariance_inplace"]["s_median"]
            out[key]["share_of_copy_x_axes"] = active * t_copy / t
            out[key]["gram"], G = timed(conv.gram, reps)
            out[key]["gram_symmetric"] = bool(np.array_equal(G, G.T))
            for ax in range(3):
                only = [f if k == ax else None for k, f in enumerate(cov.factors)]
                name = "axis_" + "xyz"[ax]
                out[key][name], _ = timed(lambda: store.rows.smooth(vnC, 1, only, passes), reps)
                out[key][name]["share_of_copy"] = t_copy / out[key][name]["s_median"]
            out[key]["scale_and_x"], _ = timed(lambda: store.rows.smooth(vnC, 1, [cov.factors[0], None, None], passes,
                                                                         scale=cov.scale(1)), reps)
        # the host route, on `host_rows` rows: row to the host, the numpy reference, row back (passes = 1 and 3)
        store.rows.set_row(0, base)
        for passes in (1, 3):
            cov = em.maps.SmoothingCovariance(grid, LENGTHS, std=std, passes=passes)

            def host_route():
                for i in range(host_rows):
                    row = store.rows.get_row(i).reshape(vnC, order='F')
                    store.rows.set_row(i, cov.sqrt_t(row, host=True).ravel(order='F'))
            t0 = time.perf_counter()
            host_route()
            dt = time.perf_counter() - t0
            out[f"passes_{passes}"]["host_route"] = {"rows_timed": host_rows, "s": dt, "s_scaled_to_store": dt * n_rows / host_rows}
        # the device equals the host reference on a row of this size, bit for bit
        store.rows.set_row(0, base)
        want = cov.sqrt_t(base.reshape(vnC, order='F'), host=True).ravel(order='F')
        with em.solver.DeviceRows(1, grid.nC) as one:
            one.set_row(0, base)
            one.smooth(vnC, 1, cov.factors, cov.passes, scale=cov.scale(1))
            out["row_bit_for_bit"] = bool(np.array_equal(one.get_row(0), want))
    print(json.dumps(out))


def step_k(which, n_rows, reps):
    import emg3d_amd as em
    rng = np.random.default_rng(3)
    grid = grid_of(em, which)
    vnC = tuple(int(n) for n in grid.vnC)
    std = np.asfortranarray(rng.uniform(0.5, 2., vnC))
    store, _ = filled_store(em, grid, n_rows, rng)
    with store:
        for passes in (1, 3):
            cov = em.maps.SmoothingCovariance(grid, LENGTHS, std=std, passes=passes)
            for _ in range(reps + 1):
                conv = fresh(em, store).with_covariance(cov, inplace=True)
            for _ in range(reps + 1):
                conv.gram()
    print(json.dumps({"step": "k", "grid": list(vnC), "rows": n_rows, "repeats": reps}))


def main(argv):
    if argv and argv[0] == '--step':
        which, rest = argv[1], argv[2:]
        if which == 'k':
            step_k(rest[0] if rest else 'c', int(rest[1]) if len(rest) > 1 else 256, int(rest[2]) if len(rest) > 2 else 3)
        else:
            step(which, int(rest[0]) if rest else 256, int(rest[1]) if len(rest) > 1 else 3, int(rest[2]) if len(rest) > 2 else 8)
        return 0
    n_rows = int(argv[0]) if len(argv) > 0 else 256
    reps = int(argv[1]) if len(argv) > 1 else 3
    host_rows = int(argv[2]) if len(argv) > 2 else 8
    out = {"rows": n_rows, "repeats": reps}
    for name, key in (('m', 'model_grid'), ('c', 'computational_grid')):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", name, str(n_rows), str(reps),
               str(host_rows)]
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
