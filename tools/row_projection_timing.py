"""A small dense matrix times the row store: DeviceRows.project (k_rows_project), DeviceRows.colsumsq and
optimize.RowStore.posterior_variance (on a plain store and on a with_covariance store), against three references taken in the same
run:

  (a) the traffic floor: project reads the source once per block of output rows and writes the result once, `passes * src + dst`
      bytes; a device-to-device copy of the store moves 2 * src bytes, and the floor is that traffic at the copy's bytes per second;
  (b) rocBLAS: torch.mm(M, T) on device tensors of the same sizes (T a tensor of the store's size, not the store);
  (c) the route through the host the interface offered before: get_row for every source row, numpy (one axpy per output row),
      set_row for every result row -- timed on `host_rows` source rows and as many output rows, each part scaled to the store.

The sizes are those of tools/row_store_timing.py: 256 rows

  (c) on the computational grid of the bench's 128^3 workload (BASELINE.json configs[1]): rows of 2097152 columns, 4.3 GB
  (m) on a uniform 64 x 64 x 48 model grid over the same extent: rows of 196608 columns

with m = 256 and m = 32 output rows.  The stores are filled from the host (row i = a random row times 1 + i / n plus a second random
row times i mod 7: no solve; the kernels' time does not depend on the values).  Host clock around calls that end in a device
synchronisation, one warm-up, median and range of `repeats`.  One process per step, each under a `timeout` of its own; the tool
stops at the first non-zero status.

    python tools/row_projection_timing.py [rows=256] [repeats=3] [host_rows=8]
    python tools/row_projection_timing.py --step c|m [rows] [repeats] [host_rows]       (one measurement, one JSON line)
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
from row_covariance_timing import LENGTHS, STEP_LIMIT_S, grid_of, timed  # noqa: E402

M_ROWS = (256, 32)


def filled_store(em, grid, n_rows, rng):
    vnC = tuple(int(n) for n in grid.vnC)
    a, b = rng.standard_normal(grid.nC), rng.standard_normal(grid.nC)
    rows = em.solver.DeviceRows(n_rows, grid.nC)
    for i in range(n_rows):
        rows.set_row(i, a * (1 + i / n_rows) + b * (i % 7))
    index = np.array([(0, 0, i, 0) for i in range(n_rows)], dtype=np.int64)
    return em.optimize.RowStore(rows, index, (1, 1, n_rows), vnC, False, [True])


def step(which, n_rows, reps, host_rows):
    import torch
    import emg3d_amd as em
    rng = np.random.default_rng(3)
    grid = grid_of(em, which)
    vnC = tuple(int(n) for n in grid.vnC)
    n_cols = grid.nC
    out = {"step": which, "grid": list(vnC), "rows": n_rows, "cols": n_cols, "repeats": reps}
    store = filled_store(em, grid, n_rows, rng)
    with store:
        nbytes = n_rows * n_cols * 8
        out["store_bytes"] = nbytes
        dev = torch.device("cuda", 0)
        a = torch.zeros(n_rows * n_cols, dtype=torch.float64, device=dev)
        b = torch.empty_like(a)

        def copy():
            b.copy_(a)
            torch.cuda.synchronize()
        out["copy"], _ = timed(copy, reps)
        del b
        bytes_per_s = 2 * nbytes / out["copy"]["s_median"]
        out["copy_bytes_per_s"] = bytes_per_s
        T = a.view(n_rows, n_cols).normal_()
        for m in M_ROWS:
            key = f"m_{m}"
            plan = em._lib.rows_project_plan(n_rows, m, n_cols)
            M = rng.standard_normal((m, n_rows))
            res = out[key] = {"plan": plan, "flops": 2.0 * m * n_rows * n_cols}
            with em.solver.DeviceRows(m, n_cols) as dst:
                res["project"], _ = timed(lambda: store.rows.project(M, out=dst), reps)
                first = dst.get_row(m - 1)
                store.rows.project(M, out=dst)
                res["same_bits_twice"] = bool(first.tobytes() == dst.get_row(m - 1).tobytes())
                res["colsumsq_of_result"], _ = timed(dst.colsumsq, reps)
            t = res["project"]["s_median"]
            res["flops_per_s"] = res["flops"] / t
            traffic = plan["passes"] * nbytes + m * n_cols * 8
            res["copy_floor_s"] = traffic / bytes_per_s
            res["project_over_floor"] = t / res["copy_floor_s"]
            Mt = torch.from_numpy(M).to(dev)
            Y = torch.empty((m, n_cols), dtype=torch.float64, device=dev)

            def mm():
                torch.mm(Mt, T, out=Y)
                torch.cuda.synchronize()
            res["torch_mm"], _ = timed(mm, reps)
            res["project_over_torch_mm"] = t / res["torch_mm"]["s_median"]
            del Y, Mt
            # the route through the host, its three parts scaled to the store
            hr = min(host_rows, n_rows)
            mh = min(m, hr)
            t0 = time.perf_counter()
            rows = [store.rows.get_row(i) for i in range(hr)]
            t1 = time.perf_counter()
            acc = np.zeros((mh, n_cols))
            for i, row in enumerate(rows):
                for k in range(mh):
                    acc[k] += M[k, i] * row
            t2 = time.perf_counter()
            with em.solver.DeviceRows(mh, n_cols) as back:
                t3 = time.perf_counter()
                for k in range(mh):
                    back.set_row(k, acc[k])
                t4 = time.perf_counter()
            res["host_route"] = {"rows_timed": hr, "out_rows_timed": mh, "s_get": t1 - t0, "s_numpy": t2 - t1, "s_set": t4 - t3,
                                 "s_scaled_to_store": (t1 - t0) * n_rows / hr + (t2 - t1) * (n_rows * m) / (hr * mh) + (t4 - t3) * m / mh}
            del rows, acc
        del a, T
        torch.cuda.empty_cache()
        out["colsumsq"], _ = timed(store.rows.colsumsq, reps)
        out["colsumsq_share_of_copy"] = (nbytes / bytes_per_s) / out["colsumsq"]["s_median"]
        # the diagnostics: a plain store, then the same rows under a smoothing covariance (converted in place)
        w = np.ones(n_rows)
        G = store.gram()
        damping = 1e-3 * float(np.trace(G)) / n_rows
        out["gram"], _ = timed(store.gram, reps)
        out["posterior_variance_plain"], pv = timed(lambda: store.posterior_variance(w, damping=damping), reps)
        out["resolution_diagonal_plain"], rd = timed(lambda: store.resolution_diagonal(w, damping=damping), reps)
        out["plain_range"] = [float(pv.min()), float(pv.max()), float(rd.min()), float(rd.max())]
        std = np.asfortranarray(rng.uniform(0.5, 2., vnC))
        cov = em.maps.SmoothingCovariance(grid, LENGTHS, std=std, passes=1)
        out["cov_diagonal_host"], prior = timed(cov.diagonal, 1)
        conv = store.with_covariance(cov, inplace=True)
        damping = 1e-3 * float(np.trace(conv.gram())) / n_rows
        out["posterior_variance_covariance"], pv = timed(lambda: conv.posterior_variance(w, damping=damping), reps)
        out["covariance_range_over_prior"] = [float((pv / prior).min()), float((pv / prior).max())]
    print(json.dumps(out))


def main(argv):
    if argv and argv[0] == '--step':
        which, rest = argv[1], argv[2:]
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
