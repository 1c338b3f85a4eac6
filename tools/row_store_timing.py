"""Row store: optimize.SurveyJacobian.park_rows and the RowStore's products against what the interface offered before them for the
same Gram matrix -- sensitivity_rows to the host, then R @ (cm * R).T in numpy --, and against torch.mm (rocBLAS) on the same rows in
a device tensor, on the workload of tools/sensitivity_rows_timing.py: the bench's 128^3 grid and tri-axial model (BASELINE.json
configs[1]; F-cycle, semicoarsening + line relaxation, tol = 1e-6, colour order), 8 point dipoles, 1 frequency, 16 receivers = 256
real rows, cubic receivers with the exact adjoint, batch = 8.

  (m) the model on a 64 x 64 x 48 model grid: park_rows(mapped=True), rows of 196608 columns
  (c) the bench's model on the computational grid: park_rows(), rows of 2097152 columns (4.3 GB)
  (k) no solve: a DeviceRows of `rows` x `cols` random doubles filled from the host, each product `repeats` times -- the step to
      run under a profiler for kernel times (rocprofv3 --kernel-trace --stats -- python tools/row_store_timing.py --step k ...)

(m) and (c) run on one open SurveyJacobian each (the forward solves are not timed): host clock around calls that end in a device
synchronisation, one warm-up, median and range of `repeats`.  park_rows and sensitivity_rows both contain the same adjoint solves;
`solves_s` is their time by the solver's own clocks (per batched solve the largest 'time' of its infos), reported apart.  The gram
times are CALL times: they contain the upload of cm (gram_cm), the allocation of the slab partials and the download of G; the rates
derived from them (`gram_store_bytes_per_s` = the store's bytes once / time, against the 5.1 TB/s copy rate of DESIGN.md;
`gram_flops_per_s` with 2 n_cols flops per element of the lower triangle of 16 x 16 tiles) are therefore lower bounds of the
kernel's.  One process per step, each under a `timeout` of its own; the tool stops at the first non-zero status.

    python tools/row_store_timing.py [workload=128F] [sources=8] [repeats=3]
    python tools/row_store_timing.py --step m|c [workload] [sources] [repeats]          (one measurement, one JSON line)
    python tools/row_store_timing.py --step k [rows=256] [cols=2097152] [repeats=3]
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
MODEL_GRID = (64, 64, 48)
COPY_RATE = 5.1e12             # the device-to-device copy rate of the MI355X, bytes/s


def timed(fn, reps):
    """One warm-up, then `reps` host-clock times of fn() (every fn ends in a device synchronisation) -> (stats, last result)."""
    fn()
    ts, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        ts.append(time.perf_counter() - t0)
    return {"s_median": float(np.median(ts)), "s_min": min(ts), "s_max": max(ts)}, res


def gram_flops(n_rows, n_cols):
    nt = -(-n_rows // 16)
    return nt * (nt + 1) // 2 * 256 * 2 * n_cols


def products(store_gram, store_matvec, store_rmatvec, n_rows, n_cols, cm, v, y, reps):
    out = {}
    out["gram_cm"], G = timed(lambda: store_gram(cm), reps)
    out["gram"], G1 = timed(lambda: store_gram(None), reps)
    out["matvec"], _ = timed(lambda: store_matvec(v), reps)
    out["rmatvec_cm"], _ = timed(lambda: store_rmatvec(y, cm), reps)
    t = out["gram"]["s_median"]
    out["gram_store_bytes_per_s"] = n_rows * n_cols * 8 / t
    out["gram_share_of_copy_rate"] = out["gram_store_bytes_per_s"] / COPY_RATE
    out["gram_flops_per_s"] = gram_flops(n_rows, n_cols) / t
    return out, G, G1


def step_k(n_rows, n_cols, reps):
    import emg3d_amd as em
    rng = np.random.default_rng(3)
    cm, v, y = rng.uniform(0.5, 2., n_cols), rng.standard_normal(n_cols), rng.standard_normal(n_rows)
    with em.solver.DeviceRows(n_rows, n_cols) as rows:
        for i in range(n_rows):
            rows.set_row(i, rng.standard_normal(n_cols))
        out, G, _ = products(rows.gram, rows.matvec, rows.rmatvec, n_rows, n_cols, cm, v, y, reps)
        out.update({"step": "k", "rows": n_rows, "cols": n_cols, "plan": {k: v for k, v in em._lib.rows_gram_plan(n_rows, n_cols).items()
                                                                       if k != "jobs"}, "symmetric": bool(np.array_equal(G, G.T))})
    print(json.dumps(out))


def step(which, wl, nsrc, reps):
    import bench
    import torch
    import emg3d_amd as em
    from sensitivity_rows_timing import bench_model_on
    FREQ = 1.0
    grid, model, _, cycle = bench.build_problem(em, wl, FREQ)
    opts = dict(cycle=cycle, semicoarsening=True, linerelaxation=True, tol=1e-6, ordering='colour', verb=0,
                receiver_interpolation='cubic', adjoint='exact')
    sources = [[-700. + 200. * k, 100. * (k % 3 - 1), -100. * (k % 2), 30. + 10. * k, 10.] for k in range(nsrc)]
    k = np.arange(NREC)
    rec = (-750. + 100. * k, 60. * (k % 4) - 90., np.full(NREC, -50.), 15. * (k % 5), 5. * (k % 3))
    out = {"step": which}
    on_model = which == 'm'
    if on_model:
        ext = [(float(n[0]), float(n[-1])) for n in (grid.nodes_x, grid.nodes_y, grid.nodes_z)]
        model_grid = em.TensorMesh([np.full(n, (hi - lo) / n) for n, (lo, hi) in zip(MODEL_GRID, ext)], origin=[lo for lo, _ in ext])
        model = bench_model_on(em, grid, model_grid)
        opts['model_grid'] = model_grid
        out["model_grid"] = list(MODEL_GRID)
    rng = np.random.default_rng(3)
    with em.optimize.SurveyJacobian(grid, model, sources, [FREQ], rec, batch=8, **opts) as sj:
        held = []

        def park():
            while held:                         # one store at a time
                held.pop().close()
            held.append(sj.park_rows(mapped=on_model))
            return held[0]
        out["park_rows"], store = timed(park, reps)
        n_rows, n_cols = store.n_rows, store.rows.n_cols
        infos = [store.info[0][r] for r in range(NREC)]
        out["solves_s"] = float(sum(max(infos[r][part]['time'] for r in range(k0, min(k0 + 8, NREC)))
                                    for k0 in range(0, NREC, 8) for part in (0, 1)))
        out.update({"rows": n_rows, "cols": n_cols, "store_bytes": store.device_bytes, "handles_bytes": int(sj.device_bytes),
                    "plan": {k: v for k, v in em._lib.rows_gram_plan(n_rows, n_cols).items() if k != "jobs"}})
        vnM = store._vnM
        # cells F-ordered, as the library returns them (a C-ordered array would be re-laid out on the host at every call)
        cm, v = np.asfortranarray(rng.uniform(0.5, 2., vnM)), np.asfortranarray(rng.standard_normal(vnM))
        y = rng.standard_normal(n_rows)
        prod, G, G1 = products(store.gram, store.matvec, store.rmatvec, n_rows, n_cols, cm, v, y, reps)
        out.update(prod)
        out["gram_symmetric"] = bool(np.array_equal(G, G.T))
        # baseline 1: the rows to the host (the same solves), then numpy
        out["sensitivity_rows_to_host"], R = timed(lambda: sj.sensitivity_rows(0, mapped=on_model), reps)
        R = R.transpose(0, 1, 4, 3, 2).reshape(nsrc * NREC, -1)        # (every row is F-ordered: this is its memory order, no copy)
        R = np.stack([R.real, R.imag], axis=1).reshape(n_rows, n_cols)         # (i_src, i_rec, part): the store's order at one frequency
        out["rows_bit_for_bit"] = bool(all(np.array_equal(store.rows.get_row(i), R[i]) for i in range(0, n_rows, 37)))
        cmf = cm.ravel(order='F')
        out["numpy_gram_cm"], Gh = timed(lambda: R @ (cmf * R).T, reps)
        out["gram_max_rel_dev_numpy"] = float(np.abs(G - Gh).max() / np.abs(Gh).max())
        # baseline 2: torch.mm (rocBLAS) on the same rows in a device tensor; with cm it needs a scaled copy of the rows
        dev = torch.device("cuda", 0)
        T = torch.from_numpy(R).to(dev)
        tc = torch.from_numpy(cmf).to(dev)

        def mm(scaled):
            g = torch.mm(T * tc if scaled else T, T.T)
            torch.cuda.synchronize()
            return g
        out["torch_mm"], Gt1 = timed(lambda: mm(False), reps)
        out["torch_mm_cm"], Gt = timed(lambda: mm(True), reps)
        out["gram_max_rel_dev_torch"] = float(np.abs(G - Gt.cpu().numpy()).max() / np.abs(Gh).max())
        out["torch_symmetric"] = bool(torch.equal(Gt, Gt.T))
    print(json.dumps(out))


def main(argv):
    if argv and argv[0] == '--step':
        which, rest = argv[1], argv[2:]
        if which == 'k':
            step_k(int(rest[0]) if rest else 256, int(rest[1]) if len(rest) > 1 else 128 ** 3, int(rest[2]) if len(rest) > 2 else 3)
        else:
            step(which, rest[0] if rest else "128F", int(rest[1]) if len(rest) > 1 else 8, int(rest[2]) if len(rest) > 2 else 3)
        return 0
    wl = argv[0] if len(argv) > 0 else "128F"
    nsrc = int(argv[1]) if len(argv) > 1 else 8
    reps = int(argv[2]) if len(argv) > 2 else 3
    out = {"workload": wl, "sources": nsrc, "frequencies": 1, "receivers": NREC, "repeats": reps}
    for name, key in (('m', 'model_grid'), ('c', 'computational_grid')):
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
