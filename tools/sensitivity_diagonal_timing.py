"""Survey sensitivity diagonal, diag(J^H W J): optimize.SurveyJacobian.sensitivity_diagonal against the only exact way the
interface offered before it -- one jtvec per datum and per real / imaginary part --, on the bench's 128^3 workload (BASELINE.json
configs[1]: grid and tri-axial model, F-cycle, semicoarsening + line relaxation, tol = 1e-6, colour order), 8 point dipoles,
1 frequency, 16 receivers, cubic receivers with the exact adjoint, W = 1 / (0.05 |data|)^2.

  (a) SurveyJacobian(batch=8).sensitivity_diagonal(W): 16 receiver solves in two batched solves, one sens_acc_add each, one
      nC-sized read-back
  (b) the jtvec loop on a SUBSET of the data (`subset` of the 128: every 128 / subset-th datum), two jtvec calls per datum on the
      same open SurveyJacobian, squared and added on the host; `s_per_datum` is its time per datum and `s_all_data_extrapolated`
      that times 128 -- an extrapolation, marked as such, not a measurement of the full loop

Both on one open SurveyJacobian (the forward solves are not timed).  Host clock around calls that end in a device synchronisation,
one warm-up repetition, median and range of `repeats`; one process per measurement: without arguments the tool runs the two
measurements one after the other as child processes, each under a `timeout` of its own, stops at the first non-zero status, and
prints one JSON line.  (b)'s subset sum is also compared with (a) restricted to the same data (`rel_dev_subset`).

    python tools/sensitivity_diagonal_timing.py [workload=128F] [sources=8] [repeats=3] [subset=4]
    python tools/sensitivity_diagonal_timing.py --step a|b [workload] [sources] [repeats] [subset]     (one measurement, one JSON line)
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
    picked = picked.reshape(nsrc, 1, NREC)
    out = {"step": which, "data": ndata}
    with em.optimize.SurveyJacobian(grid, model, sources, [FREQ], rec, batch=8, **opts) as sj:
        W = 1.0 / (0.05 * np.abs(sj.synthetic)) ** 2
        Ws = W * picked

        def diagonal():
            t0 = time.perf_counter()
            d = sj.sensitivity_diagonal(W)
            return time.perf_counter() - t0, d

        def rows():
            t0 = time.perf_counter()
            d = np.zeros(grid.vnC, order='F')
            for i, _, r in zip(*np.nonzero(picked)):
                for unit in (1.0, 1j):
                    w = np.zeros(W.shape, dtype=np.complex128)
                    w[i, 0, r] = unit
                    g = sj.jtvec(w)
                    d = d + W[i, 0, r] * g * g
            return time.perf_counter() - t0, d
        run = diagonal if which == 'a' else rows
        run()                                   # warm-up
        ts = []
        for _ in range(reps):
            t, d = run()
            ts.append(t)
        out.update({"s_median": float(np.median(ts)), "s_min": min(ts), "s_max": max(ts), "s_all": ts, "norm": float(np.linalg.norm(d))})
        if which == 'a':
            out["receiver_solves"] = sum(x is not None for x in sj.sensitivity_info[0])
            out["it_mg"] = [x['it_mg'] for x in sj.sensitivity_info[0]]
            out["norm_subset"] = float(np.linalg.norm(sj.sensitivity_diagonal(Ws)))
        else:
            n = int(picked.sum())
            out.update({"subset": n, "jtvec_calls": 2 * n, "s_per_datum": out["s_median"] / n,
                        "s_all_data_extrapolated": out["s_median"] / n * ndata})
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
    for name, key in (('a', 'sensitivity_diagonal'), ('b', 'jtvec_loop_subset')):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", name, wl, str(nsrc),
               str(reps), str(subset)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:
            print(f"step ({name}) ended with status {res.returncode}: stopping here", file=sys.stderr)
            print(json.dumps(out))
            return res.returncode
        out[key] = json.loads(res.stdout.strip().splitlines()[-1])
    a, b = out["sensitivity_diagonal"], out["jtvec_loop_subset"]
    out["rel_dev_subset"] = abs(b["norm"] / a["norm_subset"] - 1)
    out["ratio_extrapolated_loop_over_diagonal"] = b["s_all_data_extrapolated"] / a["s_median"]
    out["note"] = "the loop's time for all data is extrapolated from the subset; only the subset was run"
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
