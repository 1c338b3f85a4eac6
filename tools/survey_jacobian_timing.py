"""Gauss-Newton product of a survey, H v = J^T W J v: optimize.SurveyJacobian against one optimize.Jacobian per (source,
frequency) pair, on the bench's 128^3 workload (BASELINE.json configs[1]: grid and tri-axial model, F-cycle, semicoarsening +
line relaxation, tol = 1e-6, colour order), 8 point dipoles, 1 frequency, 16 receivers, cubic receivers with the exact adjoint,
W = 1 / (0.05 |data|)^2, a random perturbation v of sigma_x = sigma_y = sigma_z.

  (a) one Jacobian per pair: jtvec(W_i * jvec(v)) per pair, the results added on the host -- a handle, a hierarchy, a forward
      solve and an nC-sized download per pair, every product solve one system at a time
  (b) SurveyJacobian(batch=8).gauss_newton(v, W): one handle, batched solves, the sum over the sources formed on the device
  (c) SurveyJacobian(batch=1).gauss_newton(v, W): one handle, one system at a time

Every repetition is timed in two parts: `open` (handles, forward solves, data -- paid once per outer iteration of an inversion)
and `product` (one H v with everything open -- paid once per inner CG step; for (a) all eight Jacobians are open at the same time);
`total` is their sum, one H v from scratch.
Host clock around calls that end in a device synchronisation, one warm-up repetition, median and range of five, one process per
measurement: without arguments the tool runs the three measurements one after the other as child processes, each under a
`timeout` of its own, stops at the first non-zero status, and prints one JSON line with the results and whether a speed-up may
be claimed, per part: only if the median of (b) lies below the minimum of (a)'s five runs.

    python tools/survey_jacobian_timing.py [workload=128F] [sources=8] [repeats=5]
    python tools/survey_jacobian_timing.py --step a|b|c [workload] [sources] [repeats]      (one measurement, one JSON line)
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 420             # per measurement: warm-up + five repetitions of a few seconds each at 128^3


def step(which, wl, nsrc, reps):
    import bench
    import emg3d_amd as em
    FREQ = 1.0
    grid, model, _, cycle = bench.build_problem(em, wl, FREQ)
    opts = dict(cycle=cycle, semicoarsening=True, linerelaxation=True, tol=1e-6, ordering='colour', verb=0,
                receiver_interpolation='cubic', adjoint='exact')
    sources = [[-700. + 200. * k, 100. * (k % 3 - 1), -100. * (k % 2), 30. + 10. * k, 10.] for k in range(nsrc)]
    k = np.arange(16)
    rec = (-750. + 100. * k, 60. * (k % 4) - 90., np.full(16, -50.), 15. * (k % 5), 5. * (k % 3))
    rng = np.random.default_rng(9)
    sig = 1.0 / np.asarray(model.property_x).ravel(order='F')           # (the bench's model holds resistivities)
    v = (rng.standard_normal(grid.nC) * sig * 0.3).reshape(grid.vnC, order='F')

    def weights_of(syn):
        return 1.0 / (0.05 * np.abs(syn)) ** 2

    def pairs():
        t0 = time.perf_counter()
        jacs = [em.optimize.Jacobian(grid, model, src, FREQ, rec, **opts) for src in sources]
        try:
            for jac in jacs:
                jac.open()
            t1 = time.perf_counter()
            hv = np.zeros(grid.vnC, order='F')
            its = []
            for jac in jacs:
                jv = jac.jvec(v)
                it = jac.info['it_mg']
                hv = hv + jac.jtvec(weights_of(jac.synthetic) * jv)
                its.append((it, jac.info['it_mg']))
            t2 = time.perf_counter()
        finally:
            for jac in jacs:
                jac.close()
        return t1 - t0, t2 - t1, hv, its

    def survey(batch):
        t0 = time.perf_counter()
        with em.optimize.SurveyJacobian(grid, model, sources, [FREQ], rec, batch=batch, **opts) as sj:
            t1 = time.perf_counter()
            hv = sj.gauss_newton(v, weights_of(sj.synthetic))
            t2 = time.perf_counter()
            its = [(sj.jvec_info[i][0]['it_mg'], sj.info[i][0]['it_mg']) for i in range(nsrc)]
        return t1 - t0, t2 - t1, hv, its

    run = {'a': pairs, 'b': lambda: survey(8), 'c': lambda: survey(1)}[which]
    run()                                       # warm-up: library, device pool, first set-up
    t_open, t_prod = [], []
    for _ in range(reps):
        a, b, hv, its = run()
        t_open.append(a)
        t_prod.append(b)

    def stats(t):
        return {"s_median": float(np.median(t)), "s_min": min(t), "s_max": max(t), "s_all": t}
    print(json.dumps({"step": which, "open": stats(t_open), "product": stats(t_prod),
                      "total": stats([a + b for a, b in zip(t_open, t_prod)]), "hv_norm": float(np.linalg.norm(hv)),
                      "it_mg": its}))


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
    for name, key in (('a', 'jacobian_per_pair'), ('b', 'survey_jacobian_batch8'), ('c', 'survey_jacobian_batch1')):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", name, wl, str(nsrc),
               str(reps)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:
            print(f"step ({name}) ended with status {res.returncode}: stopping here", file=sys.stderr)
            print(json.dumps(out))
            return res.returncode
        out[key] = json.loads(res.stdout.strip().splitlines()[-1])
    a, b, c = out["jacobian_per_pair"], out["survey_jacobian_batch8"], out["survey_jacobian_batch1"]
    out["same_iterations"] = a["it_mg"] == b["it_mg"] == c["it_mg"]
    out["hv_rel_dev_b_vs_a"] = abs(b["hv_norm"] / a["hv_norm"] - 1)
    for part in ("open", "product", "total"):
        out[f"{part}_ms_per_pair"] = {s: 1e3 * r[part]["s_median"] / nsrc for s, r in (("a", a), ("b", b), ("c", c))}
        out[f"{part}_speedup_may_be_claimed"] = b[part]["s_median"] < a[part]["s_min"]
        out[f"{part}_ratio_median_a_over_b"] = a[part]["s_median"] / b[part]["s_median"]
    if not all(out[f"{part}_speedup_may_be_claimed"] for part in ("open", "product", "total")):
        out["note"] = "where the median of (b) is not below the minimum of (a) no speed-up is claimed; both are printed"
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
