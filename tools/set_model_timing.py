"""What SurveyJacobian.set_model saves: presenting a SECOND model to a survey whose handles are open, on the bench's 128^3
workload (BASELINE.json configs[1]: grid and tri-axial model, F-cycle, semicoarsening + line relaxation, tol = 1e-6, colour
order), 8 point dipoles, 1 frequency, 16 receivers, batch = 8.  The two models alternate: the bench's model and the same with
every resistivity scaled by a smooth factor between 0.8 and 1.25 (what a model update of an inversion looks like).

  (a) close the SurveyJacobian and open a new one on the other model -- what there was before set_model: handle, hierarchies,
      transfer weights, work buffers, launch graphs, the level-0 placement and the parked field vectors are made again
  (b) SurveyJacobian.set_model(other model) on the open one
  (c) the forward solves alone: one batched solve_sources of the 8 sources on an open handle that stands at the model already
      (sources built in HBM, fields left there) -- the part of (a) and (b) that no re-targeting can save

Both (a) and (b) contain (c) plus the data extraction; the tool prints (a) - (c) against (b) - (c), the price of presenting the
model.  No threshold is attached.  Host clock around calls that end in a device synchronisation, one warm-up repetition, median
and range of five, one process per measurement: without arguments the tool runs the three measurements one after the other as
child processes, each under a `timeout` of its own, stops at the first non-zero status, and prints one JSON line.

    python tools/set_model_timing.py [workload=128F] [sources=8] [repeats=5]
    python tools/set_model_timing.py --step a|b|c [workload] [sources] [repeats]      (one measurement, one JSON line)
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 300             # per measurement: warm-up + five repetitions of about a second each at 128^3


def step(which, wl, nsrc, reps):
    import bench
    import emg3d_amd as em
    from emg3d_amd import models
    FREQ = 1.0
    grid, model, _, cycle = bench.build_problem(em, wl, FREQ)
    opts = dict(cycle=cycle, semicoarsening=True, linerelaxation=True, tol=1e-6, ordering='colour', verb=0)
    sources = [[-700. + 200. * k, 100. * (k % 3 - 1), -100. * (k % 2), 30. + 10. * k, 10.] for k in range(nsrc)]
    k = np.arange(16)
    rec = (-750. + 100. * k, 60. * (k % 4) - 90., np.full(16, -50.), 15. * (k % 5), 5. * (k % 3))
    x, y, z = np.meshgrid(*(np.linspace(0, np.pi, n) for n in grid.vnC), indexing='ij')
    factor = 1.25 ** (np.sin(2 * x) * np.cos(y) * np.cos(3 * z))

    def scaled(name):
        p = getattr(model, name)
        return None if p is None else np.asarray(p) * factor
    other = em.Model(grid, scaled('property_x'), scaled('property_y'), scaled('property_z'), mapping=model.mapping)
    both = [other, model]
    SJ = em.optimize.SurveyJacobian
    times, its = [], None
    if which == 'a':
        sj = SJ(grid, model, sources, [FREQ], rec, batch=nsrc, **opts).open()
        for r in range(reps + 1):
            t0 = time.perf_counter()
            sj.close()
            sj = SJ(grid, both[r % 2], sources, [FREQ], rec, batch=nsrc, **opts).open()
            times.append(time.perf_counter() - t0)
        its = [sj.forward_info[i][0]['it_mg'] for i in range(nsrc)]
        norm = float(np.linalg.norm(sj.synthetic))
        sj.close()
    elif which == 'b':
        with SJ(grid, model, sources, [FREQ], rec, batch=nsrc, **opts) as sj:
            for r in range(reps + 1):
                t0 = time.perf_counter()
                sj.set_model(both[r % 2])
                times.append(time.perf_counter() - t0)
            its = [sj.forward_info[i][0]['it_mg'] for i in range(nsrc)]
            norm = float(np.linalg.norm(sj.synthetic))
    else:
        # (the model the last repetition of (a) and (b) ends on, for the same cycle counts)
        last = both[reps % 2]
        spec = em.fields.FrequencySpec(FREQ)
        with em.solver.DeviceMG.from_model(grid, models.model_parts(grid, last, raw=True), spec) as dev:
            dev.set_batch(nsrc)
            for r in range(reps + 1):
                t0 = time.perf_counter()
                for b in range(nsrc):
                    dev.select(b)
                    dev.set_source(sources[b], spec.smu0)
                _, infos = em.solver.solve_sources(grid, None, None, FREQ, handle=dev, resident=nsrc, download=False, **opts)
                times.append(time.perf_counter() - t0)
            its = [info['it_mg'] for info in infos]
            dev.select(0)
            norm = float(np.linalg.norm(dev.get_receiver_response(rec)))
    t = times[1:]                               # (the first repetition is the warm-up)
    print(json.dumps({"step": which, "s_median": float(np.median(t)), "s_min": min(t), "s_max": max(t), "s_all": t,
                      "it_mg": its, "data_norm": norm}))


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
    for name, key in (('a', 'close_and_reopen'), ('b', 'set_model'), ('c', 'forward_solves_alone')):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", name, wl, str(nsrc),
               str(reps)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:
            print(f"step ({name}) ended with status {res.returncode}: stopping here", file=sys.stderr)
            print(json.dumps(out))
            return res.returncode
        out[key] = json.loads(res.stdout.strip().splitlines()[-1])
    a, b, c = out["close_and_reopen"], out["set_model"], out["forward_solves_alone"]
    out["same_iterations"] = a["it_mg"] == b["it_mg"] == c["it_mg"]
    out["reopen_minus_solves_ms"] = 1e3 * (a["s_median"] - c["s_median"])
    out["set_model_minus_solves_ms"] = 1e3 * (b["s_median"] - c["s_median"])
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
