"""What a computational grid per frequency buys a survey whose frequencies span two decades: 0.1, 1 and 10 Hz (skin depths of about
1590, 500 and 160 m in 1 Ohm m), 4 point dipoles, 16 receivers, a layered resistivity model on a 40 x 40 x 24 model grid, ``batch``
= 4, F-cycles with semicoarsening and line relaxation, tol = 1e-6, colour order.

  (one)    ONE computational grid that serves all three: 50 m cells in the core (the highest frequency), +-41 km (the lowest):
           128 x 128 x 64 cells, ``SurveyJacobian(grid, ..., model_grid=)``;
  (fitted) three grids of 64 x 64 x 32 cells with core cells of 500, 150 and 50 m -- the same stretching, scaled with the skin
           depth --, ``SurveyJacobian([g_0.1, g_1, g_10], ..., model_grid=)``.

The two do not compute the same numbers (other discretisations); the tool reports what each costs: ``open()`` (the 12 forward solves),
one ``jvec`` and one ``jtvec`` (12 solves each), the handles' device memory and the multigrid cycles.  Host clock around calls that end
in a device synchronisation; each configuration runs once after a small warm-up survey, in a child process under a `timeout` of its
own; the tool prints one JSON line.  No threshold is attached.

    python tools/frequency_grids_timing.py
    python tools/frequency_grids_timing.py --step              (the measurement itself, one JSON line)
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 420             # 2 x (12 forward + 24 product solves), the largest grid 128 x 128 x 64
FREQS = [0.1, 1.0, 10.0]
CORE = [500., 150., 50.]       # core cell widths of the fitted grids, per entry of FREQS


def _grid(em, ncore, npad, width, fx, fz):
    hx = em.meshes.stretched_widths(ncore, npad, width, fx)
    hz = em.meshes.stretched_widths(ncore // 2, npad // 2, width, fz)
    return em.TensorMesh([hx, hx, hz], origin=(-hx.sum() / 2 + 3., -hx.sum() / 2 - 7., -hz.sum() / 2 - 400.))


def _measure(em, grid, model, model_grid, sources, rec, opts, v, seed):
    t0 = time.perf_counter()
    with em.optimize.SurveyJacobian(grid, model, sources, FREQS, rec, batch=len(sources), model_grid=model_grid, **opts) as sj:
        t1 = time.perf_counter()
        jv = sj.jvec(v, mapped=True)
        jinfo = sj.info
        t2 = time.perf_counter()
        rng = np.random.default_rng(seed)
        w = (rng.standard_normal(jv.shape) + 1j * rng.standard_normal(jv.shape)) / np.abs(sj.synthetic)
        t3 = time.perf_counter()
        jt = sj.jtvec(w, mapped=True)
        t4 = time.perf_counter()
        lhs, rhs = float(np.real(np.sum(np.conj(w) * jv))), float(np.sum(jt * v))
        return {"cells": [int(g.nC) for g in sj._held.distinct], "handles": len(list(sj._held)), "device_bytes": int(sj.device_bytes),
                "open_s": t1 - t0, "jvec_s": t2 - t1, "jtvec_s": t4 - t3,
                "it_mg_forward": [[sj.forward_info[i][j]['it_mg'] for j in range(3)] for i in range(len(sources))],
                "it_mg_jvec": [[jinfo[i][j]['it_mg'] for j in range(3)] for i in range(len(sources))],
                "it_mg_jtvec": [[sj.info[i][j]['it_mg'] for j in range(3)] for i in range(len(sources))],
                "exits": sorted({sj.forward_info[i][j]['exit'] for i in range(len(sources)) for j in range(3)}),
                "adjoint_gap": abs(lhs - rhs) / abs(lhs)}


def step():
    import emg3d_amd as em
    edges = [np.linspace(-2000., 2000., 41), np.linspace(-2000., 2000., 41), np.linspace(-2000., 400., 25)]
    model_grid = em.TensorMesh([np.diff(e) for e in edges], origin=[e[0] for e in edges])
    _, _, Z = np.meshgrid(model_grid.cell_centers_x, model_grid.cell_centers_y, model_grid.cell_centers_z, indexing='ij')
    rho = np.full(model_grid.vnC, 10.0)
    rho[Z > -1000.] = 1.0
    rho[Z > 0.] = 0.3
    model = em.Model(model_grid, rho.ravel(order='F'))
    opts = dict(cycle='F', semicoarsening=True, linerelaxation=True, tol=1e-6, ordering='colour', verb=0)
    sources = [[-600. + 400. * k, 100. * (k % 3 - 1), -150., 30. + 10. * k, 10.] for k in range(4)]
    k = np.arange(16)
    rec = (-750. + 100. * k, 60. * (k % 4) - 90., np.full(16, -50.), 15. * (k % 5), 5. * (k % 3))
    v = np.asfortranarray(np.random.default_rng(0).standard_normal(model_grid.vnC) * rho * 0.1)
    one = _grid(em, 64, 32, 50., 1.16, 1.35)
    fitted = [_grid(em, 32, 16, w, 1.15, 1.3) for w in CORE]
    # warm-up: the library, the allocator and both code paths on a small survey
    small = [_grid(em, 8, 4, w, 1.3, 1.3) for w in (500., 400., 500.)]
    _measure(em, small, model, model_grid, sources, rec, opts, v, 1)
    out = {"one": _measure(em, one, model, model_grid, sources, rec, opts, v, 2),
           "fitted": _measure(em, fitted, model, model_grid, sources, rec, opts, v, 2)}
    print(json.dumps(out))


def main(argv):
    if argv and argv[0] == '--step':
        step()
        return 0
    out = {"freqs": FREQS, "core_widths": CORE, "sources": 4, "receivers": 16, "model_cells": [40, 40, 24]}
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step"]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if res.returncode != 0:
        print(f"the measurement ended with status {res.returncode}", file=sys.stderr)
        print(json.dumps(out))
        return res.returncode
    out.update(json.loads(res.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
