"""Regridding workload for a kernel trace: grid2grid('volume') of a stretched 512^3 float64 model to 256^3 (k_volume_average)
and grid2grid('cubic' / 'linear') of a 256^3 cell array to ~200^3 (k_spline_eval_grid, k_linear_eval_grid), each `--reps`
times.  Run it under

    rocprofv3 --kernel-trace --stats -d <dir> -o regrid -- python tools/regrid_time.py

and read the kernels' average time from the stats; this script prints the wall time of each call (host transfers
included) and the bytes the volume kernel moves (input read once, output read and written)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stretched(n, width, factor):
    return width * factor ** np.linspace(0, 1, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import emg3d_amd as em
    n, m = args.n, args.m
    grid = em.TensorMesh([stretched(n, 10., 1.5), stretched(n, 11., 1.4), stretched(n, 9., 1.6)], origin=(-2000., -2100., -1900.))
    ext = [g[-1] - g[0] for g in (grid.nodes_x, grid.nodes_y, grid.nodes_z)]
    new = em.TensorMesh([np.full(m, e / m) for e in ext], origin=grid.origin)
    rng = np.random.default_rng(0)
    v = np.asfortranarray(10 ** rng.uniform(-1, 2, grid.vnC))
    nb = v.nbytes + 2 * new.n_cells * 8
    for r in range(args.reps):
        t = time.perf_counter()
        em.maps.grid2grid(grid, v, new, 'volume')
        print(f"volume {n}^3 -> {m}^3: {1e3 * (time.perf_counter() - t):8.1f} ms wall (kernel bytes {nb / 1e9:.3f} GB)", flush=True)
    k = m
    src = em.TensorMesh([stretched(k, 10., 1.3)] * 3, origin=(-1000., -1000., -1000.))
    dst = em.TensorMesh([stretched(k * 3 // 4, 13., 1.3), stretched(k * 4 // 5, 12.5, 1.3), stretched(k * 7 // 10, 14., 1.3)],
                        origin=(-990., -1010., -995.))
    c = np.asfortranarray(rng.standard_normal(src.vnC))
    for method in ('cubic', 'linear'):
        for r in range(args.reps):
            t = time.perf_counter()
            em.maps.grid2grid(src, c, dst, method)
            print(f"{method} {src.vnC} -> {dst.vnC}: {1e3 * (time.perf_counter() - t):8.1f} ms wall", flush=True)


if __name__ == "__main__":
    main()
