"""CPU: what the projected rows, the posterior variance and the resolution diagonal need on the host.  No GPU.

* emg3d_rows_project_plan (csrc/rows.hpp), the geometry the launch itself uses: the panels tile the columns once, the blocks of output
  rows tile m once, the LDS stays within 160 KiB, the column partition follows from n_cols alone, sizes < 1 answer -2;
* maps.SmoothingCovariance.diagonal() against apply(e_j, host=True)[j], 1e-12 relative: every cell of a small stretched grid, random
  cells of a larger one, passes 1 and 3, a skipped axis (length 0, one cell), scalar, per-cell and per-direction std; positivity;
* the formulae of optimize.RowStore.posterior_variance / resolution_diagonal on a dense random J: c - c^2 q and c q with q the column
  sums of squares of K^-1 J against diag(C - C J^T A^-1 J C) and diag(C J^T A^-1 J) in np.longdouble, within 16 cond(A) eps;
* the new symbols in the header and the binding."""
import os
import re

import numpy as np
import pytest

from test_row_covariance_host import graded, solve_longdouble

EPS = 2.0 ** -52
LDS_MAX = 163840
SIZES = list(range(1, 41)) + [127, 128, 129, 130, 255, 256, 257, 258, 700]
COLS = [1, 15, 16, 17, 1000, 2097152]


@pytest.fixture(scope="module")
def em():
    import __graft_entry__ as g
    g.build()
    import emg3d_amd
    return emg3d_amd


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def test_project_plan(em):
    lib = em._lib
    for n_cols in COLS:
        first = lib.rows_project_plan(1, 1, n_cols)
        block, cols, kstep, panels = first["block"], first["cols"], first["kstep"], first["panels"]
        assert block % 16 == 0 and cols % 16 == 0 and kstep % 4 == 0
        assert (panels - 1) * cols < n_cols <= panels * cols                    # the panels tile the columns once
        for n_rows in SIZES:
            for m in SIZES:
                p = lib.rows_project_plan(n_rows, m, n_cols)
                # the column partition is a function of n_cols alone
                assert (p["block"], p["cols"], p["kstep"], p["panels"]) == (block, cols, kstep, panels), (n_rows, m, n_cols)
                assert (p["passes"] - 1) * block < m <= p["passes"] * block     # the blocks tile m once
                live = m - (p["passes"] - 1) * block
                assert p["last_rows"] in (32, 64, 128, 256) and live <= p["last_rows"] <= block
                assert p["last_rows"] == 32 or live > p["last_rows"] // 2       # ... and the last block's kernel is the smallest
                assert p["grid"] == p["passes"] * panels
                big = block if p["passes"] > 1 else p["last_rows"]
                assert p["lds_bytes"] == kstep * ((big + 16) + (cols + 16)) * 8 <= LDS_MAX


def test_project_plan_refusals(em):
    import ctypes
    h = em._lib.load()
    out = (ctypes.c_int64 * 8)()
    assert h.emg3d_rows_project_plan(3, 2, 5, out) == 0
    for bad in ((0, 2, 5), (3, 0, 5), (3, 2, 0), (-1, 2, 5), (3, -7, 5), (3, 2, -1)):
        assert h.emg3d_rows_project_plan(*bad, out) == -2, bad
    assert h.emg3d_rows_project_plan(3, 2, 5, None) == -2


# ---- SmoothingCovariance.diagonal -----------------------------------------------------------------------------------------------
def _std(kind, rng, vnC):
    if kind == "scalar":
        return 1.7
    if kind == "cells":
        return rng.uniform(0.5, 2.0, vnC)
    return (rng.uniform(0.5, 2.0, vnC), 2.0, 1.0)


def _check_diagonal(em, grid, lengths, std_kind, passes, cells, rng):
    """-> the largest relative deviation of diagonal() from apply(e_j, host=True)[j] over `cells` (flat F-ordered indices)."""
    vnC = tuple(int(n) for n in grid.vnC)
    cov = em.maps.SmoothingCovariance(grid, lengths, std=_std(std_kind, rng, vnC), passes=passes)
    d = cov.diagonal()
    three = std_kind == "tuple"
    assert isinstance(d, tuple) == three
    planes = d if three else (d,)
    assert len(planes) == (3 if three else 1)
    assert all(p.shape == vnC and p.dtype == np.float64 and np.all(p > 0) for p in planes)
    worst = 0.0
    for j in cells:
        e = np.zeros(int(np.prod(vnC)))
        e[j] = 1.0
        e = e.reshape(vnC, order='F')
        got = cov.apply((e, e, e) if three else e, host=True)
        for p, g in zip(planes, got if three else (got,)):
            want = g.ravel(order='F')[j]
            worst = max(worst, abs(p.ravel(order='F')[j] - want) / want)
    return worst


@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("std_kind", ["scalar", "cells", "tuple"])
def test_covariance_diagonal(em, std_kind, passes):
    rng = np.random.default_rng(3)
    small = em.TensorMesh([graded(5, 1.3), graded(4, 1.5), graded(3, 1.4)], origin=(0, 0, 0))
    large = em.TensorMesh([graded(17, 1.3), graded(9, 1.5), graded(6, 1.4)], origin=(0, 0, 0))
    flat = em.TensorMesh([graded(5, 1.3), [40.0], graded(3, 1.4)], origin=(0, 0, 0))
    cases = [("small", small, (300.0, 200.0, 100.0), range(60)),
             ("large", large, (300.0, 200.0, 100.0), rng.choice(17 * 9 * 6, 20, replace=False)),
             ("ell = 0", small, (300.0, 0.0, 100.0), range(60)),
             ("one cell", flat, (300.0, 200.0, 100.0), range(15))]
    for name, grid, lengths, cells in cases:
        worst = _check_diagonal(em, grid, lengths, std_kind, passes, cells, rng)
        print(f"diagonal() vs apply(e_j)[j], {name}, std {std_kind}, passes {passes}: relative {worst:.3e}")
        assert worst <= 1e-12, (name, worst)


def test_covariance_diagonal_skipped_axes_are_ones(em):
    grid = em.TensorMesh([graded(5, 1.3), graded(4, 1.5), graded(3, 1.4)], origin=(0, 0, 0))
    assert np.array_equal(em.maps.SmoothingCovariance(grid, 0.0).diagonal(), np.ones(grid.vnC))
    w = np.random.default_rng(1).uniform(0.5, 2.0, grid.vnC)
    assert np.array_equal(em.maps.SmoothingCovariance(grid, 0.0, std=w).diagonal(), w * w)


# ---- the host formulae ----------------------------------------------------------------------------------------------------------
def test_formulae_against_the_dense_longdouble_route():
    rng = np.random.default_rng(12)
    n, ncell = 12, 30
    J = rng.standard_normal((n, ncell))
    c = rng.uniform(0.5, 2.0, ncell)
    w = rng.uniform(0.5, 2.0, n)
    lam = 0.3
    A = (J * c) @ J.T + lam * np.diag(1 / w)
    K = np.linalg.cholesky(A)
    T = np.linalg.solve(K, np.eye(n)) @ J
    q = (T * T).sum(axis=0)
    post, res = c - c * c * q, c * q
    Jl, cl = J.astype(np.longdouble), c.astype(np.longdouble)
    Al = (Jl * cl) @ Jl.T + np.longdouble(lam) * np.diag(1 / w.astype(np.longdouble))
    X = Jl.T @ solve_longdouble(Al, Jl)                         # J^T A^-1 J
    C = np.diag(cl)
    post_l = np.diag(C - C @ X @ C)
    res_l = np.diag(C @ X)
    tol = 16 * np.linalg.cond(A) * EPS
    e_post = float(np.abs(post - post_l).max() / c.max())
    e_res = float(np.abs(res - res_l).max())
    print(f"posterior {e_post:.3e}, resolution {e_res:.3e}, bound {tol:.3e}")
    assert e_post <= tol and e_res <= tol
    assert np.all(post >= -tol * c.max()) and np.all(post <= c + tol * c.max())
    assert np.all(res >= -tol) and np.all(res < 1 + tol)


# ---- header and binding ---------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_and_binding(em):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "emg3d_hip.h")).read()
    assert re.search(r"#define\s+EMG3D_HIP_ABI_VERSION\s+(\d+)", header).group(1) == str(em._lib.ABI_VERSION)
    assert em._lib.ABI_VERSION >= 118
    h = em._lib.load()
    for name in ("emg3d_rows_project_plan", "emg3d_rows_project", "emg3d_rows_colsumsq", "emg3d_rows_smooth_l"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in em._lib.SIGNATURES and hasattr(h, name), name
    # the header does not promise what the hardware does not give
    block = header[header.index("rows_project     :"):header.index("rows_colsumsq    :")]
    assert "NOT bit for bit" in block
