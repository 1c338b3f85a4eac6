"""CPU: the smoothing model covariance maps.SmoothingCovariance -- its tridiagonal matrices and factors, the numpy line solve that
the device kernels equal bit for bit, the L / L^T pair, and the launch geometry emg3d_rows_smooth_plan (csrc/rows_cov.hpp).  No GPU.

* per axis: T from the formulas is symmetric with smallest eigenvalue >= 1 - 1e-12, every pivot is positive, ell = 0 and n = 1 skip
  the axis;
* the host reference against a dense np.longdouble solve of T: relative max-norm error <= 4 passes cond(T) eps (Thomas on an SPD matrix
  is backward stable);
* 3-D: <L^T a, b> == <a, L b> to 1e-13, C symmetric and positive, S of a constant on a uniform axis returns it to 1e-14;
* the plan: LDS within 160 KiB, the workgroups cover the lines with less than one workgroup of excess, path 1 exactly when the LDS
  cannot hold the least number of lines;
* argument checks, and the new symbols in the header and the binding."""
import ctypes
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest

EPS = 2.0 ** -52
SIZES = list(range(1, 71)) + [128, 256, 700, 3000]
LDS_MAX = 163840


@pytest.fixture(scope="module")
def em():
    import __graft_entry__ as g
    g.build()
    import emg3d_amd
    return emg3d_amd


def graded(n, factor, h0=25.0):
    """n widths, stretched by `factor` from the middle outwards."""
    k = np.abs(np.arange(n) - (n - 1) / 2.0)
    return h0 * factor ** np.floor(k)


def dense_T(em, h, ell):
    diag, off = em.maps.smoothing_matrix(h, ell)
    return np.diag(diag) + np.diag(off, 1) + np.diag(off, -1)


def solve_longdouble(A, b):
    """Gaussian elimination with partial pivoting in np.longdouble (numpy.linalg has none)."""
    A = np.array(A, dtype=np.longdouble)
    b = np.array(b, dtype=np.longdouble)
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            b[[k, p]] = b[[p, k]]
        for i in range(k + 1, n):
            m = A[i, k] / A[k, k]
            if m != 0:
                A[i, k:] -= m * A[k, k:]
                b[i] -= m * b[k]
    x = np.zeros_like(b)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


AXES = [(n, f) for n in (1, 2, 3, 17, 40) for f in (1.3, 1.5)]
ELLS = [0.0, 30.0, 500.0, 5000.0]


def eigenvalues_below(diag, off, sigma):
    """How many eigenvalues of the symmetric tridiagonal (diag, off) lie below `sigma`: the negative pivots of T - sigma I (Sturm),
    in exact rational arithmetic on the float64 entries -- numpy.linalg.eigvalsh resolves an eigenvalue to a few eps ||T|| only."""
    q = Fraction(float(diag[0])) - sigma
    count = int(q < 0)
    for i in range(1, len(diag)):
        assert q != 0
        q = Fraction(float(diag[i])) - sigma - Fraction(float(off[i - 1])) ** 2 / q
        count += int(q < 0)
    return count


@pytest.mark.parametrize("n,factor", AXES)
def test_factors_per_axis(em, n, factor):
    """The smallest eigenvalue of T is 1 in exact arithmetic.  A float64 entry of T carries up to six roundings (off: ell^2, h + h',
    h h', the root, the product, the quotient; diag: four per term and the sums), a relative error below 8 u (u = 2^-53), which
    moves an eigenvalue by at most 8 u ||T||_inf, ||T||_inf <= 2 (1 + 2 ell^2 / h_min^2).  The bound 1 - 1e-12 can be met, and
    checked, only where that is below 1e-12: with ell = 5000 m it takes h_min >= 320 m (8 u 2 (1 + 488) = 8.7e-13), the core width
    here; the count of eigenvalues below the bound is exact.  The fine cells of the other tests (25 m) keep an eigenvalue check
    with the bound that the roundings allow there, 1 - 8 u ||T||_inf."""
    h = graded(n, factor, h0=320.0)
    for ell in ELLS:
        diag, off = em.maps.smoothing_matrix(h, ell)
        T = dense_T(em, h, ell)
        assert np.array_equal(T, T.T)
        assert 8 * 2.0 ** -53 * np.abs(T).sum(axis=1).max() < 1e-12
        assert eigenvalues_below(diag, off, 1 - Fraction(1, 10 ** 12)) == 0
        # ... and on fine cells (25 m: ||T||_inf up to 2e5), where the roundings of the entries alone exceed 1e-12, within those
        fine = graded(n, factor)
        dfine, ofine = em.maps.smoothing_matrix(fine, ell)
        norm = float(np.abs(dense_T(em, fine, ell)).sum(axis=1).max())
        assert eigenvalues_below(dfine, ofine, 1 - Fraction(8 * 2.0 ** -53 * norm)) == 0
        f = em.maps.smoothing_factors(h, ell)
        if n == 1 or ell == 0:
            assert f is None and np.array_equal(T, np.eye(n))
            continue
        lo, cp, inv = f
        assert all(a.shape == (n,) and a.dtype == np.float64 for a in f)
        assert np.all(inv > 0) and lo[0] == 0 and cp[n - 1] == 0
        assert np.array_equal(lo[1:], np.diag(T, -1))
        # the factors are those of T: L U with L = lower bidiagonal (1 / inv, lo), U = unit upper bidiagonal (cp)
        Lm = np.diag(1 / inv) + np.diag(lo[1:], -1)
        Um = np.eye(n) + np.diag(cp[:-1], 1)
        assert np.abs(Lm @ Um - T).max() <= 8 * EPS * np.abs(T).max()
    grid = em.TensorMesh([graded(n, factor), graded(5, 1.4), [10.0]])
    cov = em.maps.SmoothingCovariance(grid, (300.0, 0.0, 700.0))
    assert (cov.factors[0] is None) == (n == 1) and cov.factors[1] is None and cov.factors[2] is None


@pytest.mark.parametrize("passes", [1, 3])
def test_host_reference_against_a_dense_longdouble_solve(em, passes):
    rng = np.random.default_rng(5)
    worst = 0.0
    for n, factor in AXES:
        h = graded(n, factor)
        for ell in ELLS[1:]:
            f = em.maps.smoothing_factors(h, ell)
            if f is None:
                continue
            T = dense_T(em, h, ell)
            cond = np.linalg.cond(T)
            b = rng.standard_normal((n, 4))
            got = em.maps.smooth_lines_host(b.copy(), 0, f, passes)
            want = b.astype(np.longdouble)
            for _ in range(passes):
                want = solve_longdouble(T, want)
            err = float(np.abs(got - want).max() / np.abs(want).max())
            ratio = err / (passes * cond * EPS)
            worst = max(worst, ratio)
            assert ratio <= 4, (n, factor, ell, passes, err, cond)
    print(f"passes {passes}: largest error / (passes cond(T) eps) = {worst:.3f}")


def _cov3(em, std_kind="field", passes=2):
    grid = em.TensorMesh([graded(7, 1.3), graded(5, 1.5), graded(6, 1.4)], origin=(0, 0, 0))
    rng = np.random.default_rng(11)
    std = {"one": 1.0, "scalar": 0.7, "field": rng.uniform(0.5, 2.0, grid.vnC)}[std_kind]
    return grid, rng, em.maps.SmoothingCovariance(grid, (120.0, 60.0, 400.0), std=std, passes=passes)


@pytest.mark.parametrize("std_kind", ["one", "scalar", "field"])
def test_sqrt_and_sqrt_t_are_a_transposed_pair(em, std_kind):
    grid, rng, cov = _cov3(em, std_kind)
    a, b = rng.standard_normal(grid.vnC), rng.standard_normal(grid.vnC)
    keep = a.copy()
    lhs = np.vdot(cov.sqrt_t(a, host=True), b)
    rhs = np.vdot(a, cov.sqrt(b, host=True))
    scale = np.linalg.norm(cov.sqrt_t(a, host=True)) * np.linalg.norm(b)
    assert abs(lhs - rhs) <= 1e-13 * scale
    assert np.array_equal(a, keep)                  # the argument is not smoothed in place
    # C = L L^T: symmetric and positive
    ca, cb = cov.apply(a, host=True), cov.apply(b, host=True)
    assert abs(np.vdot(b, ca) - np.vdot(cb, a)) <= 1e-13 * np.linalg.norm(ca) * np.linalg.norm(b)
    assert np.vdot(a, ca) > 0
    assert np.array_equal(ca, cov.sqrt(cov.sqrt_t(a, host=True), host=True))
    # a 3-tuple: every plane on its own
    t = cov.sqrt_t((a, b, a), host=True)
    assert isinstance(t, tuple) and np.array_equal(t[0], cov.sqrt_t(a, host=True)) and np.array_equal(t[1], cov.sqrt_t(b, host=True))


def test_std_per_direction(em):
    grid, rng, _ = _cov3(em)
    s = [rng.uniform(0.5, 2.0, grid.vnC), 2.0, 1.0]
    cov = em.maps.SmoothingCovariance(grid, 100.0, std=tuple(s))
    a = rng.standard_normal(grid.vnC)
    got = cov.sqrt_t((a, a, a), host=True)
    for q in range(3):
        one = em.maps.SmoothingCovariance(grid, 100.0, std=s[q])
        assert np.array_equal(got[q], one.sqrt_t(a, host=True))
    w = cov.scale(3)
    assert w.shape == (3 * grid.nC,) and np.array_equal(w[:grid.nC], s[0].ravel(order='F')) and np.all(w[2 * grid.nC:] == 1)
    with pytest.raises(ValueError):
        cov.sqrt_t(a, host=True)                    # a std per direction needs three planes
    assert em.maps.SmoothingCovariance(grid, 100.0).scale(3) is None


def test_constant_on_a_uniform_axis(em):
    grid = em.TensorMesh([np.full(9, 50.0), np.full(4, 20.0), np.full(6, 10.0)])
    c = np.full(grid.vnC, 3.25)
    for axis, ell in enumerate((400.0, 35.0, 90.0)):            # S of one axis
        lengths = [0.0, 0.0, 0.0]
        lengths[axis] = ell
        one = em.maps.SmoothingCovariance(grid, lengths)
        err = np.abs(one.sqrt_t(c, host=True) - c).max() / 3.25
        print(f"axis {axis}: S of a constant, relative deviation {err:.2e}")
        assert err <= 1e-14
    cov = em.maps.SmoothingCovariance(grid, (400.0, 35.0, 90.0), passes=3)
    # ... and a delta is spread, symmetrically about its cell along a uniform axis
    d = np.zeros(grid.vnC)
    d[4, 2, 3] = 1.0
    s = cov.sqrt_t(d, host=True)
    assert np.all(s > 0) and np.abs(s[:, 2, 3] - s[::-1, 2, 3]).max() <= 1e-10 * s.max() and s[:, 2, 3].argmax() == 4


def test_plan(em):
    lib = em._lib
    others = [(1, 1), (2, 3), (17, 5), (64, 65), (70, 70), (128, 256), (700, 3000)]
    assert "n_arrays" not in inspect.signature(lib.rows_smooth_plan).parameters      # the plan cannot depend on the number of arrays
    for axis in range(3):
        for n in SIZES:
            for o in others:
                shape = list(o)
                shape.insert(axis, n)
                p = lib.rows_smooth_plan(shape, axis)
                lines = int(np.prod(shape)) // n
                assert p["lines"] == lines and p["path"] in (0, 1)
                assert 0 <= p["lds_bytes"] <= LDS_MAX
                assert p["lines_per_workgroup"] * p["workgroups"] >= lines
                assert p["lines_per_workgroup"] * (p["workgroups"] - 1) < lines
                per_line = 8 * ((n | 1) if axis == 0 else n)        # x: rows padded to an odd length
                fits = per_line * p["min_lines"] <= LDS_MAX
                assert (p["path"] == 0) == fits
                if p["path"] == 0:
                    assert p["lds_bytes"] == per_line * p["lines_per_workgroup"] and p["lines_per_workgroup"] >= p["min_lines"]
                else:
                    assert p["lds_bytes"] == 0
                assert p == lib.rows_smooth_plan(shape, axis)
    # the sizes at which the path changes (tests/test_gpu_row_covariance.py runs them)
    assert [first_path1(lib, axis) for axis in range(3)] == [640, 641, 641]
    out = (ctypes.c_int64 * 6)()
    h = lib.load()
    assert h.emg3d_rows_smooth_plan(0, 1, 1, 0, out) == -2 and h.emg3d_rows_smooth_plan(1, 1, 1, 3, out) == -2
    assert h.emg3d_rows_smooth_plan(1, 1, 1, -1, out) == -2 and h.emg3d_rows_smooth_plan(1, 1, 1, 0, None) == -2


def first_path1(lib, axis):
    """The smallest length of `axis` (the other two of length 2) that the plan sends through HBM."""
    for n in range(1, 5000):
        shape = [2, 2]
        shape.insert(axis, n)
        if lib.rows_smooth_plan(shape, axis)["path"] == 1:
            return n
    raise AssertionError("no length up to 5000 takes path 1")


def test_argument_checks(em):
    grid, rng, cov = _cov3(em)
    SC = em.maps.SmoothingCovariance
    for bad in (-1.0, (10.0, -1.0, 10.0), (1.0, 2.0), np.nan):
        with pytest.raises(ValueError):
            SC(grid, bad)
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            SC(grid, 100.0, passes=bad)
    for bad in (np.ones(grid.vnC[::-1]), np.ones(grid.nC), (1.0, 2.0), -1.0, (np.ones((2, 2, 2)), 1.0, 1.0)):
        with pytest.raises(ValueError):
            SC(grid, 100.0, std=bad)
    with pytest.raises(ValueError):
        cov.sqrt_t(np.ones(grid.vnC[::-1]), host=True)
    with pytest.raises(ValueError):
        cov.sqrt((np.ones(grid.vnC),) * 2, host=True)
    with pytest.raises(TypeError):
        cov.apply(np.ones(grid.vnC) * 1j, host=True)
    assert SC(grid, 100.0).lengths == (100.0, 100.0, 100.0) and SC(grid, (1, 2, 3), passes=np.int64(2)).passes == 2


def test_new_symbols_in_header_and_binding(em):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "emg3d_hip.h")).read()
    assert int(re.search(r"#define\s+EMG3D_HIP_ABI_VERSION\s+(\d+)", header).group(1)) >= 117
    h = em._lib.load()
    for name in ("emg3d_rows_smooth_plan", "emg3d_smooth3d", "emg3d_rows_smooth", "emg3d_rows_clone"):
        assert re.search(r"\b" + name + r"\(", header) and name in em._lib.SIGNATURES and hasattr(h, name)
