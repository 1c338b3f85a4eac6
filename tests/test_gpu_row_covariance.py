"""GPU: the smoothing model covariance on the device -- emg3d_smooth3d, DeviceRows.smooth / clone (emg3d_rows_smooth, emg3d_rows_clone;
k_rows_smooth_lines, k_rows_smooth_xtile, k_rows_smooth_hbm, k_rows_smooth_scale) and optimize.RowStore.with_covariance.

1. emg3d_smooth3d equals the numpy reference (maps.smooth_lines_host through SmoothingCovariance(host=True)) BIT FOR BIT: small and
   ragged shapes, more lines than a workgroup, per axis the first length the plan sends through HBM, 1 and 5 arrays, passes 1 .. 3,
   with and without standard deviations, L^T and L, a skipped axis, twice the same bits.
2. DeviceRows.smooth on a store filled from the host: every row equals its host reference bit for bit, a clone is a copy, the Gram
   matrix of the smoothed store equals that of a store filled with the host-smoothed rows bit for bit and the longdouble B B^T
   within the dot-product bound of tests/test_gpu_rows.py; a wrong shape answers -2.
3. RowStore.with_covariance on the survey of tests/test_gpu_row_store.py: rows, gram, rmatvec, step and the refusals; on the model
   grid the step against the dense route C = L L^T assembled on the host."""
import numpy as np
import pytest

from test_row_covariance_host import first_path1

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SHAPES = [(1, 1, 1), (2, 1, 3), (1, 5, 1), (3, 3, 3), (33, 5, 7), (64, 65, 3), (130, 4, 2)]


def _em():
    import emg3d_amd as em
    return em


def _widths(n, factor, h0):
    """Graded widths that stay near the correlation lengths on an axis of any length (runs of five cells, each `factor` times the
    one before): every step of every line solve couples neighbouring cells."""
    return h0 * factor ** (np.arange(n) % 5)


def _grid(em, shape):
    return em.TensorMesh([_widths(shape[0], 1.3, 25.0), _widths(shape[1], 1.5, 40.0), _widths(shape[2], 1.4, 10.0)])


def _host(cov, a, scale_after):
    return (cov.sqrt if scale_after else cov.sqrt_t)(a, host=True)


def _check_smooth3d(em, shape, lengths=(120.0, 60.0, 90.0), n_arrays=(1, 5), passes=(1, 2, 3)):
    """Every combination at this shape: (n_arrays) x (passes) x (std or none) x (L^T, L).  -> the number of comparisons."""
    lib = em._lib
    grid = _grid(em, shape)
    rng = np.random.default_rng(sum(shape))
    ncell = int(np.prod(shape))
    std = rng.uniform(0.5, 2.0, shape)
    data = rng.standard_normal((max(n_arrays), ncell))
    count = 0
    for p in passes:
        for s in (None, std):
            cov = em.maps.SmoothingCovariance(grid, lengths, std=1.0 if s is None else s, passes=p)
            for after in (False, True):
                want = np.array([_host(cov, a.reshape(shape, order='F'), after).ravel(order='F') for a in data])
                for na in n_arrays:
                    w = None if s is None else s.ravel(order='F')
                    got = lib.smooth3d(data[:na].copy(), shape, cov.factors, p, scale=w, scale_after=after)
                    assert np.array_equal(got, want[:na]), (shape, p, s is not None, after, na, float(np.abs(got - want[:na]).max()))
                    count += 1
                # the public methods run the same call, and twice the same bits
                a = data[0].reshape(shape, order='F')
                m = cov.sqrt if after else cov.sqrt_t
                assert np.array_equal(m(a), want[0].reshape(shape, order='F')) and np.array_equal(m(a), m(a))
    return count


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_smooth3d_equals_the_host_reference_bitwise(shape):
    em = _em()
    assert _check_smooth3d(em, shape) == 24
    for axis in range(3):                           # ... and with one axis of length 0
        lengths = [120.0, 60.0, 90.0]
        lengths[axis] = 0.0
        assert _check_smooth3d(em, shape, tuple(lengths), n_arrays=(2,), passes=(2,)) == 4


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_smooth3d_through_hbm(axis):
    """The first length the plan sends through HBM (path 1), the other two axes of length 2; and the last one that stays in LDS."""
    em = _em()
    n = first_path1(em._lib, axis)
    for length, path in ((n, 1), (n - 1, 0)):
        shape = [2, 2]
        shape.insert(axis, length)
        assert em._lib.rows_smooth_plan(shape, axis)["path"] == path
        assert _check_smooth3d(em, tuple(shape), n_arrays=(1, 5)) == 24


def test_smooth3d_apply_and_refusals():
    em = _em()
    shape = (33, 5, 7)
    grid = _grid(em, shape)
    rng = np.random.default_rng(2)
    cov = em.maps.SmoothingCovariance(grid, (120.0, 60.0, 90.0), std=rng.uniform(0.5, 2.0, shape), passes=2)
    a = rng.standard_normal(shape)
    assert np.array_equal(cov.apply(a), cov.apply(a, host=True))
    t = cov.sqrt_t((a, 2 * a, -a))
    assert all(np.array_equal(x, y) for x, y in zip(t, cov.sqrt_t((a, 2 * a, -a), host=True)))
    h, lib = em._lib.load(), em._lib
    d = np.zeros(8)
    f = [lib.ptr(np.ones(2)) for _ in range(3)]
    none = [None] * 3
    assert h.emg3d_smooth3d(0, 1, 2, 2, 2, None, *f, *none, *none, 1, 0, lib.ptr(d)) == 0
    assert h.emg3d_smooth3d(0, 1, 2, 2, 2, None, *f, *none, *none, 0, 0, lib.ptr(d)) == -2           # passes < 1
    assert h.emg3d_smooth3d(0, 0, 2, 2, 2, None, *f, *none, *none, 1, 0, lib.ptr(d)) == -2
    assert h.emg3d_smooth3d(0, 1, 2, 0, 2, None, *f, *none, *none, 1, 0, lib.ptr(d)) == -2
    assert h.emg3d_smooth3d(0, 1, 2, 2, 2, None, *f, *none, *none, 1, 0, None) == -2
    assert h.emg3d_smooth3d(0, 1, 2, 2, 2, None, f[0], None, f[2], *none, *none, 1, 0, lib.ptr(d)) == -2    # half an axis


# ---- 2. DeviceRows.smooth ------------------------------------------------------------------------------------------------------
def _gamma(n):
    return n * U / (1 - n * U)


def _fill(em, R):
    store = em.solver.DeviceRows(*R.shape)
    for i, row in enumerate(R):
        store.set_row(i, row)
    return store


_ROWS = {}


def _rows_case(em, planes):
    """17 rows of `planes` planes at (33, 5, 7) and their host reference, computed once; fewer rows take the first ones."""
    if planes not in _ROWS:
        shape = (33, 5, 7)
        grid = _grid(em, shape)
        rng = np.random.default_rng(40 + planes)
        std = tuple(rng.uniform(0.5, 2.0, shape) for _ in range(3)) if planes == 3 else rng.uniform(0.5, 2.0, shape)
        cov = em.maps.SmoothingCovariance(grid, (120.0, 60.0, 90.0), std=std, passes=2)
        ncell = int(np.prod(shape))
        R = rng.standard_normal((17, planes * ncell))
        B = np.empty_like(R)
        for i, row in enumerate(R):
            parts = tuple(p.reshape(shape, order='F') for p in row.reshape(planes, ncell))
            got = cov.sqrt_t(parts if planes == 3 else parts[0], host=True)
            B[i] = np.concatenate([g.ravel(order='F') for g in (got if planes == 3 else (got,))])
        R.setflags(write=False)
        B.setflags(write=False)
        _ROWS[planes] = (shape, cov, R, B)
    return _ROWS[planes]


@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("n_rows", [1, 3, 17])
def test_device_rows_smooth(n_rows, planes):
    em = _em()
    shape, cov, R, B = _rows_case(em, planes)
    R, B = R[:n_rows], B[:n_rows]
    with _fill(em, R) as store, store.clone() as twin:
        assert twin.n_rows == store.n_rows and twin.n_cols == store.n_cols
        assert all(np.array_equal(twin.get_row(i), R[i]) for i in range(n_rows))
        twin.smooth(shape, planes, cov.factors, cov.passes, scale=cov.scale(planes))
        assert all(np.array_equal(store.get_row(i), R[i]) for i in range(n_rows))           # the original is untouched
        for i in range(n_rows):
            got = twin.get_row(i)
            assert np.array_equal(got, B[i]), (i, float(np.abs(got - B[i]).max()))
        G = twin.gram()
        with _fill(em, B) as ref:
            assert np.array_equal(G, ref.gram())
        Bl = B.astype(np.longdouble)
        assert np.all(np.abs(G - Bl @ Bl.T) <= _gamma(B.shape[1] + 2) * (np.abs(B) @ np.abs(B).T))
        assert np.array_equal(G, G.T)
        # no scale: the same sweeps on the raw rows
        store.smooth(shape, planes, cov.factors, cov.passes)
        plain = em.maps.SmoothingCovariance(cov.grid, cov.lengths, passes=cov.passes)
        row0 = tuple(p.reshape(shape, order='F') for p in R[0].reshape(planes, -1))
        want = plain.sqrt_t(row0 if planes == 3 else row0[0], host=True)
        want = np.concatenate([g.ravel(order='F') for g in (want if planes == 3 else (want,))])
        assert np.array_equal(store.get_row(0), want)


def test_device_rows_smooth_refusals():
    em = _em()
    lib, h = em._lib, em._lib.load()
    shape, cov, R, B = _rows_case(em, 1)
    with _fill(em, R[:2]) as store:
        ptrs, keep = lib.factor_ptrs(cov.factors, shape)
        assert h.emg3d_rows_smooth(store._h, 33, 5, 6, 1, None, *ptrs, 1) == -2            # 33 * 5 * 6 != n_cols
        assert h.emg3d_rows_smooth(store._h, 33, 5, 7, 3, None, *ptrs, 1) == -2
        assert h.emg3d_rows_smooth(store._h, 33, 5, 7, 1, None, *ptrs, 0) == -2            # passes < 1
        assert h.emg3d_rows_smooth(None, 33, 5, 7, 1, None, *ptrs, 1) == -2
        assert h.emg3d_rows_clone(None, None) == -2 and h.emg3d_rows_clone(store._h, None) == -2
        with pytest.raises(ValueError):
            store.smooth((33, 5, 6), 1, cov.factors, 1)
        with pytest.raises(ValueError):
            store.smooth(shape, 1, cov.factors, 0)
        with pytest.raises(ValueError):
            store.smooth(shape, 1, cov.factors[:2], 1)
        assert all(np.array_equal(store.get_row(i), R[i]) for i in range(2))                # a refused call changes nothing


# ---- 3. RowStore.with_covariance -----------------------------------------------------------------------------------------------
def _planes(x):
    return x if isinstance(x, tuple) else (x,)


def _check_store(em, store, cov, rng, inplace):
    """with_covariance on `store`: rows, gram, rmatvec, step and the refusals.  -> (new store, stacked residual, weights, damping)."""
    n = store.n_rows
    old_rows = [store.row(i) for i in range(n)]
    new = store.with_covariance(cov, inplace=inplace)
    assert new.cov is cov and np.array_equal(new.index, store.index) and new.info == store.info and new.n_rows == n
    assert (new is store) == inplace
    for i in range(n):
        want = _planes(cov.sqrt_t(old_rows[i], host=True))
        got = _planes(new.row(i))
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), i
        if not inplace:
            assert all(np.array_equal(a, b) for a, b in zip(_planes(store.row(i)), _planes(old_rows[i])))
    G = new.gram()
    assert np.array_equal(G, G.T) and np.array_equal(G, new.rows.gram()) and np.all(np.diag(G) > 0)
    y = rng.standard_normal(n)
    bty = new.rows.rmatvec(y)                       # B^T y without cm
    want = cov.sqrt(new._cells(bty))
    assert all(np.array_equal(g, w) for g, w in zip(_planes(new.rmatvec(y)), _planes(want)))
    assert all(np.array_equal(g, w) for g, w in zip(_planes(want), _planes(cov.sqrt(new._cells(bty), host=True))))
    r = rng.standard_normal(n) * np.sqrt(np.diag(G))
    w = rng.uniform(0.5, 2.0, n)
    damping = 1e-3 * np.trace(G) / n
    step = new.step(r, w, damping=damping)
    want = new.rmatvec(np.linalg.solve(new.gram() + damping * np.diag(1 / w), r))
    assert all(np.array_equal(g, x) for g, x in zip(_planes(step), _planes(want))) and np.abs(_planes(step)[0]).max() > 0
    cm = np.ones(cov.vnC)
    for call in (lambda: new.gram(cm), lambda: new.rmatvec(y, cm), lambda: new.step(r, w, cm=cm), lambda: new.matvec(cm),
                 lambda: new.with_covariance(cov)):
        with pytest.raises(ValueError, match="store it was made from"):
            call()
    return new, r, w, damping


@pytest.mark.parametrize("components", [False, True], ids=["sum", "components"])
def test_with_covariance_on_the_survey(components):
    em = _em()
    from test_gpu_row_store import _model
    from test_gpu_sensitivity_diagonal import FREQS, OPTS, SOURCES, _survey
    grid, rec, rng, sig = _survey(em)
    model = _model(em, grid, sig, "iso")
    vnC = tuple(int(n) for n in grid.vnC)
    std = tuple(rng.uniform(0.5, 2.0, vnC) for _ in range(3)) if components else rng.uniform(0.5, 2.0, vnC)
    cov = em.maps.SmoothingCovariance(grid, (150.0, 100.0, 60.0), std=std, passes=2)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, tol=1e-8, **OPTS) as sj:
        store = sj.park_rows(components=components)
        G0 = store.gram()
        with _check_store(em, store, cov, rng, inplace=False)[0] as new:
            assert np.array_equal(store.gram(), G0) and store.cov is None
            v = rng.standard_normal(vnC)
            assert store.matvec(v).shape == (store.n_rows,)                 # the original keeps every product
            G1 = new.gram()
            rows1 = [new.row(i) for i in range(new.n_rows)]
        with pytest.raises(RuntimeError, match="closed"):
            new.row(0)
        with pytest.raises(ValueError, match="shape"):
            store.with_covariance(em.maps.SmoothingCovariance(em.TensorMesh([[1.0] * 4, [1.0] * 8, [1.0] * 8]), 1.0))
        if not components:
            with pytest.raises(ValueError, match="three planes"):
                store.with_covariance(em.maps.SmoothingCovariance(grid, 100.0, std=(1.0, 2.0, 3.0)))
        assert np.array_equal(store.gram(), G0)                             # a refused call changes nothing
        same = _check_store(em, store, cov, rng, inplace=True)[0]          # ... and now converted in place: identical to `new`
        assert same is store and np.array_equal(store.gram(), G1)
        assert all(np.array_equal(a, b) for i in range(store.n_rows) for a, b in zip(_planes(store.row(i)), _planes(rows1[i])))


def test_with_covariance_on_a_model_grid_against_the_dense_route():
    """The model-grid `mapped` case of tests/test_gpu_row_store.py (7 x 5 x 4 = 140 cells): C assembled on the host in longdouble from
    cov.apply(unit vector, host=True), the step C J^T (J C J^T + damping W^-1)^-1 r solved densely in longdouble
    (Gaussian elimination with partial pivoting) and rounded to float64 at the end.  The device step solves a system with the matrix G + damping W^-1 of condition number kappa, whose entries differ from
    the dense route's by rounding (relative u per entry, summed: the Gram bound); a backward-stable solve of both gives solutions
    that differ by at most a small multiple of kappa eps, and the outer products C J^T y add a few eps more: 16 kappa eps."""
    em = _em()
    from conftest import load_golden
    from test_gpu_jacobian import OPTS as JOPTS
    from test_gpu_model_grid import SOURCES as MSOURCES, _models
    from test_model_grid_host import grid_pairs
    g = load_golden("survey_jacobian.npz")
    model_grid, grid = grid_pairs(em, ['unaligned'])['unaligned']
    model = _models(em, model_grid, 'Resistivity')
    rec = tuple(g['rec'])
    rng = np.random.default_rng(9)
    vnM = tuple(int(n) for n in model_grid.vnC)
    cov = em.maps.SmoothingCovariance(model_grid, (300.0, 200.0, 100.0), std=rng.uniform(0.5, 2.0, vnM), passes=2)
    kw = dict(JOPTS, tol=1e-6, batch=2, model_grid=model_grid)
    with em.optimize.SurveyJacobian(grid, model, MSOURCES, [1.5, -1.2], rec, **kw) as sj:
        store = sj.park_rows(mapped=True)
        n, ncell = store.n_rows, model_grid.nC
        J = np.array([store.row(i).ravel(order='F') for i in range(n)]).astype(np.longdouble)
        new, r, w, damping = _check_store(em, store, cov, rng, inplace=False)
        with new:
            step = new.step(r, w, damping=damping).ravel(order='F')
        C = np.empty((ncell, ncell), dtype=np.longdouble)
        for j in range(ncell):
            e = np.zeros(ncell)
            e[j] = 1.0
            C[:, j] = cov.apply(e.reshape(vnM, order='F'), host=True).ravel(order='F')
        A = J @ C @ J.T + damping * np.diag(1 / w.astype(np.longdouble))
        kappa = np.linalg.cond(A.astype(np.float64))
        from test_row_covariance_host import solve_longdouble
        dense = (C @ (J.T @ solve_longdouble(A, r))).astype(np.float64)
        err = float(np.abs(step - dense).max() / np.abs(dense).max())
        print(f"step vs dense route: relative error {err:.3e}, cond {kappa:.3e}, error / (cond eps) = {err / (kappa * 2 * U):.3f}")
        assert err <= 16 * kappa * 2 * U
        with pytest.raises(ValueError, match="shape"):
            store.with_covariance(em.maps.SmoothingCovariance(grid, 100.0))                 # the computational grid's shape
