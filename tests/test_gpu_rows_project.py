"""GPU: a small dense matrix times the row store -- DeviceRows.project / colsumsq / smooth(after=True) (emg3d_rows_project,
emg3d_rows_colsumsq, emg3d_rows_smooth_l; k_rows_project on v_mfma_f64_16x16x4_f64, k_rows_colsumsq).

1. Exact integers (R in -8 .. 8, M in -4 .. 4: every partial sum is an integer far below 2^53, so any order of summation gives the
   same float64): project EQUALS the integer product at every (n_rows, m, n_cols) of tail rows, tail tiles, a block of output rows
   and one more, tail columns, a panel and one more, several panels; the source is unchanged.
2. Random floats against np.longdouble within the dot-product bound gamma_{n_rows + 2} |M| |R|; twice the same bits.
3. Locality: the rows of M permuted, a store of some of the columns, zero padding, a NaN in one column, m across a block boundary.
4. Principal rows: M = Lambda_k^-1/2 U_k^T from eigh(gram()) gives orthonormal rows.
5. colsumsq bit for bit its numpy loop; smooth(after=True) bit for bit SmoothingCovariance.sqrt(host=True); the refusals."""
import numpy as np
import pytest

from test_gpu_row_covariance import _fill, _grid
from test_row_covariance_host import first_path1

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
N_ROWS = [1, 3, 4, 5, 15, 16, 17, 33, 129]


def _em():
    import emg3d_amd as em
    return em


def _plan():
    p = _em()._lib.rows_project_plan(1, 1, 1)
    return p["block"], p["cols"]


def _rows(store):
    return np.array([store.get_row(i) for i in range(store.n_rows)])


def _project(store, M):
    with store.project(M) as y:
        assert y.n_rows == M.shape[0] and y.n_cols == store.n_cols
        return _rows(y)


# ---- 1. exact integers --------------------------------------------------------------------------------------------------------
_INT = {}


def _int_data():
    """One draw, shared by all cases: the first rows and columns of it."""
    if not _INT:
        B, P = _plan()
        rng = np.random.default_rng(118)
        _INT["R"] = rng.integers(-8, 9, (max(N_ROWS), 2 * P + 7))
        _INT["M"] = rng.integers(-4, 5, (B + 1, max(N_ROWS)))
        for a in _INT.values():
            a.setflags(write=False)
    return _INT["R"], _INT["M"]


@pytest.mark.parametrize("n_rows", N_ROWS)
def test_exact_integer_data(n_rows):
    em = _em()
    B, P = _plan()
    Rall, Mall = _int_data()
    for n_cols in (1, 15, 16, 17, P - 1, P, P + 1, 2 * P + 7):
        Ri = Rall[:n_rows, :n_cols]
        R = Ri.astype(np.float64)
        with _fill(em, R) as store:
            for m in (1, 15, 16, 17, B, B + 1):
                Mi = Mall[:m, :n_rows]
                got = _project(store, Mi.astype(np.float64))
                want = Mi @ Ri                                  # int64
                bad = np.argwhere(got != want)
                assert got.shape == want.shape and bad.size == 0, (n_rows, m, n_cols, bad[:8])
            assert np.array_equal(_rows(store), R), (n_rows, n_cols)         # the source is unchanged, row for row


# ---- 2. random floats ---------------------------------------------------------------------------------------------------------
def _gamma(n):
    return n * U / (1 - n * U)


@pytest.mark.parametrize("case", ["17 to 40", "33 to 5"])
def test_random_float_data(case):
    em = _em()
    B, P = _plan()
    n_rows, m, n_cols = (17, 40, P + 1) if case == "17 to 40" else (33, 5, 3 * P + 7)
    rng = np.random.default_rng(n_rows)
    R = rng.standard_normal((n_rows, n_cols)) * 10.0 ** rng.uniform(-3, 3, (n_rows, 1))
    M = rng.standard_normal((m, n_rows))
    with _fill(em, R) as store:
        got = _project(store, M)
        again = _project(store, M)
    assert got.tobytes() == again.tobytes()                     # twice the same bits
    exact = M.astype(np.longdouble) @ R.astype(np.longdouble)
    bound = _gamma(n_rows + 2) * (np.abs(M) @ np.abs(R))
    ratio = float((np.abs(got - exact) / bound).max())
    print(f"project {n_rows} -> {m}, {n_cols} columns: largest error / (gamma_(n_rows+2) |M| |R|) = {ratio:.3f}")
    assert ratio <= 1.0


# ---- 3. locality ----------------------------------------------------------------------------------------------------------------
_LOC = {}


def _loc_case():
    """A source of 17 rows and 2 P + 7 columns, M with B + 1 rows, and the result, computed once."""
    if not _LOC:
        em = _em()
        B, P = _plan()
        rng = np.random.default_rng(7)
        R = rng.standard_normal((17, 2 * P + 7))
        M = rng.standard_normal((B + 1, 17))
        with _fill(em, R) as store:
            Y = _project(store, M)
        for a in (R, M, Y):
            a.setflags(write=False)
        _LOC.update(R=R, M=M, Y=Y)
    return _LOC["R"], _LOC["M"], _LOC["Y"]


def test_rows_of_m_permuted_and_a_block_boundary():
    em = _em()
    B, P = _plan()
    R, M, Y = _loc_case()
    perm = np.random.default_rng(8).permutation(M.shape[0])
    with _fill(em, R) as store:
        assert np.array_equal(_project(store, M[perm]), Y[perm])
        # m = B + 1 is the stack of its two blocks on their own; a row alone is that row
        assert np.array_equal(np.vstack([_project(store, M[:B]), _project(store, M[B:])]), Y)
        assert np.array_equal(_project(store, M[40:41]), Y[40:41])
        # out= of the right size is reused
        with em.solver.DeviceRows(M.shape[0], R.shape[1]) as out:
            assert store.project(M, out=out) is out
            assert np.array_equal(_rows(out), Y)
            assert store.project(M[perm], out=out) is out and np.array_equal(_rows(out), Y[perm])


def test_a_store_of_some_columns():
    em = _em()
    B, P = _plan()
    R, M, Y = _loc_case()
    with _fill(em, np.ascontiguousarray(R[:, 5:5 + P + 3])) as part:
        assert np.array_equal(_project(part, M), Y[:, 5:5 + P + 3])


def test_zero_padding_changes_nothing():
    em = _em()
    R, M, Y = _loc_case()
    Rz = np.vstack([R, np.zeros((3, R.shape[1]))])
    Mz = np.hstack([M, np.zeros((M.shape[0], 3))])
    with _fill(em, Rz) as store:
        assert np.all(_project(store, Mz) == Y)


@pytest.mark.parametrize("where", ["inside", "last"])
def test_a_nan_stays_in_its_column(where):
    em = _em()
    R, M, Y = _loc_case()
    assert R.shape[1] % 16 != 0
    col = 70 if where == "inside" else R.shape[1] - 1
    Rn = R.copy()
    Rn[9, col] = np.nan
    with _fill(em, Rn) as store:
        got = _project(store, M)
    assert np.all(np.isnan(got[:, col]))
    keep = np.arange(R.shape[1]) != col
    assert np.array_equal(got[:, keep], Y[:, keep])


# ---- 4. principal rows ----------------------------------------------------------------------------------------------------------
def test_principal_rows_are_orthonormal():
    em = _em()
    n_rows, n_cols, k = 33, 200, 7
    R = np.random.default_rng(33).standard_normal((n_rows, n_cols))
    with _fill(em, R) as store:
        G = store.gram()
        lam, Uv = np.linalg.eigh(G)
        cond = float(lam[-1] / lam[0])
        assert cond < 1e3
        M = (Uv[:, -k:] / np.sqrt(lam[-k:])).T
        with store.project(M) as pr:
            Gk = pr.gram()
    dev = float(np.abs(Gk - np.eye(k)).max())
    tol = 8 * n_cols * 2 * U * cond
    print(f"principal rows: |gram - I| = {dev:.3e}, cond(G) = {cond:.3e}, bound {tol:.3e}")
    assert dev <= tol


# ---- 5. colsumsq, smooth(after=True), refusals ------------------------------------------------------------------------------------
def _colsumsq_loop(R, s=None):
    acc = np.zeros(R.shape[1])
    for i in range(R.shape[0]):
        acc = acc + R[i] * R[i] if s is None else acc + s[i] * (R[i] * R[i])
    return acc


def test_colsumsq_equals_its_numpy_loop_bitwise():
    em = _em()
    B, P = _plan()
    rng = np.random.default_rng(5)
    for n_rows, n_cols in ((1, 1), (3, 17), (17, 257), (33, 2 * P + 7)):
        R = rng.standard_normal((n_rows, n_cols)) * 10.0 ** rng.uniform(-3, 3, (n_rows, 1))
        s = rng.uniform(0.1, 3.0, n_rows)
        with _fill(em, R) as store:
            for sv in (None, s):
                got, want = store.colsumsq(sv), _colsumsq_loop(R, sv)
                assert got.shape == (n_cols,) and got.tobytes() == want.tobytes(), (n_rows, n_cols, sv is not None)
            with pytest.raises(ValueError):
                store.colsumsq(np.ones(n_rows + 1))


def _smooth_case(em, shape, planes, passes, n_rows, scaled=True, lengths=(120.0, 60.0, 90.0)):
    grid = _grid(em, shape)
    rng = np.random.default_rng(sum(shape) + planes + passes)
    ncell = int(np.prod(shape))
    one = lambda: rng.uniform(0.5, 2.0, shape)
    std = (tuple(one() for _ in range(3)) if planes == 3 else one()) if scaled else 1.0
    cov = em.maps.SmoothingCovariance(grid, lengths, std=std, passes=passes)
    R = rng.standard_normal((n_rows, planes * ncell))

    def host(f, row):
        parts = tuple(p.reshape(shape, order='F') for p in row.reshape(planes, ncell))
        got = f(parts if planes == 3 else parts[0], host=True)
        return np.concatenate([g.ravel(order='F') for g in (got if planes == 3 else (got,))])
    with _fill(em, R) as store, store.clone() as twin:
        store.smooth(shape, planes, cov.factors, cov.passes, scale=cov.scale(planes), after=True)
        twin.smooth(shape, planes, cov.factors, cov.passes, scale=cov.scale(planes))
        for i in range(n_rows):
            got, want = store.get_row(i), host(cov.sqrt, R[i])
            assert got.tobytes() == want.tobytes(), (shape, planes, passes, i, float(np.abs(got - want).max()))
            assert twin.get_row(i).tobytes() == host(cov.sqrt_t, R[i]).tobytes(), (shape, planes, passes, i)       # after=False: L^T still


@pytest.mark.parametrize("n_rows", [1, 5])
def test_smooth_after_equals_sqrt_bitwise(n_rows):
    em = _em()
    for planes in (1, 3):
        for passes in (1, 3):
            _smooth_case(em, (33, 5, 7), planes, passes, n_rows)
    _smooth_case(em, (3, 5, 1), 1, 2, n_rows)                               # y is the last active axis
    nz = first_path1(em._lib, 2)
    assert em._lib.rows_smooth_plan((2, 2, nz), 2)["path"] == 1
    _smooth_case(em, (2, 2, nz), 1, 2, n_rows)                              # the HBM path carries the scale
    _smooth_case(em, (1, 1, 1), 1, 1, n_rows)                               # the scale kernel alone
    _smooth_case(em, (33, 5, 7), 1, 2, n_rows, scaled=False)               # no scale: L == L^T


def test_refusals():
    em = _em()
    lib, h = em._lib, em._lib.load()
    rng = np.random.default_rng(2)
    R = rng.standard_normal((5, 40))
    M = rng.standard_normal((3, 5))
    with _fill(em, R) as store, em.solver.DeviceRows(3, 40) as ok, em.solver.DeviceRows(4, 40) as rows4, \
            em.solver.DeviceRows(3, 41) as cols41:
        Mc = np.ascontiguousarray(M)
        assert h.emg3d_rows_project(store._h, lib.ptr(Mc), 3, ok._h) == 0
        assert h.emg3d_rows_project(store._h, lib.ptr(Mc), 5, store._h) == -2              # dst is src
        assert h.emg3d_rows_project(store._h, lib.ptr(Mc), 3, rows4._h) == -2              # wrong m
        assert h.emg3d_rows_project(store._h, lib.ptr(Mc), 3, cols41._h) == -2             # wrong n_cols
        assert h.emg3d_rows_project(store._h, lib.ptr(Mc), 0, ok._h) == -2
        assert h.emg3d_rows_project(store._h, None, 3, ok._h) == -2
        assert h.emg3d_rows_project(None, lib.ptr(Mc), 3, ok._h) == -2
        assert h.emg3d_rows_project(store._h, lib.ptr(Mc), 3, None) == -2
        assert h.emg3d_rows_colsumsq(None, None, lib.ptr(np.zeros(40))) == -2
        assert h.emg3d_rows_colsumsq(store._h, None, None) == -2
        for out in (store, rows4, cols41, "a store"):
            with pytest.raises(ValueError, match="out"):
                store.project(M if out is not store else rng.standard_normal((5, 5)), out=out)
        for bad in (rng.standard_normal((3, 4)), rng.standard_normal((3, 6)), rng.standard_normal(5), np.zeros((0, 5))):
            with pytest.raises(ValueError, match="shape"):
                store.project(bad)
        with pytest.raises(TypeError, match="real"):
            store.project(M + 0j)
        assert np.array_equal(_rows(store), R)                                              # a refused call changes nothing
        closed = em.solver.DeviceRows(3, 40)
        closed.close()
        with pytest.raises(RuntimeError, match="closed"):
            store.project(M, out=closed)
    with pytest.raises(RuntimeError, match="closed"):
        store.project(M)
    with pytest.raises(RuntimeError, match="closed"):
        store.colsumsq()
