"""GPU: the row store through the C ABI and solver.DeviceRows, filled from the host (no solve) -- emg3d_rows_gram (k_rows_gram on
v_mfma_f64_16x16x4_f64, k_rows_gram_reduce), emg3d_rows_matvec, emg3d_rows_rmatvec.

1. Exact integer data: rows from {-8 .. 8}, cm from {1 .. 4}: every partial sum is an integer below 2^28, so every f64 result is exact
   WHATEVER the order, and must equal the integer result -- a wrong fragment map (the f32 C/D map on the f64 instruction, rows and
   columns swapped), a dropped tail column, tail row tile or slab boundary all give another integer.  The rows are random and not
   symmetric in (row, column).
2. Random float data against longdouble numpy within the standard dot-product bound gamma_{n_cols + 2} (|R| |cm| |R|^T), which holds
   for any summation order and with fused multiply-adds; rmatvec bit for bit the ascending numpy loop; the determinism contract.
3. Round trip, bytes, refusals, and the out-of-memory answer of the check before the allocation."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ROWS = [1, 15, 16, 17, 255, 256, 257, 700]
U = 2.0 ** -53


def _lib():
    from emg3d_amd import _lib
    return _lib


def _n_cols():
    S = _lib().rows_gram_plan(1, 1)["slab"]
    return S, [1, 3, 4, 5, 63, 64, 65, S - 1, S, S + 1, 3 * S + 7]


def _fill(em, R):
    store = em.solver.DeviceRows(*R.shape)
    for i, row in enumerate(R):
        store.set_row(i, row)
    return store


# ---- 1. exact integers --------------------------------------------------------------------------------------------------------
_INT = {}


def _int_data(n_cols):
    """One draw of 700 rows per n_cols, shared by all n_rows (the first n_rows rows of it)."""
    if n_cols not in _INT:
        rng = np.random.default_rng(1000 + n_cols)
        _INT[n_cols] = (rng.integers(-8, 9, (700, n_cols)), rng.integers(1, 5, n_cols), rng.integers(-8, 9, n_cols),
                        rng.integers(-8, 9, 700))
    return _INT[n_cols]


@pytest.mark.parametrize("n_rows", N_ROWS)
def test_exact_integer_data(n_rows):
    """All n_cols of the plan test (1 .. 3 S + 7: tail columns, one slab, a slab boundary, several slabs) at this n_rows (tail rows, a
    tail tile, one block, a block boundary, six blocks = 21 jobs).  The reference is formed by float64 matrix products, which are
    exact on these integers in any order (every partial sum is an integer below 2^28 < 2^53); where it is cheap it is formed in
    int64 as well."""
    import emg3d_amd as em
    S, cols = _n_cols()
    for n_cols in cols:
        Ri, cmi, vi, yi = _int_data(n_cols)
        Ri, yi = Ri[:n_rows], yi[:n_rows]
        assert 64 * 4 * n_cols < 2 ** 28
        R, cm, v, y = (a.astype(np.float64) for a in (Ri, cmi, vi, yi))
        G = ((R * cm) @ R.T).astype(np.int64)
        G1 = (R @ R.T).astype(np.int64)
        if n_rows * n_rows * n_cols <= 2e7:
            assert np.array_equal(G, (Ri * cmi) @ Ri.T) and np.array_equal(G1, Ri @ Ri.T)
        with _fill(em, R) as store:
            got, got1 = store.gram(cm), store.gram()
            assert got.shape == (n_rows, n_rows)
            bad = np.argwhere(got != G)
            assert bad.size == 0, (n_rows, n_cols, bad[:8], got[tuple(bad[0])], G[tuple(bad[0])])
            assert np.array_equal(got1, G1), (n_rows, n_cols)
            assert np.array_equal(store.matvec(v), Ri @ vi), (n_rows, n_cols)
            assert np.array_equal(store.rmatvec(y, cm), cmi * (yi @ Ri)), (n_rows, n_cols)
            assert np.array_equal(store.rmatvec(y), yi @ Ri), (n_rows, n_cols)


# ---- 2. random floats ---------------------------------------------------------------------------------------------------------
def _gamma(n):
    return n * U / (1 - n * U)


def _rmatvec_loop(R, y, cm=None):
    acc = np.zeros(R.shape[1])
    for i in range(R.shape[0]):
        acc = acc + y[i] * R[i]
    return acc if cm is None else cm * acc


@pytest.mark.parametrize("shape", ["17xS+1", "33x3S+7"])
def test_random_float_data(shape):
    import emg3d_amd as em
    S, _ = _n_cols()
    n_rows, n_cols = {"17xS+1": (17, S + 1), "33x3S+7": (33, 3 * S + 7)}[shape]
    rng = np.random.default_rng(77)
    R = rng.standard_normal((n_rows, n_cols)) * 10 ** rng.uniform(-3, 3, (n_rows, 1))
    cm = rng.uniform(0.1, 10., n_cols) * rng.choice([-1., 1.], n_cols, p=[0.1, 0.9])
    v, y = rng.standard_normal(n_cols), rng.standard_normal(n_rows)
    Rl = R.astype(np.longdouble)
    bound = _gamma(n_cols + 2) * ((np.abs(R) * np.abs(cm)) @ np.abs(R).T)
    with _fill(em, R) as store:
        G = store.gram(cm)
        err = np.abs(G - (Rl * cm) @ Rl.T)
        print(f"{shape}: gram, largest error / bound {float((err / bound).max()):.3f}")
        assert np.all(err <= bound)
        G1 = store.gram()
        assert np.all(np.abs(G1 - Rl @ Rl.T) <= _gamma(n_cols + 2) * (np.abs(R) @ np.abs(R).T))
        mv = store.matvec(v)
        errv = np.abs(mv - Rl @ v.astype(np.longdouble))
        boundv = _gamma(n_cols + 2) * (np.abs(R) @ np.abs(v))
        print(f"{shape}: matvec, largest error / bound {float((errv / boundv).max()):.3f}")
        assert np.all(errv <= boundv)
        assert np.array_equal(store.rmatvec(y, cm), _rmatvec_loop(R, y, cm))
        assert np.array_equal(store.rmatvec(y), _rmatvec_loop(R, y))
        # exactly symmetric, and the same bits at every call
        assert np.array_equal(G, G.T) and np.array_equal(G1, G1.T)
        assert np.array_equal(store.gram(cm), G) and np.array_equal(store.gram(), G1) and np.array_equal(store.matvec(v), mv)
    # A store filled with the rows in a permuted order gives the permuted G bit for bit: the summation order of an element follows
    # from n_cols alone, not from where its rows stand.  cm multiplies ONE operand of a product -- the row of the smaller index --,
    # so this holds where that factor cannot round differently: without cm, and with a cm of powers of two (exact products).  With a
    # general cm the row that carries the factor may change with the permutation, and the pair agrees to rounding (the bound above).
    perm = rng.permutation(n_rows)
    cm2 = 2.0 ** rng.integers(-3, 4, n_cols)
    with _fill(em, R) as store:
        G2 = store.gram(cm2)
    with _fill(em, R[perm]) as store:
        P1, P2, P = store.gram(), store.gram(cm2), store.gram(cm)
        assert np.array_equal(P1, G1[np.ix_(perm, perm)])
        assert np.array_equal(P2, G2[np.ix_(perm, perm)])
        assert np.all(np.abs(P - ((Rl * cm) @ Rl.T)[np.ix_(perm, perm)]) <= bound[np.ix_(perm, perm)])
        assert np.array_equal(store.matvec(v), mv[perm])


# ---- 3. round trip and errors -------------------------------------------------------------------------------------------------
def test_round_trip_bytes_and_refusals():
    import emg3d_amd as em
    lib = _lib()
    h = lib.load()
    rng = np.random.default_rng(5)
    R = rng.standard_normal((5, 37))
    with _fill(em, R) as store:
        assert store.device_bytes == (5 * 37 * 8 + 255) // 256 * 256
        for i in (4, 0, 2):
            assert np.array_equal(store.get_row(i), R[i])
        store.set_row(2, R[0])
        assert np.array_equal(store.get_row(2), R[0]) and np.array_equal(store.get_row(1), R[1])
        # the products' workspace is counted once it exists, grows to the largest call and is kept
        block = store.device_bytes
        store.gram(np.ones(37))
        grown = store.device_bytes
        assert grown > block
        store.gram(), store.matvec(np.ones(37)), store.rmatvec(np.ones(5)), store.gram(np.ones(37))
        assert store.device_bytes == grown
        buf = np.zeros(37)
        G = np.zeros((5, 5))
        for bad in (-1, 5, 2 ** 40):
            assert h.emg3d_rows_set(store._h, bad, lib.ptr(buf)) == -2 and h.emg3d_rows_get(store._h, bad, lib.ptr(buf)) == -2
        assert h.emg3d_rows_set(store._h, 0, None) == -2 and h.emg3d_rows_get(store._h, 0, None) == -2
        assert h.emg3d_rows_set(None, 0, lib.ptr(buf)) == -2
        assert h.emg3d_rows_gram(store._h, None, None) == -2 and h.emg3d_rows_gram(None, None, lib.ptr(G)) == -2
        assert h.emg3d_rows_matvec(store._h, None, lib.ptr(buf)) == -2 and h.emg3d_rows_matvec(store._h, lib.ptr(buf), None) == -2
        assert h.emg3d_rows_rmatvec(store._h, None, None, lib.ptr(buf)) == -2
        assert h.emg3d_rows_rmatvec(store._h, lib.ptr(buf), None, None) == -2
        assert np.array_equal(store.get_row(0), R[0])         # (the refused calls wrote nothing)
        with pytest.raises(IndexError):
            store.set_row(5, buf)
        with pytest.raises(ValueError):
            store.set_row(0, buf[:-1])
        with pytest.raises(ValueError):
            store.gram(np.ones(36))
    with pytest.raises(RuntimeError, match="closed"):
        store.gram()
    out = ctypes.c_void_p()
    assert h.emg3d_rows_create(0, 0, 5, ctypes.byref(out)) == -2 and h.emg3d_rows_create(0, 5, 0, ctypes.byref(out)) == -2
    assert h.emg3d_rows_create(0, 5, 5, None) == -2


def test_a_store_that_cannot_fit_is_refused_before_it_allocates():
    """8 rows of 2^40 columns are 2^46 bytes: out of memory from the check against emg3d_hip_mem_info, with the bytes needed and
    free in the message; a small store works in the same process afterwards."""
    import emg3d_amd as em
    lib = _lib()
    out = ctypes.c_void_p()
    assert lib.load().emg3d_rows_create(0, 8, 2 ** 40, ctypes.byref(out)) == 2 and not out.value
    free = lib.mem_info(0)
    with pytest.raises(lib.HipLibraryError, match=rf"{8 * 2 ** 40 * 8} bytes.*bytes are free"):
        em.solver.DeviceRows(8, 2 ** 40)
    assert lib.mem_info(0)["free"] >= free["free"] - (64 << 20)         # (nothing of that size was taken)
    R = np.arange(12.).reshape(3, 4)
    with _fill(em, R) as store:
        assert np.array_equal(store.gram(), R @ R.T)
