"""GPU, end to end: optimize.SurveyJacobian.park_rows -- the rows of sensitivity_rows parked in a device row store
(emg3d_mg_sens_rows_park, k_rows_park) -- and the RowStore's products, on the 8 x 8 x 8 survey of tests/test_gpu_sensitivity_diagonal.py
(3 sources x (1 Hz, s = 2) x 4 receivers, batch = 2) and the model-grid case of tests/test_gpu_model_grid.py.

* every parked row equals the matching real or imaginary part of sensitivity_rows(...) BIT FOR BIT: components, mapped, an isotropic
  and a tri-axial model with a log map, a model grid;
* index and selection: 3 * 4 * 2 + 3 * 4 rows in the order (i_freq, i_src, i_rec, part); a masked receiver loses its rows and solves;
* gram within the dot-product bound of tests/test_gpu_rows.py against longdouble numpy on the same rows, rmatvec bit for bit the numpy
  loop, step bit for bit its definition;
* the store is a snapshot: set_model leaves it as it was, a new park_rows gives the new rows."""
import numpy as np
import pytest

from test_gpu_sensitivity_diagonal import FREQS, OPTS, SOURCES, _survey

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _model(em, grid, sig, kind):
    if kind == "iso":
        return em.Model(grid, sig, mapping='Conductivity')
    return em.Model(grid, np.log10(sig), np.log10(1.5 * sig), np.log10(0.6 * sig), mapping='LgConductivity')


def _check_rows(sj, store, components, mapped, sel=None):
    """Every row of the store against sensitivity_rows of its frequency; -> the number of rows compared."""
    want = [sj.sensitivity_rows(j, components=components, mapped=mapped) for j in range(sj.n_freq)]
    for i, (j, s, r, part) in enumerate(store.index):
        got = store.row(i)
        ref = want[j] if components else (want[j],)
        got = got if components else (got,)
        assert len(got) == len(ref)
        for g, w in zip(got, ref):
            w = w[s, r]
            w = (w.real, w.imag)[part] if np.iscomplexobj(w) else w
            assert part == 0 or sj.freqs[j] > 0
            assert g.shape == w.shape and np.abs(w).max() > 0
            assert np.array_equal(g, w), (i, j, s, r, part, float(np.abs(g - w).max()))
    return len(store.index)


def _index(sel=None):
    return [(j, s, r, part) for j in range(2) for s in range(3) for r in range(4) if sel is None or sel[s, j, r]
            for part in range(2 if FREQS[j] > 0 else 1)]


@pytest.mark.parametrize("mapped", [False, True], ids=["sigma", "mapped"])
@pytest.mark.parametrize("components", [False, True], ids=["sum", "components"])
@pytest.mark.parametrize("kind", ["iso", "tri-log"])
def test_parked_rows_equal_sensitivity_rows_bitwise(kind, components, mapped):
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = _model(em, grid, sig, kind)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, tol=1e-8, **OPTS) as sj:
        before = sj.device_bytes
        store = sj.park_rows(components=components, mapped=mapped)
        assert np.array_equal(store.index, _index()) and store.n_rows == 3 * 4 * 2 + 3 * 4
        ncols = (3 if components else 1) * grid.nC
        assert store.rows.n_cols == ncols
        chain = 3 * grid.nC * 8 if mapped else 0
        assert store.device_bytes == (36 * ncols * 8 + 255) // 256 * 256 + (chain + 255) // 256 * 256
        assert all(len(row) == 4 and all(p is not None and p[0]['exit'] == 0 for p in row) for row in store.info)
        assert all(p[1]['exit'] == 0 for p in store.info[0]) and all(p[1] is None for p in store.info[1])
        assert _check_rows(sj, store, components, mapped) == 36
        assert sj.device_bytes >= before            # (the store is not the handles': only their row buffers may have grown)
    with pytest.raises(RuntimeError, match="closed"):
        store.row(0)                                 # the SurveyJacobian closed its store


@pytest.mark.parametrize("components", [False, True], ids=["sum", "components"])
@pytest.mark.parametrize('kind', ['Resistivity', 'Conductivity-tri'])
def test_parked_rows_on_a_model_grid(kind, components):
    """12 x 10 x 8 from 7 x 5 x 4 (tests/test_gpu_model_grid.py), 3 sources x (1.5 Hz, s = 1.2), batch = 2: the rows have the model
    grid's size, the device applies Q (.) A^T (F (.) .) before it parks them; mapped=False is refused."""
    import emg3d_amd as em
    from conftest import load_golden
    from test_gpu_jacobian import OPTS as JOPTS
    from test_gpu_model_grid import SOURCES as MSOURCES, _models
    from test_model_grid_host import grid_pairs
    g = load_golden("survey_jacobian.npz")
    model_grid, grid = grid_pairs(em, ['unaligned'])['unaligned']
    model = _models(em, model_grid, kind)
    rec = tuple(g['rec'])
    n_rec = len(rec[0])
    kw = dict(JOPTS, tol=1e-6, batch=2, model_grid=model_grid)
    with em.optimize.SurveyJacobian(grid, model, MSOURCES, [1.5, -1.2], rec, **kw) as sj:
        with pytest.raises(ValueError, match="model grid"):
            sj.park_rows()
        sel = np.zeros((3, 2, n_rec), dtype=bool)
        sel[[0, 2]] = True
        sel[:, :, 1] = False                        # sources 0 and 2, every receiver but 1
        with sj.park_rows(data=sel, components=components, mapped=True) as store:
            assert store.rows.n_cols == (3 if components else 1) * model_grid.nC
            assert store.n_rows == 2 * (n_rec - 1) * 3 and store.info[0][1] is None and store.info[1][1] is None
            assert _check_rows(sj, store, components, True) == store.n_rows
            assert store.row(0)[0].shape == tuple(model_grid.vnC) if components else store.row(0).shape == tuple(model_grid.vnC)


def _gamma(n):
    return n * U / (1 - n * U)


def test_index_products_and_step():
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = _model(em, grid, sig, "iso")
    vnC = tuple(int(n) for n in grid.vnC)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, tol=1e-8, **OPTS) as sj:
        store = sj.park_rows()
        n = store.n_rows
        assert n == 36 and store.index.shape == (36, 4) and np.array_equal(store.index, _index())
        R = np.array([store.row(i).ravel(order='F') for i in range(n)])
        cm = rng.uniform(0.5, 2.0, vnC)
        cmf = cm.ravel(order='F')
        Rl = R.astype(np.longdouble)
        # gram
        G = store.gram(cm)
        bound = _gamma(R.shape[1] + 2) * ((np.abs(R) * cmf) @ np.abs(R).T)
        err = np.abs(G - (Rl * cmf) @ Rl.T)
        print(f"gram vs longdouble: largest error / bound {float((err / bound).max()):.3f}")
        assert np.all(err <= bound) and np.array_equal(G, G.T) and np.array_equal(store.gram(cm), G)
        assert np.all(np.abs(store.gram() - Rl @ Rl.T) <= _gamma(R.shape[1] + 2) * (np.abs(R) @ np.abs(R).T))
        assert np.all(np.linalg.eigvalsh(G) > -1e-12 * np.abs(G).max())
        # rmatvec: the ascending loop
        y = rng.standard_normal(n)
        acc = np.zeros(R.shape[1])
        for i in range(n):
            acc = acc + y[i] * R[i]
        got = store.rmatvec(y, cm)
        assert got.shape == vnC and np.array_equal(got.ravel(order='F'), cmf * acc)
        assert np.array_equal(store.rmatvec(y).ravel(order='F'), acc)
        # matvec: J v without a solve, stacked; data() folds it
        v = rng.standard_normal(vnC)
        jv = store.matvec(v)
        vf = v.ravel(order='F')
        assert np.all(np.abs(jv - Rl @ vf.astype(np.longdouble)) <= _gamma(R.shape[1] + 2) * (np.abs(R) @ np.abs(vf)))
        d = store.data(jv)
        assert d.shape == (3, 2, 4) and d.dtype == np.complex128 and np.all(d[:, 1].imag == 0) and np.all(d[:, 0].imag != 0)
        assert np.array_equal(store.stack(d), jv)
        assert np.array_equal(store.rmatvec(d, cm), store.rmatvec(jv, cm))         # a data array is stacked first
        # ... and it is the derivative jvec computes with solves (to the solves' accuracy)
        full = sj.jvec(v)
        assert np.abs(d - full).max() <= 1e-5 * np.abs(full).max()
        # step: its definition, composed from the public pieces
        W = rng.uniform(0.5, 2.0, (3, 2, 4))
        resid = (rng.standard_normal((3, 2, 4)) + 1j * rng.standard_normal((3, 2, 4))) * np.abs(sj.synthetic)
        resid[:, 1] = resid[:, 1].real
        r, w = store.stack(resid), store.stack(W)
        damping = 1e-3 * np.trace(G) / n
        want = store.rmatvec(np.linalg.solve(store.gram(cm) + damping * np.diag(1 / w), r), cm)
        assert np.array_equal(store.step(resid, W, cm=cm, damping=damping), want)
        assert np.array_equal(store.step(r, w, cm=cm, damping=damping), want) and np.abs(want).max() > 0
        with pytest.raises(ValueError):
            store.matvec(v[:-1])
        with pytest.raises(ValueError):
            store.matvec((v, v, v))                 # a tuple needs a store parked with components=True
        with pytest.raises(ValueError):
            store.rmatvec(y[:-1])


def test_selection_and_set_model():
    """A mask without receiver 2 at frequency 0 removes its rows (6) and its solves (info None); the rest are the same rows.  After
    set_model the store still holds the rows of the model it was parked for; a new park_rows gives the new ones."""
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = _model(em, grid, sig, "iso")
    other = em.Model(grid, sig * 10 ** rng.uniform(-0.2, 0.2, grid.nC), mapping='Conductivity')
    sel = np.ones((3, 2, 4), dtype=bool)
    sel[:, 0, 2] = False
    sel[1, 1, 0] = False                            # one datum of a receiver that is still solved for
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, tol=1e-8, **OPTS) as sj:
        store = sj.park_rows(data=sel)
        assert store.n_rows == 36 - 6 - 1 and np.array_equal(store.index, _index(sel))
        assert store.info[0][2] is None and all(store.info[0][r] is not None for r in (0, 1, 3))
        assert all(p is not None for p in store.info[1])
        assert _check_rows(sj, store, False, False) == 29
        old = [store.row(i) for i in range(store.n_rows)]
        G = store.gram()
        with pytest.raises(TypeError):
            sj.park_rows(data=np.ones((3, 2, 4)))
        with pytest.raises(ValueError):
            sj.park_rows(data=np.zeros((3, 2, 4), dtype=bool))
        with pytest.raises(ValueError):
            sj.park_rows(data=np.ones((2, 2), dtype=bool))
        sj.set_model(other)
        assert all(np.array_equal(store.row(i), old[i]) for i in range(store.n_rows)) and np.array_equal(store.gram(), G)
        new = sj.park_rows(data=sel)
        assert not np.array_equal(new.row(0), old[0])
        assert _check_rows(sj, new, False, False) == 29
        store.close()
        assert np.array_equal(new.gram(), new.gram())          # closing one store leaves the other
    with pytest.raises(RuntimeError, match="closed"):
        sj.park_rows()
