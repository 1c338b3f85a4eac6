"""GPU: optimize.RowStore.project / resolution_diagonal / posterior_variance.

1. On the model-grid `mapped` survey of tests/test_gpu_row_covariance.py (140 cells) against the dense route in np.longdouble: C = diag(cm),
   or assembled from cov.apply(unit vector, host=True); A = J C J^T + damping W^-1 solved by Gaussian elimination with partial
   pivoting; diag(C - C J^T A^-1 J C) and diag(C J^T A^-1 J).  The device route factorises a matrix whose entries differ from the
   dense route's by rounding and whose condition number is kappa: 16 kappa eps max(diag C), the form and the factor that file
   uses for `step`.
2. On the small computational-grid survey (one plane and `components`): posterior_variance equals its definition spelled out with
   gram, project, smooth, colsumsq and cov.diagonal bit for bit; 0 <= resolution <= 1 and posterior <= prior up to that bound; a
   larger damping resolves every cell less; the temporary store is gone after the call.
3. The refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _em():
    import emg3d_amd as em
    return em


def _planes(x):
    return x if isinstance(x, tuple) else (x,)


def _flat(x):
    return np.concatenate([p.ravel(order='F') for p in _planes(x)])


# ---- 1. the dense route -----------------------------------------------------------------------------------------------------------
def test_against_the_dense_route_on_a_model_grid():
    em = _em()
    from conftest import load_golden
    from test_gpu_jacobian import OPTS as JOPTS
    from test_gpu_model_grid import SOURCES as MSOURCES, _models
    from test_model_grid_host import grid_pairs
    from test_row_covariance_host import solve_longdouble
    g = load_golden("survey_jacobian.npz")
    model_grid, grid = grid_pairs(em, ['unaligned'])['unaligned']
    model = _models(em, model_grid, 'Resistivity')
    rec = tuple(g['rec'])
    rng = np.random.default_rng(9)
    vnM = tuple(int(n) for n in model_grid.vnC)
    cov = em.maps.SmoothingCovariance(model_grid, (300.0, 200.0, 100.0), std=rng.uniform(0.5, 2.0, vnM), passes=2)
    cm = rng.uniform(0.5, 2.0, vnM)
    kw = dict(JOPTS, tol=1e-6, batch=2, model_grid=model_grid)
    with em.optimize.SurveyJacobian(grid, model, MSOURCES, [1.5, -1.2], rec, **kw) as sj:
        store = sj.park_rows(mapped=True)
        n, ncell = store.n_rows, model_grid.nC
        J = np.array([store.row(i).ravel(order='F') for i in range(n)]).astype(np.longdouble)
        w = rng.uniform(0.5, 2.0, n)
        Winv = np.diag(1 / w.astype(np.longdouble))

        def dense(C, damping):
            A = J @ C @ J.T + np.longdouble(damping) * Winv
            X = J.T @ solve_longdouble(A, J)                    # J^T A^-1 J
            return np.linalg.cond(A.astype(np.float64)), np.diag(C - C @ X @ C), np.diag(C @ X)

        # a diagonal cm on the plain store
        Cd = np.diag(cm.ravel(order='F').astype(np.longdouble))
        damping = 1e-3 * np.trace(store.gram(cm)) / n
        kappa, post, res = dense(Cd, damping)
        got_post = store.posterior_variance(w, cm=cm, damping=damping).ravel(order='F')
        got_res = store.resolution_diagonal(w, cm=cm, damping=damping).ravel(order='F')
        cmax = float(cm.max())
        assert cmax >= 1.0                          # (so that the resolution, of order one, is held to no more than the bound)
        e_post = float(np.abs(got_post - post).max() / cmax)
        e_res = float(np.abs(got_res - res).max())
        print(f"diagonal cm: cond {kappa:.3e}; posterior error / (cond eps max C) = {e_post / (kappa * 2 * U):.3f}, "
              f"resolution error / (cond eps) = {e_res / (kappa * 2 * U):.3f}")
        assert e_post <= 16 * kappa * 2 * U and e_res <= 16 * kappa * 2 * U
        # the smoothing covariance
        C = np.empty((ncell, ncell), dtype=np.longdouble)
        for j in range(ncell):
            e = np.zeros(ncell)
            e[j] = 1.0
            C[:, j] = cov.apply(e.reshape(vnM, order='F'), host=True).ravel(order='F')
        with store.with_covariance(cov) as new:
            damping = 1e-3 * np.trace(new.gram()) / n
            got = new.posterior_variance(w, damping=damping).ravel(order='F')
        kappa, post, _ = dense(C, damping)
        cmax = float(np.diag(C).max())
        err = float(np.abs(got - post).max() / cmax)
        print(f"smoothing covariance: cond {kappa:.3e}; posterior error / (cond eps max diag C) = {err / (kappa * 2 * U):.3f}")
        assert err <= 16 * kappa * 2 * U


# ---- 2. the small survey ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("components", [False, True], ids=["sum", "components"])
def test_on_the_survey(components, monkeypatch):
    em = _em()
    from test_gpu_row_store import _model
    from test_gpu_sensitivity_diagonal import FREQS, OPTS, SOURCES, _survey
    grid, rec, rng, sig = _survey(em)
    model = _model(em, grid, sig, "iso")
    vnC = tuple(int(n) for n in grid.vnC)
    planes = 3 if components else 1
    std = tuple(rng.uniform(0.5, 2.0, vnC) for _ in range(3)) if components else rng.uniform(0.5, 2.0, vnC)
    cov = em.maps.SmoothingCovariance(grid, (150.0, 100.0, 60.0), std=std, passes=2)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, tol=1e-8, **OPTS) as sj:
        store = sj.park_rows(components=components)
        n = store.n_rows
        w = rng.uniform(0.5, 2.0, n)
        with store.with_covariance(cov) as new:
            G = new.gram()
            damping = 1e-3 * np.trace(G) / n
            A = G + damping * np.diag(1 / w)
            kappa = np.linalg.cond(A)
            got = new.posterior_variance(w, damping=damping)
            assert isinstance(got, tuple) == components and all(p.shape == vnC for p in _planes(got))
            # ... is its definition, bit for bit
            P = np.linalg.solve(np.linalg.cholesky(A), np.eye(n))
            with new.project(P) as T:
                assert T.n_rows == n and T.n_cols == new.rows.n_cols
                T.smooth(vnC, planes, cov.factors, cov.passes, scale=cov.scale(planes), after=True)
                q = T.colsumsq()
            prior = _flat(cov.diagonal())
            assert _flat(got).tobytes() == (prior - q).tobytes()
            tol = 16 * kappa * 2 * U * float(prior.max())
            assert np.all(_flat(got) <= prior + tol) and np.all(_flat(got) >= -tol)
            # the temporary store is gone: a second call allocates nothing that stays
            made, orig = [], em.solver.DeviceRows.project

            def spy(self, M, out=None):
                made.append(orig(self, M, out=out))
                return made[-1]
            monkeypatch.setattr(em.solver.DeviceRows, "project", spy)
            b1 = new.device_bytes
            again = new.posterior_variance(w, damping=damping)
            monkeypatch.undo()
            assert _flat(again).tobytes() == _flat(got).tobytes() and new.device_bytes == b1
            assert len(made) == 1 and made[0]._h is None and made[0].n_rows == n
        # the plain store: resolution and posterior with a diagonal cm
        cm = tuple(rng.uniform(0.5, 2.0, vnC) for _ in range(3)) if components else rng.uniform(0.5, 2.0, vnC)
        c = _flat(cm)
        G = store.gram(cm)
        b0 = store.device_bytes                                 # (the block and the workspace of gram)
        damping = 1e-3 * np.trace(G) / n
        kappa = np.linalg.cond(G + damping * np.diag(1 / w))
        tol = 16 * kappa * 2 * U
        res = store.resolution_diagonal(w, cm=cm, damping=damping)
        post = store.posterior_variance(w, cm=cm, damping=damping)
        assert isinstance(res, tuple) == components and all(p.shape == vnC for p in _planes(res))
        r, p = _flat(res), _flat(post)
        assert np.all(r >= -tol) and np.all(r <= 1 + tol) and r.max() > 0
        assert np.all(p <= c + tol * c.max()) and np.all(p >= -tol * c.max())
        with store.project(np.linalg.solve(np.linalg.cholesky(G + damping * np.diag(1 / w)), np.eye(n))) as T:
            q = T.colsumsq()
        assert r.tobytes() == (c * q).tobytes() and p.tobytes() == (c - c * c * q).tobytes()
        # a larger damping resolves every cell less
        more = _flat(store.resolution_diagonal(w, cm=cm, damping=10 * damping))
        assert np.all(more <= r + tol) and more.sum() < r.sum()
        # no cm: c = 1
        r1 = _flat(store.resolution_diagonal(w, damping=damping))
        p1 = _flat(store.posterior_variance(w, damping=damping))
        assert np.all(np.abs((1.0 - r1) - p1) <= 4 * U)
        # device bytes: those before plus workspace growth only (at most the operand K^-1 of project) -- no second block stays
        grown = store.device_bytes
        store.resolution_diagonal(w, cm=cm, damping=damping)
        assert store.device_bytes == grown and 0 <= grown - b0 <= n * n * 8 + 256


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    em = _em()
    from test_gpu_row_store import _model
    from test_gpu_sensitivity_diagonal import FREQS, OPTS, SOURCES, _survey
    grid, rec, rng, sig = _survey(em)
    model = _model(em, grid, sig, "iso")
    vnC = tuple(int(n) for n in grid.vnC)
    cov = em.maps.SmoothingCovariance(grid, (150.0, 100.0, 60.0), passes=1)
    with em.optimize.SurveyJacobian(grid, model, SOURCES[:1], FREQS, rec, batch=2, tol=1e-6, **OPTS) as sj:
        store = sj.park_rows()
        n = store.n_rows
        w = np.ones(n)
        with store.with_covariance(cov) as new:
            with pytest.raises(ValueError, match=r"diag\(L X L\^-1\) is not a column sum.*posterior_variance"):
                new.resolution_diagonal(w, damping=1.0)
            with pytest.raises(ValueError, match="store it was made from"):
                new.posterior_variance(w, cm=np.ones(vnC), damping=1.0)
        # A not positive definite: every row the same, no damping
        dup = em.optimize.RowStore(store.rows.clone(), store.index, store._shape, store._vnM, store.components, store._real)
        with dup:
            row0 = dup.rows.get_row(0)
            for i in range(1, n):
                dup.rows.set_row(i, row0)
            for call in (dup.posterior_variance, dup.resolution_diagonal):
                with pytest.raises(ValueError, match="damping"):
                    call(w, damping=0.0)
            assert dup.posterior_variance(w, damping=1e-3 * float(row0 @ row0)).shape == vnC        # ... and with damping it is
        with pytest.raises(ValueError, match="shape"):
            store.project(np.ones((2, n + 1)))
        with pytest.raises(TypeError, match="real"):
            store.project(np.ones((2, n)) * 1j)
        with store.project(np.eye(n)[:2]) as two:
            assert np.array_equal(two.get_row(1), store.rows.get_row(1))
