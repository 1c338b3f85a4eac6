"""CPU-only: optimize.Jacobian's argument checks (raised before the library is touched), the fixture
tests/golden/jacobian.npz against its generator's own asserts, and numpy restatements of the two operators the device
builds -- C(v) (cells -> edges) and the linear receiver operator P -- against the vectors the fixture stores."""
import numpy as np
import pytest

from conftest import load_golden


def _edge_shapes(vnC):
    nx, ny, nz = (int(n) for n in vnC)
    return ((nx, ny + 1, nz + 1), (nx + 1, ny, nz + 1), (nx + 1, ny + 1, nz))


def cells2edges_pec(vnC, vol, v3):
    """C(v): per component 1/4 of the sum of V_c v_c over the four cells around an edge; boundary (PEC) edges 0."""
    nx, ny, nz = (int(n) for n in vnC)
    out = [np.zeros(s) for s in _edge_shapes(vnC)]
    for c, v in enumerate(v3):
        if v is None:
            continue
        w = vol * np.asarray(v).reshape(vnC, order='F') / 4
        for a in (0, 1):
            for b in (0, 1):
                if c == 0:
                    out[0][:, a:ny + a, b:nz + b] += w
                elif c == 1:
                    out[1][a:nx + a, :, b:nz + b] += w
                else:
                    out[2][a:nx + a, b:ny + b, :] += w
    out[0][:, [0, -1], :] = 0; out[0][:, :, [0, -1]] = 0
    out[1][[0, -1], :, :] = 0; out[1][:, :, [0, -1]] = 0
    out[2][[0, -1], :, :] = 0; out[2][:, [0, -1], :] = 0
    return np.r_[out[0].ravel('F'), out[1].ravel('F'), out[2].ravel('F')]


def linear_receiver_matrix(grid, rec, fac):
    """Dense P (n_rec x nE): trilinear weights on the trimmed points of every component times the rotation factors."""
    shp = _edge_shapes(grid.vnC)
    off = np.cumsum([0] + [int(np.prod(s)) for s in shp])
    points = ((grid.cell_centers_x, grid.nodes_y, grid.nodes_z), (grid.nodes_x, grid.cell_centers_y, grid.nodes_z),
              (grid.nodes_x, grid.nodes_y, grid.cell_centers_z))
    nrec = fac.shape[1]
    P = np.zeros((nrec, grid.nE))
    for c in range(3):
        if not np.any(abs(fac[c]) > 1e-10):
            continue
        for r in range(nrec):
            idx, t = [], []
            for a in range(3):
                p = points[c][a][1:-1]
                x = rec[a][r]
                assert p[0] <= x <= p[-1]
                i = int(np.clip(np.searchsorted(p, x, side='left') - 1, 0, p.size - 2))
                idx.append(i + 1)
                t.append((x - p[i]) / (p[i + 1] - p[i]))
            for d0 in (0, 1):
                for d1 in (0, 1):
                    for d2 in (0, 1):
                        wgt = (t[0] if d0 else 1 - t[0]) * (t[1] if d1 else 1 - t[1]) * (t[2] if d2 else 1 - t[2])
                        lin = (idx[0] + d0) + shp[c][0] * ((idx[1] + d1) + shp[c][1] * (idx[2] + d2))
                        P[r, off[c] + lin] += fac[c][r] * wgt
    return P


def _setup():
    import emg3d_amd as em
    g = load_golden("gradient.npz")
    j = load_golden("jacobian.npz")
    grid = em.TensorMesh([g['hx'], g['hy'], g['hz']], origin=g['origin'])
    return em, g, j, grid


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the HIP library fails the test."""
    from emg3d_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "_open", boom)


def test_argument_errors_come_before_the_library(no_library):
    em, g, j, grid = _setup()
    rec = tuple(g['rec'])
    src, freq = g['src'], float(g['freq'])
    model = em.Model(grid, g['res'])
    with pytest.raises(NotImplementedError, match="permeability"):
        em.optimize.Jacobian(grid, em.Model(grid, g['res'], mu_r=np.full(grid.nC, 1.5)), src, freq, rec)
    with pytest.raises(NotImplementedError, match="permittivity"):
        em.optimize.Jacobian(grid, em.Model(grid, g['res'], epsilon_r=np.full(grid.nC, 3.)), src, freq, rec)
    with pytest.raises(NotImplementedError, match="magnetic"):
        em.optimize.Jacobian(grid, model, src, freq, rec, electric=False)
    with pytest.raises(ValueError, match="receiver_interpolation"):
        em.optimize.Jacobian(grid, model, src, freq, rec, receiver_interpolation='nearest')
    with pytest.raises(ValueError, match="nvec"):
        em.optimize.Jacobian(grid, model, src, freq, rec, nvec=0)
    with pytest.raises(ValueError, match="rec"):
        em.optimize.Jacobian(grid, model, src, freq, rec[:3])
    with pytest.raises(NotImplementedError, match="Krylov"):
        em.optimize.Jacobian(grid, model, src, freq, rec, sslsolver=True)
    jac = em.optimize.Jacobian(grid, model, src, freq, rec, nvec=2)
    nx, ny, nz = grid.vnC
    for bad in (np.zeros(grid.nC), np.zeros((nx, ny, nz + 1)), np.zeros((2, nx, ny)), (np.zeros(grid.vnC), None),
                (None, None, None), (np.zeros(grid.vnC), np.zeros((2, nx, ny, nz)), None),
                (np.zeros((2, nx, ny, nz)), np.zeros((3, nx, ny, nz)), None)):
        with pytest.raises(ValueError, match="`v`"):
            jac.jvec(bad)
    with pytest.raises(TypeError, match="real"):
        jac.jvec(np.zeros(grid.vnC, dtype=complex))
    n = rec[0].size
    for bad in (np.zeros(n + 1), np.zeros((2, n + 1)), np.zeros((2, 2, n)), np.zeros((0, n))):
        with pytest.raises(ValueError, match="`w`"):
            jac.jtvec(bad)
    # well-formed arguments on a Jacobian that is not open: no silent work
    with pytest.raises(RuntimeError, match="closed"):
        jac.jvec(np.zeros(grid.vnC))
    with pytest.raises(RuntimeError, match="closed"):
        jac.jtvec(np.zeros(n))


def test_fixture_gaps_are_below_the_generators_asserts():
    j = load_golden("jacobian.npz")
    assert float(j['fd_gap_ref']) < 1e-6 and float(j['adjoint_gap_ref']) < 1e-6
    for tag in ('iso', 'tri'):
        for case in ('full', 'vz'):
            jv, fd = j[f'{tag}_{case}_jv'], j[f'{tag}_{case}_jv_fd']
            gap = np.linalg.norm(fd - jv) / np.linalg.norm(jv)
            assert gap < 1e-6 and abs(gap - float(j[f'{tag}_{case}_fd_gap_ref'])) < 1e-12
            jt = -(j[f'{tag}_jt_gx'] + j[f'{tag}_jt_gy'] + j[f'{tag}_jt_gz']) if case == 'full' else -j[f'{tag}_jt_gz']
            lhs = np.real(np.sum(np.conj(j[f'{tag}_w']) * jv))
            rhs = np.sum(jt.ravel('F') * j[f'{tag}_v'])
            gap = abs(lhs - rhs) / abs(lhs)
            assert gap < 1e-6 and abs(gap - float(j[f'{tag}_{case}_adjoint_gap_ref'])) < 1e-12


def test_numpy_restatements_agree_with_the_stored_vectors():
    em, g, j, grid = _setup()
    vol = grid.cell_volumes.reshape(grid.vnC, order='F')
    rec = tuple(g['rec'])
    fac = em.fields._rotation(*rec[3:])
    P = linear_receiver_matrix(grid, rec, fac)
    for tag in ('iso', 'tri'):
        e0, v, w = j[f'{tag}_efield'], j[f'{tag}_v'], j[f'{tag}_w']
        smu0 = complex(j[f'{tag}_smu0'])
        for case, v3 in (('full', (v, v, v)), ('vz', (None, None, v))):
            want = j[f'{tag}_{case}_src']
            got = smu0 * cells2edges_pec(grid.vnC, vol, v3) * e0
            assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
        assert np.abs(P @ e0 - j[f'{tag}_d_lin']).max() <= 1e-14 * np.abs(j[f'{tag}_d_lin']).max()
        want = j[f'{tag}_jt_src']
        assert np.abs(P.T @ np.conj(w) - want).max() <= 1e-14 * np.abs(want).max()
