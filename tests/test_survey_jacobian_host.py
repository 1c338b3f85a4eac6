"""Host side of optimize.SurveyJacobian: argument checks that need no device, and the fixture tests/golden/survey_jacobian.npz
against the invariants of its generator (shapes, J^T w re-summed from the per-pair arrays in the defined order)."""
import numpy as np
import pytest

from conftest import load_golden


def _setup():
    import emg3d_amd as em
    g = load_golden("survey_jacobian.npz")
    grid = em.TensorMesh([g['hx'], g['hy'], g['hz']], origin=g['origin'])
    return em, g, grid


def test_argument_checks_need_no_device():
    """The errors of Jacobian, raised by the constructor (no handle exists before open()); a closed object refuses products."""
    em, g, grid = _setup()
    rec = tuple(g['rec'])
    sig = g['iso_sig_x']
    model = em.Model(grid, sig, mapping='Conductivity')
    SJ = em.optimize.SurveyJacobian
    args = (g['sources'], g['freqs'], rec)
    with pytest.raises(ValueError, match="receiver_interpolation"):
        SJ(grid, model, *args, receiver_interpolation='quintic')
    with pytest.raises(ValueError, match="adjoint"):
        SJ(grid, model, *args, adjoint='nearly')
    with pytest.raises(NotImplementedError, match="magnetic"):
        SJ(grid, model, *args, electric=False, adjoint='reference')
    with pytest.raises(NotImplementedError, match="permeability"):
        SJ(grid, em.Model(grid, sig, mu_r=np.full(grid.nC, 1.5), mapping='Conductivity'), *args)
    with pytest.raises(NotImplementedError, match="permittivity"):
        SJ(grid, em.Model(grid, sig, epsilon_r=np.full(grid.nC, 5.), mapping='Conductivity'), *args)
    with pytest.raises(NotImplementedError, match="Krylov"):
        SJ(grid, model, *args, sslsolver='bicgstab')
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError, match="batch"):
            SJ(grid, model, *args, batch=bad)
    with pytest.raises(ValueError, match="rec"):
        SJ(grid, model, g['sources'], g['freqs'], rec[:4])
    with pytest.raises(ValueError, match="no sources"):
        SJ(grid, model, [], g['freqs'], rec)
    with pytest.raises(ValueError, match="no sources"):
        SJ(grid, model, g['sources'], [], rec)
    # tri-axial models are taken; nothing touches a device before open()
    tri = em.Model(grid, g['tri_sig_x'], g['tri_sig_y'], g['tri_sig_z'], mapping='Conductivity')
    sj = SJ(grid, tri, *args, batch=8, tol=1e-8)
    assert (sj.n_src, sj.n_freq, sj.n_rec) == (2, 2, 5) and sj.synthetic is None and sj.partial is None
    assert sj.receiver_interpolation == 'cubic' and sj.adjoint == 'exact'
    for call in (lambda: sj.jvec(np.zeros(grid.vnC)), lambda: sj.jtvec(np.zeros((2, 2, 5))),
                 lambda: sj.gauss_newton(np.zeros(grid.vnC))):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    # argument shapes are checked before the handles are asked for
    with pytest.raises(ValueError, match="`v`"):
        sj.jvec(np.zeros((3,) + tuple(grid.vnC)))
    with pytest.raises(ValueError, match="`w`"):
        sj.jtvec(np.zeros((2, 2, 4)))
    with pytest.raises(ValueError, match="weights"):
        sj.gauss_newton(np.zeros(grid.vnC), weights=np.ones(4))
    with pytest.raises(TypeError, match="weights"):
        sj.gauss_newton(np.zeros(grid.vnC), weights=np.ones(5) * 1j)
    with pytest.raises(TypeError, match="real"):
        SJ(grid, model, g['sources'], [1.0, -1.0], rec).jtvec(np.full((2, 2, 5), 1j))
    sj.close()


def test_fixture_invariants():
    """Shapes, finiteness, and the survey's J^T w re-summed per component from the per-pair arrays: per frequency the
    sequential sum over the sources from zeros, then the sequential sum over `freqs` from zeros (optimize._sum_survey)."""
    em, g, grid = _setup()
    from emg3d_amd import optimize
    s = load_golden("survey_gradient.npz")
    ns, nf, nrec = 2, 2, 5
    vnC = tuple(int(n) for n in grid.vnC)
    assert vnC == (12, 10, 8)
    for key in ('hx', 'hy', 'hz', 'origin', 'sources', 'freqs', 'rec'):
        assert np.array_equal(g[key], s[key]), key
    assert g['sources'].shape == (ns, 5) and g['freqs'].tolist() == [1.5, 0.7] and g['rec'].shape == (5, nrec)
    for tag in ('iso', 'tri'):
        for key in ('sig_x', 'sig_y', 'sig_z', 'v'):
            assert g[f'{tag}_{key}'].shape == (grid.nC,) and np.isfinite(g[f'{tag}_{key}']).all()
        for key in ('w', 'synthetic', 'jv'):
            a = g[f'{tag}_{key}']
            assert a.shape == (ns, nf, nrec) and a.dtype == np.complex128 and np.isfinite(a).all(), key
        assert g[f'{tag}_jt_pair'].shape == (3, ns, nf) + vnC and g[f'{tag}_jt'].shape == (3,) + vnC
        assert g[f'{tag}_adj_gap'].shape == (ns, nf) and g[f'{tag}_cubic_adj_gap'].shape == (ns, nf)
        assert 0 < g[f'{tag}_adj_gap'].max() < 1e-5 and 0 < g[f'{tag}_cubic_adj_gap'].max() < 1e-5
        for c in range(3):
            want = np.zeros(vnC)
            for j in range(nf):
                gf = np.zeros(vnC)
                for i in range(ns):
                    gf = gf + g[f'{tag}_jt_pair'][c, i, j]
                want = want + gf
            assert np.array_equal(want, g[f'{tag}_jt'][c])
            assert np.abs(want).max() > 0
            # the package's summation routine on the per-frequency sums in the gradient's sign
            partial = [-(np.zeros(vnC) + g[f'{tag}_jt_pair'][c, 0, j] + g[f'{tag}_jt_pair'][c, 1, j]) for j in range(nf)]
            _, got = optimize._sum_survey(partial, np.zeros((ns, nf)), vnC)
            assert np.array_equal(-got, want)
    assert np.array_equal(g['iso_sig_x'], g['iso_sig_y']) and np.array_equal(g['iso_sig_x'], g['iso_sig_z'])
    assert not np.array_equal(g['tri_sig_x'], g['tri_sig_y']) and not np.array_equal(g['tri_sig_y'], g['tri_sig_z'])
    assert float(g['adj_gap_linear']) == max(g['iso_adj_gap'].max(), g['tri_adj_gap'].max())
    assert float(g['adj_gap_cubic']) == max(g['iso_cubic_adj_gap'].max(), g['tri_cubic_adj_gap'].max())
