"""CPU-only: the host side of sensitivities on a model grid (optimize.SurveyJacobian(model_grid=)) -- the old-cell offsets the
transpose of volume averaging gathers with (``emg3d_volume_average_old_offsets``, O(n) host work inside the library), the F / Q
rules of ``maps.regrid_factors`` per property map, the argument checks that need no device, and the plumbing of
``FrequencyHandles.set_model_grid`` / ``set_regrid_factors`` against a NumPy stand-in of the handle.

Also home of what tests/test_gpu_model_grid.py shares: the grid pairs and the dense NumPy restatement of volume averaging."""
import numpy as np
import pytest

from conftest import load_golden


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from emg3d_amd import _lib
    return _lib


# ---- grid pairs (model grid -> computational grid) -----------------------------------------------------------------------
def _mesh(em, edges):
    return em.TensorMesh([np.diff(e) for e in edges], origin=[e[0] for e in edges])


def _split(a, b, fractions):
    """Edges from a to b at the given interior fractions."""
    return a + (b - a) * np.r_[0.0, np.asarray(fractions, dtype=np.float64), 1.0]


def grid12(em):
    g = load_golden("survey_jacobian.npz")
    return em.TensorMesh([g['hx'], g['hy'], g['hz']], origin=g['origin'])


def grid_pairs(em, names=None):
    """name -> (model_grid, grid).  The computational grid of the first four is the 12 x 10 x 8 grid of survey_jacobian.npz:
    'unaligned' a 7 x 5 x 4 model grid over the same extent with no interior edge in common; 'inside' a 5 x 4 x 1 model grid strictly
    inside, its x range within the last two computational cells (the boundary model cells own the clipped rest: more than 8 x
    segments, the kernel's long path); 'beyond' a 6 x 5 x 4 model grid whose outermost cells lie wholly outside (empty model cells);
    '48' the 48 x 40 x 32 grid of test_gpu_jacobian._model48 from 20 x 16 x 12."""
    grid = grid12(em)
    ex = [grid.nodes_x, grid.nodes_y, grid.nodes_z]
    lo, hi = [e[0] for e in ex], [e[-1] for e in ex]
    out = {}
    out['unaligned'] = (_mesh(em, [_split(lo[0], hi[0], [0.11, 0.23, 0.41, 0.52, 0.69, 0.87]),
                                   _split(lo[1], hi[1], [0.17, 0.43, 0.61, 0.83]),
                                   _split(lo[2], hi[2], [0.29, 0.47, 0.71])]), grid)
    x10, x12 = ex[0][10], ex[0][12]
    out['inside'] = (_mesh(em, [_split(x10 + 0.13 * (x12 - x10), x10 + 0.91 * (x12 - x10), [0.2, 0.45, 0.6, 0.8]),
                                _split(lo[1] + 0.21 * (hi[1] - lo[1]), lo[1] + 0.77 * (hi[1] - lo[1]), [0.3, 0.5, 0.8]),
                                _split(lo[2] + 0.33 * (hi[2] - lo[2]), lo[2] + 0.61 * (hi[2] - lo[2]), [])]), grid)
    ext = [h - l for l, h in zip(lo, hi)]
    out['beyond'] = (_mesh(em, [np.r_[lo[0] - 0.5 * ext[0], lo[0] - 0.1 * ext[0], _split(lo[0], hi[0], [0.3, 0.55])[1:-1],
                                      hi[0] + 0.05 * ext[0], hi[0] + 0.4 * ext[0], hi[0] + 0.9 * ext[0]],
                                np.r_[lo[1] - 0.3 * ext[1], lo[1] - 0.02 * ext[1], _split(lo[1], hi[1], [0.37, 0.7])[1:-1],
                                      hi[1] + 0.1 * ext[1], hi[1] + 0.2 * ext[1]],
                                np.r_[lo[2] - 0.2 * ext[2], lo[2] - 0.05 * ext[2], lo[2] + 0.45 * ext[2], hi[2] + 0.15 * ext[2],
                                      hi[2] + 0.3 * ext[2]]]), grid)
    if names is None or '48' in names:
        hx = em.meshes.stretched_widths(32, 8, 50., 1.2)
        hy = em.meshes.stretched_widths(24, 8, 50., 1.2)
        hz = em.meshes.stretched_widths(16, 8, 50., 1.2)
        g48 = em.TensorMesh([hx, hy, hz], origin=(-hx.sum() / 2, -hy.sum() / 2, -hz.sum() / 2))
        e48 = [g48.nodes_x, g48.nodes_y, g48.nodes_z]
        rng = np.random.default_rng(2048)
        coarse = []
        for e, n in zip(e48, (20, 16, 12)):
            # n cells over the same extent, the interior edges at random: none is shared with the fine grid
            t = np.sort(rng.uniform(0.02, 0.98, n - 1))
            coarse.append(_split(e[0], e[-1], t))
        out['48'] = (_mesh(em, coarse), g48)
    return out if names is None else {k: out[k] for k in names}


PAIRS = ('unaligned', 'inside', 'beyond', '48')


# ---- the dense NumPy restatement -----------------------------------------------------------------------------------------
def axis_matrices(em, model_grid, grid):
    """Per axis ``(W, nseg)``: ``W[o, i]`` = the summed lengths of the segments of computational cell ``o`` in model cell ``i``,
    ``nseg[i]`` = the number of segments model cell ``i`` owns -- from ``maps._volume_average_weights``."""
    out = []
    for c in 'xyz':
        x1, x2 = getattr(model_grid, 'nodes_' + c), getattr(grid, 'nodes_' + c)
        w, i1, i2 = em.maps._volume_average_weights(x1, x2)
        W = np.zeros((x2.size - 1, x1.size - 1))
        np.add.at(W, (i2, i1), w)
        out.append((W, np.bincount(i1, minlength=x1.size - 1)))
    return out


def dense_adjoint(mats, y, vol, F=None, Q=None):
    """``(Q (.) A^T (F (.) y), bound)`` in NumPy: ``bound = (N + 8) 2^-52 sum_k |t_k|`` per model cell, ``N`` the number of
    terms of the cell's sum, the right-hand side from the same statement with absolute values."""
    (Wx, nx), (Wy, ny), (Wz, nz) = mats
    t = (y if F is None else F * y) / vol
    res = np.einsum('ai,bj,ck,abc->ijk', Wx, Wy, Wz, t)
    mag = np.einsum('ai,bj,ck,abc->ijk', Wx, Wy, Wz, np.abs(t))
    if Q is not None:
        res, mag = Q * res, np.abs(Q) * mag
    N = nx[:, None, None] * ny[None, :, None] * nz[None, None, :]
    return res, (N + 8) * 2.0 ** -52 * mag


def dense_forward(mats, v, vol):
    """``A v`` in NumPy."""
    (Wx, _), (Wy, _), (Wz, _) = mats
    return np.einsum('ai,bj,ck,ijk->abc', Wx, Wy, Wz, v) / vol


def volumes(grid):
    return grid.cell_volumes.reshape(grid.vnC, order='F')


# ---- 1. the old-cell offsets ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', PAIRS)
def test_old_cell_offsets_are_monotone_and_cover_every_segment(lib, name):
    import emg3d_amd as em
    model_grid, grid = grid_pairs(em, [name])[name]
    longest = 0
    for c in 'xyz':
        x1, x2 = getattr(model_grid, 'nodes_' + c), getattr(grid, 'nodes_' + c)
        w, i1, i2, ptr = em.maps._volume_average_segments(x1, x2)
        n = x1.size - 1
        assert np.all(np.diff(i1) >= 0) and np.all(np.diff(i2) >= 0)        # ascending coordinate: sorted by both cells
        iptr = em.maps._volume_average_old_offsets(i1, n)
        assert iptr.shape == (n + 1,) and iptr[0] == 0 and iptr[-1] == w.size
        assert np.all(np.diff(iptr) >= 0)
        for i in range(n):
            assert np.all(i1[iptr[i]:iptr[i + 1]] == i)
        assert np.array_equal(np.diff(iptr), np.bincount(i1, minlength=n))
        # the segments of the new grid's extent sum to it, whatever the old grid covers (clipping at both ends)
        assert abs(w.sum() - (x2[-1] - x2[0])) <= 1e-12 * (x2[-1] - x2[0])
        if c == 'x':
            longest = int(np.diff(iptr).max())
        if name == 'beyond':
            assert np.diff(iptr)[0] == 0 and np.diff(iptr)[-1] == 0         # model cells wholly outside own nothing
    if name == 'inside':
        assert longest > 8                                                  # beyond the kernel's register-resident rows
    elif name == 'unaligned':
        assert longest <= 8


def test_old_cell_offsets_reject_bad_arguments(lib):
    h = lib.load()
    ok = np.array([0, 0, 1, 3], dtype=np.int64)
    iptr = np.zeros(5, dtype=np.int64)
    assert h.emg3d_volume_average_old_offsets(lib.ptr(ok), 4, 4, lib.ptr(iptr)) == 0
    assert iptr.tolist() == [0, 2, 3, 3, 4]
    assert h.emg3d_volume_average_old_offsets(lib.ptr(ok), 4, 3, lib.ptr(iptr)) == -2            # a cell beyond the last
    down = np.array([0, 2, 1], dtype=np.int64)
    assert h.emg3d_volume_average_old_offsets(lib.ptr(down), 3, 4, lib.ptr(iptr)) == -2          # not ascending
    assert h.emg3d_volume_average_old_offsets(None, 3, 4, lib.ptr(iptr)) == -2
    assert h.emg3d_volume_average_old_offsets(lib.ptr(ok), 4, 0, lib.ptr(iptr)) == -2


# ---- 2. the F / Q rules ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mapping', ['Conductivity', 'Resistivity', 'LgConductivity', 'LnConductivity', 'LgResistivity',
                                     'LnResistivity'])
def test_regrid_factor_rules(mapping):
    """Linear maps (regridded in log10): F = sigma_c resp. -sigma_c, Q = 1 / p_m; logarithmic maps: F = chain_factor(sigma_c),
    Q = 1.  Directions that share property_x share its factors (the same objects: uploaded once)."""
    import emg3d_amd as em
    from emg3d_amd import maps
    mgrid = em.TensorMesh([np.ones(3), np.ones(2), np.ones(2)])
    rng = np.random.default_rng(7)
    log = maps.MAPS[mapping].log
    p = [rng.standard_normal(mgrid.nC) if log else rng.uniform(0.5, 20.0, mgrid.nC) for _ in range(3)]
    sig = [rng.uniform(0.01, 3.0, (4, 3, 2)) for _ in range(3)]
    want_F = {'Conductivity': lambda s: s, 'Resistivity': lambda s: -s, 'LgConductivity': lambda s: s * np.log(10),
              'LnConductivity': lambda s: s, 'LgResistivity': lambda s: -s * np.log(10), 'LnResistivity': lambda s: -s}[mapping]
    tri = em.Model(mgrid, *p, mapping=mapping)
    F, Q = maps.regrid_factors(tri, sig)
    for c in range(3):
        assert np.array_equal(F[c], want_F(sig[c])) and F[c] is not sig[c]
        assert Q[c].shape == tuple(mgrid.vnC)
        assert np.array_equal(Q[c], np.ones(mgrid.vnC) if log else 1.0 / p[c].reshape(mgrid.vnC, order='F'))
    assert F[1] is not F[0] and Q[2] is not Q[0]
    iso = em.Model(mgrid, p[0], mapping=mapping)
    F, Q = maps.regrid_factors(iso, (sig[0],) * 3)
    assert F[1] is F[0] and F[2] is F[0] and Q[1] is Q[0] and Q[2] is Q[0]
    vti = em.Model(mgrid, p[0], None, p[2], mapping=mapping)
    F, Q = maps.regrid_factors(vti, (sig[0], sig[0], sig[2]))
    assert F[1] is F[0] and F[2] is not F[0] and Q[1] is Q[0] and np.array_equal(F[2], want_F(sig[2]))
    # a scalar property is expanded to the model grid
    F, Q = maps.regrid_factors(em.Model(mgrid, p[0][0], mapping=mapping), (sig[0],) * 3)
    assert Q[0].shape == tuple(mgrid.vnC)


# ---- 3. argument checks that need no device ----------------------------------------------------------------------------------
def test_argument_checks_need_no_device():
    import emg3d_amd as em
    g = load_golden("survey_jacobian.npz")
    model_grid, grid = grid_pairs(em, ['unaligned'])['unaligned']
    rec = tuple(g['rec'])
    SJ = em.optimize.SurveyJacobian
    args = (g['sources'], g['freqs'], rec)
    rng = np.random.default_rng(8)
    model = em.Model(model_grid, rng.uniform(0.5, 5.0, model_grid.nC))
    # the model must live on the model grid
    with pytest.raises(ValueError, match="model_grid"):
        SJ(grid, em.Model(grid, np.ones(grid.nC)), *args, model_grid=model_grid)
    with pytest.raises(NotImplementedError, match="permeability"):
        SJ(grid, em.Model(model_grid, np.ones(model_grid.nC), mu_r=np.full(model_grid.nC, 2.0)), *args, model_grid=model_grid)
    sj = SJ(grid, model, *args, model_grid=model_grid, tol=1e-6)
    assert sj.model_grid is model_grid and sj.synthetic is None
    vm, vc = np.zeros(model_grid.vnC), np.zeros(grid.vnC)
    w = np.zeros((2, 2, 5))
    # conductivity products are not defined on a model grid: the default mapped=False says so, before anything else
    for call in (lambda: sj.jvec(vm), lambda: sj.jtvec(w), lambda: sj.gauss_newton(vm), lambda: sj.jvec(vm, mapped=False),
                 lambda: sj.jtvec(w, components=True)):
        with pytest.raises(ValueError, match="model's own property"):
            call()
    with pytest.raises(TypeError, match="mapped"):
        sj.jvec(vm, mapped=1)
    # perturbations live on the model grid
    with pytest.raises(ValueError, match="`v`"):
        sj.jvec(vc, mapped=True)
    with pytest.raises(ValueError, match="`v`"):
        sj.gauss_newton(vc, mapped=True)
    for call in (lambda: sj.jvec(vm, mapped=True), lambda: sj.jtvec(w, mapped=True), lambda: sj.gauss_newton(vm, mapped=True)):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    # without a model grid nothing changes: perturbations on the computational grid, mapped=False allowed
    plain = SJ(grid, em.Model(grid, np.ones(grid.nC)), *args)
    assert plain.model_grid is None
    with pytest.raises(RuntimeError, match="closed"):
        plain.jvec(vc)
    with pytest.raises(ValueError, match="`v`"):
        plain.jvec(vm)
    # model_gradient
    grad = np.zeros(grid.vnC)
    with pytest.raises(ValueError, match="model_grid"):
        em.optimize.model_gradient(grid, em.Model(grid, np.ones(grid.nC)), grad, method='transpose')
    with pytest.raises(ValueError, match="method"):
        em.optimize.model_gradient(grid, model, grad, model_grid, method='linear')
    with pytest.raises(NotImplementedError, match="isotropic"):
        em.optimize.model_gradient(grid, em.Model(model_grid, 1.0, 2.0), grad, model_grid, method='transpose')
    with pytest.raises(TypeError, match="real"):
        em.maps.volume_average_adjoint(model_grid.nodes_x, model_grid.nodes_y, model_grid.nodes_z, grid.nodes_x, grid.nodes_y,
                                       grid.nodes_z, np.zeros(grid.vnC, dtype=complex), volumes(grid))
    with pytest.raises(ValueError, match="grid"):
        em.maps.volume_average_adjoint(model_grid.nodes_x, model_grid.nodes_y, model_grid.nodes_z, grid.nodes_x, grid.nodes_y,
                                       grid.nodes_z, np.zeros(model_grid.vnC), volumes(grid))


# ---- 4. FrequencyHandles against a stand-in of the handle ----------------------------------------------------------------------
class _StandIn:
    """What FrequencyHandles asks of a DeviceMG, recorded."""

    def __init__(self, log, key):
        self.log, self.key, self._smu0 = log, key, None

    def retarget(self, spec):
        pass

    def set_batch(self, n):
        self.log.append((self.key, 'set_batch', n))

    def set_model_grid(self, model_grid):
        self.log.append((self.key, 'set_model_grid', model_grid))

    def set_regrid_factors(self, F, Q):
        self.log.append((self.key, 'set_regrid_factors', F, Q))

    def close(self):
        self.log.append((self.key, 'close'))


def test_frequency_handles_link_open_and_later_handles(monkeypatch):
    import emg3d_amd as em
    from emg3d_amd import solver
    log = []
    monkeypatch.setattr(solver.DeviceMG, 'from_model',
                        classmethod(lambda cls, grid, parts, spec, device=0: _StandIn(log, np.dtype(spec.dtype).str)))
    grid, mgrid = object(), object()
    c128, f64 = em.fields.FrequencySpec(1.5), em.fields.FrequencySpec(-1.5)
    F, Q = (np.ones(2),) * 3, (np.ones(1),) * 3
    with solver.FrequencyHandles(grid, None, 0, nsys=2) as handles:
        with pytest.raises(RuntimeError, match="model grid"):
            handles.set_regrid_factors(F, Q)
        first = handles.target(c128)
        assert [e[1] for e in log] == ['set_batch']                         # no link yet: nothing more is asked
        handles.set_model_grid(mgrid)
        handles.set_regrid_factors(F, Q)
        assert log[1:] == [(first.key, 'set_model_grid', mgrid), (first.key, 'set_regrid_factors', F, Q)]
        later = handles.target(f64)                                         # created later: linked at creation, factors too
        assert later is not first
        assert log[3:] == [(later.key, 'set_batch', 2), (later.key, 'set_model_grid', mgrid),
                           (later.key, 'set_regrid_factors', F, Q)]
        assert handles.target(c128) is first and len(log) == 6              # an open handle is not linked again
        F2 = (np.zeros(2),) * 3
        handles.set_regrid_factors(F2, Q)                                   # another model: every open handle
        assert [(e[0], e[1]) for e in log[6:]] == [(first.key, 'set_regrid_factors'), (later.key, 'set_regrid_factors')]
        assert all(e[2] is F2 for e in log[6:])
    assert [e[1] for e in log[8:]] == ['close', 'close']
