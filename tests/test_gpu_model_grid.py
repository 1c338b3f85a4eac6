"""GPU: sensitivities on the model grid -- the exact transpose of volume averaging (k_volume_average_adjoint) and
optimize.SurveyJacobian(model_grid=).

Rounding bound B (all "within B" below): a result that is a sum of N terms may differ from its NumPy restatement by
(N + 8) 2^-52 sum_k |t_k| -- the recursive-summation bound for both sides (2^-52 = two unit roundoffs) plus the handful of
operations that form a term (F y, / vol, (w_z w_y) w_x, the product, Q, and a merged pair of clipped segments); the right-hand
side comes from the restatement with absolute values (test_model_grid_host.dense_adjoint).  The restatement builds dense per-axis
matrices from maps._volume_average_weights."""
import numpy as np
import pytest

from conftest import load_golden
from test_gpu_jacobian import OPTS, _model48
from test_model_grid_host import PAIRS, axis_matrices, dense_adjoint, dense_forward, grid_pairs, volumes

pytestmark = pytest.mark.gpu

SOURCES = [[-100., 30., 20., 25., 5.], [140., -60., -25., -50., 20.], [20., 100., -40., 80., -30.]]


def _adjoint(em, model_grid, grid, y):
    return em.maps.volume_average_adjoint(model_grid.nodes_x, model_grid.nodes_y, model_grid.nodes_z, grid.nodes_x, grid.nodes_y,
                                          grid.nodes_z, y, volumes(grid))


# ---- 1. the kernel, no solves -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', PAIRS)
def test_adjoint_kernel_vs_dense_numpy(name):
    """maps.volume_average_adjoint against the dense A^T y within B per model cell; <A v, y> = <v, A^T y> within B of the double
    sum; model cells no computational cell reaches are exact zeros; a second call repeats bit for bit."""
    import emg3d_amd as em
    model_grid, grid = grid_pairs(em, [name])[name]
    mats = axis_matrices(em, model_grid, grid)
    rng = np.random.default_rng(51)
    y = np.asfortranarray(rng.standard_normal(grid.vnC))
    v = np.asfortranarray(rng.standard_normal(model_grid.vnC))
    vol = volumes(grid)
    got = _adjoint(em, model_grid, grid, y)
    want, bound = dense_adjoint(mats, y, vol)
    assert got.shape == tuple(model_grid.vnC) and got.dtype == np.float64 and got.flags.f_contiguous
    err = np.abs(got - want)
    print(f"{name}: max |err| / bound {np.max(err[bound > 0] / bound[bound > 0]):.3f}, longest x row {mats[0][1].max()}")
    assert np.all(err <= bound)
    assert np.abs(want).max() > 0
    empty = (mats[0][1][:, None, None] * mats[1][1][None, :, None] * mats[2][1][None, None, :]) == 0
    assert empty.any() == (name == 'beyond')
    assert np.all(got[empty] == 0) and not np.any(np.signbit(got[empty]))
    if name == 'inside':
        assert mats[0][1].max() > 8             # the plain loop beyond the register-resident row
    assert np.array_equal(_adjoint(em, model_grid, grid, y), got)
    # the adjoint identity, A v by the device's volume averaging
    Av = em.maps.grid2grid(model_grid, v, grid, method='volume')
    assert np.abs(Av - dense_forward(mats, v, vol)).max() <= 1e-12 * np.abs(v).max()        # (the restatement itself: rows sum to 1)
    lhs, rhs = np.sum(Av * y), np.sum(v * got)
    nterms = int(np.prod([m[1].sum() for m in mats]))
    mag = np.sum(np.abs(v) * dense_adjoint(mats, np.abs(y), vol)[0])
    print(f"{name}: <A v, y> - <v, A^T y> = {lhs - rhs:.3e}, bound {(nterms + 8) * 2.0 ** -52 * mag:.3e}")
    assert abs(lhs - rhs) <= (nterms + 8) * 2.0 ** -52 * mag


# ---- 2. the handle ----------------------------------------------------------------------------------------------------------
def _align(nbytes):
    return (max(nbytes, 8) + 255) // 256 * 256


@pytest.mark.parametrize('name', ['unaligned', 'inside', 'beyond'])
@pytest.mark.parametrize('freq', [1.5, -1.5], ids=['c128', 'f64'])
def test_handle_reads_the_accumulators_back_on_the_model_grid(name, freq):
    """grad_acc3 / grad_acc filled from random fields (as test_grad_acc3_is_the_sequential_sum_of_gradient3): the _get_model calls
    equal Q (.) A^T_NumPy (F (.) _get()) within B and leave the accumulators unchanged; device_bytes grows by the tables, the
    scratch and the factors and repeats after set_model and another set of factors; status -7 before the link."""
    import emg3d_amd as em
    from emg3d_amd import models
    from emg3d_amd.solver import DeviceMG
    g = load_golden("survey_jacobian.npz")
    model_grid, grid = grid_pairs(em, [name])[name]
    mats = axis_matrices(em, model_grid, grid)
    vol = volumes(grid)
    nC, nM, nsys = grid.nC, model_grid.nC, 3
    model = em.Model(grid, g['tri_sig_x'], g['tri_sig_y'], g['tri_sig_z'], mapping='Conductivity')
    spec = em.fields.FrequencySpec(freq)
    rng = np.random.default_rng(52)
    real = freq < 0
    fields = [[rng.standard_normal(grid.nE) if real else rng.standard_normal(grid.nE) + 1j * rng.standard_normal(grid.nE)
               for _ in range(nsys)] for _ in range(2)]
    use = np.array([1, 0, 1], dtype=np.int32)
    F = tuple(np.asfortranarray(rng.standard_normal(grid.vnC)) for _ in range(3))
    Q = tuple(np.asfortranarray(rng.standard_normal(model_grid.vnC)) for _ in range(3))
    out = [np.empty(nM) for _ in range(3)]
    ptrs = [o.ctypes.data for o in out]
    with DeviceMG.from_model(grid, models.model_parts(grid, model, raw=True), spec) as dev:
        dev.set_batch(nsys)
        dev.vec_alloc(1)
        dev.bvec_alloc(1)
        for b in range(nsys):
            dev.select(b)
            dev.set_efield(em.Field(grid, fields[1][b].copy(), freq=freq))
            dev.bvec_set(0, b, fields[0][b])
        dev.grad_acc3_reset()
        dev.grad_acc3_add(0, spec.smu0, use)
        dev.grad_acc_reset()
        dev.grad_acc_add(0, spec.smu0, use)
        acc3, acc1 = dev.grad_acc3_get(), dev.grad_acc_get()
        assert all(np.abs(a).max() > 0 for a in acc3)
        # no model grid yet
        lib = dev._lib
        assert lib.emg3d_mg_grad_acc3_get_model(dev._h, *ptrs) == -7
        assert lib.emg3d_mg_grad_acc_get_model(dev._h, ptrs[0]) == -7
        assert lib.emg3d_mg_set_regrid_factors(dev._h, *(a.ctypes.data for a in F + Q)) == -7
        with pytest.raises(RuntimeError, match="model grid"):
            dev.grad_acc3_get_model()
        with pytest.raises(RuntimeError, match="model grid"):
            dev.set_regrid_factors(F, Q)
        before = dev.device_bytes
        dev.set_model_grid(model_grid)
        tables = sum(3 * _align(8 * (n + m + 1)) + _align(8 * (m + 1)) + _align(8 * (n + 1))
                     for n, m in zip(model_grid.vnC, grid.vnC))
        linked = dev.device_bytes
        assert linked - before == tables + _align(8 * nC) + _align(8 * 3 * nM)
        assert lib.emg3d_mg_grad_acc3_get_model(dev._h, *ptrs) == -7            # linked, but no factors yet
        dev.set_regrid_factors(F, Q)
        full = dev.device_bytes
        assert full - linked == 3 * _align(8 * nC) + 3 * _align(8 * nM)
        got3, got1 = dev.grad_acc3_get_model(), dev.grad_acc_get_model()
        worst = 0.0
        for c in range(3):
            want, bound = dense_adjoint(mats, acc3[c].reshape(grid.vnC, order='F'), vol, F[c], Q[c])
            err = np.abs(got3[c].reshape(model_grid.vnC, order='F') - want)
            assert np.all(err <= bound), c
            worst = max(worst, np.max(err[bound > 0] / bound[bound > 0]))
        want, bound = dense_adjoint(mats, acc1.reshape(grid.vnC, order='F'), vol, F[0], Q[0])
        err = np.abs(got1.reshape(model_grid.vnC, order='F') - want)
        assert np.all(err <= bound) and np.abs(want).max() > 0
        print(f"{name}: max |err| / bound {max(worst, np.max(err[bound > 0] / bound[bound > 0])):.3f}")
        # the accumulators are read, not consumed; a second read-back repeats
        assert all(np.array_equal(a, b) for a, b in zip(dev.grad_acc3_get(), acc3)) and np.array_equal(dev.grad_acc_get(), acc1)
        assert all(np.array_equal(a, b) for a, b in zip(dev.grad_acc3_get_model(), got3))
        # another model and other factors on the open handle: nothing is allocated, the new factors are the ones applied
        dev.set_model(grid, em.Model(grid, 2 * g['tri_sig_x'], g['tri_sig_y'], 3 * g['tri_sig_z'], mapping='Conductivity'))
        dev.set_regrid_factors(tuple(2 * f for f in F), Q)
        dev.set_model_grid(model_grid)
        assert dev.device_bytes == full
        again = dev.grad_acc3_get_model()
        assert all(np.array_equal(a, 2 * b) for a, b in zip(again, got3))     # (a factor of two is exact)
        # the directions must go on sharing factors as at the first call; a model grid of another size is refused
        with pytest.raises(ValueError, match="share"):
            dev.set_regrid_factors((F[0], F[0], F[0]), Q)
        with pytest.raises(ValueError, match="shape"):
            dev.set_regrid_factors(F, (Q[0].ravel(), Q[1], Q[2]))
        with pytest.raises(ValueError, match="another size"):
            dev.set_model_grid(grid)
        assert all(np.array_equal(a, b) for a, b in zip(dev.grad_acc3_get_model(), again))


# ---- 3. the class against itself ------------------------------------------------------------------------------------------------
def _reference_volume_average(model_grid, grid, v):
    """Volume averaging in plain Python, the reference's loops and order of operations (emg3d/maps.py:453-523)."""
    import emg3d_amd as em
    segs = [em.maps._volume_average_weights(getattr(model_grid, 'nodes_' + c), getattr(grid, 'nodes_' + c)) for c in 'xyz']
    (wx, ix1, ix2), (wy, iy1, iy2), (wz, iz1, iz2) = segs
    out = np.zeros(grid.vnC, order='F')
    for iz in range(wz.size):
        for iy in range(wy.size):
            wzy = wz[iz] * wy[iy]
            for ix in range(wx.size):
                out[ix2[ix], iy2[iy], iz2[iz]] += wzy * wx[ix] * v[ix1[ix], iy1[iy], iz1[iz]]
    return out / volumes(grid)


def _models(em, model_grid, kind, seed=53):
    rng = np.random.default_rng(seed)
    if kind == 'Resistivity':
        return em.Model(model_grid, 10 ** rng.uniform(-0.5, 1.0, model_grid.nC), mapping='Resistivity')
    if kind == 'LgConductivity':
        return em.Model(model_grid, rng.uniform(-1.0, 0.5, model_grid.nC), mapping='LgConductivity')
    sig = 10 ** rng.uniform(-1.0, 0.5, model_grid.nC)
    return em.Model(model_grid, sig, sig * 10 ** rng.uniform(-0.3, 0.3, model_grid.nC), sig * 10 ** rng.uniform(-0.3, 0.3, model_grid.nC),
                    mapping='Conductivity')


def _host_factors(model, sigma):
    """F and Q per direction, written out per map (not through maps.regrid_factors)."""
    props = [model.property_x, model.property_y if model.case == 3 else model.property_x,
             model.property_z if model.case == 3 else model.property_x]
    if model.mapping == 'Resistivity':
        return [-s for s in sigma], [1.0 / p for p in props]
    if model.mapping == 'Conductivity':
        return [s.copy() for s in sigma], [1.0 / p for p in props]
    assert model.mapping == 'LgConductivity'
    return [s * np.log(10) for s in sigma], [np.ones(p.shape) for p in props]


@pytest.mark.parametrize('kind', ['Resistivity', 'LgConductivity', 'Conductivity-tri'])
def test_class_on_a_model_grid_against_the_class_on_the_computational_grid(kind):
    """sj_m (model on the 7 x 5 x 4 grid, model_grid=) against sj_c (no model grid, on model.interpolate2grid): the same solves
    (data and infos identical); sj_m.jvec(v, mapped=True) bit for bit sj_c.jvec(v_c) with v_c = F (.) A (Q (.) v) restated on the host in
    the reference's loop order; sj_m.partial == Q (.) A^T_NumPy (F (.) sj_c.partial) within B; jtvec and gauss_newton are the negated
    sums of the partials in the order of `freqs`."""
    import emg3d_amd as em
    g = load_golden("survey_jacobian.npz")
    model_grid, grid = grid_pairs(em, ['unaligned'])['unaligned']
    mats, vol = axis_matrices(em, model_grid, grid), volumes(grid)
    model = _models(em, model_grid, kind)
    tri = model.case == 3
    rec = tuple(g['rec'])
    freqs = [1.5, -1.2]
    rng = np.random.default_rng(54)
    v = np.asfortranarray(rng.standard_normal(model_grid.vnC) * (1.0 if model.map.log else model.property_x * 0.3))
    shape = (3, 2, rec[0].size)
    w = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    w[:, 1] = w[:, 1].real
    W = rng.uniform(0.5, 2.0, shape)
    kw = dict(OPTS, tol=1e-6, batch=2)
    cmodel = model.interpolate2grid(model_grid, grid)
    with em.optimize.SurveyJacobian(grid, cmodel, SOURCES, freqs, rec, **kw) as sj_c, \
            em.optimize.SurveyJacobian(grid, model, SOURCES, freqs, rec, model_grid=model_grid, **kw) as sj_m:
        assert np.array_equal(sj_m.synthetic, sj_c.synthetic)
        for ra, rb in zip(sj_m.forward_info, sj_c.forward_info):
            assert all(a['it_mg'] == b['it_mg'] and a['abs_error'] == b['abs_error'] for a, b in zip(ra, rb))
        dev = next(iter(sj_c._held))
        sigma = [dev.get_sigma(c) for c in range(3)] if tri else [dev.get_sigma(0)] * 3
        F, Q = _host_factors(model, sigma)
        # J_m v
        v_c = [F[c] * _reference_volume_average(model_grid, grid, Q[c] * v) for c in range(3 if tri else 1)]
        jv = sj_m.jvec(v, mapped=True)
        assert np.array_equal(jv, sj_c.jvec(tuple(v_c) if tri else v_c[0])) and np.abs(jv).max() > 0
        if tri:
            vz = np.asfortranarray(rng.standard_normal(model_grid.vnC))
            assert np.array_equal(sj_m.jvec((None, None, vz), mapped=True),
                                  sj_c.jvec((None, None, F[2] * _reference_volume_average(model_grid, grid, Q[2] * vz))))
        # J_m^T w: the per-frequency sums
        jt = sj_m.jtvec(w, mapped=True)
        part_m = sj_m.partial.copy()
        sj_c.jtvec(w, components=tri)
        part_c = sj_c.partial.copy()
        assert part_m.shape == ((3, 2) if tri else (2,)) + tuple(model_grid.vnC)
        assert jt.shape == tuple(model_grid.vnC) and jt.dtype == np.float64 and jt.flags.f_contiguous
        worst = 0.0
        for j in range(2):
            for c in range(3 if tri else 1):
                want, bound = dense_adjoint(mats, part_c[c, j] if tri else part_c[j], vol, F[c], Q[c])
                err = np.abs((part_m[c, j] if tri else part_m[j]) - want)
                assert np.all(err <= bound), (j, c)
                assert np.abs(want).max() > 0
                worst = max(worst, np.max(err[bound > 0] / bound[bound > 0]))
        print(f"{kind}: partials, max |err| / bound {worst:.3f}")
        zero = np.zeros(model_grid.vnC)
        if tri:
            per = [-((zero + part_m[c, 0]) + part_m[c, 1]) for c in range(3)]
            assert np.array_equal(jt, (per[0] + per[1]) + per[2])
            jt3 = sj_m.jtvec(w, components=True, mapped=True)
            assert all(np.array_equal(a, b) for a, b in zip(jt3, per)) and np.array_equal(sj_m.partial, part_m)
        else:
            assert np.array_equal(jt, -((zero + part_m[0]) + part_m[1]))
        # Gauss-Newton: both products chunk by chunk
        hv = sj_m.gauss_newton(v, W, mapped=True)
        assert np.array_equal(hv, sj_m.jtvec(W * jv, mapped=True)) and np.abs(hv).max() > 0


def _run(em, model_grid, grid, model, rec, v, w, W, batch, then=None):
    kw = dict(OPTS, tol=1e-6, batch=batch, model_grid=model_grid)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, [1.5, -1.2], rec, **kw) as sj:
        if then is not None:
            before = sj.device_bytes
            sj.set_model(then)
            assert sj.device_bytes == before
        out = dict(syn=sj.synthetic.copy(), jv=sj.jvec(v, mapped=True), jt=sj.jtvec(w, mapped=True))
        out['partial'] = sj.partial.copy()
        out['hv'] = sj.gauss_newton(v, W, mapped=True)
    return out


def test_batch_invariance_and_set_model_bitwise():
    """batch = 1, 2, 3 give identical results; set_model(model on the model grid) on an open object equals a fresh object."""
    import emg3d_amd as em
    g = load_golden("survey_jacobian.npz")
    model_grid, grid = grid_pairs(em, ['unaligned'])['unaligned']
    model, other = _models(em, model_grid, 'Resistivity'), _models(em, model_grid, 'Resistivity', seed=55)
    rec = tuple(g['rec'])
    rng = np.random.default_rng(56)
    v = np.asfortranarray(rng.standard_normal(model_grid.vnC))
    shape = (3, 2, rec[0].size)
    w = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    w[:, 1] = w[:, 1].real
    W = rng.uniform(0.5, 2.0, shape)
    one = _run(em, model_grid, grid, model, rec, v, w, W, 1)
    assert np.abs(one['jt']).max() > 0 and np.abs(one['hv']).max() > 0
    for batch in (2, 3):
        got = _run(em, model_grid, grid, model, rec, v, w, W, batch)
        assert all(np.array_equal(got[k], one[k]) for k in one), batch
    moved = _run(em, model_grid, grid, other, rec, v, w, W, 2, then=model)
    assert all(np.array_equal(moved[k], one[k]) for k in one)
    lg = _models(em, model_grid, 'LgConductivity')                  # the map may change with the model: other factor rules
    fresh = _run(em, model_grid, grid, lg, rec, v, w, W, 2)
    moved = _run(em, model_grid, grid, model, rec, v, w, W, 2, then=lg)
    assert all(np.array_equal(moved[k], fresh[k]) for k in fresh)
    assert not np.array_equal(fresh['jt'], one['jt'])


# ---- 4. adjoint pair and symmetry ----------------------------------------------------------------------------------------------
def test_adjoint_and_symmetry_48_from_20():
    """48 x 40 x 32 <- 20 x 16 x 12, a tri-axial resistivity model on the model grid, the survey, solver options, assertions and
    margin of test_gpu_survey_jacobian.py::test_adjoint_and_symmetry_48: each gap < 10 x adj_gap_cubic of the fixture.  The
    regridding layers are exact transposes of one another up to rounding, so the solves' tolerance sets the gaps as it does
    there."""
    em, grid, _, src, rec, rng = _model48()
    model_grid, g48 = grid_pairs(em, ['48'])['48']
    assert tuple(g48.vnC) == tuple(grid.vnC) == (48, 40, 32) and tuple(model_grid.vnC) == (20, 16, 12)
    assert all(np.array_equal(a, b) for a, b in zip(g48.h, grid.h)) and np.array_equal(g48.origin, grid.origin)
    ref_gap = float(load_golden("survey_jacobian.npz")['adj_gap_cubic'])
    rho = 10 ** rng.uniform(-0.3, 1.0, model_grid.nC)
    model = em.Model(model_grid, rho, rho * 10 ** rng.uniform(-0.3, 0.3, model_grid.nC), rho * 10 ** rng.uniform(-0.3, 0.3, model_grid.nC),
                     mapping='Resistivity')
    sources = [src, [310., -120., -60., -50., 20.], [20., 260., -90., 80., -30.]]
    freqs = [1.5, -0.8]
    vnM = tuple(int(n) for n in model_grid.vnC)
    v = (rng.standard_normal(model_grid.nC) * rho * 0.3).reshape(vnM, order='F')
    u = (rng.standard_normal(model_grid.nC) * rho * 0.3).reshape(vnM, order='F')
    kw = dict(OPTS, tol=1e-8, receiver_interpolation='cubic', adjoint='exact')
    with em.optimize.SurveyJacobian(grid, model, sources, freqs, rec, batch=3, model_grid=model_grid, **kw) as sj:
        syn = sj.synthetic
        shape = syn.shape
        w = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.abs(syn)
        w[:, 1] = w[:, 1].real
        W = 1.0 / np.abs(syn) ** 2
        jv = sj.jvec(v, mapped=True)
        jt = sj.jtvec(w, mapped=True)
        hv = sj.gauss_newton(v, W, mapped=True)
        hu = sj.gauss_newton(u, W, mapped=True)
    assert jt.shape == vnM and np.isfinite(jv).all() and np.isfinite(jt).all()
    lhs, rhs = np.real(np.sum(np.conj(w) * jv)), np.sum(jt * v)
    gap_adj = abs(lhs - rhs) / abs(lhs)
    uhv, vhu = np.sum(u * hv), np.sum(v * hu)
    gap_sym = abs(uhv - vhu) / abs(uhv)
    vhv, quad = np.sum(v * hv), np.sum(W * np.abs(jv) ** 2)
    gap_quad = abs(vhv - quad) / abs(quad)
    print(f"48x40x32 <- 20x16x12: adjoint gap {gap_adj:.2e}, symmetry gap {gap_sym:.2e}, v.Hv vs sum W |Jv|^2 {gap_quad:.2e} "
          f"(reference gap, cubic receivers: {ref_gap:.2e})")
    assert vhv > 0
    assert gap_adj < 10 * ref_gap
    assert gap_sym < 10 * ref_gap
    assert gap_quad < 10 * ref_gap


# ---- 5. the derivative of the regridding, no solves --------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['unaligned', 'inside'])
@pytest.mark.parametrize('mapping', ['Resistivity', 'Conductivity', 'LgConductivity', 'LnResistivity'])
def test_regridding_derivative_vs_central_differences(name, mapping):
    """A central difference of Model.interpolate2grid with a relative step of 1e-5 against diag(p_c) A diag(1 / p_m) v (the two
    linear maps, regridded in log10) resp. A v (logarithmic maps), and of the conductivity on the computational grid against
    F (.) A (Q (.) v) with maps.regrid_factors: agreement below 1e-6 of max|.| -- truncation is ~1e-10 (h^2), round-off ~1e-11
    (eps / h), a missing or wrong factor is O(1)."""
    import emg3d_amd as em
    model_grid, grid = grid_pairs(em, [name])[name]
    mats, vol = axis_matrices(em, model_grid, grid), volumes(grid)
    rng = np.random.default_rng(57)
    log = em.maps.MAPS[mapping].log
    p = rng.uniform(-1.0, 1.0, model_grid.vnC) if log else 10 ** rng.uniform(-0.5, 1.0, model_grid.vnC)
    scale = np.ones(model_grid.vnC) if log else p
    v = rng.standard_normal(model_grid.vnC) * scale
    h = 1e-5

    def on_grid(q):
        m = em.Model(model_grid, q, mapping=mapping).interpolate2grid(model_grid, grid)
        return m.property_x, m.conductivity('property_x')
    p_c, sigma_c = on_grid(p)
    (pp, sp), (pm, sm) = on_grid(p + h * v), on_grid(p - h * v)
    fd_p, fd_s = (pp - pm) / (2 * h), (sp - sm) / (2 * h)
    want_p = dense_forward(mats, v, vol) if log else p_c * dense_forward(mats, v / p, vol)
    e_p = np.abs(fd_p - want_p).max() / np.abs(want_p).max()
    F, Q = em.maps.regrid_factors(em.Model(model_grid, p, mapping=mapping), (sigma_c,) * 3)
    want_s = F[0] * dense_forward(mats, Q[0] * v, vol)
    e_s = np.abs(fd_s - want_s).max() / np.abs(want_s).max()
    print(f"{name} {mapping}: d p_c {e_p:.2e}, d sigma_c {e_s:.2e}")
    assert np.abs(want_p).max() > 0 and np.abs(want_s).max() > 0
    assert e_p < 1e-6
    assert e_s < 1e-6


# ---- 6. errors and unchanged paths ----------------------------------------------------------------------------------------------
def test_errors_and_unchanged_paths():
    import emg3d_amd as em
    g = load_golden("survey_jacobian.npz")
    model_grid, grid = grid_pairs(em, ['unaligned'])['unaligned']
    mats, vol = axis_matrices(em, model_grid, grid), volumes(grid)
    rec = tuple(g['rec'])
    model = _models(em, model_grid, 'Resistivity')
    rng = np.random.default_rng(58)
    v = np.asfortranarray(rng.standard_normal(model_grid.vnC))
    w = rng.standard_normal((3, 1, rec[0].size))
    with em.optimize.SurveyJacobian(grid, model, SOURCES, [1.5], rec, model_grid=model_grid, **dict(OPTS, tol=1e-6)) as sj:
        for call in (lambda: sj.jvec(v), lambda: sj.jvec(v, mapped=False), lambda: sj.jtvec(w, mapped=False),
                     lambda: sj.gauss_newton(v)):
            with pytest.raises(ValueError, match="model's own property"):
                call()
        with pytest.raises(ValueError, match="`v`"):
            sj.jvec(np.zeros(grid.vnC), mapped=True)
        with pytest.raises(ValueError, match="model_grid"):
            sj.set_model(em.Model(grid, np.ones(grid.nC)))
        assert sj.jvec(v, mapped=True).shape == (3, 1, rec[0].size)
    # model_gradient: 'cubic' stays what it was, 'transpose' is the operator of the class
    grad = np.asfortranarray(rng.standard_normal(grid.vnC))
    with pytest.raises(ValueError, match="model_grid"):
        em.optimize.model_gradient(grid, model, grad, method='transpose')
    cubic = em.optimize.model_gradient(grid, model, grad, model_grid)
    rho = model.property_x
    assert np.array_equal(cubic, em.maps.grid2grid(grid, -grad, model_grid, method='cubic') * (-1.0 / rho ** 2))
    assert np.array_equal(cubic, em.optimize.model_gradient(grid, model, grad, model_grid, method='cubic'))
    got = em.optimize.model_gradient(grid, model, grad, model_grid, method='transpose')
    sigma_c = model.interpolate2grid(model_grid, grid).conductivity('property_x')
    want, bound = dense_adjoint(mats, -grad, vol, -sigma_c, 1.0 / rho)
    assert got.shape == tuple(model_grid.vnC) and np.all(np.abs(got - want) <= bound) and np.abs(want).max() > 0
    # ... and same-grid calls are untouched
    same = em.Model(grid, np.full(grid.nC, 2.0))
    assert np.array_equal(em.optimize.model_gradient(grid, same, grad), -grad * (-1.0 / 4.0))
