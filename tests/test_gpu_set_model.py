"""GPU: another model on an open handle -- DeviceMG.set_model / emg3d_mg_set_model, FrequencyHandles.set_model,
Jacobian.set_model, SurveyJacobian.set_model and survey_gradient(handles=).

The claim is always the same: a re-targeted handle is a fresh handle, bit for bit -- fields, cycle counts, every norm of the
info dicts, the products of the Jacobians -- while nothing is allocated.  No reference is needed for that; the models are those
of tests/golden/survey_jacobian.npz (12 x 10 x 8) and of test_gpu_jacobian.py's 48 x 40 x 32 model."""
import numpy as np
import pytest

from conftest import load_golden
from test_gpu_jacobian import INFO_KEYS, OPTS, _model48

pytestmark = pytest.mark.gpu

SRC = [30., -20., -40., 20., 10.]
SOURCES = [SRC, [-110., 60., -70., -50., 20.], [150., 90., -30., 80., -30.]]


def _grid12(em):
    g = load_golden("survey_jacobian.npz")
    return g, em.TensorMesh([g['hx'], g['hy'], g['hz']], origin=g['origin'])


def _models12(em, g, grid, case, **kw):
    """Two models of the same anisotropy case: the fixture's conductivities, and another in another map (resistivity)."""
    rng = np.random.default_rng(7)
    s3 = [g['tri_sig_x'], g['tri_sig_y'], g['tri_sig_z']]
    r3 = [10 ** rng.uniform(-0.5, 1.5, grid.nC) for _ in range(3)]
    pick = (lambda a: (a[0], a[1], a[2])) if case == 3 else (lambda a: (a[0],))
    return em.Model(grid, *pick(s3), mapping='Conductivity', **kw), em.Model(grid, *pick(r3), mapping='Resistivity', **kw)


def _same_info(a, b):
    assert (a is None) == (b is None)
    if a is None:
        return
    for key in INFO_KEYS:
        assert a[key] == b[key], key
    assert np.array_equal(a['error_at_cycle'], b['error_at_cycle'])


def _solve(em, grid, dev, freq, **kw):
    """One solve on the handle (source built in HBM); returns (field, info)."""
    sf = em.SourceField(grid, freq=freq)
    e, info = em.solve(grid, None, sf, handle=dev, return_info=True, source=(SRC, 0), **dict(OPTS, tol=1e-6, **kw))
    return np.array(e.field), info


def _spec(em, freq):
    return em.fields.FrequencySpec(freq)


@pytest.mark.parametrize('freq', [1.5, -1.5], ids=['c128', 'f64'])
@pytest.mark.parametrize('case', [0, 3], ids=['iso', 'tri'])
def test_retargeted_handle_is_a_fresh_handle(freq, case):
    """from_model(m1), solve, set_model(m2), solve == a handle created from m2; the same after a following set_smu0 to another
    frequency; and set_model before the first solve."""
    import emg3d_amd as em
    from emg3d_amd import models
    from emg3d_amd.solver import DeviceMG
    g, grid = _grid12(em)
    m1, m2 = _models12(em, g, grid, case)
    other = freq * 0.4
    with DeviceMG.from_model(grid, models.model_parts(grid, m2, raw=True), _spec(em, freq)) as fresh:
        e_ref, i_ref = _solve(em, grid, fresh, freq)
        sig_ref = [fresh.get_sigma(c) for c in range(3)]
        fresh.retarget(_spec(em, other))
        e_ref2, i_ref2 = _solve(em, grid, fresh, other)
    assert i_ref['exit'] == 0 and i_ref['it_mg'] > 1 and np.abs(e_ref).max() > 0
    with DeviceMG.from_model(grid, models.model_parts(grid, m1, raw=True), _spec(em, freq)) as dev:
        e1, _ = _solve(em, grid, dev, freq)
        assert not np.array_equal(e1, e_ref)
        nbytes = dev.device_bytes
        dev.set_model(grid, m2)
        assert dev.device_bytes == nbytes
        for c in range(3):
            assert np.array_equal(dev.get_sigma(c), sig_ref[c])
        e2, i2 = _solve(em, grid, dev, freq)
        assert np.array_equal(e2, e_ref)
        _same_info(i2, i_ref)
        dev.retarget(_spec(em, other))
        e3, i3 = _solve(em, grid, dev, other)
        assert np.array_equal(e3, e_ref2)
        _same_info(i3, i_ref2)
    with DeviceMG.from_model(grid, models.model_parts(grid, m1, raw=True), _spec(em, freq)) as dev:
        dev.set_model(grid, m2)                      # no hierarchy yet: level 0 only
        e4, i4 = _solve(em, grid, dev, freq)
        assert np.array_equal(e4, e_ref)
        _same_info(i4, i_ref)


@pytest.mark.parametrize('freq', [1.5, -1.5], ids=['c128', 'f64'])
def test_retargeted_handle_with_epsilon_r(freq):
    """An epsilon_r handle: the refresh uses the handle's current s eps_0, also after set_smu0(..., sval)."""
    import emg3d_amd as em
    from emg3d_amd import models
    from emg3d_amd.solver import DeviceMG
    g, grid = _grid12(em)
    eps = np.random.default_rng(8).uniform(1, 40, grid.nC)
    m1, m2 = _models12(em, g, grid, 3, epsilon_r=eps)
    other = freq * 3
    with DeviceMG.from_model(grid, models.model_parts(grid, m2, raw=True), _spec(em, other)) as fresh:
        e_ref, i_ref = _solve(em, grid, fresh, other)
    with DeviceMG.from_model(grid, models.model_parts(grid, m1, raw=True), _spec(em, freq)) as dev:
        _solve(em, grid, dev, freq)
        dev.retarget(_spec(em, other))
        dev.set_model(grid, m2)
        e2, i2 = _solve(em, grid, dev, other)
    assert np.array_equal(e2, e_ref)
    _same_info(i2, i_ref)


def test_retargeted_batched_handle():
    """set_batch(3) with solve_sources: three systems through the re-targeted operator."""
    import emg3d_amd as em
    from emg3d_amd import models
    from emg3d_amd.solver import DeviceMG
    g, grid = _grid12(em)
    m1, m2 = _models12(em, g, grid, 3)
    kw = dict(OPTS, tol=1e-6)
    ref, iref = em.solver.solve_sources(grid, m2, SOURCES, 1.5, **kw)
    with DeviceMG.from_model(grid, models.model_parts(grid, m1, raw=True), _spec(em, 1.5)) as dev:
        dev.set_batch(3)
        em.solver.solve_sources(grid, None, SOURCES, 1.5, handle=dev, download=False, **kw)
        dev.set_model(grid, m2)
        got, igot = em.solver.solve_sources(grid, None, SOURCES, 1.5, handle=dev, **kw)
    for a, b, ia, ib in zip(got, ref, igot, iref):
        assert np.array_equal(a.field, b.field) and np.abs(b.field).max() > 0
        _same_info(ia, ib)


def test_retargeted_handle_48():
    """48 x 40 x 32, sc + lr: several hierarchies, transposed model copies and every factor cache are refreshed."""
    import emg3d_amd as em
    from emg3d_amd import models
    from emg3d_amd.solver import DeviceMG
    _, grid, s3, _, _, rng = _model48()
    m1 = em.Model(grid, *s3, mapping='Conductivity')
    m2 = em.Model(grid, *(np.log(s * 10 ** rng.uniform(-0.5, 0.5, grid.nC)) for s in s3), mapping='LnConductivity')
    src = [-120., 40., 30., 25., 5.]

    def solve(dev):
        sf = em.SourceField(grid, freq=1.5)
        e, info = em.solve(grid, None, sf, handle=dev, return_info=True, source=(src, 0), **dict(OPTS, tol=1e-6))
        return np.array(e.field), info
    with DeviceMG.from_model(grid, models.model_parts(grid, m2, raw=True), _spec(em, 1.5)) as fresh:
        e_ref, i_ref = solve(fresh)
    with DeviceMG.from_model(grid, models.model_parts(grid, m1, raw=True), _spec(em, 1.5)) as dev:
        solve(dev)
        nbytes = dev.device_bytes
        dev.set_model(grid, m2)
        assert dev.device_bytes == nbytes
        e2, i2 = solve(dev)
    assert i_ref['exit'] == 0 and i_ref['it_mg'] > 2
    assert np.array_equal(e2, e_ref)
    _same_info(i2, i_ref)


def test_refusals_leave_the_handle_usable():
    import emg3d_amd as em
    from emg3d_amd import _lib, models
    from emg3d_amd.solver import DeviceMG
    g, grid = _grid12(em)
    iso, _ = _models12(em, g, grid, 0)
    tri, _ = _models12(em, g, grid, 3)
    spec = _spec(em, 1.5)
    # handles that do not keep sigma and V apart: the library says which entry point refused
    with DeviceMG.from_sigma_volume(grid, *models.sigma_volume(grid, iso), smu0=spec.smu0) as dev:
        with pytest.raises(_lib.HipLibraryError, match="emg3d_mg_set_model"):
            dev.set_model(grid, iso)
        with pytest.raises(_lib.HipLibraryError, match="emg3d_mg_get_sigma"):
            dev.get_sigma()
    with DeviceMG.from_model(grid, models.model_parts(grid, iso, raw=True), spec) as dev:
        before, ibefore = _solve(em, grid, dev, 1.5)
        with pytest.raises(ValueError, match="anisotropy case"):
            dev.set_model(grid, tri)
        h2 = np.ones(4) * 50.
        small = em.TensorMesh([h2, h2, h2], origin=(0., 0., 0.))
        with pytest.raises(ValueError, match="cells"):
            dev.set_model(small, em.Model(small, 1.))
        # the library's own checks, behind the host's: a changed alias pattern, an unknown map code
        lib = _lib.load()
        p = np.ones(grid.nC)
        q = np.ones(grid.nC)
        assert lib.emg3d_mg_set_model(dev._h, 0, _lib.ptr(p), _lib.ptr(q), None) == -2
        assert lib.emg3d_mg_set_model(dev._h, 6, _lib.ptr(p), None, None) == -2
        assert lib.emg3d_mg_set_model(dev._h, -1, _lib.ptr(p), _lib.ptr(p), _lib.ptr(p)) == -2
        assert lib.emg3d_mg_get_sigma(dev._h, 3, _lib.ptr(p)) == -2
        with pytest.raises(_lib.HipLibraryError, match="emg3d_mg_get_sigma"):
            dev.get_sigma(-1)
        after, iafter = _solve(em, grid, dev, 1.5)
        assert np.array_equal(after, before)
        _same_info(iafter, ibefore)
    # a map code of 6 at creation
    parts = models.model_parts(grid, iso, raw=True)
    with pytest.raises(_lib.HipLibraryError, match="emg3d_mg_create_vs"):
        DeviceMG.from_model_parts(grid, *parts, smu0=spec.smu0, map_code=6)
    with pytest.raises(_lib.HipLibraryError, match="emg3d_mg_create_vse"):
        DeviceMG.from_model_parts(grid, *parts, smu0=spec.smu0, map_code=6, epsilon_r=np.ones(grid.vnC), sval=spec.sval)


def _products(sj, v, w, W):
    out = dict(syn=sj.synthetic.copy(), finfo=sj.forward_info)
    out['jv'] = sj.jvec(v); out['jv_info'] = sj.info
    out['jt'] = sj.jtvec(w); out['jt_info'] = sj.info
    out['jt3'] = np.stack(sj.jtvec(w, components=True)); out['jt3_info'] = sj.info
    out['hv'] = sj.gauss_newton(v, W); out['hv_info'] = sj.info
    return out


def _same_products(a, b):
    for key in ('syn', 'jv', 'jt', 'jt3', 'hv'):
        assert np.array_equal(a[key], b[key]), key
        assert np.isfinite(b[key]).all() and np.abs(b[key]).max() > 0
    for key in ('finfo', 'jv_info', 'jt_info', 'jt3_info', 'hv_info'):
        for ra, rb in zip(a[key], b[key]):
            for da, db in zip(ra, rb):
                _same_info(da, db)


def test_survey_jacobian_set_model():
    """3 sources, [1.5 Hz, Laplace -1.5], batch 2 (a short last chunk): after set_model(m2) everything equals a new
    SurveyJacobian on m2 -- with batch 2 and with batch 3 --, and device_bytes has not moved."""
    import emg3d_amd as em
    g, grid = _grid12(em)
    m1, m2 = _models12(em, g, grid, 3)
    rec = tuple(g['rec'])
    freqs = [1.5, -1.5]
    vnC = tuple(int(n) for n in grid.vnC)
    rng = np.random.default_rng(41)
    v = g['tri_v'].reshape(vnC, order='F')
    shape = (3, 2, rec[0].size)
    w = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    w[:, 1] = w[:, 1].real
    W = rng.uniform(0.5, 2.0, shape)
    kw = dict(OPTS, tol=1e-6)
    SJ = em.optimize.SurveyJacobian
    with SJ(grid, m1, SOURCES, freqs, rec, batch=2, **kw) as sj:
        first = _products(sj, v, w, W)['syn']               # (every product once: accumulators and hierarchies exist)
        nbytes = sj.device_bytes
        assert sj.set_model(m2) is sj and sj.model is m2
        assert sj.info is None and sj.partial is None
        assert sj.device_bytes == nbytes
        got = _products(sj, v, w, W)
    assert not np.array_equal(first, got['syn'])
    for batch in (2, 3):
        with SJ(grid, m2, SOURCES, freqs, rec, batch=batch, **kw) as sj:
            _same_products(got, _products(sj, v, w, W))


def test_jacobian_set_model():
    import emg3d_amd as em
    g, grid = _grid12(em)
    m1, m2 = _models12(em, g, grid, 3)
    rec = tuple(g['rec'])
    vnC = tuple(int(n) for n in grid.vnC)
    rng = np.random.default_rng(42)
    v = rng.standard_normal((2,) + vnC) * 0.1
    w = rng.standard_normal((2, rec[0].size)) + 1j * rng.standard_normal((2, rec[0].size))
    kw = dict(OPTS, tol=1e-6, nvec=2)

    def products(jac):
        out = dict(syn=jac.synthetic.copy(), finfo=[[jac.forward_info]])
        out['jv'] = jac.jvec(v); out['jv_info'] = [jac.info]
        out['jt'] = jac.jtvec(w); out['jt_info'] = [jac.info]
        out['jt3'] = np.stack(jac.jtvec(w, components=True)); out['jt3_info'] = [jac.info]
        out['hv'], out['hv_info'] = out['jt'], out['jt_info']
        return out
    with em.optimize.Jacobian(grid, m1, SRC, 1.5, rec, **kw) as jac:
        products(jac)
        nbytes = jac.device_bytes
        assert jac.set_model(m2) is jac
        assert jac.device_bytes == nbytes
        got = products(jac)
    with em.optimize.Jacobian(grid, m2, SRC, 1.5, rec, **kw) as jac:
        _same_products(got, products(jac))


def test_survey_gradient_on_the_callers_handles():
    """Two survey_gradient calls on one FrequencyHandles with set_model between them: phi, grad and partial of two plain calls."""
    import emg3d_amd as em
    from emg3d_amd import models
    from emg3d_amd.solver import FrequencyHandles
    g, grid = _grid12(em)
    m1 = em.Model(grid, g['iso_sig_x'], mapping='Conductivity')
    m2 = em.Model(grid, np.log10(1 / g['tri_sig_y']), mapping='LgResistivity')
    rec = tuple(g['rec'])
    freqs = [1.5, -1.5]
    rng = np.random.default_rng(43)
    shape = (3, 2, rec[0].size)
    obs = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * 1e-12
    obs[:, 1] = obs[:, 1].real
    obs[1, 0, 2] = np.nan
    kw = dict(OPTS, tol=1e-6, batch=2, adjoint='exact')
    sg = em.optimize.survey_gradient
    plain = [sg(grid, m, SOURCES, freqs, rec, obs, **kw) for m in (m1, m2)]
    with FrequencyHandles(grid, models.model_parts(grid, m1, raw=True), 0, nsys=2, bvecs=1) as handles:
        kept = [sg(grid, m1, SOURCES, freqs, rec, obs, handles=handles, **kw)]
        nbytes = sum(dev.device_bytes for dev in handles)
        handles.set_model(m2)
        kept.append(sg(grid, m2, SOURCES, freqs, rec, obs, handles=handles, **kw))
        assert sum(dev.device_bytes for dev in handles) == nbytes and len(list(handles)) == 2
    assert not np.array_equal(plain[0][1], plain[1][1])
    for (phi_a, grad_a, info_a), (phi_b, grad_b, info_b) in zip(kept, plain):
        assert phi_a == phi_b and phi_b > 0
        assert np.array_equal(grad_a, grad_b) and np.abs(grad_b).max() > 0
        assert np.array_equal(info_a['partial'], info_b['partial'])
        assert np.array_equal(info_a['synthetic'], info_b['synthetic'], equal_nan=True)
        for key in ('forward', 'backward'):
            for ra, rb in zip(info_a[key], info_b[key]):
                for da, db in zip(ra, rb):
                    _same_info(da, db)
