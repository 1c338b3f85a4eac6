"""CPU-only: the six property maps on the host -- ``maps.Map*``, ``Model(mapping=...)``, ``VolumeModel``, ``model_parts``,
``optimize.model_gradient`` -- against the reference's own maps (tests/golden/property_maps.npz, written by
tests/golden/make_property_maps_golden.py, which imports the reference), and the argument errors of ``set_model``,
``survey_gradient(handles=)`` and ``mapped=`` that are raised before the library is touched."""
import numpy as np
import pytest

from conftest import load_golden

NAMES = ('Conductivity', 'Resistivity', 'LgConductivity', 'LnConductivity', 'LgResistivity', 'LnResistivity')
LOG = NAMES[2:]


@pytest.fixture(scope="module")
def gold():
    g = load_golden("property_maps.npz")
    assert tuple(g['names']) == NAMES and list(g['codes']) == list(range(6))
    return g


def _grid(em, g, tag=''):
    return em.TensorMesh([g[tag + 'hx'], g[tag + 'hy'], g[tag + 'hz']], origin=g[tag + 'origin'])


def _model(em, g, grid, name, case=3):
    p = g[f'{name}_p']
    return em.Model(grid, p[0], p[1] if case in (1, 3) else None, p[2] if case in (2, 3) else None, mapping=name)


@pytest.mark.parametrize('name', NAMES)
def test_maps_equal_the_reference_bitwise(gold, name):
    from emg3d_amd import maps
    m = getattr(maps, 'Map' + name)()
    assert m.name == name and isinstance(m.description, str) and m.code == NAMES.index(name)
    assert m.log == (name in LOG)
    p = gold[f'{name}_p']
    back = m.backward(p)
    assert np.array_equal(back, gold[f'{name}_back'])
    assert np.array_equal(m.forward(back[0]), gold[f'{name}_fwdback'])
    grad = gold['grad'].copy()
    assert m.derivative_chain(grad, p[0]) is None           # in place
    assert np.array_equal(grad, gold[f'{name}_chain'])
    # the chain factor from the conductivity alone: the same derivative (the roundings of its products may differ)
    np.testing.assert_allclose(gold['grad'] * m.chain_factor(back[0]), gold[f'{name}_chain'], rtol=4e-16)


def test_model_accepts_what_the_map_allows(gold):
    import emg3d_amd as em
    grid = _grid(em, gold)
    neg = -np.ones(grid.nC)
    for name in NAMES:
        model = em.Model(grid, gold[f'{name}_p'][0], mapping=name)
        assert model.map.name == name and model.mapping == name
        assert np.array_equal(model.conductivity('property_x'), gold[f'{name}_back'][0])
        if name in LOG:
            assert np.array_equal(em.Model(grid, neg, mapping=name).property_x.ravel('F'), neg)
        else:
            with pytest.raises(ValueError, match="finite and positive"):
                em.Model(grid, neg, mapping=name)
        for bad in (np.nan, np.inf):
            with pytest.raises(ValueError, match="finite"):
                em.Model(grid, np.full(grid.nC, bad), mapping=name)
        with pytest.raises(ValueError, match="positive"):        # mu_r / epsilon_r are never mapped
            em.Model(grid, gold[f'{name}_p'][0], mu_r=neg, mapping=name)
    with pytest.raises(ValueError, match="mapping"):
        em.Model(grid, 1., mapping='LgSomething')
    assert repr(em.Model(grid, 1.)) == f"Model [Resistivity]; isotropic; {tuple(grid.vnC)}"


@pytest.mark.parametrize('name', NAMES)
def test_volume_model_equals_the_reference_bitwise(gold, name):
    import emg3d_amd as em
    grid = _grid(em, gold)
    model = _model(em, gold, grid, name)
    for key, freq in (('eta_f', 1.5), ('eta_s', -1.5)):
        vm = em.VolumeModel(grid, model, em.SourceField(grid, freq=freq))
        assert vm.eta_x.dtype == gold[f'{name}_{key}'].dtype
        assert np.array_equal(vm.eta_x, gold[f'{name}_{key}'])


@pytest.mark.parametrize('name', NAMES)
def test_interpolate2grid_takes_log_for_the_other_maps_only(gold, name, monkeypatch):
    """The host part of Model.interpolate2grid: which arrays go to grid2grid, and the default of `log` (reference
    models.py:390)."""
    import emg3d_amd as em
    from emg3d_amd import maps
    grid, grid2 = _grid(em, gold), _grid(em, gold, 'g2_')
    calls = []

    def fake(**kw):
        calls.append(kw)
        return np.full(grid2.vnC, -1.0 if name in LOG else 1.0)
    monkeypatch.setattr(maps, 'grid2grid', fake)
    new = _model(em, gold, grid, name).interpolate2grid(grid, grid2)
    assert new.mapping == name and new.case == 3 and len(calls) == 3
    for c, kw in enumerate(calls):
        assert kw['log'] is (name not in LOG) and kw['method'] == 'volume' and kw['extrapolate'] is True
        assert np.array_equal(kw['values'], gold[f'{name}_p'][c])
    calls.clear()
    _model(em, gold, grid, name, case=0).interpolate2grid(grid, grid2, log=name in LOG, method='cubic')
    assert len(calls) == 1 and calls[0]['log'] is (name in LOG) and calls[0]['method'] == 'cubic'


@pytest.mark.parametrize('name', NAMES)
def test_model_gradient_chain_rule(gold, name):
    """optimize.model_gradient(grid, model, grad) is the map's derivative_chain applied to -grad; rtol=1e-15 is the bound of
    the resistivity check in test_gpu_grid2grid.py."""
    import emg3d_amd as em
    grid = _grid(em, gold)
    model = _model(em, gold, grid, name, case=0)
    before = model.property_x.copy()
    grad = -gold['grad']
    got = em.optimize.model_gradient(grid, model, grad)
    np.testing.assert_allclose(got, gold[f'{name}_chain'], rtol=1e-15, atol=0)
    assert np.array_equal(grad, -gold['grad']) and np.array_equal(model.property_x, before)         # inputs untouched


def test_model_parts_raw(gold):
    """The two existing mappings: today's tuple (five arrays and a bool); the logarithmic ones: the property arrays, False and
    the map code as an attribute."""
    import emg3d_amd as em
    from emg3d_amd import models
    grid = _grid(em, gold)
    vol = grid.cell_volumes.reshape(grid.vnC, order='F')
    for name in NAMES:
        for case in (0, 3):
            model = _model(em, gold, grid, name, case)
            parts = models.model_parts(grid, model, raw=True)
            assert isinstance(parts, tuple) and len(parts) == 6
            assert type(parts[5]) is bool and parts[5] == (name == 'Resistivity')
            assert parts.map_code == NAMES.index(name) and parts.epsilon_r is None
            p = gold[f'{name}_p']
            assert np.array_equal(parts[0], p[0]) and np.array_equal(parts[3], vol) and np.array_equal(parts[4], vol)
            if case == 0:
                assert parts[1] is parts[0] and parts[2] is parts[0]
            else:
                assert np.array_equal(parts[1], p[1]) and np.array_equal(parts[2], p[2])
            assert all(a.flags.f_contiguous and a.dtype == np.float64 for a in parts[:5])
            # raw=False, sigma_volume, eta_factored: conductivities for every map
            cooked = models.model_parts(grid, model)
            assert len(cooked) == 5 and cooked.map_code is None
            assert np.array_equal(cooked[0], gold[f'{name}_back'][0])
            assert np.array_equal(models.sigma_volume(grid, model)[0], vol * gold[f'{name}_back'][0])
            sf = em.SourceField(grid, freq=1.5)
            fac = models.eta_factored(grid, model, sf)
            assert np.array_equal(fac[4] * fac[0], gold[f'{name}_eta_f'])


class _Untouched:
    """Stands where the loaded library would: any call fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called: {name}")


def _fake_handle(em, grid, model):
    """A DeviceMG that remembers what from_model_parts records about its first model, without a library behind it."""
    from emg3d_amd import models, solver
    dev = solver.DeviceMG.__new__(solver.DeviceMG)
    parts = models.model_parts(grid, model, raw=True)
    dev._lib, dev._h = _Untouched(), None
    dev.nC, dev._vnC = int(grid.nC), tuple(int(n) for n in grid.vnC)
    dev._alias = (parts[1] is parts[0], parts[2] is parts[0])
    dev._zeta = solver._cells(parts[4])
    dev._eps = parts.epsilon_r is not None
    dev._epsr = None if parts.epsilon_r is None else solver._cells(parts.epsilon_r)
    return dev


def test_set_model_refuses_before_anything_is_uploaded(gold):
    import emg3d_amd as em
    from emg3d_amd import solver
    grid, grid2 = _grid(em, gold), _grid(em, gold, 'g2_')
    iso = _model(em, gold, grid, 'LgConductivity', case=0)
    tri = _model(em, gold, grid, 'LgConductivity', case=3)
    dev = _fake_handle(em, grid, iso)
    with pytest.raises(ValueError, match="anisotropy case"):
        dev.set_model(grid, tri)
    with pytest.raises(ValueError, match="anisotropy case"):
        _fake_handle(em, grid, tri).set_model(grid, _model(em, gold, grid, 'Resistivity', case=1))
    with pytest.raises(ValueError, match="cells"):
        dev.set_model(grid2, em.Model(grid2, 1.))
    p = gold['Conductivity_p'][0]
    with pytest.raises(ValueError, match="epsilon_r"):
        dev.set_model(grid, em.Model(grid, p, epsilon_r=np.full(grid.nC, 2.), mapping='Conductivity'))
    with pytest.raises(ValueError, match="mu_r"):
        dev.set_model(grid, em.Model(grid, p, mu_r=np.full(grid.nC, 2.), mapping='Conductivity'))
    eps = _fake_handle(em, grid, em.Model(grid, p, epsilon_r=np.full(grid.nC, 2.), mapping='Conductivity'))
    with pytest.raises(ValueError, match="epsilon_r"):
        eps.set_model(grid, iso)
    # FrequencyHandles: every handle is asked before the first upload, `parts` stays
    handles = solver.FrequencyHandles(grid, 'first parts', 0)
    handles._handles = {('<c16',): _fake_handle(em, grid, iso), ('<f8',): _fake_handle(em, grid, iso)}
    with pytest.raises(ValueError, match="anisotropy case"):
        handles.set_model(tri)
    assert handles.parts == 'first parts'
    handles._handles = {}


def test_survey_gradient_handles_and_mapped_arguments(gold):
    import emg3d_amd as em
    from emg3d_amd import solver
    grid, grid2 = _grid(em, gold), _grid(em, gold, 'g2_')
    model = _model(em, gold, grid, 'LgConductivity', case=0)
    rec = (np.array([100., 200.]), np.array([0., 0.]), np.array([-50., -50.]), np.array([0., 0.]), np.array([0., 0.]))
    sources = [[0., 0., -100., 0., 0.]] * 3
    obs = np.zeros((3, 1, 2), dtype=complex)
    sg = em.optimize.survey_gradient
    with pytest.raises(ValueError, match="nsys"):
        sg(grid, model, sources, [1.0], rec, obs, batch=2, handles=solver.FrequencyHandles(grid, None, 0, nsys=3, bvecs=1))
    with pytest.raises(ValueError, match="bvecs"):
        sg(grid, model, sources, [1.0], rec, obs, batch=2, handles=solver.FrequencyHandles(grid, None, 0, nsys=2))
    with pytest.raises(ValueError, match="another grid"):
        sg(grid, model, sources, [1.0], rec, obs, batch=2, handles=solver.FrequencyHandles(grid2, None, 0, nsys=2, bvecs=1))
    with pytest.raises(TypeError, match="FrequencyHandles"):
        sg(grid, model, sources, [1.0], rec, obs, batch=2, handles=object())
    # mapped= must be a bool; a closed Jacobian says so for the mapped products as for the others
    v = np.zeros(grid.vnC)
    jac = em.optimize.Jacobian(grid, model, sources[0], 1.0, rec)
    sj = em.optimize.SurveyJacobian(grid, model, sources, [1.0], rec)
    for obj, w in ((jac, np.zeros(2)), (sj, obs)):
        for call in (lambda m: obj.jvec(v, mapped=m), lambda m: obj.jtvec(w, mapped=m)):
            with pytest.raises(TypeError, match="mapped"):
                call('yes')
            with pytest.raises(RuntimeError, match="closed"):
                call(True)
        with pytest.raises(RuntimeError, match="closed"):
            obj.set_model(model)
    with pytest.raises(TypeError, match="mapped"):
        sj.gauss_newton(v, mapped=1)
    with pytest.raises(RuntimeError, match="closed"):
        sj.gauss_newton(v, mapped=True)
