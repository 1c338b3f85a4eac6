"""GPU: the property maps on the device -- k_sigma_of_map behind emg3d_mg_create_vs / emg3d_mg_set_model / emg3d_mg_get_sigma --
and what is built on them: solves of log-mapped models, the `mapped=True` products of the Jacobians, the misfit gradient in
log10 conductivity, Model.interpolate2grid for the six maps.

Reference: tests/golden/property_maps.npz (the reference's own maps, tests/golden/make_property_maps_golden.py).

MAP_ULP is the bound on |device sigma - NumPy sigma| in units in the last place, per map code.  Codes 0 and 1 are a copy and an
IEEE division: 0.  Codes 2-5 go through the device's exp10 / exp, which are not NumPy's pow / exp; the bound is twice the largest
deviation MEASURED on the fixture's 3 x 960 values per map, at least 1: the fixture has a few thousand cells, other inputs land
elsewhere within the functions' error.  Measured on an MI355X: 1 ulp for each of the codes 2, 3, 4, 5 -- in all
three components, and also on the 1001 and the 1 075 200 drawn values of the two shape tests below -- hence the bound 2."""
import numpy as np
import pytest

from conftest import load_golden
from test_gpu_jacobian import OPTS

pytestmark = pytest.mark.gpu

NAMES = ('Conductivity', 'Resistivity', 'LgConductivity', 'LnConductivity', 'LgResistivity', 'LnResistivity')
MAP_ULP = {0: 0, 1: 0, 2: 2, 3: 2, 4: 2, 5: 2}        # codes 2-5: twice the measured 1 ulp
SRC = [30., -20., -40., 20., 10.]


def _ulp(a, b):
    """Largest distance of two arrays of positive doubles in units in the last place."""
    a, b = np.ascontiguousarray(a).ravel(), np.ascontiguousarray(b).ravel()
    assert np.all(a > 0) and np.all(b > 0) and np.isfinite(a).all() and np.isfinite(b).all()
    return int(np.abs(a.view(np.int64) - b.view(np.int64)).max())


def _grid(em, g, tag=''):
    return em.TensorMesh([g[tag + 'hx'], g[tag + 'hy'], g[tag + 'hz']], origin=g[tag + 'origin'])


def _handle(em, grid, model, freq=1.5):
    from emg3d_amd import models
    from emg3d_amd.solver import DeviceMG
    return DeviceMG.from_model(grid, models.model_parts(grid, model, raw=True), em.fields.FrequencySpec(freq))


def _solve(em, grid, dev, freq=1.5):
    e, info = em.solve(grid, None, em.SourceField(grid, freq=freq), handle=dev, return_info=True, source=(SRC, 0),
                       **dict(OPTS, tol=1e-6))
    return np.array(e.field), info


@pytest.mark.parametrize('code', range(6), ids=NAMES)
def test_map_kernel_on_the_fixture(code):
    """get_sigma of a tri-axial handle against the reference's backward(p): codes 0, 1 bit for bit, 2-5 within MAP_ULP; and the
    handle solves exactly like a 'Conductivity' handle that is given the downloaded sigma."""
    import emg3d_amd as em
    g = load_golden("property_maps.npz")
    grid = _grid(em, g)
    name = NAMES[code]
    p, back = g[f'{name}_p'], g[f'{name}_back']
    with _handle(em, grid, em.Model(grid, p[0], p[1], p[2], mapping=name)) as dev:
        sig = [dev.get_sigma(c) for c in range(3)]
        dist = [_ulp(sig[c], back[c]) for c in range(3)]
        print(f"map code {code} ({name}): largest deviation from NumPy {max(dist)} ulp (x / y / z: {dist})")
        e_map, i_map = _solve(em, grid, dev)
    assert max(dist) <= MAP_ULP[code], (dist, MAP_ULP[code])
    with _handle(em, grid, em.Model(grid, *sig, mapping='Conductivity')) as dev:
        e_sig, i_sig = _solve(em, grid, dev)
    assert i_map['exit'] == 0 and np.abs(e_map).max() > 0
    assert np.array_equal(e_map, e_sig) and i_map['it_mg'] == i_sig['it_mg']
    assert np.array_equal(i_map['error_at_cycle'], i_sig['error_at_cycle'])


def _drawn(em, grid, code, seed):
    """A model in map `code` with log10(sigma) uniform in [-3, 1] (the fixture's range), and NumPy's conductivity of it."""
    from emg3d_amd import maps
    m = maps.MAPS[NAMES[code]]()
    lg = np.random.default_rng(seed).uniform(-3, 1, grid.nC)
    p = lg if code == 2 else m.forward(10 ** lg)
    return em.Model(grid, p, mapping=NAMES[code]), m.backward(p).reshape(grid.vnC, order='F')


def test_map_kernel_tail_of_the_last_block():
    """13 x 11 x 7 = 1001 cells: three full blocks and a tail of 233 threads' worth."""
    import emg3d_amd as em
    grid = em.TensorMesh([np.full(13, 40.), np.full(11, 50.), np.full(7, 60.)], origin=(0., 0., 0.))
    for code in range(6):
        model, want = _drawn(em, grid, code, 100 + code)
        with _handle(em, grid, model) as dev:
            got = dev.get_sigma()
        dist = _ulp(got, want)
        print(f"13 x 11 x 7, map code {code}: {dist} ulp")
        assert got.shape == (13, 11, 7) and dist <= MAP_ULP[code], (code, dist)


def test_map_kernel_second_pass_of_the_grid_stride_loop():
    """112 x 96 x 100 = 1 075 200 cells, more than the 256 x 4096 threads of a capped launch: one isotropic handle, created in
    one map and given the others with set_model; no solve."""
    import emg3d_amd as em
    grid = em.TensorMesh([np.full(112, 40.), np.full(96, 50.), np.full(100, 60.)], origin=(0., 0., 0.))
    assert grid.nC > 256 * 4096
    model, want = _drawn(em, grid, 2, 200)
    with _handle(em, grid, model) as dev:
        for code in (2, 0, 1, 3, 4, 5):
            if code != 2:
                model, want = _drawn(em, grid, code, 200 + code)
                dev.set_model(grid, model)
            got = dev.get_sigma()
            dist = _ulp(got, want)
            print(f"112 x 96 x 100, map code {code}: {dist} ulp")
            assert dist <= MAP_ULP[code], (code, dist)


@pytest.mark.parametrize('name', ['LgConductivity', 'LnResistivity'])
@pytest.mark.parametrize('case', [0, 3], ids=['iso', 'tri'])
def test_mapped_products(name, case):
    """jvec(v, mapped=True) == jvec(D v), jtvec(w, mapped=True) == D jtvec(w) (tri-axial: the sum of the D_c g_c), bit for bit,
    with D = d sigma / d p from get_sigma by multiplication; the adjoint identity of the mapped pair within the gap
    test_gpu_survey_jacobian.py::test_products_vs_reference allows for the unmapped pair on the same survey and settings."""
    import emg3d_amd as em
    sv = load_golden("survey_jacobian.npz")
    g = load_golden("property_maps.npz")
    grid = _grid(em, g)
    p = g[f'{name}_p']
    model = em.Model(grid, *(p if case == 3 else p[:1]), mapping=name)
    with _handle(em, grid, model) as dev:
        sig = [dev.get_sigma(c) for c in range(3)]
    ln10 = np.log(10)
    D = [s * ln10 for s in sig] if name == 'LgConductivity' else [-s for s in sig]
    rec = tuple(sv['rec'])
    vnC = tuple(int(n) for n in grid.vnC)
    v, w = sv['tri_v'].reshape(vnC, order='F'), sv['tri_w']
    kw = dict(OPTS, tol=1e-8, ordering='lex', receiver_interpolation='linear')
    with em.optimize.SurveyJacobian(grid, model, sv['sources'], sv['freqs'], rec, batch=2, **kw) as sj:
        jv_m = sj.jvec(v, mapped=True)
        jv = sj.jvec(tuple(d * v for d in D))
        jt_m = sj.jtvec(w, mapped=True)
        partial_m = np.array(sj.partial)
        jt3_m = sj.jtvec(w, components=True, mapped=True)
        jt3 = sj.jtvec(w, components=True)
        jt = sj.jtvec(w)
        hv_m = sj.gauss_newton(v, mapped=True)
        hv = sj.jtvec(jv_m, mapped=True)
    assert np.isfinite(jv_m).all() and np.abs(jv_m).max() > 0 and np.abs(jt_m).max() > 0
    assert np.array_equal(jv_m, jv)
    for c in range(3):
        assert np.array_equal(jt3_m[c], D[c] * jt3[c])
    if case == 0:
        assert np.array_equal(jt_m, D[0] * jt) and partial_m.shape == (2,) + vnC
    else:
        assert np.array_equal(jt_m, (D[0] * jt3[0] + D[1] * jt3[1]) + D[2] * jt3[2]) and partial_m.shape == (3, 2) + vnC
    assert np.array_equal(hv_m, hv)
    lhs, rhs = np.real(np.sum(np.conj(w) * jv_m)), np.sum(jt_m * v)
    gap = abs(lhs - rhs) / abs(lhs)
    print(f"{name} {case}: adjoint gap of the mapped pair {gap:.2e} (allowed: 10 x {float(sv['adj_gap_linear']):.2e})")
    assert gap < 10 * float(sv['adj_gap_linear'])


def test_mapped_products_single_pair_class():
    """optimize.Jacobian: the same identities, two vectors at a time."""
    import emg3d_amd as em
    sv = load_golden("survey_jacobian.npz")
    g = load_golden("property_maps.npz")
    grid = _grid(em, g)
    p = g['LgResistivity_p']
    model = em.Model(grid, p[0], p[1], p[2], mapping='LgResistivity')
    with _handle(em, grid, model) as dev:
        D = [-dev.get_sigma(c) * np.log(10) for c in range(3)]
    rec = tuple(sv['rec'])
    rng = np.random.default_rng(51)
    v = rng.standard_normal((2,) + tuple(grid.vnC))
    w = rng.standard_normal((2, rec[0].size)) + 1j * rng.standard_normal((2, rec[0].size))
    with em.optimize.Jacobian(grid, model, sv['sources'][0], 1.5, rec, nvec=2, **dict(OPTS, tol=1e-6)) as jac:
        assert np.array_equal(jac.jvec(v, mapped=True), jac.jvec(tuple(d * v for d in D)))
        jt3 = jac.jtvec(w, components=True)
        jt3_m = jac.jtvec(w, components=True, mapped=True)
        jt_m = jac.jtvec(w, mapped=True)
    for c in range(3):
        assert np.array_equal(jt3_m[c], D[c] * jt3[c]) and np.abs(jt3[c]).max() > 0
    assert np.array_equal(jt_m, (D[0] * jt3[0] + D[1] * jt3[1]) + D[2] * jt3[2])


def test_gradient_in_log10_conductivity_is_the_derivative_of_the_misfit():
    """The finite-difference check of test_gpu_gradient.py::test_gradient_is_the_derivative_of_the_misfit -- its grid, source,
    receiver, data, cells, one-sided step 1e-4 and tolerance 1e-3 -- with the model in log10 conductivity: survey_gradient on
    one FrequencyHandles (set_model per trial model) + model_gradient."""
    import emg3d_amd as em
    from emg3d_amd import models
    from emg3d_amd.solver import FrequencyHandles
    hx, hy, hz = np.ones(24) * 100., np.ones(16) * 100., np.ones(16) * 100.
    grid = em.TensorMesh([hx, hy, hz], origin=(0., 0., 0.))
    src = [450., 800., 800., 0., 0.]
    rec = (np.array([1950.]), np.array([800.]), np.array([800.]), np.array([0.]), np.array([0.]))
    kw = dict(cycle='F', tol=1e-11, maxit=80, verb=0)
    lg_true = np.zeros(grid.vnC)
    lg_true[9:14, 6:10, 5:9] = -2.
    e_obs = em.solve(grid, em.Model(grid, lg_true, mapping='LgConductivity'), em.get_source_field(grid, src, 1.0), **kw)
    obs = em.get_receiver_response(grid, e_obs, rec)
    w = 1 / (0.05 * np.abs(obs)) ** 2
    lg = np.zeros(grid.vnC)
    model = em.Model(grid, lg, mapping='LgConductivity')
    obs3, w3 = obs.reshape(1, 1, 1), w.reshape(1, 1, 1)
    with FrequencyHandles(grid, models.model_parts(grid, model, raw=True), 0, nsys=1, bvecs=1) as handles:
        phi0, grad, info = em.optimize.survey_gradient(grid, model, [src], [1.0], rec, obs3, w3, handles=handles, **kw)
        assert phi0 > 0 and info['backward'][0][0]['exit'] == 0
        dphi = em.optimize.model_gradient(grid, model, grad)
        for ijk in [(11, 8, 7), (10, 9, 6), (14, 8, 8)]:
            d = 1e-4
            l2 = lg.copy()
            l2[ijk] += d
            m2 = em.Model(grid, l2, mapping='LgConductivity')
            handles.set_model(m2)
            phi1, _, _ = em.optimize.survey_gradient(grid, m2, [src], [1.0], rec, obs3, w3, handles=handles, **kw)
            fd = (phi1 - phi0) / d
            print(f"cell {ijk}: finite difference {fd:.6e}, model_gradient {dphi[ijk]:.6e}, ratio - 1 = {fd / dphi[ijk] - 1:.2e}")
            assert abs(fd / dphi[ijk] - 1) < 1e-3, (ijk, fd, dphi[ijk])


@pytest.mark.parametrize('name', NAMES)
def test_interpolate2grid_vs_reference(name):
    """Model.interpolate2grid with its defaults (volume averaging on the device; of log10 of the values unless the map is a
    logarithm already) equals the reference's, bit for bit as maps.grid2grid(method='volume') does."""
    import emg3d_amd as em
    g = load_golden("property_maps.npz")
    grid, grid2 = _grid(em, g), _grid(em, g, 'g2_')
    p = g[f'{name}_p']
    new = em.Model(grid, p[0], p[1], p[2], mapping=name).interpolate2grid(grid, grid2)
    assert new.mapping == name
    for c, got in enumerate((new.property_x, new.property_y, new.property_z)):
        assert np.array_equal(got, g[f'{name}_interp'][c]), (name, c)
