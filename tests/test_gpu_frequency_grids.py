"""GPU: a computational grid per frequency -- optimize.SurveyJacobian and shard.solve_survey with a sequence for ``grid``.

Everything is compared BIT FOR BIT with existing code: entry j of a survey on the grids ``[A, B, A]`` against the single-grid object
``SurveyJacobian(grids[j], model, sources, [freqs[j]], rec, model_grid=M)``.  ``M`` (7 x 5 x 4) and ``A`` (12 x 10 x 8) are the
'unaligned' pair of tests/test_model_grid_host.py, ``B`` (16 x 12 x 8) shares no node with either and reaches beyond ``M`` on all six
sides (tests/test_frequency_grids_host.py); three sources, five receivers, tol 1e-6: 5-6 F-cycles per solve."""
import numpy as np
import pytest

from conftest import load_golden
from test_frequency_grids_host import SOURCES, copy_of, survey_grids
from test_gpu_jacobian import INFO_KEYS, OPTS
from test_gpu_model_grid import _models

pytestmark = pytest.mark.gpu

FREQS = [1.5, 0.7, -1.2]
KW = dict(OPTS, tol=1e-6)


def _rec():
    return tuple(load_golden("survey_jacobian.npz")['rec'])


def _vectors(M, n_freq, n_rec, seed, real=()):
    """(v on the model grid, data-space w with real columns at the Laplace-domain entries, weights W)."""
    rng = np.random.default_rng(seed)
    v = np.asfortranarray(rng.standard_normal(M.vnC))
    shape = (3, n_freq, n_rec)
    w = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    for j in real:
        w[:, j] = w[:, j].real
    return v, w, rng.uniform(0.5, 2.0, shape)


def _same_infos(a, b):
    return all(a[k] == b[k] for k in ('it_mg', 'abs_error'))


def _handles(sj):
    """(position of the grid among the distinct ones, dtype) of every open handle."""
    return [(k, dev.dtype.str) for k, member in enumerate(sj._held.members) for dev in member]


# ---- 1. each frequency is its single-grid object -----------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['Resistivity', 'Conductivity-tri'])
def test_each_frequency_is_its_single_grid_object(kind):
    """[A, B, A] at (1.5 Hz, 0.7 Hz, s = 1.2), batch = 2 (chunks of 2 + 1): data, forward infos, J v, the per-frequency sums of
    J^T w, J^T w itself as the negated sequential sum of them in the order of `freqs` (per direction with components=True), and
    the Gauss-Newton product; three handles (A/c128, B/c128, A/f64)."""
    import emg3d_amd as em
    M, A, B = survey_grids(em)
    grids = [A, B, A]
    model = _models(em, M, kind)
    tri = model.case == 3
    rec = _rec()
    v, w, W = _vectors(M, 3, rec[0].size, 61, real=(2,))
    if not model.map.log:
        v = np.asfortranarray(v * model.property_x * 0.3)
    with em.optimize.SurveyJacobian(grids, model, SOURCES, FREQS, rec, batch=2, model_grid=M, **KW) as sj:
        assert sj.grid is grids and sj.grid_index == [0, 1, 0] and sj.grids == grids
        assert _handles(sj) == [(0, '<c16'), (0, '<f8'), (1, '<c16')] and len(list(sj._held)) == 3
        syn, finfo = sj.synthetic.copy(), sj.forward_info
        jv = sj.jvec(v, mapped=True)
        jt = sj.jtvec(w, mapped=True)
        part = sj.partial.copy()
        if tri:
            jt3 = sj.jtvec(w, components=True, mapped=True)
            assert np.array_equal(sj.partial, part)
        hv = sj.gauss_newton(v, W, mapped=True)
        assert np.array_equal(hv, sj.jtvec(W * jv, mapped=True))
        assert len(list(sj._held)) == 3
    assert syn.shape == jv.shape == (3, 3, rec[0].size) and np.isfinite(syn).all() and np.isfinite(jv).all()
    assert part.shape == ((3, 3) if tri else (3,)) + tuple(M.vnC)
    assert jt.shape == tuple(M.vnC) and np.abs(jt).max() > 0 and np.abs(hv).max() > 0
    assert all(np.abs(syn[:, j]).min() > 0 and np.abs(jv[:, j]).max() > 0 for j in range(3))
    assert np.all(syn[:, 2].imag == 0) and np.all(jv[:, 2].imag == 0)
    for j in range(3):
        with em.optimize.SurveyJacobian(grids[j], model, SOURCES, [FREQS[j]], rec, batch=2, model_grid=M, **KW) as one:
            assert np.array_equal(syn[:, j], one.synthetic[:, 0]), j
            assert all(_same_infos(finfo[i][j], one.forward_info[i][0]) for i in range(3)), j
            assert np.array_equal(jv[:, j], one.jvec(v, mapped=True)[:, 0]), j
            one.jtvec(w[:, j:j + 1], mapped=True)
            got = part[:, j] if tri else part[j]
            want = one.partial[:, 0] if tri else one.partial[0]
            assert got.shape == want.shape and np.array_equal(got, want) and np.abs(want).max() > 0, j
    zero = np.zeros(M.vnC)
    if tri:
        per = [-(((zero + part[c, 0]) + part[c, 1]) + part[c, 2]) for c in range(3)]
        assert np.array_equal(jt, (per[0] + per[1]) + per[2])
        assert all(np.array_equal(a, b) for a, b in zip(jt3, per))
    else:
        assert np.array_equal(jt, -(((zero + part[0]) + part[1]) + part[2]))


# ---- 2. rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('solves', [2, 1])
def test_rows_from_different_grids_fill_one_store(solves):
    """The same survey, a mask that drops receiver 2 at 0.7 Hz: sensitivity_rows(j, receivers=[3, 0]) and every row of park_rows
    against the single-grid objects; gram and matvec of the store against a DeviceRows filled with the same rows."""
    import emg3d_amd as em
    from emg3d_amd import solver
    M, A, B = survey_grids(em)
    grids = [A, B, A]
    model = _models(em, M, 'Resistivity')
    rec = _rec()
    n_rec = rec[0].size
    data = np.ones((3, 3, n_rec), dtype=bool)
    data[:, 1, 2] = False
    want_index = [(j, s, r, part) for j in range(3) for s in range(3) for r in range(n_rec) if data[s, j, r]
                  for part in range(2 if FREQS[j] > 0 else 1)]
    v = _vectors(M, 3, n_rec, 62)[0]
    with em.optimize.SurveyJacobian(grids, model, SOURCES, FREQS, rec, batch=2, model_grid=M, **KW) as sj:
        some = [sj.sensitivity_rows(j, receivers=[3, 0], mapped=True, solves=solves) for j in range(3)]
        store = sj.park_rows(data, mapped=True, solves=solves)
        assert np.array_equal(store.index, want_index) and store.n_rows == len(want_index) == 3 * 5 * 2 + 3 * 4 * 2 + 3 * 5
        assert store.solves == solves and store.rows.n_cols == M.nC
        assert store.info[1][2] is None and all(store.info[j][r] is not None for j in range(3) for r in range(n_rec) if (j, r) != (1, 2))
        rows = [store.row(i) for i in range(store.n_rows)]
        G, Jv = store.gram(), store.matvec(v)
    for j in range(3):
        with em.optimize.SurveyJacobian(grids[j], model, SOURCES, [FREQS[j]], rec, batch=2, model_grid=M, **KW) as one:
            want = one.sensitivity_rows(0, receivers=[3, 0], mapped=True, solves=solves)
            assert some[j].dtype == want.dtype and some[j].shape == want.shape == (3, 2) + tuple(M.vnC)
            assert np.array_equal(some[j], want), j
            assert all(np.abs(want[s, k]).max() > 0 for s in range(3) for k in range(2))
            every = one.sensitivity_rows(0, mapped=True, solves=solves)
        for i, (jf, s, r, part) in enumerate(want_index):
            if jf != j:
                continue
            ref = every[s, r]
            ref = (ref.real, ref.imag)[part] if np.iscomplexobj(ref) else ref
            assert rows[i].shape == ref.shape and np.array_equal(rows[i], ref), (i, jf, s, r, part)
    with solver.DeviceRows(len(rows), M.nC) as plain:
        for i, row in enumerate(rows):
            plain.set_row(i, np.ascontiguousarray(row.ravel(order='F')))
        assert np.array_equal(G, plain.gram()) and np.array_equal(Jv, plain.matvec(np.ascontiguousarray(v.ravel(order='F'))))
    assert np.array_equal(G, G.T) and np.abs(G).max() > 0 and np.abs(Jv).min() > 0


# ---- 3. a shared handle, and one regridding per distinct grid ----------------------------------------------------------------------
def test_shared_handle_and_regrid_count(monkeypatch):
    """[A, B, A] at three frequencies: two handles; entry 2 runs on A's handle re-targeted, behind entry 0's parked fields, and
    equals its single-grid object; a J v of an isotropic model regrids its perturbation once per distinct grid."""
    import emg3d_amd as em
    M, A, B = survey_grids(em)
    grids, freqs = [A, B, A], [1.5, 0.7, 0.4]
    model = _models(em, M, 'Resistivity')
    rec = _rec()
    v, w, _ = _vectors(M, 3, rec[0].size, 63)
    volume = []
    grid2grid = em.maps.grid2grid

    def counting(grid, values, new_grid, method='linear', *args, **kwargs):
        if method == 'volume':
            volume.append((grid, new_grid))
        return grid2grid(grid, values, new_grid, method, *args, **kwargs)
    monkeypatch.setattr(em.maps, 'grid2grid', counting)
    with em.optimize.SurveyJacobian(grids, model, SOURCES, freqs, rec, batch=2, model_grid=M, **KW) as sj:
        assert _handles(sj) == [(0, '<c16'), (1, '<c16')]
        assert sj._slot == {0: 0, 1: 0, 2: 2}
        assert len(volume) == 2                                     # open(): the model, once per distinct grid
        syn = sj.synthetic.copy()
        for _ in range(2):
            del volume[:]
            jv = sj.jvec(v, mapped=True)
            assert [(a is M, b is A or b is B) for a, b in volume] == [(True, True)] * 2 and volume[0][1] is not volume[1][1]
        del volume[:]
        sj.jtvec(w, mapped=True)
        assert volume == []
        part = sj.partial.copy()
        assert _handles(sj) == [(0, '<c16'), (1, '<c16')]
    with em.optimize.SurveyJacobian(A, model, SOURCES, [0.4], rec, batch=2, model_grid=M, **KW) as one:
        assert np.array_equal(syn[:, 2], one.synthetic[:, 0]) and np.array_equal(jv[:, 2], one.jvec(v, mapped=True)[:, 0])
        one.jtvec(w[:, 2:3], mapped=True)
        assert np.array_equal(part[2], one.partial[0]) and np.abs(part[2]).max() > 0
    assert not np.array_equal(syn[:, 0], syn[:, 2])


# ---- 4. a sequence that repeats one grid ---------------------------------------------------------------------------------------------
def _run(em, grid, model, M, rec, v, w, W, batch=2, then=None, freqs=FREQS):
    with em.optimize.SurveyJacobian(grid, model, SOURCES, freqs, rec, batch=batch, model_grid=M, **KW) as sj:
        if then is not None:
            before = sj.device_bytes
            sj.set_model(then)
            assert sj.device_bytes == before
        out = dict(syn=sj.synthetic.copy(), jv=sj.jvec(v, mapped=True), jt=sj.jtvec(w, mapped=True))
        out['partial'] = sj.partial.copy()
        out['hv'] = sj.gauss_newton(v, W, mapped=True)
        out['rows'] = sj.sensitivity_rows(len(freqs) - 1, receivers=[1], mapped=True)
        out['bytes'] = sj.device_bytes
        out['handles'] = len(list(sj._held))
    return out


def test_a_sequence_that_repeats_one_grid_is_the_single_mesh_call():
    import emg3d_amd as em
    M, A, _ = survey_grids(em)
    model = _models(em, M, 'Resistivity')
    rec = _rec()
    freqs = [1.5, -1.2]
    v, w, W = _vectors(M, 2, rec[0].size, 64, real=(1,))
    single = _run(em, A, model, M, rec, v, w, W, freqs=freqs)
    assert single['handles'] == 2 and np.abs(single['jt']).max() > 0 and np.abs(single['hv']).max() > 0
    for seq in ([A, A], [A, copy_of(em, A)]):
        got = _run(em, seq, model, M, rec, v, w, W, freqs=freqs)
        assert all(np.array_equal(got[k], single[k]) for k in single), [k for k in single if not np.array_equal(got[k], single[k])]


# ---- 5. set_model and batch ----------------------------------------------------------------------------------------------------------
def test_set_model_and_batch_bitwise():
    import emg3d_amd as em
    M, A, B = survey_grids(em)
    grids = [A, B, A]
    model, other = _models(em, M, 'Resistivity'), _models(em, M, 'Resistivity', seed=55)
    rec = _rec()
    v, w, W = _vectors(M, 3, rec[0].size, 65, real=(2,))
    one = _run(em, grids, model, M, rec, v, w, W, batch=1)
    three = _run(em, grids, model, M, rec, v, w, W, batch=3)
    assert np.abs(one['jt']).max() > 0 and np.abs(one['hv']).max() > 0 and one['handles'] == three['handles'] == 3
    results = [k for k in one if k != 'bytes']
    assert all(np.array_equal(three[k], one[k]) for k in results)
    moved = _run(em, grids, other, M, rec, v, w, W, batch=3, then=model)
    assert all(np.array_equal(moved[k], three[k]) for k in three)            # device_bytes too: nothing was created
    assert not np.array_equal(_run(em, grids, other, M, rec, v, w, W, batch=3)['syn'], three['syn'])


# ---- 6. solve_survey -------------------------------------------------------------------------------------------------------------------
def test_solve_survey_on_frequency_grids():
    import emg3d_amd as em
    M, A, B = survey_grids(em)
    grids = [A, B, A]
    model = _models(em, M, 'Resistivity')
    rec = _rec()
    resp, infos, efs = em.shard.solve_survey(grids, model, SOURCES, FREQS, rec, batch=2, return_fields=True, model_grid=M, **KW)
    assert resp.shape == (3, 3, rec[0].size) and resp.dtype == np.complex128 and np.abs(resp).min() > 0
    for j in range(3):
        on_j = model.interpolate2grid(M, grids[j])
        r1, i1, e1 = em.shard.solve_survey(grids[j], on_j, SOURCES, [FREQS[j]], rec, batch=2, return_fields=True, **KW)
        assert np.array_equal(resp[:, j], r1[:, 0]), j
        for i in range(3):
            assert all(infos[i][j][k] == i1[i][0][k] for k in INFO_KEYS), (i, j)
            e = efs[i][j]
            assert e.shape == (grids[j].nE,) and (e.vnEx, e.vnEy, e.vnEz) == (grids[j].vnEx, grids[j].vnEy, grids[j].vnEz)
            assert e.dtype == (np.float64 if FREQS[j] < 0 else np.complex128)
            assert np.array_equal(np.asarray(e), np.asarray(e1[i][0])) and np.abs(np.asarray(e)).max() > 0
    # a single mesh with a model grid: the model is regridded, nothing else changes
    r2, i2 = em.shard.solve_survey(B, model, SOURCES, [0.7], rec, batch=2, model_grid=M, **KW)
    assert np.array_equal(r2[:, 0], resp[:, 1]) and all(i2[i][0]['it_mg'] == infos[i][1]['it_mg'] for i in range(3))
