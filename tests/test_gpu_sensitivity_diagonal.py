"""GPU: the survey sensitivity diagonal diag(J^H W J) -- emg3d_mg_sens_acc_add (k_sens_acc) through the C ABI against the
longdouble host restatement, and optimize.SurveyJacobian.sensitivity_diagonal against the rows jtvec gives one datum at a time.

Tolerances (tests/test_sensitivity_diagonal_host.py): kernel level 4 x the float64-versus-longdouble deviation of the restatement
recorded on the CPU, end to end twice that; both relative to the max of the result."""
import numpy as np
import pytest

from test_sensitivity_diagonal_host import (NSYS, SHAPES, TOL_KERNEL, TOL_SURVEY, _deviation, kernel_case, row_identity_gap)

pytestmark = pytest.mark.gpu

OPTS = dict(cycle='F', semicoarsening=True, linerelaxation=True, verb=0)


def _handle(em, grid, smu0, nsys):
    from emg3d_amd import models
    from emg3d_amd.solver import DeviceMG
    model = em.Model(grid, np.ones(grid.nC), mapping='Conductivity')
    dev = DeviceMG.from_sigma_volume(grid, *models.sigma_volume(grid, model), smu0=smu0)
    if nsys > 1:
        dev.set_batch(nsys)
    return dev


def _upload(dev, case):
    """Forward fields with bvec_set into batched vector 0, adjoint fields with select + vec_set into the level-0 field array."""
    dev.bvec_alloc(1)
    for b in range(dev.nsys):
        dev.bvec_set(0, b, case['fwd'][b])
        dev.select(b)
        dev.vec_set(dev.EFIELD, case['adj'][b])


def _raw(dev, case, weights, split, fwd_bvec=0):
    a = complex(case['smu0'])
    w = np.ascontiguousarray(weights, dtype=np.float64)
    return dev._lib.emg3d_mg_sens_acc_add(dev._h, fwd_bvec, a.real, a.imag, case['use_fwd'].ctypes.data, case['use_adj'].ctypes.data,
                                          w.ctypes.data, int(split))


# ---- 1. the kernel through the C ABI --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsys", NSYS)
@pytest.mark.parametrize("real", [False, True], ids=["c128", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_sens_acc_add_vs_longdouble(shape, real, nsys):
    """Both forms against the longdouble restatement within TOL_KERNEL.  The systems that are masked out, and the active ones
    whose weights are all zero, hold NaN fields: they contribute exactly nothing or the result shows it.  _get leaves the
    accumulators alone, a second call adds the same terms again, the call is deterministic, and the errors are -2."""
    import emg3d_amd as em
    from emg3d_amd import maps
    case = kernel_case(shape, real, nsys)
    grid, W = case['grid'], case['W']
    args = (grid, case['fwd'], case['adj'], case['smu0'], case['W_eff'])
    want1 = maps.sensitivity_diagonal(*args, dtype=np.longdouble).ravel(order='F')
    want3 = [w.ravel(order='F') for w in maps.sensitivity_diagonal(*args, components=True, dtype=np.longdouble)]
    use = (case['use_fwd'], case['use_adj'])
    with _handle(em, grid, case['smu0'], nsys) as dev:
        assert dev.nsys == nsys
        _upload(dev, case)
        # an accumulator that was never reset, a bad vector
        assert _raw(dev, case, W, 0) == -2 and _raw(dev, case, W, 1) == -2
        dev.grad_acc_reset()
        dev.grad_acc3_reset()
        for bad in (-2, -1, 1, 9):
            assert _raw(dev, case, W, 0, fwd_bvec=bad) == -2
        with pytest.raises(ValueError):
            dev.sens_acc_add(dev.EFIELD, case['smu0'], *use, W)
        before = dev.device_bytes
        dev.sens_acc_add(0, case['smu0'], *use, W)
        grown = dev.device_bytes - before
        assert nsys * nsys * 8 <= grown < nsys * nsys * 8 + 256           # the weight table, once
        dev.sens_acc_add(0, case['smu0'], *use, W, split=True)
        assert dev.device_bytes - before == grown
        got1, got3 = dev.grad_acc_get(), dev.grad_acc3_get()
        e1, e3 = _deviation(got1, want1), [_deviation(g, w) for g, w in zip(got3, want3)]
        print(f"{shape} {'f64' if real else 'c128'} nsys {nsys}: one {e1:.2e}, split {e3[0]:.2e} {e3[1]:.2e} {e3[2]:.2e} "
              f"(tolerance {TOL_KERNEL:.1e})")
        assert np.isfinite(got1).all() and got1.min() >= 0 and got1.max() > 0
        assert e1 <= TOL_KERNEL and all(e <= TOL_KERNEL for e in e3)
        # the _get calls leave the accumulators unchanged
        assert np.array_equal(dev.grad_acc_get(), got1)
        assert all(np.array_equal(a, b) for a, b in zip(dev.grad_acc3_get(), got3))
        # a non-finite weight, a pair without any weight, no system used: the error resp. nothing added
        for bad in (np.nan, np.inf, -np.inf):
            Wb = W.copy()
            Wb[-1, -1] = bad
            assert _raw(dev, case, Wb, 0) == -2 and _raw(dev, case, Wb, 1) == -2
            with pytest.raises(ValueError):
                dev.sens_acc_add(0, case['smu0'], *use, Wb)
        dev.sens_acc_add(0, case['smu0'], *use, np.zeros_like(W))
        dev.sens_acc_add(0, case['smu0'], *use, np.zeros_like(W), split=True)
        none = np.zeros(nsys, dtype=np.int32)
        dev.sens_acc_add(0, case['smu0'], none, case['use_adj'], W)
        dev.sens_acc_add(0, case['smu0'], case['use_fwd'], none, W, split=True)
        with pytest.raises(ValueError):
            dev.sens_acc_add(0, case['smu0'], case['use_fwd'][:-1], case['use_adj'], W)
        with pytest.raises(ValueError):
            dev.sens_acc_add(0, case['smu0'], *use, W[:, :-1] if nsys > 1 else np.ones((2, 2)))
        assert np.array_equal(dev.grad_acc_get(), got1)
        assert all(np.array_equal(a, b) for a, b in zip(dev.grad_acc3_get(), got3))
        # two calls accumulate
        dev.sens_acc_add(0, case['smu0'], *use, W)
        dev.sens_acc_add(0, case['smu0'], *use, W, split=True)
        two1, two3 = dev.grad_acc_get(), dev.grad_acc3_get()
        assert _deviation(two1, 2 * want1) <= TOL_KERNEL
        assert all(_deviation(g, 2 * w) <= TOL_KERNEL for g, w in zip(two3, want3))
        # deterministic
        dev.grad_acc_reset()
        dev.grad_acc3_reset()
        assert np.array_equal(dev.grad_acc_get(), np.zeros(grid.nC))
        for _ in range(2):
            dev.sens_acc_add(0, case['smu0'], *use, W)
            dev.sens_acc_add(0, case['smu0'], *use, W, split=True)
        assert np.array_equal(dev.grad_acc_get(), two1)
        assert all(np.array_equal(a, b) for a, b in zip(dev.grad_acc3_get(), two3))


@pytest.mark.parametrize("real", [False, True], ids=["c128", "f64"])
def test_row_is_the_transpose_of_the_jvec_source(real):
    """The identity of tests/test_sensitivity_diagonal_host.py with C(v) from the device's maps.cellaverages2edges."""
    from emg3d_amd import maps

    def cells2edges(v3, vol):
        nx, ny, nz = vol.shape
        outs = [np.zeros(s, order='F') for s in ((nx, ny + 1, nz + 1), (nx + 1, ny, nz + 1), (nx + 1, ny + 1, nz))]
        maps.cellaverages2edges(*(np.asfortranarray(v) for v in v3), np.asfortranarray(vol), *outs)
        return outs
    for shape in SHAPES[:2]:
        case = kernel_case(shape, real, 3)
        v = np.random.default_rng(3).standard_normal(shape)
        gap = row_identity_gap(case, v, cells2edges)
        print(f"transpose identity {shape} {'f64' if real else 'c128'}: {gap:.2e}")
        assert gap < 1e-13


# ---- 2. end to end ----------------------------------------------------------------------------------------------------------
SOURCES = [[-40., 20., -30., 25., 5.], [60., -35., 15., -50., 20.], [10., 45., 40., 80., -30.]]
FREQS = [1.0, -2.0]


def _survey(em):
    h = [np.array([95., 70., 52., 40., 44., 57., 76., 104.]) * f for f in (1.0, 0.9, 1.1)]
    grid = em.TensorMesh(h, origin=tuple(-x.sum() / 2 for x in h))
    rec = (np.array([-55., 30., 5., 48.]), np.array([12., -44., 50., 7.]), np.array([-20., 35., -8., 41.]),
           np.array([0., 40., -60., 110.]), np.array([0., 15., -25., 5.]))
    rng = np.random.default_rng(50)
    sig = 10 ** rng.uniform(-1, 0.5, grid.nC)
    return grid, rec, rng, sig


def _weights(rng, keep=None):
    """(n_src, n_freq, n_rec) weights; ``keep``: only that many of them are not zero (the jtvec loop costs two solves each)."""
    W = rng.uniform(0.5, 2.0, (3, 2, 4))
    if keep is not None:
        mask = np.zeros(W.size, dtype=bool)
        mask[rng.permutation(W.size)[:keep]] = True
        W = W * mask.reshape(W.shape)
    return W


def _rows_diagonal(sj, W, components=False, mapped=False):
    """sum_d W_d (jtvec(e_d)^2 + jtvec(i e_d)^2) on the open SurveyJacobian, one datum at a time -> (result, jtvec calls)."""
    shape = (sj.n_src, sj.n_freq, sj.n_rec)
    vnC = tuple(int(n) for n in sj.grid.vnC)
    out = [np.zeros(vnC) for _ in range(3 if components else 1)]
    calls = 0
    for j in range(sj.n_freq):
        for i in range(sj.n_src):
            for r in range(sj.n_rec):
                if not W[i, j, r] > 0:
                    continue
                for unit in ((1.0,) if sj.freqs[j] < 0 else (1.0, 1j)):
                    w = np.zeros(shape, dtype=np.complex128)
                    w[i, j, r] = unit
                    row = sj.jtvec(w, components=components, mapped=mapped)
                    calls += 1
                    out = [o + W[i, j, r] * g * g for o, g in zip(out, row if components else (row,))]
    return (tuple(out) if components else out[0]), calls


def test_diagonal_equals_the_rows_of_jtvec():
    """8 x 8 x 8 stretched, 3 sources x (1 Hz, s = 2) x 4 receivers, batch = 2 (receiver chunks of 2 + 2, source chunks of 2 + 1),
    every datum weighted: 24 data, 36 jtvec calls (two for each of the 12 frequency-domain data, one for each of the 12
    Laplace-domain data, which have no imaginary part).  The receiver-field solves
    are the solves jtvec(e_d) runs, so both sides start from the same fields: TOL_SURVEY."""
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = em.Model(grid, sig, mapping='Conductivity')
    W = _weights(rng)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, tol=1e-8, **OPTS) as sj:
        before = sj.device_bytes
        got = sj.sensitivity_diagonal(W)
        grown = sj.device_bytes - before
        info, partial = sj.sensitivity_info, sj.sensitivity_partial.copy()
        assert np.array_equal(sj.sensitivity_diagonal(W), got) and sj.device_bytes - before == grown
        want, calls = _rows_diagonal(sj, W)
        unit = sj.sensitivity_diagonal()
    assert calls == 36
    # two handles (one per dtype): an accumulator and a 2 x 2 weight table each
    assert 2 * grid.nC * 8 <= grown < 2 * (grid.nC * 8 + 256 + 256)
    assert got.shape == tuple(grid.vnC) and got.dtype == np.float64 and got.flags.f_contiguous
    assert got.min() >= 0 and got.max() > 0
    assert partial.shape == (2,) + tuple(grid.vnC) and np.array_equal((0 + partial[0]) + partial[1], got)
    assert all(len(row) == 4 and all(x is not None and x['exit'] == 0 for x in row) for row in info) and len(info) == 2
    err = _deviation(got, want)
    print(f"diagonal vs jtvec rows: {err:.2e} (tolerance {TOL_SURVEY:.1e})")
    assert err <= TOL_SURVEY
    assert unit.max() > 0 and not np.array_equal(unit, got)


def test_components_and_mapped_on_a_triaxial_model():
    """Tri-axial 'LgConductivity' model: components=True, and with mapped=True the chain factor squared, against the rows."""
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = em.Model(grid, np.log10(sig), np.log10(1.5 * sig), np.log10(0.6 * sig), mapping='LgConductivity')
    W = _weights(rng, keep=5)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, tol=1e-8, **OPTS) as sj:
        got3 = sj.sensitivity_diagonal(W, components=True)
        assert sj.sensitivity_partial.shape == (3, 2) + tuple(grid.vnC)
        one = sj.sensitivity_diagonal(W)
        got3m = sj.sensitivity_diagonal(W, components=True, mapped=True)
        want3, _ = _rows_diagonal(sj, W, components=True)
        want1, _ = _rows_diagonal(sj, W)
        want3m, _ = _rows_diagonal(sj, W, components=True, mapped=True)
        with pytest.raises(NotImplementedError):
            sj.sensitivity_diagonal(W, mapped=True)
        with pytest.raises(TypeError):
            sj.sensitivity_diagonal(W, mapped=1)
    errs = [_deviation(g, w) for g, w in zip(got3 + got3m + (one,), want3 + want3m + (want1,))]
    print("tri-axial: x y z " + " ".join(f"{e:.2e}" for e in errs[:3]) + ", mapped " + " ".join(f"{e:.2e}" for e in errs[3:6]) +
          f", one output {errs[6]:.2e} (tolerance {TOL_SURVEY:.1e})")
    assert all(g.max() > 0 for g in got3 + got3m)
    assert all(e <= TOL_SURVEY for e in errs)


@pytest.mark.parametrize("kind", ["magnetic", "reference-cubic", "linear"])
def test_other_receivers_and_adjoint_rules(kind):
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = em.Model(grid, sig, mapping='Conductivity')
    kw = dict(magnetic=dict(electric=False), linear=dict(receiver_interpolation='linear'),
              **{'reference-cubic': dict(adjoint='reference', receiver_interpolation='cubic')})[kind]
    W = _weights(rng, keep=5)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, tol=1e-8, **kw, **OPTS) as sj:
        got = sj.sensitivity_diagonal(W)
        want, _ = _rows_diagonal(sj, W)
    err = _deviation(got, want)
    print(f"{kind}: {err:.2e} (tolerance {TOL_SURVEY:.1e})")
    assert got.max() > 0 and err <= TOL_SURVEY


def test_batch_sizes_set_model_and_skipped_receivers():
    """batch = 1 against batch = 8 (the handle's width 1 resp. 3: other chunks, another order of the same non-negative terms)
    within TOL_SURVEY; after set_model the result is that of a new SurveyJacobian bit for bit, with nothing allocated; a receiver
    whose weights are NaN for every source at one frequency is not solved for, and the rows still agree."""
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = em.Model(grid, sig, mapping='Conductivity')
    model2 = em.Model(grid, sig * 10 ** rng.uniform(-0.2, 0.2, grid.nC), mapping='Conductivity')
    W = _weights(rng)
    Wn = _weights(rng, keep=8)
    Wn[:, 1, 2] = np.nan                # receiver 2 has no datum at the second entry of `freqs`
    Wn[0, 0, 2] = 1.25                  # ... and one at the first
    Wn[:, 0, 0] = 0.0                   # zero for every source counts as no datum too
    kw = dict(tol=1e-8, **OPTS)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=1, **kw) as sj:
        one = sj.sensitivity_diagonal(W)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=8, **kw) as sj:
        eight = sj.sensitivity_diagonal(W)
        err = _deviation(one, eight)
        print(f"batch 1 vs batch 8: {err:.2e} (tolerance {TOL_SURVEY:.1e})")
        assert err <= TOL_SURVEY
        before = sj.device_bytes
        sj.set_model(model2)
        assert sj.sensitivity_info is None and sj.sensitivity_partial is None
        after = sj.sensitivity_diagonal(W)
        assert sj.device_bytes == before and not np.array_equal(after, eight)
        got = sj.sensitivity_diagonal(Wn)
        info = sj.sensitivity_info
        want, _ = _rows_diagonal(sj, np.nan_to_num(Wn))
    with em.optimize.SurveyJacobian(grid, model2, SOURCES, FREQS, rec, batch=8, **kw) as sj:
        assert np.array_equal(sj.sensitivity_diagonal(W), after)
    solved = [[x is not None for x in row] for row in info]
    wanted = [[bool(np.any(np.nan_to_num(Wn[:, j, r]) != 0)) for r in range(4)] for j in range(2)]
    assert solved == wanted and not solved[1][2] and not solved[0][0] and solved[0][2]
    assert sum(map(sum, solved)) == sum(map(sum, wanted))
    err = _deviation(got, want)
    print(f"skipped receivers: {err:.2e} (tolerance {TOL_SURVEY:.1e})")
    assert err <= TOL_SURVEY


def test_refusals():
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = em.Model(grid, sig, mapping='Conductivity')
    kw = dict(tol=1e-6, **OPTS)
    with em.optimize.SurveyJacobian(grid, model, SOURCES[:1], FREQS[:1], rec, batch=1, **kw) as sj:
        for bad in (-np.ones((1, 1, 4)), np.full((1, 1, 4), np.inf), np.ones((1, 1, 4)) * 1j, np.ones((2, 1, 4))):
            with pytest.raises((ValueError, TypeError)):
                sj.sensitivity_diagonal(bad)
        W = np.ones((1, 1, 4))
        W[0, 0, 1] = -0.5
        with pytest.raises(ValueError, match="negative"):
            sj.sensitivity_diagonal(W)
    with pytest.raises(RuntimeError):
        sj.sensitivity_diagonal()
    coarse = em.TensorMesh([np.array([h[0:2].sum(), h[2:4].sum(), h[4:6].sum(), h[6:8].sum()]) for h in grid.h], origin=grid.origin)
    cmodel = em.Model(coarse, np.full(coarse.nC, 1.0), mapping='Conductivity')
    with em.optimize.SurveyJacobian(grid, cmodel, SOURCES[:1], FREQS[:1], rec, batch=1, model_grid=coarse, **kw) as sj:
        with pytest.raises(ValueError, match="model grid"):
            sj.sensitivity_diagonal()
        with pytest.raises(ValueError, match="model grid"):
            sj.sensitivity_diagonal(mapped=True)
