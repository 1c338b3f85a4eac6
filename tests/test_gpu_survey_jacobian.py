"""GPU: optimize.SurveyJacobian -- J v, J^T w and the Gauss-Newton product over the (source, frequency) pairs of a survey.

The three batched device pieces bit for bit against their single-system twins (jvec_source_b / jvec_source, grad_acc3 /
gradient(components=True), set_receiver_adjoint_b / set_receiver_adjoint), the class bit for bit against optimize.Jacobian per
pair and against itself for other batch sizes, against the reference (tests/golden/survey_jacobian.npz: the reference's own
functions composed per pair by tests/golden/make_survey_jacobian_golden.py), and the adjoint / symmetry identities on a
48 x 40 x 32 model against the reference-side adjoint gap of the fixture."""
import numpy as np
import pytest

from conftest import load_golden, relerr
from test_gpu_jacobian import INFO_KEYS, OPTS, _boundary_edges, _model48

pytestmark = pytest.mark.gpu


def _grid12(em):
    g = load_golden("survey_jacobian.npz")
    return g, em.TensorMesh([g['hx'], g['hy'], g['hz']], origin=g['origin'])


def _model(em, g, grid, tag):
    return em.Model(grid, g[f'{tag}_sig_x'], g[f'{tag}_sig_y'], g[f'{tag}_sig_z'], mapping='Conductivity')


def _handle(em, grid, model, freq, nsys):
    from emg3d_amd import models
    from emg3d_amd.solver import DeviceMG
    smu0 = em.fields.FrequencySpec(freq).smu0
    dev = DeviceMG.from_sigma_volume(grid, *models.sigma_volume(grid, model), smu0=smu0)
    if nsys > 1:
        dev.set_batch(nsys)
    return dev, smu0


def _random_fields(rng, n, nE, real):
    return [rng.standard_normal(nE) if real else rng.standard_normal(nE) + 1j * rng.standard_normal(nE) for _ in range(n)]


# ---- 1. the device pieces -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("freq", [1.5, -1.5], ids=["c128", "f64"])
def test_jvec_source_b_equals_jvec_source_per_system(freq):
    """nsys = 3, use = [1, 0, 1]: slices 0 and 2 equal jvec_source on the selected system bit for bit, slice 1 keeps its
    sentinel, PEC edges are exact zeros, a second call repeats, v_z only leaves the x- and y-sources zero, and the forward
    fields must be a saved batched vector."""
    import emg3d_amd as em
    g, grid = _grid12(em)
    model = _model(em, g, grid, 'tri')
    rng = np.random.default_rng(31)
    nsys, nE = 3, grid.nE
    fwd = _random_fields(rng, nsys, nE, freq < 0)
    v3 = [np.asfortranarray(rng.standard_normal(grid.vnC)) for _ in range(3)]
    sentinel = np.full(nE, 7.25) if freq < 0 else np.full(nE, 7.25 - 3.5j)
    use = np.array([1, 0, 1], dtype=np.int32)
    bnd = _boundary_edges(grid)
    nxy = bnd.size - (grid.vnC[0] + 1) * (grid.vnC[1] + 1) * grid.vnC[2]
    dev, smu0 = _handle(em, grid, model, freq, nsys)
    with dev:
        dev.vec_alloc(1)
        dev.bvec_alloc(1)
        for b in range(nsys):
            dev.bvec_set(0, b, fwd[b])
        for case, vs in (('xyz', tuple(v3)), ('same', (v3[0], v3[0], v3[0])), ('vz', (None, None, v3[2]))):
            want = []
            for b in range(nsys):
                dev.select(b)
                dev.vec_set(0, fwd[b])
                dev.jvec_source(0, smu0, *vs)
                want.append(dev.vec_get(dev.SFIELD))
                dev.vec_set(dev.SFIELD, sentinel)
            dev.jvec_source_b(0, smu0, *vs, use)
            got = [dev.bvec_get(dev.SFIELD, b) for b in range(nsys)]
            for b in (0, 2):
                assert np.abs(want[b]).max() > 0, case
                assert np.array_equal(got[b], want[b]), (case, b)
                assert np.all(got[b][bnd] == 0)
            assert np.array_equal(got[1], sentinel), case
            if case == 'vz':
                assert np.all(got[0][:nxy] == 0) and np.all(got[2][:nxy] == 0) and np.abs(got[0][nxy:]).max() > 0
            dev.jvec_source_b(0, smu0, *vs, use)
            assert all(np.array_equal(dev.bvec_get(dev.SFIELD, b), got[b]) for b in range(nsys)), case
        # no system used: nothing is written
        dev.jvec_source_b(0, smu0, *v3, np.zeros(nsys, dtype=np.int32))
        assert all(np.array_equal(dev.bvec_get(dev.SFIELD, b), got[b]) for b in range(nsys))
        a = complex(smu0)
        ptrs = [x.ctypes.data for x in v3]
        for bad in (-2, -1, 1, 9):
            assert dev._lib.emg3d_mg_jvec_source_b(dev._h, bad, a.real, a.imag, *ptrs, use.ctypes.data) == -2
        with pytest.raises(ValueError):
            dev.jvec_source_b(dev.EFIELD, smu0, *v3, use)
        with pytest.raises(ValueError):
            dev.jvec_source_b(0, smu0, *v3, use[:2])
        assert all(np.array_equal(dev.bvec_get(dev.SFIELD, b), got[b]) for b in range(nsys))


def test_widest_batch_with_the_highest_system_used():
    """nsys = 64, the widest batch set_batch takes, use = systems 0, 31 and 63 (bit 63 of the mask), on the 8 x 5 x 6 grid:
    jvec_source_b per used slice equals jvec_source bit for bit -- PEC edges included, which take a path of their own --, the
    61 other slices keep their sentinel, and grad_acc3 / grad_acc equal the sequential sums of the three systems' gradients."""
    import emg3d_amd as em
    f = load_golden("receiver_adjoint.npz")
    grid = em.TensorMesh([f['B_hx'], f['B_hy'], f['B_hz']], origin=f['B_origin'])
    assert tuple(grid.vnC) == (8, 5, 6)
    rng = np.random.default_rng(37)
    model = em.Model(grid, 10 ** rng.uniform(-1, 0.5, grid.nC), mapping='Conductivity')
    nsys, nE, freq = 64, grid.nE, 1.5
    used = (0, 31, 63)
    use = np.zeros(nsys, dtype=np.int32)
    use[list(used)] = 1
    fwd = dict(zip(used, _random_fields(rng, 3, nE, False)))
    bwd = dict(zip(used, _random_fields(rng, 3, nE, False)))
    v3 = [np.asfortranarray(rng.standard_normal(grid.vnC)) for _ in range(3)]
    sentinel = np.full(nE, 7.25 - 3.5j)
    bnd = _boundary_edges(grid)
    dev, smu0 = _handle(em, grid, model, freq, nsys)
    with dev:
        assert dev.nsys == nsys
        dev.vec_alloc(1)
        dev.bvec_alloc(1)
        want, g3, g1 = {}, {}, {}
        for b in range(nsys):
            dev.select(b)
            if b in used:
                dev.bvec_set(0, b, fwd[b])
                dev.vec_set(0, fwd[b])
                dev.jvec_source(0, smu0, *v3)
                want[b] = dev.vec_get(dev.SFIELD)
                dev.set_efield(em.Field(grid, bwd[b].copy(), freq=freq))
                g3[b] = dev.gradient(0, smu0, components=True)
                g1[b] = dev.gradient(0, smu0)
            dev.vec_set(dev.SFIELD, sentinel)
        dev.jvec_source_b(0, smu0, *v3, use)
        for b in range(nsys):
            got = dev.bvec_get(dev.SFIELD, b)
            if b in used:
                assert np.array_equal(got, want[b]), b
                assert np.all(got[bnd] == 0) and np.abs(got).max() > 0
            else:
                assert np.array_equal(got, sentinel), b
        dev.grad_acc3_reset()
        dev.grad_acc3_add(0, smu0, use)
        dev.grad_acc_reset()
        dev.grad_acc_add(0, smu0, use)
        acc3, acc1 = [np.zeros(grid.nC) for _ in range(3)], np.zeros(grid.nC)
        for b in used:
            acc3 = [a + x for a, x in zip(acc3, g3[b])]
            acc1 = acc1 + g1[b]
        assert all(np.array_equal(a, w) for a, w in zip(dev.grad_acc3_get(), acc3))
        assert np.array_equal(dev.grad_acc_get(), acc1) and np.abs(acc1).max() > 0


@pytest.mark.parametrize("freq, nsys", [(1.5, 3), (-1.5, 3), (1.5, 1)], ids=["c128-3", "f64-3", "c128-1"])
def test_grad_acc3_is_the_sequential_sum_of_gradient3(freq, nsys):
    """Each of the three accumulators == the sequential sum of gradient(components=True) over the used systems, bit for bit; two
    adds chain; the accumulators are the handle's own (counted by device_bytes) and independent of the single accumulator."""
    import emg3d_amd as em
    g, grid = _grid12(em)
    model = _model(em, g, grid, 'tri')
    rng = np.random.default_rng(32)
    fwd = _random_fields(rng, nsys, grid.nE, freq < 0)
    bwd = _random_fields(rng, nsys, grid.nE, freq < 0)
    use = np.array([1, 0, 1][:nsys], dtype=np.int32)
    dev, smu0 = _handle(em, grid, model, freq, nsys)
    with dev:
        assert dev.nsys == nsys
        dev.vec_alloc(1)
        dev.bvec_alloc(1)
        g3, g1 = [], []
        for b in range(nsys):
            dev.select(b)
            dev.set_efield(em.Field(grid, bwd[b].copy(), freq=freq))
            dev.bvec_set(0, b, fwd[b])
            dev.vec_set(0, fwd[b])
            g3.append(dev.gradient(0, smu0, components=True))
            g1.append(dev.gradient(0, smu0))
        assert all(np.abs(x).max() > 0 for t in g3 for x in t)
        before = dev.device_bytes
        dev.grad_acc3_reset()
        grown = dev.device_bytes - before
        assert 3 * grid.nC * 8 <= grown < 3 * grid.nC * 8 + 256
        assert all(np.array_equal(a, np.zeros(grid.nC)) for a in dev.grad_acc3_get())
        want = [np.zeros(grid.nC) for _ in range(3)]
        for rounds in range(2):              # the second call adds the same values once more, in the same order
            for b in range(nsys):
                if use[b]:
                    want = [w + x for w, x in zip(want, g3[b])]
            dev.grad_acc3_add(0, smu0, use)
            got = dev.grad_acc3_get()
            assert all(np.array_equal(a, w) for a, w in zip(got, want)), rounds
        # independent of the single accumulator, which still equals the sum of the one-output gradients
        dev.grad_acc_reset()
        dev.grad_acc_add(0, smu0, use)
        one = np.zeros(grid.nC)
        for b in range(nsys):
            if use[b]:
                one = one + g1[b]
        assert np.array_equal(dev.grad_acc_get(), one)
        assert all(np.array_equal(a, w) for a, w in zip(dev.grad_acc3_get(), want))
        dev.grad_acc3_add(0, smu0, np.zeros(nsys, dtype=np.int32))
        assert all(np.array_equal(a, w) for a, w in zip(dev.grad_acc3_get(), want))
        a = complex(smu0)
        for bad in (-2, -1, 1, 7):
            assert dev._lib.emg3d_mg_grad_acc3_add(dev._h, bad, a.real, a.imag, use.ctypes.data) == -2
        with pytest.raises(ValueError):
            dev.grad_acc3_add(dev.EFIELD, smu0, use)
        dev.grad_acc3_reset()
        assert all(np.array_equal(a, np.zeros(grid.nC)) for a in dev.grad_acc3_get())
        assert np.array_equal(dev.grad_acc_get(), one)


ADJ_CASES = (('linear', False), ('cubic', False), ('linear', True), ('cubic', True))


@pytest.mark.parametrize('sfx', ['c', 'r'])
@pytest.mark.parametrize('tag', ['A', 'B'])
def test_set_receiver_adjoint_b_equals_the_per_system_call(tag, sfx):
    """Grids A (12 x 10 x 8) and B (8 x 5 x 6: a NaN receiver, a component that falls back to linear) of receiver_adjoint.npz,
    linear and cubic, electric and magnetic, nsys = 4 with use = [1, 1, 0, 1]: every used slice equals set_receiver_adjoint on
    the selected system with that row bit for bit, the all-zero row gives an all-zero slice, the unused slice keeps its
    sentinel, accumulate doubles.  The single-system call runs the same table build (RcvAdjPlan) with one row, so this checks the
    batching -- slice addressing, row offsets, the untouched slice; the table build itself is checked against the reference's
    dense operators by tests/test_gpu_receiver_adjoint.py::test_adjoint_kernels_vs_reference."""
    import emg3d_amd as em
    f = load_golden("receiver_adjoint.npz")
    grid = em.TensorMesh([f[f'{tag}_hx'], f[f'{tag}_hy'], f[f'{tag}_hz']], origin=f[f'{tag}_origin'])
    rec = tuple(f[f'{tag}_rec'])
    n = rec[0].size
    freq = float(f[f'{tag}_freq']) * (1 if sfx == 'c' else -1)
    rng = np.random.default_rng(33)
    nsys = 4
    w = np.stack([f[f'w_{sfx}'][:n], np.zeros(n), f[f'w_{sfx}'][4:4 + n], rng.standard_normal(n)]).astype(
        np.complex128 if sfx == 'c' else np.float64)
    if sfx == 'c':
        w[3] = w[3] + 1j * rng.standard_normal(n)
    use = np.array([1, 1, 0, 1], dtype=np.int32)
    sentinel = np.full(grid.nE, -2.5, dtype=w.dtype)
    model = em.Model(grid, np.ones(grid.nC), mapping='Conductivity')
    bnd = _boundary_edges(grid)
    dev, smu0 = _handle(em, grid, model, freq, nsys)
    with dev:
        for method, magnetic in ADJ_CASES:
            kw = dict(method=method, magnetic=magnetic, smu0=smu0 if magnetic else None)
            want = []
            for b in range(nsys):
                dev.select(b)
                dev.set_receiver_adjoint(rec, w[b], **kw)
                want.append(dev.vec_get(dev.SFIELD))
                dev.vec_set(dev.SFIELD, sentinel)
            dev.set_receiver_adjoint_b(rec, w, use, **kw)
            got = [dev.bvec_get(dev.SFIELD, b) for b in range(nsys)]
            for b in (0, 1, 3):
                assert np.array_equal(got[b], want[b]), (method, magnetic, b)
                assert np.all(got[b][bnd] == 0)
            assert np.abs(got[0]).max() > 0 and np.abs(got[3]).max() > 0
            assert np.all(got[1] == 0)
            assert np.array_equal(got[2], sentinel)
            dev.set_receiver_adjoint_b(rec, w, use, accumulate=True, **kw)
            for b in (0, 1, 3):
                assert np.array_equal(dev.bvec_get(dev.SFIELD, b), 2 * want[b]), (method, magnetic, b)
            assert np.array_equal(dev.bvec_get(dev.SFIELD, 2), sentinel)
        with pytest.raises(ValueError):
            dev.set_receiver_adjoint_b(rec, w, use[:3])


# ---- 2. against the single-pair class -------------------------------------------------------------------------------------
def _same_info(a, b):
    assert (a is None) == (b is None)
    if a is not None:
        for key in INFO_KEYS:
            assert a[key] == b[key], (key, a[key], b[key])
        assert np.array_equal(a['error_at_cycle'], b['error_at_cycle'])


@pytest.mark.parametrize('kind', ['linear', 'cubic-exact', 'cubic-reference'])
def test_survey_products_equal_the_single_pair_class(kind):
    """12 x 10 x 8, tri-axial: data and J v per pair, J^T w (one output and per direction) as the sequential sums of
    Jacobian.jtvec, and gauss_newton == jtvec(W * jvec(v)) -- all bit for bit."""
    import emg3d_amd as em
    g, grid = _grid12(em)
    model = _model(em, g, grid, 'tri')
    rec = tuple(g['rec'])
    sources, freqs = g['sources'], [float(x) for x in g['freqs']]
    ns, nf = len(sources), len(freqs)
    vnC = tuple(int(n) for n in grid.vnC)
    v = g['tri_v'].reshape(vnC, order='F')
    w = g['tri_w'].copy()
    w[1, 0, 2] = np.nan                     # a missing datum counts as zero
    ropts = {'linear': dict(receiver_interpolation='linear'), 'cubic-exact': dict(receiver_interpolation='cubic', adjoint='exact'),
             'cubic-reference': dict(receiver_interpolation='cubic', adjoint='reference')}[kind]
    kw = dict(OPTS, tol=1e-8, ordering='lex', **ropts)
    rng = np.random.default_rng(34)
    W = rng.uniform(0.5, 2.0, (ns, nf, rec[0].size))
    with em.optimize.SurveyJacobian(grid, model, sources, freqs, rec, batch=2, **kw) as sj:
        syn = sj.synthetic.copy()
        finfo = sj.forward_info
        jv = sj.jvec(v)
        jv_info = sj.info
        jvz = sj.jvec((None, None, v))
        jt = sj.jtvec(w)
        jt_info, partial = sj.info, sj.partial.copy()
        jt3 = sj.jtvec(w, components=True)
        partial3 = sj.partial.copy()
        two_step = sj.jtvec(W * jv)
        two_step3 = sj.jtvec(W * jv, components=True)
        hv = sj.gauss_newton(v, W)
        hv3 = sj.gauss_newton(v, W, components=True)
        assert sj.device_bytes > 0
    assert jv.shape == (ns, nf, rec[0].size) and jt.shape == vnC and jt.dtype == np.float64 and jt.flags.f_contiguous
    assert partial.shape == (nf,) + vnC and partial3.shape == (3, nf) + vnC
    want, want3 = np.zeros(vnC, order='F'), [np.zeros(vnC, order='F') for _ in range(3)]
    for j in range(nf):
        gf, gf3 = np.zeros(vnC, order='F'), [np.zeros(vnC, order='F') for _ in range(3)]
        for i in range(ns):
            with em.optimize.Jacobian(grid, model, sources[i], freqs[j], rec, **kw) as jac:
                assert np.array_equal(syn[i, j], jac.synthetic)
                _same_info(finfo[i][j], jac.forward_info)
                assert np.array_equal(jv[i, j], jac.jvec(v))
                _same_info(jv_info[i][j], jac.info)
                assert np.array_equal(jvz[i, j], jac.jvec((None, None, v)))
                one = jac.jtvec(w[i, j])
                _same_info(jt_info[i][j], jac.info)
                gf = gf + one
                gf3 = [a + b for a, b in zip(gf3, jac.jtvec(w[i, j], components=True))]
        assert np.array_equal(-partial[j], gf)
        for c in range(3):
            assert np.array_equal(-partial3[c, j], gf3[c])
        want = want + gf
        want3 = [a + b for a, b in zip(want3, gf3)]
    assert np.abs(want).max() > 0
    assert np.array_equal(jt, want)
    for c in range(3):
        assert jt3[c].shape == vnC and np.array_equal(jt3[c], want3[c])
    assert np.array_equal(hv, two_step) and np.abs(hv).max() > 0
    for c in range(3):
        assert np.array_equal(hv3[c], two_step3[c])


# ---- 3. independence of the batch size -----------------------------------------------------------------------------------
SOURCES = [[-100., 30., 20., 25., 5.], [140., -60., -25., -50., 20.], [20., 100., -40., 80., -30.]]


def _run_survey(em, grid, model, rec, freqs, v, w, W, batch, **kw):
    with em.optimize.SurveyJacobian(grid, model, SOURCES, freqs, rec, batch=batch, **kw) as sj:
        out = dict(syn=sj.synthetic.copy(), finfo=sj.forward_info)
        out['jv'] = sj.jvec(v); out['jv_info'] = sj.info
        out['jt'] = sj.jtvec(w); out['jt_info'] = sj.info; out['partial'] = sj.partial.copy()
        out['jt3'] = np.stack(sj.jtvec(w, components=True)); out['partial3'] = sj.partial.copy()
        out['hv'] = sj.gauss_newton(v, W); out['hv_info'] = sj.info; out['hv_jinfo'] = sj.jvec_info
    return out


def _same_run(a, b):
    for key in ('syn', 'jv', 'jt', 'partial', 'jt3', 'partial3', 'hv'):
        assert np.array_equal(a[key], b[key]), key
    for key in ('finfo', 'jv_info', 'jt_info', 'hv_info', 'hv_jinfo'):
        for ra, rb in zip(a[key], b[key]):
            for da, db in zip(ra, rb):
                _same_info(da, db)


@pytest.mark.parametrize('electric', [True, False], ids=['electric', 'magnetic'])
def test_batch_invariance_bitwise(electric):
    """3 sources x (one Laplace-domain value, one frequency) on the 12 x 10 x 8 grid with batch = 1, 2, 3 (chunks of 1, of 2 + 1,
    of 3): every output, the per-frequency sums and every solve's cycle count and norms are identical; the pair with an
    all-zero row of w -- the middle system of the chunk of three -- is skipped (info None); a second SurveyJacobian, opened after
    the first was closed, reproduces it."""
    import emg3d_amd as em
    g, grid = _grid12(em)
    model = _model(em, g, grid, 'tri')
    rec = tuple(g['rec'])
    freqs = [-1.2, 1.5]
    vnC = tuple(int(n) for n in grid.vnC)
    v = g['tri_v'].reshape(vnC, order='F')
    rng = np.random.default_rng(35)
    shape = (3, 2, rec[0].size)
    w = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    w[:, 0] = w[:, 0].real                  # Laplace domain: real data
    w[1, 1, :] = 0                          # a pair without data
    w[2, 0, 3] = np.nan
    W = rng.uniform(0.5, 2.0, shape)
    W[0, 1, 1] = np.nan                     # "no datum"
    kw = dict(OPTS, tol=1e-6, electric=electric)
    one = _run_survey(em, grid, model, rec, freqs, v, w, W, 1, **kw)
    assert one['syn'].dtype == np.complex128 and np.all(one['syn'][:, 0].imag == 0) and np.isfinite(one['syn']).all()
    assert one['jt_info'][1][1] is None and one['jt_info'][0][1] is not None and one['jt_info'][1][0] is not None
    assert all(x is not None for row in one['hv_info'] for x in row)
    assert np.abs(one['jt']).max() > 0 and np.abs(one['partial'][0]).max() > 0 and np.abs(one['partial'][1]).max() > 0
    assert relerr(one['jt'], one['jt3'].sum(axis=0)) < 1e-12
    for batch in (2, 3):
        _same_run(_run_survey(em, grid, model, rec, freqs, v, w, W, batch, **kw), one)
    _same_run(_run_survey(em, grid, model, rec, freqs, v, w, W, 1, **kw), one)


def test_frequency_shards_combine():
    """sj.partial of two frequency shards goes through shard.combine_survey_gradient unchanged: -grad == jtvec of all."""
    import emg3d_amd as em
    g, grid = _grid12(em)
    model = _model(em, g, grid, 'iso')
    rec = tuple(g['rec'])
    freqs = [1.5, -1.2, 0.7]
    rng = np.random.default_rng(36)
    w = rng.standard_normal((3, 3, rec[0].size))
    kw = dict(OPTS, tol=1e-6, batch=2)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, freqs, rec, **kw) as sj:
        full = sj.jtvec(w)
    parts = []
    for r in range(2):
        with em.optimize.SurveyJacobian(grid, model, SOURCES, freqs[r::2], rec, **kw) as sj:
            sj.jtvec(w[:, r::2])
            parts.append((sj.partial, np.zeros((3, len(freqs[r::2])))))
    _, grad = em.shard.combine_survey_gradient(parts, len(freqs))
    assert np.array_equal(-grad, full)


# ---- 4. against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['iso', 'tri'])
def test_products_vs_reference(tag):
    """Linear receivers, tol = 1e-8, the reference's update order: data, J v and J^T w per component within the bound
    test_gpu_jacobian.py::test_products_vs_reference uses for solve-level results (relerr < 1e-5)."""
    import emg3d_amd as em
    g, grid = _grid12(em)
    model = _model(em, g, grid, tag)
    rec = tuple(g['rec'])
    vnC = tuple(int(n) for n in grid.vnC)
    v, w = g[f'{tag}_v'].reshape(vnC, order='F'), g[f'{tag}_w']
    kw = dict(OPTS, tol=1e-8, ordering='lex', receiver_interpolation='linear')
    with em.optimize.SurveyJacobian(grid, model, g['sources'], g['freqs'], rec, batch=2, **kw) as sj:
        assert all(info['exit'] == 0 for row in sj.forward_info for info in row)
        syn = sj.synthetic
        jv = sj.jvec(v)
        assert all(info['exit'] == 0 for row in sj.info for info in row)
        jt3 = sj.jtvec(w, components=True)
        assert all(info['exit'] == 0 for row in sj.info for info in row)
        partial3 = sj.partial
        jt = sj.jtvec(w)
    e_syn, e_jv = relerr(syn, g[f'{tag}_synthetic']), relerr(jv, g[f'{tag}_jv'])
    e_jt = [relerr(jt3[c], g[f'{tag}_jt'][c]) for c in range(3)]
    e_tot = relerr(jt, g[f'{tag}_jt'].sum(axis=0))
    print(f"{tag}: data {e_syn:.2e}, J v {e_jv:.2e}, J^T w x / y / z {e_jt[0]:.2e} / {e_jt[1]:.2e} / {e_jt[2]:.2e}, sum {e_tot:.2e}")
    assert e_syn < 1e-5 and e_jv < 1e-5
    assert all(e < 1e-5 for e in e_jt) and e_tot < 1e-5
    for j in range(len(g['freqs'])):
        for c in range(3):
            assert relerr(-partial3[c, j], g[f'{tag}_jt_pair'][c, 0, j] + g[f'{tag}_jt_pair'][c, 1, j]) < 1e-5
    lhs, rhs = np.real(np.sum(np.conj(w) * jv)), np.sum(jt * v)
    gap = abs(lhs - rhs) / abs(lhs)
    print(f"{tag}: adjoint gap of the survey {gap:.2e} (reference, largest pair: {float(g['adj_gap_linear']):.2e})")
    assert gap < 10 * float(g['adj_gap_linear'])


# ---- 5. adjoint and symmetry on a larger model -------------------------------------------------------------------------------
def test_adjoint_and_symmetry_48():
    """48 x 40 x 32 stretched tri-axial model, 3 sources x (frequency, Laplace value), cubic receivers with the exact adjoint,
    tol = 1e-8: the adjoint identity of (jvec, jtvec), the symmetry of gauss_newton and v . H v == sum W |J v|^2, each relative
    and below 10 x the reference-side adjoint gap of the fixture for cubic receivers -- the margin of
    test_gpu_receiver_adjoint.py::test_cubic_exact_is_an_adjoint_pair (gap < 10 * ref_gap): the gaps are set by the solves'
    tolerance, and this grid's solves are no more accurate than the fixture's."""
    em, grid, s3, src, rec, rng = _model48()
    g = load_golden("survey_jacobian.npz")
    ref_gap = float(g['adj_gap_cubic'])
    model = em.Model(grid, *s3, mapping='Conductivity')
    sources = [src, [310., -120., -60., -50., 20.], [20., 260., -90., 80., -30.]]
    freqs = [1.5, -0.8]
    vnC = tuple(int(n) for n in grid.vnC)
    v = (rng.standard_normal(grid.nC) * s3[0] * 0.3).reshape(vnC, order='F')
    u = (rng.standard_normal(grid.nC) * s3[0] * 0.3).reshape(vnC, order='F')
    kw = dict(OPTS, tol=1e-8, receiver_interpolation='cubic', adjoint='exact')
    with em.optimize.SurveyJacobian(grid, model, sources, freqs, rec, batch=3, **kw) as sj:
        syn = sj.synthetic
        shape = syn.shape
        w = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.abs(syn)
        w[:, 1] = w[:, 1].real
        W = 1.0 / np.abs(syn) ** 2
        jv = sj.jvec(v)
        jt = sj.jtvec(w)
        hv = sj.gauss_newton(v, W)
        hu = sj.gauss_newton(u, W)
    assert np.isfinite(jv).all() and np.isfinite(jt).all()
    lhs, rhs = np.real(np.sum(np.conj(w) * jv)), np.sum(jt * v)
    gap_adj = abs(lhs - rhs) / abs(lhs)
    uhv, vhu = np.sum(u * hv), np.sum(v * hu)
    gap_sym = abs(uhv - vhu) / abs(uhv)
    vhv, quad = np.sum(v * hv), np.sum(W * np.abs(jv) ** 2)
    gap_quad = abs(vhv - quad) / abs(quad)
    print(f"48x40x32 survey: adjoint gap {gap_adj:.2e}, symmetry gap {gap_sym:.2e}, v.Hv vs sum W |Jv|^2 {gap_quad:.2e} "
          f"(reference gap, cubic receivers: {ref_gap:.2e})")
    assert vhv > 0
    assert gap_adj < 10 * ref_gap
    assert gap_sym < 10 * ref_gap
    assert gap_quad < 10 * ref_gap
