"""GPU: the survey gradient (optimize.survey_gradient) -- the accumulating gradient kernel bit for bit against the per-system
kernel, the survey against the reference (tests/golden/survey_gradient.npz: the reference's own functions composed per pair as
in gradient.npz, summed in the defined order), independence of the batch size bit for bit, agreement with the per-pair path
optimize.gradient, the combination of frequency shards, and the error paths."""
import numpy as np
import pytest

from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu

SOLVER = dict(cycle='F', semicoarsening=True, linerelaxation=True, verb=0)


def _grid(em, g):
    return em.TensorMesh([g['hx'], g['hy'], g['hz']], origin=g['origin'])


# ---- 1. the kernel primitive ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("freq, nsys", [(1.5, 3), (-1.5, 3), (1.5, 1)], ids=["c128-3", "f64-3", "c128-1"])
def test_grad_acc_is_the_sequential_sum_of_the_system_gradients(freq, nsys):
    """grad_acc_add == ((acc + g_0) + g_2) with g_b = DeviceMG.gradient of system b, bit for bit; a second call adds once more;
    reset zeroes; bad vector ids are refused; the accumulator is counted by device_bytes."""
    import emg3d_amd as em
    from emg3d_amd import models
    from emg3d_amd.solver import DeviceMG
    g = load_golden("gradient.npz")
    grid = _grid(em, g)
    model = em.Model(grid, g['res'])
    sf = em.SourceField(grid, freq=freq)
    rng = np.random.default_rng(5)

    def rand():
        a = rng.standard_normal(grid.nE)
        return a if freq < 0 else a + 1j * rng.standard_normal(grid.nE)
    fwd = [rand() for _ in range(nsys)]
    bwd = [rand() for _ in range(nsys)]
    use = np.array([1, 0, 1][:nsys], dtype=np.int32)
    with DeviceMG.from_sigma_volume(grid, *models.sigma_volume(grid, model), smu0=sf.smu0) as dev:
        if nsys > 1:
            dev.set_batch(nsys)
        assert dev.nsys == nsys
        dev.vec_alloc(1)
        dev.bvec_alloc(1)
        gb = []
        for b in range(nsys):
            dev.select(b)
            dev.set_efield(em.Field(grid, bwd[b].copy(), freq=freq))
            dev.bvec_set(0, b, fwd[b])
            dev.vec_set(0, fwd[b])
            gb.append(dev.gradient(0, sf.smu0))
        assert all(np.abs(x).max() > 0 for x in gb)
        before = dev.device_bytes
        dev.grad_acc_reset()
        grown = dev.device_bytes - before
        assert grid.nC * 8 <= grown < grid.nC * 8 + 256
        assert np.array_equal(dev.grad_acc_get(), np.zeros(grid.nC))
        want = np.zeros(grid.nC)
        for b in range(nsys):
            if use[b]:
                want = want + gb[b]
        dev.grad_acc_add(0, sf.smu0, use)
        assert np.array_equal(dev.grad_acc_get(), want)
        # the accumulator is the handle's own: the per-system gradient (staged in the residual buffer), another mask and
        # another frequency leave it alone
        dev.select(0)
        dev.gradient(0, sf.smu0)
        dev.set_mask(np.ones(nsys, dtype=np.int32) - use)
        dev.set_mask(np.ones(nsys, dtype=np.int32))
        dev.set_smu0(2 * sf.smu0)
        dev.set_smu0(sf.smu0)
        assert np.array_equal(dev.grad_acc_get(), want)
        # a second call adds the same values once more, in the same order
        for b in range(nsys):
            if use[b]:
                want = want + gb[b]
        dev.grad_acc_add(0, sf.smu0, use)
        assert np.array_equal(dev.grad_acc_get(), want)
        # no system selected: nothing changes
        dev.grad_acc_add(0, sf.smu0, np.zeros(nsys, dtype=np.int32))
        assert np.array_equal(dev.grad_acc_get(), want)
        assert dev.device_bytes - before == grown
        # the forward fields must be a saved batched vector
        a = complex(sf.smu0)
        for bad in (-2, -1, 1, 7):
            assert dev._lib.emg3d_mg_grad_acc_add(dev._h, bad, a.real, a.imag, use.ctypes.data) == -2
        with pytest.raises(ValueError):
            dev.grad_acc_add(dev.EFIELD, sf.smu0, use)
        assert np.array_equal(dev.grad_acc_get(), want)
        dev.grad_acc_reset()
        assert np.array_equal(dev.grad_acc_get(), np.zeros(grid.nC))


@pytest.mark.parametrize("freq", [1.5, -1.5], ids=["c128", "f64"])
def test_both_spellings_address_the_same_accumulators(freq):
    """grad_acc_*(components=True) and sens_acc_add(components=True) are grad_acc3_* and sens_acc_add(split=True): equal results
    on one handle, and an add through one spelling shows in a get through the other.  4 x 3 x 2 cells, three systems of which
    the middle one is masked out, a weight table with one zero entry; the summed accumulator is not touched by any of it."""
    import emg3d_amd as em
    from emg3d_amd import models
    from emg3d_amd.solver import DeviceMG
    grid = em.TensorMesh([[40., 50., 60., 70.], [30., 45., 65.], [55., 80.]], origin=(-110., -70., -60.))
    model_grid = em.TensorMesh([[110., 110.], [140.], [60., 75.]], origin=(-110., -70., -60.))
    assert tuple(grid.vnC) == (4, 3, 2)
    sf = em.SourceField(grid, freq=freq)
    rng = np.random.default_rng(7)
    nsys, use = 3, np.array([1, 0, 1], dtype=np.int32)
    W = rng.uniform(0.5, 2.0, (nsys, nsys))
    W[2, 0] = 0.0

    def rand():
        a = rng.standard_normal(grid.nE)
        return a if freq < 0 else a + 1j * rng.standard_normal(grid.nE)
    model = em.Model(grid, rng.uniform(0.5, 2.0, grid.nC), mapping='Conductivity')
    with DeviceMG.from_sigma_volume(grid, *models.sigma_volume(grid, model), smu0=sf.smu0) as dev:
        dev.set_batch(nsys)
        dev.bvec_alloc(1)
        for b in range(nsys):
            dev.bvec_set(0, b, rand())
            dev.select(b)
            dev.vec_set(dev.EFIELD, rand())
        dev.set_model_grid(model_grid)
        dev.set_regrid_factors(tuple(rng.uniform(0.5, 2.0, grid.vnC) for _ in range(3)),
                               tuple(rng.uniform(0.5, 2.0, model_grid.vnC) for _ in range(3)))

        def same(a, b):
            return len(a) == len(b) == 3 and all(np.array_equal(x, y) for x, y in zip(a, b))

        def both():
            """The three accumulators through either spelling, on the handle's grid and on the model grid."""
            new, old = dev.grad_acc_get(components=True), dev.grad_acc3_get()
            assert isinstance(new, tuple) and same(new, old)
            assert same(dev.grad_acc_get_model(components=True), dev.grad_acc3_get_model())
            return old
        dev.grad_acc_reset()
        dev.grad_acc_add(0, sf.smu0, use)
        one = dev.grad_acc_get()
        assert np.abs(one).max() > 0
        # the gradient: new spelling, then the same through the kept one, and an add through each on top of the other
        dev.grad_acc_reset(components=True)
        assert same(both(), [np.zeros(grid.nC)] * 3)
        dev.grad_acc_add(0, sf.smu0, use, components=True)
        new = both()
        assert all(np.abs(x).max() > 0 for x in new)
        dev.grad_acc3_reset()
        assert same(both(), [np.zeros(grid.nC)] * 3)
        dev.grad_acc3_add(0, sf.smu0, use)
        assert same(both(), new)
        dev.grad_acc_add(0, sf.smu0, use, components=True)
        mixed = both()
        dev.grad_acc_reset(components=True)
        dev.grad_acc3_add(0, sf.smu0, use)
        dev.grad_acc3_add(0, sf.smu0, use)
        assert same(both(), mixed)
        # the sensitivity diagonal likewise
        dev.grad_acc3_reset()
        dev.sens_acc_add(0, sf.smu0, use, use, W, components=True)
        new = both()
        assert all(np.abs(x).max() > 0 for x in new)
        dev.grad_acc_reset(components=True)
        dev.sens_acc_add(0, sf.smu0, use, use, W, split=True)
        assert same(both(), new)
        dev.sens_acc_add(0, sf.smu0, use, use, W, components=True)
        mixed = both()
        dev.grad_acc3_reset()
        dev.sens_acc_add(0, sf.smu0, use, use, W, split=True)
        dev.sens_acc_add(0, sf.smu0, use, use, W, split=True)
        assert same(both(), mixed)
        assert np.array_equal(dev.grad_acc_get(), one) and np.array_equal(dev.grad_acc_get(components=False), one)


# ---- 2. + 4. against the reference fixture and against the per-pair path -----------------------------------------------------
@pytest.fixture(scope="module")
def fixture_run():
    import emg3d_amd as em
    g = load_golden("survey_gradient.npz")
    grid = _grid(em, g)
    model = em.Model(grid, g['res'])
    opts = dict(SOLVER, tol=1e-8, ordering='lex')
    out = em.optimize.survey_gradient(grid, model, g['sources'], g['freqs'], tuple(g['rec']), g['observed'], g['weights'], **opts)
    return g, grid, model, opts, out


def test_survey_gradient_vs_reference(fixture_run):
    """Tolerances: the project's own for two chained tol = 1e-8 solves (tests/test_gpu_gradient.py); the fixture's sums do not
    cancel (asserted by its generator), so they carry over to the G_f and the total."""
    g, grid, model, opts, (phi, grad, info) = fixture_run
    ns, nf = g['misfit'].shape
    assert np.isnan(g['observed']).sum() == 1
    for i in range(ns):
        for j in range(nf):
            assert info['forward'][i][j]['exit'] == 0 and info['backward'][i][j]['exit'] == 0
            assert relerr(info['synthetic'][i, j], g['synthetic'][i, j]) < 1e-6
            assert abs(info['misfit'][i, j] / g['misfit'][i, j] - 1) < 1e-5
    assert np.isfinite(info['synthetic']).all() and np.isfinite(info['misfit']).all() and np.isfinite(grad).all()
    assert abs(phi / float(g['phi']) - 1) < 1e-5
    assert info['partial'].shape == (nf,) + tuple(grid.vnC) and grad.shape == tuple(grid.vnC)
    for j in range(nf):
        assert relerr(info['partial'][j], g['partial'][j]) < 1e-5
    assert relerr(grad, g['grad']) < 1e-5


def test_survey_gradient_vs_per_pair_gradient(fixture_run):
    """The host sum of optimize.gradient() over the pairs (a handle of its own each), in the defined order."""
    import emg3d_amd as em
    g, grid, model, opts, (phi, grad, info) = fixture_run
    ns, nf = g['misfit'].shape
    want = np.zeros(grid.vnC, order='F')
    dev_syn = dev_mis = 0.0
    for j in range(nf):
        gf = np.zeros(grid.vnC, order='F')
        for i in range(ns):
            p, gp, pinfo = em.optimize.gradient(grid, model, g['sources'][i], float(g['freqs'][j]), tuple(g['rec']),
                                                g['observed'][i, j], g['weights'][i, j], **opts)
            gf = gf + gp
            dev_syn = max(dev_syn, relerr(info['synthetic'][i, j], pinfo['synthetic']))
            dev_mis = max(dev_mis, abs(info['misfit'][i, j] / p - 1))
        want = want + gf
    dev_grad = relerr(grad, want)
    print(f"survey_gradient against the sum of gradient(): grad {dev_grad:.3e}, misfit {dev_mis:.3e}, synthetic {dev_syn:.3e}")
    assert dev_syn < 1e-6
    assert dev_mis < 1e-5
    assert dev_grad < 1e-5


# ---- 3. + 5. independence of the batch size, frequency shards ----------------------------------------------------------------------
def _same(a, b):
    """Bit-for-bit equality of two survey_gradient results, the cycle counts and norms of every solve included."""
    (pa, ga, ia), (pb, gb, ib) = a, b
    assert pa == pb
    assert np.array_equal(ga, gb)
    for key in ('partial', 'synthetic', 'misfit'):
        assert np.array_equal(ia[key], ib[key]), key
    for key in ('forward', 'backward'):
        for ra, rb in zip(ia[key], ib[key]):
            for da, db in zip(ra, rb):
                assert (da is None) == (db is None), key
                if da is not None:
                    assert da['it_mg'] == db['it_mg'] and da['exit'] == db['exit'] == 0, key
                    assert np.array_equal(da['error_at_cycle'], db['error_at_cycle']), key


SOURCES = [[-100., 30., 20., 25., 5.], [140., -60., -25., -50., 20.], [20., 100., -40., 80., -30.]]
FREQS = [1.5, -1.2, 0.7]            # (the second: a Laplace-domain value)


@pytest.fixture(scope="module")
def small_survey():
    """3 sources x 3 frequencies on the 12 x 10 x 8 grid of gradient.npz; observed data from the perturbed model."""
    import emg3d_amd as em
    g = load_golden("gradient.npz")
    grid = _grid(em, g)
    model = em.Model(grid, g['res'])
    res_true = g['res'].copy().reshape(grid.vnC, order='F')
    res_true[5:9, 3:7, 2:5] *= 4.0
    rec = tuple(g['rec'])
    obs, _ = em.shard.solve_survey(grid, em.Model(grid, res_true.ravel('F')), SOURCES, FREQS, rec, tol=1e-6, **SOLVER)
    weights = 1.0 / (0.05 * np.abs(obs)) ** 2
    obs = obs.copy()
    obs[1, 0, :] = np.nan             # a pair without data: the middle system of a chunk of three
    obs[2, 1, 3] = np.nan
    return grid, model, rec, obs, weights


def test_batch_invariance_bitwise(small_survey):
    import emg3d_amd as em
    grid, model, rec, obs, weights = small_survey
    freqs = FREQS[:2]
    obs, weights = obs[:, :2], weights[:, :2]

    def run(batch, **kw):
        return em.optimize.survey_gradient(grid, model, SOURCES, freqs, rec, obs, weights, batch=batch, tol=1e-6, **SOLVER, **kw)
    one = run(1)
    assert one[2]['backward'][1][0] is None and one[2]['backward'][0][0] is not None
    assert np.abs(one[1]).max() > 0 and np.abs(one[2]['partial'][1]).max() > 0
    _same(run(2), one)              # (the last chunk is shorter)
    _same(run(3), one)
    _same(run(2, adjoint='exact'), run(1, adjoint='exact'))
    # magnetic receivers: the data are of another size, so the misfit is taken against zeros (bitwise equality is the check)
    zero = np.where(np.isnan(obs), np.nan, 0.0)
    mag = [em.optimize.survey_gradient(grid, model, SOURCES, freqs, rec, zero, None, batch=b, tol=1e-6, electric=False,
                                       adjoint='exact', **SOLVER) for b in (2, 1)]
    assert np.abs(mag[0][1]).max() > 0
    _same(*mag)


def test_batch_invariance_bitwise_many_levels():
    """48 x 40 x 32 stretched isotropic model, sc + lr: a deep hierarchy with large levels' working copies -- where a frozen
    system or a stale working copy would show."""
    import emg3d_amd as em
    hx = em.meshes.stretched_widths(36, 6, 50., 1.25)
    hy = em.meshes.stretched_widths(30, 5, 50., 1.3)
    hz = em.meshes.stretched_widths(24, 4, 50., 1.35)
    grid = em.TensorMesh([hx, hy, hz], origin=(-hx.sum() / 2, -hy.sum() / 2, -hz.sum() / 2))
    assert tuple(grid.vnC) == (48, 40, 32)
    rng = np.random.default_rng(11)
    model = em.Model(grid, 10 ** rng.uniform(-0.3, 1.0, grid.nC))
    sources = [[-300., 40., 30., 25., 5.], [310., -120., -60., -50., 20.], [20., 260., -90., 80., -30.]]
    freqs = [1.0, -0.8]
    rec = (np.array([450., -520., 120., 600.]), np.array([80., 210., -330., -60.]), np.array([-40., 20., 110., 50.]),
           np.array([0., 40., -70., 10.]), np.array([0., 10., -15., 60.]))
    obs = np.zeros((3, 2, 4))
    obs[1, 0, :] = np.nan
    obs[0, 1, 2] = np.nan
    runs = [em.optimize.survey_gradient(grid, model, sources, freqs, rec, obs, None, batch=b, tol=1e-6, **SOLVER) for b in (1, 2, 3)]
    assert np.abs(runs[0][1]).max() > 0 and runs[0][2]['backward'][1][0] is None
    _same(runs[1], runs[0])
    _same(runs[2], runs[0])


def test_frequency_shards_combine_bitwise(small_survey):
    import emg3d_amd as em
    grid, model, rec, obs, weights = small_survey

    def run(sl):
        return em.optimize.survey_gradient(grid, model, SOURCES, FREQS[sl], rec, obs[:, sl], weights[:, sl], batch=2, tol=1e-6,
                                           **SOLVER)
    phi, grad, info = run(slice(None))
    parts = [run(slice(r, None, 2)) for r in range(2)]
    got_phi, got_grad = em.shard.combine_survey_gradient([(p[2]['partial'], p[2]['misfit']) for p in parts], len(FREQS))
    assert got_phi == phi and np.array_equal(got_grad, grad)
    # without a process group gather_survey_gradient sums the local arrays
    loc_phi, loc_grad = em.shard.gather_survey_gradient(info['partial'], info['misfit'], FREQS)
    assert loc_phi == phi and np.array_equal(loc_grad, grad)


# ---- 6. error paths ---------------------------------------------------------------------------------------------------
def test_error_paths():
    import emg3d_amd as em
    g = load_golden("gradient.npz")
    grid = _grid(em, g)
    rec = tuple(g['rec'])
    obs = np.zeros((2, 1, 5), dtype=complex)
    srcs = SOURCES[:2]
    model = em.Model(grid, g['res'])
    with pytest.raises(NotImplementedError):
        em.optimize.survey_gradient(grid, model, srcs, [1.0], rec, obs, sslsolver=True)
    with pytest.raises(NotImplementedError, match="isotropic"):
        em.optimize.survey_gradient(grid, em.Model(grid, g['res'], 2 * g['res']), srcs, [1.0], rec, obs)
    with pytest.raises(NotImplementedError, match="permeability"):
        em.optimize.survey_gradient(grid, em.Model(grid, g['res'], mu_r=np.full(grid.nC, 1.5)), srcs, [1.0], rec, obs)
    with pytest.raises(ValueError, match="observed"):
        em.optimize.survey_gradient(grid, model, srcs, [1.0], rec, obs[:, :, :4])
    with pytest.raises(ValueError, match="adjoint"):
        em.optimize.survey_gradient(grid, model, srcs, [1.0], rec, obs, adjoint='nearly')
