"""GPU: optimize.Jacobian -- the products J v and J^T w of the sensitivity matrix of one (source, frequency) pair.

Kernel level and solve level against tests/golden/jacobian.npz (the reference's own functions composed by
tests/golden/make_jacobian_golden.py: sources s mu_0 C(v) E and P^T conj(w), the solves, a central finite difference of
the reference's forward data), then without a reference on a 48 x 40 x 32 model: finite differences of the existing
solve() + receivers, batched against one-at-a-time products, and a second Jacobian after the first has been closed."""
import numpy as np
import pytest

from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu

OPTS = dict(cycle='F', semicoarsening=True, linerelaxation=True, verb=0)
INFO_KEYS = ('exit', 'exit_message', 'it_mg', 'abs_error', 'rel_error', 'ref_error', 'tol')


def _setup(tag):
    import emg3d_amd as em
    g = load_golden("gradient.npz")
    j = load_golden("jacobian.npz")
    grid = em.TensorMesh([g['hx'], g['hy'], g['hz']], origin=g['origin'])
    model = em.Model(grid, j[f'{tag}_sig_x'], j[f'{tag}_sig_y'], j[f'{tag}_sig_z'], mapping='Conductivity')
    return em, g, j, grid, model


def _handle(em, grid, model, freq):
    from emg3d_amd.solver import DeviceMG
    from emg3d_amd import models
    sf = em.SourceField(grid, freq=freq)
    return DeviceMG.from_sigma_volume(grid, *models.sigma_volume(grid, model), smu0=sf.smu0), sf.smu0


def _boundary_edges(grid):
    """True on the PEC boundary edges of [fx|fy|fz]."""
    nx, ny, nz = (int(n) for n in grid.vnC)
    bx = np.zeros((nx, ny + 1, nz + 1), bool); bx[:, [0, -1], :] = True; bx[:, :, [0, -1]] = True
    by = np.zeros((nx + 1, ny, nz + 1), bool); by[[0, -1], :, :] = True; by[:, :, [0, -1]] = True
    bz = np.zeros((nx + 1, ny + 1, nz), bool); bz[[0, -1], :, :] = True; bz[:, [0, -1], :] = True
    return np.r_[bx.ravel('F'), by.ravel('F'), bz.ravel('F')]


@pytest.mark.parametrize('tag', ['iso', 'tri'])
def test_source_kernels_vs_reference(tag):
    """emg3d_mg_jvec_source and emg3d_mg_set_receiver_adjoint with the reference's forward field uploaded: the bound of
    test_gpu_gradient.py for device-built sources; deterministic; boundary edges exactly zero."""
    em, g, j, grid, model = _setup(tag)
    rec = tuple(g['rec'])
    v, w = j[f'{tag}_v'], j[f'{tag}_w']
    bnd = _boundary_edges(grid)
    dev, smu0 = _handle(em, grid, model, float(g['freq']))
    with dev:
        dev.vec_alloc(1)
        dev.vec_set(0, j[f'{tag}_efield'])
        for case, v3 in (('full', (v, v, v)), ('vz', (None, None, v))):
            dev.jvec_source(0, smu0, *v3)
            got = dev.vec_get(dev.SFIELD)
            err = relerr(got, j[f'{tag}_{case}_src'])
            print(f"jvec_source {tag} {case}: relerr {err:.2e}")
            assert err < 1e-12
            assert np.all(got[bnd] == 0)
            dev.jvec_source(0, smu0, *v3)
            assert np.array_equal(dev.vec_get(dev.SFIELD), got)
        nx, ny, nz = (int(n) for n in grid.vnC)
        assert np.all(got[:nx * (ny + 1) * (nz + 1) + (nx + 1) * ny * (nz + 1)] == 0)       # v_z only: no x- / y-source
        dev.set_receiver_adjoint(rec, np.conj(w))
        got = dev.vec_get(dev.SFIELD)
        err = relerr(got, j[f'{tag}_jt_src'])
        print(f"receiver_adjoint {tag}: relerr {err:.2e}")
        assert err < 1e-12
        assert np.all(got[bnd] == 0)
        dev.set_receiver_adjoint(rec, np.conj(w))
        assert np.array_equal(dev.vec_get(dev.SFIELD), got)
        dev.set_receiver_adjoint(rec, np.conj(w), accumulate=True)
        assert np.array_equal(dev.vec_get(dev.SFIELD), 2 * got)
        # a receiver in an outermost cell has no datum (NaN): it contributes nothing
        rec2 = tuple(np.r_[c, e] for c, e in zip(rec, (grid.nodes_x[0] + 0.25 * grid.h[0][0], 0., 0., 30., 20.)))
        dev.set_receiver_adjoint(rec2, np.r_[np.conj(w), 1 + 1j])
        assert np.array_equal(dev.vec_get(dev.SFIELD), got)


@pytest.mark.parametrize('tag', ['iso', 'tri'])
def test_linear_receivers_vs_reference(tag):
    em, g, j, grid, model = _setup(tag)
    rec = tuple(g['rec'])
    field = em.Field(grid, j[f'{tag}_efield'].copy(), freq=float(g['freq']))
    rec2 = tuple(np.r_[c, e] for c, e in zip(rec, (grid.nodes_x[0] + 0.25 * grid.h[0][0], 0., 0., 30., 20.)))
    dev, smu0 = _handle(em, grid, model, float(g['freq']))
    with dev:
        dev.set_efield(field)
        got = dev.get_receiver_response(rec, method='linear')
        err = relerr(got, j[f'{tag}_d_lin'])
        print(f"linear receivers {tag}: relerr {err:.2e}")
        assert err < 1e-12
        lin2 = dev.get_receiver_response(rec2, method='linear')
        cub2 = dev.get_receiver_response(rec2)
        assert np.array_equal(lin2[:-1], got) and np.isnan(lin2[-1]) and np.isnan(cub2[-1])
        # the default keeps today's result
        assert np.array_equal(dev.get_receiver_response(rec, method='cubic'), dev.get_receiver_response(rec))
    host = em.get_receiver_response(grid, field, rec, method='linear')
    assert relerr(host, j[f'{tag}_d_lin']) < 1e-12
    assert np.isnan(em.get_receiver_response(grid, field, rec2, method='linear')[-1])
    assert np.array_equal(em.get_receiver_response(grid, field, rec, method='cubic'), em.get_receiver_response(grid, field, rec))


@pytest.mark.parametrize('tag', ['iso', 'tri'])
def test_gradient3_vs_reference(tag):
    em, g, j, grid, model = _setup(tag)
    freq = float(g['freq'])
    dev, smu0 = _handle(em, grid, model, freq)
    with dev:
        dev.vec_alloc(1)
        dev.vec_set(0, j[f'{tag}_efield'])
        dev.set_efield(em.Field(grid, j[f'{tag}_lam'].copy(), freq=freq))
        gx, gy, gz = dev.gradient(0, smu0, components=True)
        one = dev.gradient(0, smu0)
    assert np.array_equal((gx + gy) + gz, one)
    for got, key in ((gx, 'gx'), (gy, 'gy'), (gz, 'gz')):
        err = relerr(got.reshape(grid.vnC, order='F'), j[f'{tag}_jt_{key}'])
        print(f"gradient3 {tag} {key}: relerr {err:.2e}")
        assert err < 1e-14


def test_cellaverages2edges_is_the_transpose():
    """sum(e2c(f) * v) == sum(f * c2e(v)) for random complex f with non-zero boundary values (both sides are sums of ~4 nE
    products in float64: 1e-13 relative), and c2e equals its numpy restatement to the rounding of a four-term sum."""
    import emg3d_amd as em
    g = load_golden("gradient.npz")
    grid = em.TensorMesh([g['hx'], g['hy'], g['hz']], origin=g['origin'])
    nx, ny, nz = (int(n) for n in grid.vnC)
    vol = grid.cell_volumes.reshape(grid.vnC, order='F')
    rng = np.random.default_rng(5)
    for dtype in (np.complex128, np.float64):
        def rnd(shape):
            a = rng.standard_normal(shape)
            return (a + 1j * rng.standard_normal(shape)).astype(dtype) if dtype == np.complex128 else a
        f = em.Field(grid, rnd(grid.nE), freq=1. if dtype == np.complex128 else -1.)
        v = [np.asfortranarray(rnd(grid.vnC)) for _ in range(3)]
        o = [np.zeros(grid.vnC, order='F', dtype=dtype) for _ in range(3)]
        em.maps.edges2cellaverages(f.fx, f.fy, f.fz, vol, *o)
        out = em.Field(grid, dtype=dtype, freq=f._freq)
        em.maps.cellaverages2edges(v[0], v[1], v[2], vol, out.fx, out.fy, out.fz)
        lhs = sum(np.sum(a * b) for a, b in zip(o, v))
        rhs = np.sum(np.asarray(f.field) * np.asarray(out.field))
        print(f"transpose {np.dtype(dtype).name}: {abs(lhs - rhs) / abs(lhs):.2e}")
        assert abs(lhs - rhs) <= 1e-13 * abs(lhs)
        # numpy restatement: every statement of edges2cellaverages, transposed (boundary edges see their cell 2 or 4 times)
        want = [np.zeros(s, dtype=dtype) for s in ((nx, ny + 1, nz + 1), (nx + 1, ny, nz + 1), (nx + 1, ny + 1, nz))]

        def lo(n):          # cell max(e - 1, 0) of edge e = 0 .. n
            return np.maximum(np.arange(n + 1) - 1, 0)

        def hi(n):          # cell min(e, n - 1)
            return np.minimum(np.arange(n + 1), n - 1)
        for a in (lo, hi):
            for b in (lo, hi):
                want[0] += (vol * v[0] / 4)[:, a(ny), :][:, :, b(nz)]
                want[1] += (vol * v[1] / 4)[a(nx), :, :][:, :, b(nz)]
                want[2] += (vol * v[2] / 4)[a(nx), :, :][:, b(ny), :]
        for got, w in zip((out.fx, out.fy, out.fz), want):
            assert relerr(got, w) < 1e-14
        # ADDED into the outputs; a missing component is left alone
        keep = np.array(out.fy)
        em.maps.cellaverages2edges(v[0], None, None, vol, out.fx, None, None)
        assert relerr(out.fx, 2 * want[0]) < 1e-14 and np.array_equal(out.fy, keep)


@pytest.mark.parametrize('tag', ['iso', 'tri'])
def test_products_vs_reference(tag):
    """Solve level in the reference's update order: data, J v and J^T w against the stored results (two chained iterative
    solves at tol 1e-8: the bound of test_gradient_vs_reference), J v against the finite difference of the reference's
    forward data, and the adjoint test with linear receivers."""
    em, g, j, grid, model = _setup(tag)
    rec = tuple(g['rec'])
    v, w = j[f'{tag}_v'].reshape(grid.vnC, order='F'), j[f'{tag}_w']
    fd_gap, adj_gap = float(j['fd_gap_ref']), float(j['adjoint_gap_ref'])
    kw = dict(OPTS, tol=1e-8, ordering='lex')
    with em.optimize.Jacobian(grid, model, g['src'], float(g['freq']), rec, **kw) as jac:
        assert jac.forward_info['exit'] == 0
        assert relerr(jac.synthetic, j[f'{tag}_d_lin']) < 1e-5
        jv = {'full': jac.jvec(v), 'vz': jac.jvec((None, None, v))}
        assert jac.info['exit'] == 0
        gx, gy, gz = jac.jtvec(w, components=True)
        jt = jac.jtvec(w)
        assert jac.info['exit'] == 0
    assert jt.shape == tuple(grid.vnC) and jt.dtype == np.float64 and jt.flags.f_contiguous
    assert np.array_equal(jt, (gx + gy) + gz)
    ref_jt = {'full': -(j[f'{tag}_jt_gx'] + j[f'{tag}_jt_gy'] + j[f'{tag}_jt_gz']), 'vz': -j[f'{tag}_jt_gz']}
    got_jt = {'full': jt, 'vz': gz}
    for key, ref in (('gx', gx), ('gy', gy), ('gz', gz)):
        assert relerr(ref, -j[f'{tag}_jt_{key}']) < 1e-5
    for case in ('full', 'vz'):
        e_jv, e_jt = relerr(jv[case], j[f'{tag}_{case}_jv']), relerr(got_jt[case], ref_jt[case])
        fd = j[f'{tag}_{case}_jv_fd']
        e_fd = np.linalg.norm(jv[case] - fd) / np.linalg.norm(fd)
        lhs = np.real(np.sum(np.conj(w) * jv[case]))
        rhs = np.sum(got_jt[case] * v)
        gap = abs(lhs - rhs) / abs(lhs)
        print(f"{tag} {case}: J v {e_jv:.2e}, J^T w {e_jt:.2e}, vs FD {e_fd:.2e}, adjoint gap {gap:.2e} "
              f"(reference {adj_gap:.2e})")
        assert e_jv < 1e-5 and e_jt < 1e-5
        assert e_fd < 1e-5 + fd_gap
        assert gap < 10 * adj_gap
    if tag == 'iso':        # the one-shot wrappers: open, one product, close
        assert relerr(em.optimize.jvec(grid, model, g['src'], float(g['freq']), rec, v, **kw), jv['full']) < 1e-12
        assert relerr(em.optimize.jtvec(grid, model, g['src'], float(g['freq']), rec, w, **kw), jt) < 1e-12


def test_cubic_receivers_reproduce_the_gradient():
    """receiver_interpolation='cubic': data and J v use the cubic-spline receivers, J^T w the reference's
    receivers-as-sources rule, so that jtvec(weights * residual) == -gradient(...)[1]; the pair is not an adjoint pair (the
    adjoint quantity only has to be finite)."""
    import emg3d_amd as em
    g = load_golden("gradient.npz")
    j = load_golden("jacobian.npz")
    grid = em.TensorMesh([g['hx'], g['hy'], g['hz']], origin=g['origin'])
    model = em.Model(grid, g['res'])
    rec = tuple(g['rec'])
    kw = dict(OPTS, tol=1e-8, ordering='lex')
    v, w = j['iso_v'].reshape(grid.vnC, order='F'), j['iso_w']
    phi, grad, info = em.optimize.gradient(grid, model, g['src'], float(g['freq']), rec, g['observed'], g['weights'], **kw)
    with em.optimize.Jacobian(grid, model, g['src'], float(g['freq']), rec, receiver_interpolation='cubic', **kw) as jac:
        assert relerr(jac.synthetic, g['synthetic']) < 1e-6
        residual = jac.synthetic - g['observed']
        got = jac.jtvec(g['weights'] * residual)
        jv = jac.jvec(v)
        jt = jac.jtvec(w)
    err = relerr(got, -grad)
    lhs, rhs = np.real(np.sum(np.conj(w) * jv)), np.sum(jt * v)
    print(f"cubic: jtvec(W r) vs -gradient {err:.2e}; Re sum conj(w) J v = {lhs:.6f}, v . J^T w = {rhs:.6f}, "
          f"gap {abs(lhs - rhs) / abs(lhs):.2f}")
    assert err < 1e-5
    assert np.isfinite(abs(lhs - rhs) / abs(lhs))


# ---- without a reference: the default (colour) ordering on a 48 x 40 x 32 stretched tri-axial model ----------------------

def _model48():
    import emg3d_amd as em
    hx = em.meshes.stretched_widths(32, 8, 50., 1.2)
    hy = em.meshes.stretched_widths(24, 8, 50., 1.2)
    hz = em.meshes.stretched_widths(16, 8, 50., 1.2)
    grid = em.TensorMesh([hx, hy, hz], origin=(-hx.sum() / 2, -hy.sum() / 2, -hz.sum() / 2))
    assert tuple(grid.vnC) == (48, 40, 32)
    rng = np.random.default_rng(48)
    sig = 1 / 10 ** rng.uniform(-0.3, 1.0, grid.nC)
    s3 = (sig, sig * 10 ** rng.uniform(-0.3, 0.3, grid.nC), sig * 10 ** rng.uniform(-0.3, 0.3, grid.nC))
    src = [-120., 40., 30., 25., 5.]
    rec = (np.array([300., 420., -380., 110., 520., -200.]), np.array([60., -190., 210., 15., -80., -300.]),
           np.array([-40., 60., 20., -90., 45., 110.]), np.array([0., 40., -70., 90., 10., 200.]),
           np.array([0., 10., -15., 30., 60., -40.]))
    return em, grid, s3, src, rec, rng


def test_jvec_vs_finite_differences_of_solve():
    """J v (cubic receivers: the data of the existing solve() + get_receiver_response) against central differences at steps
    h and h / 2: ||J v - FD(h/2)|| <= 2 ||FD(h) - FD(h/2)|| + 1e-5 ||J v||.  The first term is the measured truncation
    error (the error of FD(h/2) is a third of the difference of the two for an h^2 law).  h = 1e-2: the truncation term is
    then ~1e-5 of ||J v|| (the reference's own data gave 8e-6 at this step on the 12 x 10 x 8 set-up), and with tol = 1e-10
    the solver's noise in the difference quotient, tol ||d|| / h = 1e-8 ||d||, stays below 1e-5 ||J v||."""
    em, grid, s3, src, rec, rng = _model48()
    freq, h = 1.5, 1e-2
    kw = dict(OPTS, tol=1e-10, maxit=60)
    v = (rng.standard_normal(grid.nC) * s3[0] * 0.3).reshape(grid.vnC, order='F')
    sfield = em.get_source_field(grid, src, freq)

    def data(step):
        m = em.Model(grid, *(s + step * v.ravel('F') for s in s3), mapping='Conductivity')
        e, info = em.solve(grid, m, sfield, return_info=True, **kw)
        assert info['exit'] == 0
        return em.get_receiver_response(grid, e, rec)
    fd1 = (data(h) - data(-h)) / (2 * h)
    fd2 = (data(h / 2) - data(-h / 2)) / h
    d0 = data(0.)
    model = em.Model(grid, *s3, mapping='Conductivity')
    with em.optimize.Jacobian(grid, model, src, freq, rec, receiver_interpolation='cubic', **kw) as jac:
        assert relerr(jac.synthetic, d0) < 1e-8
        jv = jac.jvec(v)
        assert jac.info['exit'] == 0
    nrm = np.linalg.norm(jv)
    trunc, err = np.linalg.norm(fd1 - fd2), np.linalg.norm(jv - fd2)
    noise = kw['tol'] * np.linalg.norm(d0) / h
    print(f"48x40x32: ||Jv - FD(h/2)|| / ||Jv|| = {err / nrm:.2e}, ||FD(h) - FD(h/2)|| / ||Jv|| = {trunc / nrm:.2e}, "
          f"solver noise / ||Jv|| = {noise / nrm:.2e}")
    assert trunc < 1e-4 * nrm and noise < 1e-5 * nrm          # the step and the tolerance are as the bound assumes
    assert err <= 2 * trunc + 1e-5 * nrm


def test_batched_products_equal_single_products_bit_for_bit():
    """nvec = 4: four (and five: groups of four) vectors through the same cycles equal the single products of an nvec = 1
    Jacobian bit for bit, info dicts included; a second Jacobian after the first has closed its handle gives the same
    results (nothing is left behind in the pooled blocks)."""
    em, grid, s3, src, rec, rng = _model48()
    freq = 1.5
    kw = dict(OPTS, tol=1e-6)
    model = em.Model(grid, *s3, mapping='Conductivity')
    V = np.stack([(rng.standard_normal(grid.nC) * s3[0] * 0.3).reshape(grid.vnC, order='F') for _ in range(4)])
    n = rec[0].size
    W = rng.standard_normal((5, n)) + 1j * rng.standard_normal((5, n))
    W[2, 1:] = 0

    def singles():
        with em.optimize.Jacobian(grid, model, src, freq, rec, **kw) as jac:
            out = dict(syn=jac.synthetic.copy(), fwd=jac.forward_info, jv=[], jv_info=[], jt=[], jt_info=[])
            for x in V:
                out['jv'].append(jac.jvec(x)); out['jv_info'].append(jac.info)
            out['jvz'] = jac.jvec((None, None, V[0]))
            for x in W:
                out['jt'].append(jac.jtvec(x)); out['jt_info'].append(jac.info)
            out['jt3'] = jac.jtvec(W[0], components=True)
        return out

    def same_info(a, b):
        for key in INFO_KEYS:
            assert a[key] == b[key], (key, a[key], b[key])
        assert np.array_equal(a['error_at_cycle'], b['error_at_cycle'])
    one = singles()
    with em.optimize.Jacobian(grid, model, src, freq, rec, nvec=4, **kw) as jac:
        assert np.array_equal(jac.synthetic, one['syn'])
        same_info(jac.forward_info, one['fwd'])
        jv = jac.jvec(V)
        jv_info = jac.info
        jvz = jac.jvec((None, None, V[:1]))
        jt = jac.jtvec(W)
        jt_info = jac.info
        jt3 = jac.jtvec(W[:2], components=True)
    assert jv.shape == (4, n) and jt.shape == (5,) + tuple(grid.vnC) and len(jv_info) == 4 and len(jt_info) == 5
    assert np.array_equal(jv, np.stack(one['jv'])) and np.array_equal(jvz[0], one['jvz'])
    assert np.array_equal(jt, np.stack(one['jt']))
    for c in range(3):
        assert jt3[c].shape == (2,) + tuple(grid.vnC) and np.array_equal(jt3[c][0], one['jt3'][c])
    for a, b in zip(jv_info + jt_info, one['jv_info'] + one['jt_info']):
        same_info(a, b)
    # a second Jacobian on the same device, after the first one has closed its handle
    two = singles()
    assert np.array_equal(two['syn'], one['syn'])
    for key in ('jv', 'jt'):
        assert all(np.array_equal(a, b) for a, b in zip(one[key], two[key]))
