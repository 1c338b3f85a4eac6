"""GPU: the exact transposes of the cubic-spline and magnetic receiver operators (DeviceMG.set_receiver_adjoint(method=,
magnetic=), fields.get_receiver_adjoint) and what optimize.Jacobian / optimize.gradient build on them with adjoint='exact'.

Kernel level against tests/golden/receiver_adjoint.npz (dense operators filled column by column by the reference,
tests/golden/make_receiver_adjoint_golden.py), the adjoint identity against the EXISTING forward kernels on the device, the
adjoint test of the products against the reference-side gaps of the fixture, batched against single products, and
gradient(adjoint='exact') as the derivative of the misfit on a stretched 48 x 40 x 32 grid with off-node receivers."""
import numpy as np
import pytest

from conftest import load_golden, relerr
from test_gpu_jacobian import OPTS, _boundary_edges, _model48

pytestmark = pytest.mark.gpu

CASES = (('el_cubic', 'cubic', False), ('mag_cubic', 'cubic', True), ('mag_linear', 'linear', True))


def _no_datum(grid):
    """A receiver in the outermost cells: outside the trimmed points of every component, its datum is NaN."""
    return (grid.nodes_x[0] + 0.25 * grid.h[0][0], grid.nodes_y[0] + 0.25 * grid.h[1][0], grid.nodes_z[0] + 0.25 * grid.h[2][0],
            30., 20.)


def _grid(em, f, tag):
    return em.TensorMesh([f[f'{tag}_hx'], f[f'{tag}_hy'], f[f'{tag}_hz']], origin=f[f'{tag}_origin'])


def _handle(em, grid, freq):
    from emg3d_amd.solver import DeviceMG
    from emg3d_amd import models
    smu0 = em.fields.FrequencySpec(freq).smu0
    model = em.Model(grid, np.ones(grid.nC), mapping='Conductivity')
    return DeviceMG.from_sigma_volume(grid, *models.sigma_volume(grid, model), smu0=smu0), smu0


@pytest.mark.parametrize('sfx', ['c', 'r'])
@pytest.mark.parametrize('tag', ['A', 'B'])
def test_adjoint_kernels_vs_reference(tag, sfx):
    """P^T w of the three new operators against the dense transposes of the reference (the bound of test_gpu_jacobian.py for
    device-built sources), complex and Laplace domain; exact zeros on the PEC boundary; bit-wise repeatable; accumulate adds;
    a receiver set without data gives a zero source; the stateless entry equals the handle's."""
    import emg3d_amd as em
    f = load_golden("receiver_adjoint.npz")
    grid = _grid(em, f, tag)
    rec = tuple(f[f'{tag}_rec'])
    n = rec[0].size
    w = f[f'w_{sfx}'][:n]
    freq = float(f[f'{tag}_freq']) * (1 if sfx == 'c' else -1)
    bnd = _boundary_edges(grid)
    dev, smu0 = _handle(em, grid, freq)
    assert np.allclose(complex(smu0), complex(f[f'smu0_{sfx}']), rtol=1e-14, atol=0)
    with dev:
        for key, method, magnetic in CASES:
            kw = dict(method=method, magnetic=magnetic, smu0=smu0 if magnetic else None)
            dev.set_receiver_adjoint(rec, w, **kw)
            got = dev.vec_get(dev.SFIELD)
            err = relerr(got, f[f'{tag}_{key}_{sfx}'])
            print(f"receiver adjoint {tag} {key} {sfx}: relerr {err:.2e}")
            assert err < 1e-12
            assert np.all(got[bnd] == 0)
            dev.set_receiver_adjoint(rec, w, **kw)
            assert np.array_equal(dev.vec_get(dev.SFIELD), got)
            dev.set_receiver_adjoint(rec, w, accumulate=True, **kw)
            assert np.array_equal(dev.vec_get(dev.SFIELD), 2 * got)
            # one more receiver without a datum changes nothing; only such receivers: a zero source
            rec2 = tuple(np.r_[c, e] for c, e in zip(rec, _no_datum(grid)))
            dev.set_receiver_adjoint(rec2, np.r_[w, 1.5], **kw)
            assert np.array_equal(dev.vec_get(dev.SFIELD), got)
            dev.set_receiver_adjoint(tuple(np.array([c, c]) for c in _no_datum(grid)), w[:2], **kw)
            assert np.all(dev.vec_get(dev.SFIELD) == 0)
            host = em.fields.get_receiver_adjoint(grid, rec, w, method=method, electric=not magnetic, freq=freq)
            assert isinstance(host, em.Field) and host.dtype == got.dtype and np.array_equal(np.asarray(host), got)


@pytest.mark.parametrize('sfx', ['c', 'r'])
@pytest.mark.parametrize('tag', ['A', 'B'])
def test_adjoint_identity_against_the_forward_kernels(tag, sfx):
    """sum w (P e) == sum (P^T w) e with P the forward receiver kernels that were there before (spline filter + evaluation,
    linear evaluation, k_hfield) and a random field with non-zero boundary values: both sides are sums of a few hundred
    products in float64, compared at 1e-12 of sum |w| |P e|."""
    import emg3d_amd as em
    f = load_golden("receiver_adjoint.npz")
    grid = _grid(em, f, tag)
    rec = tuple(f[f'{tag}_rec'])
    n = rec[0].size
    w = f[f'w_{sfx}'][:n]
    freq = float(f[f'{tag}_freq']) * (1 if sfx == 'c' else -1)
    rng = np.random.default_rng(21)
    e = rng.standard_normal(grid.nE)
    if sfx == 'c':
        e = e + 1j * rng.standard_normal(grid.nE)
    dev, smu0 = _handle(em, grid, freq)
    with dev:
        dev.set_efield(em.Field(grid, e.copy(), freq=freq))
        for key, method, magnetic in CASES:
            kw = dict(method=method, magnetic=magnetic, smu0=smu0 if magnetic else None)
            d = dev.get_receiver_response(rec, **kw)
            dev.set_receiver_adjoint(rec, w, **kw)
            s = dev.vec_get(dev.SFIELD)
            nan = np.isnan(d)
            assert np.array_equal(nan, f[f'{tag}_nan'][CASES.index((key, method, magnetic))])
            wd = np.where(nan, 0, w * d)
            lhs, rhs, scale = np.sum(wd), np.sum(s * e), np.sum(np.abs(wd))
            print(f"adjoint identity {tag} {key} {sfx}: {abs(lhs - rhs) / scale:.2e}")
            assert scale > 0 and abs(lhs - rhs) <= 1e-12 * scale


def _setup_a():
    import emg3d_amd as em
    g = load_golden("gradient.npz")
    j = load_golden("jacobian.npz")
    f = load_golden("receiver_adjoint.npz")
    grid = em.TensorMesh([g['hx'], g['hy'], g['hz']], origin=g['origin'])
    model = em.Model(grid, g['res'])
    kw = dict(OPTS, tol=1e-8, ordering='lex')
    return em, g, j, f, grid, model, kw


def _gap(w, jv, jt, v):
    lhs, rhs = np.real(np.sum(np.conj(w) * jv)), np.sum(jt * v)
    return abs(lhs - rhs) / abs(lhs), lhs, rhs


def test_cubic_exact_is_an_adjoint_pair():
    """receiver_interpolation='cubic', adjoint='exact' on the 12 x 10 x 8 grid: the adjoint gap is within 10 x the gap of the
    reference's own solves with the dense P (the margin test_products_vs_reference gives the linear pair) -- with the
    reference's rule it is 0.74; adjoint='reference' still reproduces gradient(); jtvec(W r) == -gradient(adjoint='exact')."""
    em, g, j, f, grid, model, kw = _setup_a()
    rec, src, freq = tuple(g['rec']), g['src'], float(g['freq'])
    v, w = j['iso_v'].reshape(grid.vnC, order='F'), j['iso_w']
    ref_gap = float(f['gap_cubic_ref'])
    with em.optimize.Jacobian(grid, model, src, freq, rec, receiver_interpolation='cubic', adjoint='exact', **kw) as jac:
        assert relerr(jac.synthetic, g['synthetic']) < 1e-6
        jv = jac.jvec(v)
        jt = jac.jtvec(w)
        assert jac.info['exit'] == 0
        wr = g['weights'] * (jac.synthetic - g['observed'])
        jt_wr = jac.jtvec(wr)
    gap, lhs, rhs = _gap(w, jv, jt, v)
    print(f"cubic exact: Re sum conj(w) J v = {lhs:.10f}, v . J^T w = {rhs:.10f}, gap {gap:.2e} (reference {ref_gap:.2e})")
    assert gap < 10 * ref_gap
    phi, grad, info = em.optimize.gradient(grid, model, src, freq, rec, g['observed'], g['weights'], adjoint='exact', **kw)
    err = relerr(jt_wr, -grad)
    print(f"cubic exact: jtvec(W r) vs -gradient(adjoint='exact') {err:.2e}")
    assert err < 1e-5
    # the default keeps the reference's rule (what test_cubic_receivers_reproduce_the_gradient asserts)
    phi_r, grad_r, _ = em.optimize.gradient(grid, model, src, freq, rec, g['observed'], g['weights'], **kw)
    with em.optimize.Jacobian(grid, model, src, freq, rec, receiver_interpolation='cubic', adjoint='reference', **kw) as jac:
        got = jac.jtvec(g['weights'] * (jac.synthetic - g['observed']))
        gap_r, _, _ = _gap(w, jac.jvec(v), jac.jtvec(w), v)
    assert phi_r == phi
    assert relerr(got, -grad_r) < 1e-5
    assert np.isfinite(gap_r)
    print(f"cubic reference rule: gap {gap_r:.2f}; exact vs reference gradient {relerr(grad, grad_r):.2e}")


@pytest.mark.parametrize('method', ['linear', 'cubic'])
def test_magnetic_receivers_are_an_adjoint_pair(method):
    em, g, j, f, grid, model, kw = _setup_a()
    rec, src, freq = tuple(g['rec']), g['src'], float(g['freq'])
    v, w = j['iso_v'].reshape(grid.vnC, order='F'), j['iso_w']
    ref_gap = float(f[f'gap_mag_{method}_ref'])
    with em.optimize.Jacobian(grid, model, src, freq, rec, receiver_interpolation=method, adjoint='exact', electric=False,
                              **kw) as jac:
        assert jac.synthetic.shape == (rec[0].size,) and np.all(np.isfinite(jac.synthetic))
        if method == 'cubic':      # the magnetic data of gradient.npz (reference: get_h_field + cubic receivers)
            assert relerr(jac.synthetic, g['m_synthetic']) < 1e-5
        jv = jac.jvec(v)
        jt = jac.jtvec(w)
        assert jac.info['exit'] == 0
    gap, lhs, rhs = _gap(w, jv, jt, v)
    print(f"magnetic {method}: Re sum conj(w) J v = {lhs:.10e}, v . J^T w = {rhs:.10e}, gap {gap:.2e} (reference {ref_gap:.2e})")
    assert gap < 10 * ref_gap


def test_batched_exact_products_equal_single_products():
    """nvec = 3 against nvec = 1 for jtvec with the exact cubic adjoint, per selected system: bit for bit."""
    em, grid, s3, src, rec, rng = _model48()
    freq = 1.5
    kw = dict(OPTS, tol=1e-6)
    model = em.Model(grid, *s3, mapping='Conductivity')
    n = rec[0].size
    W = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
    opts = dict(receiver_interpolation='cubic', adjoint='exact', **kw)
    with em.optimize.Jacobian(grid, model, src, freq, rec, **opts) as jac:
        one = [jac.jtvec(x) for x in W]
    with em.optimize.Jacobian(grid, model, src, freq, rec, nvec=3, **opts) as jac:
        got = jac.jtvec(W)
    assert got.shape == (3,) + tuple(grid.vnC)
    assert np.array_equal(got, np.stack(one))


def test_exact_gradient_is_the_derivative_of_the_misfit():
    """-gradient(adjoint='exact') . v against central differences of the misfit (existing solve() + cubic receivers) along a
    random v at steps h and h / 2, on the stretched 48 x 40 x 32 grid with off-node receivers:

        |v . (-grad) - FD(h/2)| <= 2 |FD(h) - FD(h/2)| + noise + 1e-5 |v . (-grad)|,   noise = tol sum_i w_i |r_i| |d_i| / h.

    The first term is the measured truncation error (that of FD(h/2) is a third of the difference for an h^2 law); a solve at
    `tol` leaves the data wrong by ~ tol |d_i|, the misfit by w_i |r_i| tol |d_i|, and the difference quotient by that over
    h.  h = 1e-2 and tol = 1e-10 as in test_jvec_vs_finite_differences_of_solve (there the truncation term was ~1e-5 of the
    derivative); both terms are asserted to be as small as the bound assumes.  How far adjoint='reference' misses the same
    quotient is printed."""
    em, grid, s3, src, rec, rng = _model48()
    freq, h = 1.5, 1e-2
    kw = dict(OPTS, tol=1e-10, maxit=60)
    sig = s3[0]
    v = (rng.standard_normal(grid.nC) * sig * 0.3).reshape(grid.vnC, order='F')
    sfield = em.get_source_field(grid, src, freq)

    def data(step):
        m = em.Model(grid, sig + step * v.ravel('F'), mapping='Conductivity')
        e, info = em.solve(grid, m, sfield, return_info=True, **kw)
        assert info['exit'] == 0
        return em.get_receiver_response(grid, e, rec)
    d0 = data(0.)
    n = d0.size
    observed = d0 * (1 + 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)))
    weights = 1 / np.abs(observed) ** 2

    def phi(step):
        return em.optimize.misfit(data(step), observed, weights)[0]
    fd1 = (phi(h) - phi(-h)) / (2 * h)
    fd2 = (phi(h / 2) - phi(-h / 2)) / h
    model = em.Model(grid, sig, mapping='Conductivity')
    phi0, grad, info = em.optimize.gradient(grid, model, src, freq, rec, observed, weights, adjoint='exact', **kw)
    assert info['forward']['exit'] == 0 and info['backward']['exit'] == 0
    assert abs(phi0 - em.optimize.misfit(d0, observed, weights)[0]) <= 1e-8 * phi0
    dd = np.sum(v * -grad)
    trunc, err = abs(fd1 - fd2), abs(dd - fd2)
    noise = kw['tol'] * np.sum(weights * np.abs(d0 - observed) * np.abs(d0)) / h
    _, grad_r, _ = em.optimize.gradient(grid, model, src, freq, rec, observed, weights, **kw)
    err_r = abs(np.sum(v * -grad_r) - fd2)
    print(f"48x40x32: v.(-grad) = {dd:.8e}, FD(h/2) = {fd2:.8e}; |v.(-grad) - FD(h/2)| / |v.(-grad)| = {err / abs(dd):.2e}, "
          f"truncation {trunc / abs(dd):.2e}, noise {noise / abs(dd):.2e}; adjoint='reference' misses by {err_r / abs(dd):.2e}")
    assert trunc < 1e-4 * abs(dd) and noise < 1e-5 * abs(dd)          # the step and the tolerance are as the bound assumes
    assert err <= 2 * trunc + noise + 1e-5 * abs(dd)
