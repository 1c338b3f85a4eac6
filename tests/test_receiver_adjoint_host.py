"""CPU-only: the transposed receiver operators that tests/golden/receiver_adjoint.npz stores (dense matrices filled column by
column by the reference, tests/golden/make_receiver_adjoint_golden.py) against the oracle's forward operator, a NumPy
restatement of what the device does for the cubic-spline receivers -- scatter of the 64 stencil weights, the transposed
prefilter as D F D^-1, trimmed write -- against the fixture, the identity F^T = D F D^-1 itself, and the argument checks of
the new Python options (raised before the library is touched); and the one rule for the residual / adjoint source
(optimize._adjoint_source) against the two expressions it replaced."""
import numpy as np
import pytest

from conftest import load_golden


def _edge_shapes(vnC):
    nx, ny, nz = (int(n) for n in vnC)
    return ((nx, ny + 1, nz + 1), (nx + 1, ny, nz + 1), (nx + 1, ny + 1, nz))


def _grid(f, tag):
    import emg3d_amd as em
    return em.TensorMesh([f[f'{tag}_hx'], f[f'{tag}_hy'], f[f'{tag}_hz']], origin=f[f'{tag}_origin'])


def transposed_prefilter(c):
    """F_0^T F_1^T F_2^T of the separable B-spline prefilter: per axis D F D^-1, D = diag(1/2, 1, ..., 1, 1/2)."""
    from oracle import interp as oi
    c = np.array(c, copy=True)
    for ax in (2, 1, 0):
        c = np.moveaxis(c, ax, 0)
        if c.shape[0] > 1:
            c[0] *= 2; c[-1] *= 2
            # spline_prefilter filters every axis of its argument: one line at a time along this axis only
            flat = c.reshape(c.shape[0], -1)
            for k in range(flat.shape[1]):
                flat[:, k] = oi.spline_prefilter(flat[:, k])
            c = flat.reshape(c.shape)
            c[0] /= 2; c[-1] /= 2
        c = np.moveaxis(c, 0, ax)
    return c


def cubic_receiver_adjoint(grid, rec, w):
    """NumPy restatement of P^T w for the cubic-spline receivers on the electric components (the forward rules of
    oracle.interp.get_receiver_response: skipped components, linear fallback with fill value 0, NaN receivers)."""
    from oracle import interp as oi
    nodes = (grid.nodes_x, grid.nodes_y, grid.nodes_z)
    centers = (grid.cell_centers_x, grid.cell_centers_y, grid.cell_centers_z)
    shapes = _edge_shapes(grid.vnC)
    n = max(np.atleast_1d(x).size for x in rec)
    xyz = [np.broadcast_to(np.asarray(c, dtype=float), (n,)) for c in rec[:3]]
    fac = np.array([np.broadcast_to(f, (n,)) for f in oi.rotation(*rec[3:])])
    w = np.asarray(w)
    active = [bool(np.any(np.abs(fac[c]) > 1e-10)) for c in range(3)]
    pts = [[(centers[a] if a == c else nodes[a])[1:-1] for a in range(3)] for c in range(3)]
    cubic = [all(p.size >= 4 for p in pts[c]) for c in range(3)]
    coords = {c: np.stack([oi.notaknot_index_coords(pts[c][a], xyz[a]) for a in range(3)]) for c in range(3)
              if active[c] and cubic[c]}
    dead = np.zeros(n, bool)
    for c, co in coords.items():
        for a in range(3):
            dead |= ~((co[a] >= 0) & (co[a] <= pts[c][a].size - 1))
    out = []
    for c in range(3):
        full = np.zeros(shapes[c], dtype=w.dtype)
        if active[c]:
            m = tuple(p.size for p in pts[c])
            coef = np.zeros(m, dtype=w.dtype)
            for r in range(n):
                if dead[r]:
                    continue
                if cubic[c]:
                    idx, wts = [], []
                    for a in range(3):
                        cc = coords[c][a][r]
                        start = int(np.floor(cc)) - 1
                        wts.append(oi._bspline3_weights(cc - np.floor(cc)))
                        ii = []
                        for l in range(4):
                            jj, s2 = start + l, 2 * m[a] - 2
                            if jj < 0:
                                jj = s2 * int(-jj / s2) + jj
                                jj = jj + s2 if jj <= 1 - m[a] else -jj
                            elif jj >= m[a]:
                                jj -= s2 * int(jj / s2)
                                if jj >= m[a]:
                                    jj = s2 - jj
                            ii.append(jj)
                        idx.append(ii)
                    for a0 in range(4):
                        for a1 in range(4):
                            for a2 in range(4):
                                coef[idx[0][a0], idx[1][a1], idx[2][a2]] += w[r] * fac[c][r] * (wts[0][a0] * wts[1][a1] * wts[2][a2])
                else:       # linear, fill value 0: outside this component's points nothing is added
                    if any(not (pts[c][a][0] <= xyz[a][r] <= pts[c][a][-1]) for a in range(3)):
                        continue
                    ii, tt = [], []
                    for a in range(3):
                        p = pts[c][a]
                        i = int(np.clip(np.searchsorted(p, xyz[a][r]) - 1, 0, p.size - 2))
                        ii.append(i); tt.append((xyz[a][r] - p[i]) / (p[i + 1] - p[i]))
                    for a0 in range(2):
                        for a1 in range(2):
                            for a2 in range(2):
                                wg = (tt[0] if a0 else 1 - tt[0]) * (tt[1] if a1 else 1 - tt[1]) * (tt[2] if a2 else 1 - tt[2])
                                coef[ii[0] + a0, ii[1] + a1, ii[2] + a2] += w[r] * fac[c][r] * wg
            if cubic[c]:
                coef = transposed_prefilter(coef)
            full[1:-1, 1:-1, 1:-1] += coef
        out.append(full.ravel('F'))
    return np.concatenate(out)


def test_transposed_prefilter_identity():
    """F^T = D F D^-1 for the mirror-initialised prefilter, n = 2 ... 33 (and F itself is not symmetric)."""
    from oracle import interp as oi
    for n in range(2, 34):
        F = np.stack([oi.spline_prefilter(col) for col in np.eye(n)], axis=1)
        d = np.ones(n); d[0] = d[-1] = 0.5
        assert np.abs(F.T - (d[:, None] * F) / d[None, :]).max() <= 1e-15 * np.abs(F).max(), n
        if n > 2:
            assert np.abs(F - F.T).max() > 0.1


def test_fixture_is_the_transpose_of_the_oracles_receivers():
    """sum w (P e) == sum (P^T w) e on grid B (linear fallback of the y-component, four-point axes, one NaN receiver) with the
    oracle's get_receiver_response as P and a random field; both sides are sums of a few hundred products."""
    from oracle import interp as oi
    f = load_golden("receiver_adjoint.npz")
    grid = _grid(f, 'B')
    rec = tuple(f['B_rec'])
    n = rec[0].size
    rng = np.random.default_rng(8)
    e = rng.standard_normal(grid.nE) + 1j * rng.standard_normal(grid.nE)
    d = oi.get_receiver_response(grid.h, grid.origin, e, rec)
    nan = np.isnan(d)
    assert np.array_equal(nan, f['B_nan'][0]) and list(np.flatnonzero(nan)) == [3]
    for key, w in (('B_el_cubic_c', f['w_c'][:n]), ('B_el_cubic_r', f['w_r'][:n])):
        lhs = np.sum(np.where(nan, 0, w * d))
        rhs = np.sum(f[key] * e)
        scale = np.sum(np.abs(np.where(nan, 0, w * d)))
        assert abs(lhs - rhs) <= 1e-12 * scale, (key, abs(lhs - rhs) / scale)


@pytest.mark.parametrize('tag', ['A', 'B'])
def test_numpy_restatement_reproduces_the_fixture(tag):
    f = load_golden("receiver_adjoint.npz")
    grid = _grid(f, tag)
    rec = tuple(f[f'{tag}_rec'])
    n = rec[0].size
    for sfx in ('c', 'r'):
        want = f[f'{tag}_el_cubic_{sfx}']
        got = cubic_receiver_adjoint(grid, rec, f[f'w_{sfx}'][:n])
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"restatement {tag} {sfx}: {err:.2e}")
        assert err < 1e-12


def test_fixture_gaps_and_shapes():
    f = load_golden("receiver_adjoint.npz")
    for key in ('gap_cubic_ref', 'gap_mag_cubic_ref', 'gap_mag_linear_ref'):
        assert 0 < float(f[key]) < 1e-4
    assert f['A_nan'].sum() == 0 and f['B_nan'][0].sum() == 1
    for tag in ('A', 'B'):
        grid = _grid(f, tag)
        for key in ('el_cubic', 'mag_cubic', 'mag_linear'):
            assert f[f'{tag}_{key}_c'].shape == (grid.nE,) and np.iscomplexobj(f[f'{tag}_{key}_c'])
            assert f[f'{tag}_{key}_r'].shape == (grid.nE,) and not np.iscomplexobj(f[f'{tag}_{key}_r'])
            assert np.abs(f[f'{tag}_{key}_c']).max() > 0


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the HIP library fails the test."""
    from emg3d_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "_open", boom)


def test_argument_errors_come_before_the_library(no_library):
    import emg3d_amd as em
    g = load_golden("gradient.npz")
    grid = em.TensorMesh([g['hx'], g['hy'], g['hz']], origin=g['origin'])
    rec, src, freq = tuple(g['rec']), g['src'], float(g['freq'])
    model = em.Model(grid, g['res'])
    with pytest.raises(ValueError, match="adjoint"):
        em.optimize.Jacobian(grid, model, src, freq, rec, adjoint='transpose')
    with pytest.raises(NotImplementedError, match="magnetic"):
        em.optimize.Jacobian(grid, model, src, freq, rec, electric=False, receiver_interpolation='cubic')
    jac = em.optimize.Jacobian(grid, model, src, freq, rec, electric=False, adjoint='exact')
    assert jac.adjoint == 'exact' and jac.electric is False and jac.receiver_interpolation == 'linear'
    jac = em.optimize.Jacobian(grid, model, src, freq, rec, receiver_interpolation='cubic', electric=False, adjoint='exact')
    with pytest.raises(RuntimeError, match="closed"):
        jac.jtvec(np.zeros(rec[0].size))
    assert em.optimize.Jacobian(grid, model, src, freq, rec).adjoint == 'reference'
    with pytest.raises(ValueError, match="adjoint"):
        em.optimize.gradient(grid, model, src, freq, rec, g['observed'], adjoint='both')
    with pytest.raises(ValueError, match="method"):
        em.fields.get_receiver_adjoint(grid, rec, np.ones(rec[0].size), method='nearest')
    with pytest.raises(ValueError, match="freq"):
        em.fields.get_receiver_adjoint(grid, rec, np.ones(rec[0].size), electric=False)
    with pytest.raises(ValueError, match="rec"):
        em.fields.get_receiver_adjoint(grid, rec[:3], np.ones(rec[0].size))
    with pytest.raises(TypeError, match="real"):
        em.fields.get_receiver_adjoint(grid, rec, 1j * np.ones(rec[0].size), freq=-1.0)


class _SourceRecorder:
    """Stands in for a DeviceMG: keeps what ``optimize._adjoint_source`` asks of it."""

    def __init__(self):
        self.sources, self.adjoints = [], []

    def set_source(self, src, smu0, strength=0, accumulate=False, electric=True):
        self.sources.append((int(src[0]), strength, accumulate, electric))

    def set_receiver_adjoint(self, rec, w, **kwargs):
        self.adjoints.append((np.array(w), kwargs))


@pytest.mark.parametrize('electric', [True, False], ids=['electric', 'magnetic'])
@pytest.mark.parametrize('freq', [1.5, -1.2], ids=['c128', 'f64'])
def test_adjoint_source_rule_equals_both_expressions_it_replaced(freq, electric):
    """The reference rule of optimize._adjoint_source -- strengths ``conj(w r) / s mu_0`` (magnetic: ``/ s mu_0`` again), zero
    strengths skipped -- gives bit for bit (np.array_equal; the sign of a zero component is not seen) the strengths and the skip
    set of the two expressions the entry points used before: ``conj(r) conj(w) / s mu_0`` with the tests ``isnan(r)`` and
    ``strength == 0`` (gradient, survey_gradient), and ``where(isnan(w r), 0, conj(w r)) / s mu_0`` with the test ``== 0`` before
    the division (the Jacobians; electric receivers only there).  Data: random residuals (complex for a frequency, real for a
    Laplace value) with purely real, purely imaginary, zero and one NaN entry; real weights with zeros and, for the frequency,
    one complex weight, 2 + 0.5j: its components are powers of two, so its product with a residual rounds once whether or not
    the vectorised array product fuses multiply and add.  (For a general complex weight NumPy's array and scalar products differ
    in the last bit on CPUs with FMA, so the two earlier expressions did; the weights of a least-squares misfit are real.)"""
    import emg3d_amd as em
    from emg3d_amd import optimize
    n = 4000
    rng = np.random.default_rng(17)
    smu0 = em.fields.FrequencySpec(freq).smu0
    r = rng.standard_normal(n) * 10.0 ** rng.uniform(-14, -8, n)
    w = rng.uniform(0.5, 2, n) * 10.0 ** rng.uniform(20, 26, n)
    if freq > 0:
        r = r + 1j * rng.standard_normal(n) * 10.0 ** rng.uniform(-14, -8, n)
        r[0:40] = r[0:40].real
        r[40:80] = 1j * r[40:80].imag
        w = w.astype(complex)
        w[100] = 2 + 0.5j
    r[80:120:3] = 0
    r[7] = np.nan
    w[60:400:7] = 0
    rec = (np.arange(n, dtype=float),) + (np.zeros(n),) * 4        # (the x-coordinate names the receiver)

    # the rule as gradient() and survey_gradient() had it
    old_a = {}
    for i in range(n):
        if np.isnan(r[i]):
            continue
        st = r[i].conj() * np.conj(w[i]) / smu0
        if not electric:
            st = st / smu0
        if st == 0:
            continue
        old_a[i] = st
    # the rule as Jacobian and SurveyJacobian had it (electric receivers)
    cw_jac = np.where(np.isnan(w * r), 0, np.conj(w * r))
    old_b = {i: cw_jac[i] / smu0 for i in range(n) if not cw_jac[i] == 0}

    cw = np.conj(w * r)
    cw = np.where(np.isnan(cw), 0, cw)
    dev = _SourceRecorder()
    assert optimize._adjoint_source(dev, rec, smu0, cw, method='cubic', exact=False, electric=electric)
    got = {k: st for k, st, _, _ in dev.sources}
    assert not dev.adjoints and len(got) == len(dev.sources) and 1000 < len(got) < n - 50
    assert [acc for _, _, acc, _ in dev.sources] == [False] + [True] * (len(got) - 1)
    assert all(el is electric for _, _, _, el in dev.sources)
    assert 7 not in got and 100 in got and 82 in got and 80 not in got and 81 not in got
    keys = sorted(got)
    assert keys == sorted(old_a)
    assert np.array_equal(np.array([got[k] for k in keys]), np.array([old_a[k] for k in keys]))
    if electric:
        assert keys == sorted(old_b)
        assert np.array_equal(np.array([got[k] for k in keys]), np.array([old_b[k] for k in keys]))
    # nothing usable: no call, False; exact or linear receivers: one set_receiver_adjoint with cw as it is
    none = _SourceRecorder()
    assert not optimize._adjoint_source(none, rec, smu0, np.zeros(n), method='cubic', exact=False, electric=electric)
    assert not optimize._adjoint_source(none, rec, smu0, np.zeros(n), method='cubic', exact=True, electric=electric)
    assert not none.sources and not none.adjoints
    for method, exact in (('cubic', True), ('linear', False)):
        one = _SourceRecorder()
        assert optimize._adjoint_source(one, rec, smu0, cw, method=method, exact=exact, electric=electric)
        assert not one.sources and len(one.adjoints) == 1
        assert np.array_equal(one.adjoints[0][0], cw)
        assert one.adjoints[0][1] == dict(method=method, magnetic=not electric, smu0=smu0)
