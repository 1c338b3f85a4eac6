"""GPU: explicit rows of J -- emg3d_mg_sens_rows (k_sens_rows) through the C ABI and DeviceMG.sens_rows against the longdouble host
restatement, on the model grid against the device's own transpose of volume averaging, and
optimize.SurveyJacobian.sensitivity_rows against the rows jtvec gives one datum at a time and against jvec.

Tolerances (tests/test_sensitivity_rows_host.py): kernel level 4 x the float64-versus-longdouble deviation of the restatement
recorded on the CPU, end to end twice that; every row relative to its own largest magnitude."""
import numpy as np
import pytest

from conftest import load_golden
from test_gpu_sensitivity_diagonal import FREQS, OPTS, SOURCES, _handle, _survey, _upload
from test_sensitivity_diagonal_host import NSYS, SHAPES, TOL_KERNEL, _deviation
from test_sensitivity_rows_host import (TOL_ROWS_KERNEL, TOL_ROWS_SURVEY, host_rows, row_deviation, row_identity_gaps, rows_case)

pytestmark = pytest.mark.gpu


def _align(nbytes):
    return (max(nbytes, 8) + 255) // 256 * 256


def _raw(dev, smu0, use_fwd, use_adj, split, on_model, out, fwd_bvec=0):
    a = complex(smu0)
    uf, ua = (np.ascontiguousarray(u, dtype=np.int32) for u in (use_fwd, use_adj))
    return dev._lib.emg3d_mg_sens_rows(dev._h, fwd_bvec, a.real, a.imag, uf.ctypes.data, ua.ctypes.data, int(split), int(on_model),
                                       out.ctypes.data)


# ---- 1. the kernel through the C ABI --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsys", NSYS)
@pytest.mark.parametrize("real", [False, True], ids=["c128", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_sens_rows_vs_longdouble(shape, real, nsys):
    """Both forms against the longdouble restatement, row by row in the contracted order, within TOL_ROWS_KERNEL of the row's largest
    magnitude.  The systems that are masked out hold NaN fields and leave no trace; a second call with fewer pairs returns only its
    own rows; device_bytes grows by exactly the row buffer at the first call and not again for a smaller one; sum W |rows|^2 is what
    sens_acc_add puts into the accumulators of the same handle, within that module's TOL_KERNEL; the errors are -2 and -7."""
    import emg3d_amd as em
    case = rows_case(shape, real, nsys)
    grid, smu0, W = case['grid'], case['smu0'], case['W']
    use = (case['use_fwd'], case['use_adj'])
    pairs, nC, npart = len(case['pairs']), int(grid.nC), 1 if real else 2
    want3, want1 = host_rows(case, True, dtype=np.longdouble), host_rows(case, dtype=np.longdouble)
    with _handle(em, grid, smu0, nsys) as dev:
        assert dev.nsys == nsys
        _upload(dev, case)
        lib = dev._lib
        assert lib.emg3d_mg_sens_rows_count(use[0].ctypes.data, use[1].ctypes.data, nsys) == pairs
        out = np.full(pairs * 3 * npart * nC, np.nan)
        before = dev.device_bytes
        # a bad vector (the live field included), empty masks, no model grid: nothing is allocated
        for bad in (-2, -1, 1, 9):
            assert _raw(dev, smu0, *use, 0, 0, out, fwd_bvec=bad) == -2
        none = np.zeros(nsys, dtype=np.int32)
        assert _raw(dev, smu0, none, use[1], 0, 0, out) == -2 and _raw(dev, smu0, use[0], none, 1, 0, out) == -2
        assert _raw(dev, smu0, *use, 0, 1, out) == -7 and _raw(dev, smu0, *use, 1, 1, out) == -7
        with pytest.raises(ValueError):
            dev.sens_rows(dev.EFIELD, smu0, *use)
        with pytest.raises(ValueError):
            dev.sens_rows(0, smu0, none, use[1])
        with pytest.raises(ValueError):
            dev.sens_rows(0, smu0, use[0][:-1], use[1])
        with pytest.raises(RuntimeError, match="model grid"):
            dev.sens_rows(0, smu0, *use, model_grid=True)
        assert dev.device_bytes == before and np.isnan(out).all()
        # the largest call first: the split form
        got3 = dev.sens_rows(0, smu0, *use, components=True)
        grown = dev.device_bytes - before
        assert grown == _align(pairs * 3 * npart * nC * 8)
        got1 = dev.sens_rows(0, smu0, *use)
        assert dev.device_bytes - before == grown
        assert got3.shape == (pairs, 3) + shape and got1.shape == (pairs, 1) + shape
        assert got3.dtype == got1.dtype == (np.float64 if real else np.complex128) and got1[0, 0].flags.f_contiguous
        assert np.isfinite(got3.real).all() and np.isfinite(got3.imag).all() and np.isfinite(got1.real).all()
        e3, e1 = row_deviation(got3, want3), row_deviation(got1, want1)
        print(f"{shape} {'f64' if real else 'c128'} nsys {nsys}: {pairs} rows, one {e1:.2e}, split {e3:.2e} "
              f"(tolerance {TOL_ROWS_KERNEL:.1e})")
        assert e1 <= TOL_ROWS_KERNEL and e3 <= TOL_ROWS_KERNEL
        # the planar layout of the C ABI: [p][dir][part][cell]
        assert _raw(dev, smu0, *use, 1, 0, out) == 0
        planes = out.reshape(pairs, 3, npart, nC)
        flat3 = np.stack([[g.ravel(order='F') for g in row] for row in got3])
        assert np.array_equal(planes[:, :, 0], flat3.real) and (real or np.array_equal(planes[:, :, 1], flat3.imag))
        # fewer pairs: the last active system of each mask alone is the last row, and nothing else comes back
        last_f, last_a = np.zeros(nsys, dtype=np.int32), np.zeros(nsys, dtype=np.int32)
        last_f[case['jf'][-1]] = last_a[case['ia'][-1]] = 1
        few = dev.sens_rows(0, smu0, last_f, last_a, components=True)
        assert few.shape == (1, 3) + shape and np.array_equal(few[0], got3[-1])
        assert np.array_equal(dev.sens_rows(0, smu0, *use), got1) and dev.device_bytes - before == grown
        # the diagonal of the same handle: the same rows, squared, weighted and added in the same order
        dev.grad_acc_reset()
        dev.grad_acc3_reset()
        dev.sens_acc_add(0, smu0, *use, W)
        dev.sens_acc_add(0, smu0, *use, W, split=True)
        acc1, acc3 = dev.grad_acc_get(), dev.grad_acc3_get()
        sum1, sum3 = np.zeros(shape), [np.zeros(shape) for _ in range(3)]
        for p, (ba, bf) in enumerate(case['pairs']):
            if W[ba, bf] != 0:
                sum1 = sum1 + W[ba, bf] * (got1[p, 0].real ** 2 + got1[p, 0].imag ** 2)
                sum3 = [s + W[ba, bf] * (r.real ** 2 + r.imag ** 2) for s, r in zip(sum3, got3[p])]
        errs = [_deviation(sum1.ravel(order='F'), acc1)] + [_deviation(s.ravel(order='F'), a) for s, a in zip(sum3, acc3)]
        print("    sum W |rows|^2 vs sens_acc_add: " + " ".join(f"{e:.2e}" for e in errs) + f" (tolerance {TOL_KERNEL:.1e})")
        assert acc1.max() > 0 and all(e <= TOL_KERNEL for e in errs)


@pytest.mark.parametrize("real", [False, True], ids=["c128", "f64"])
def test_row_is_the_transpose_of_the_jvec_source(real):
    """The identity of tests/test_sensitivity_rows_host.py, per pair and direction, with C(v) from the device's
    maps.cellaverages2edges."""
    from emg3d_amd import maps

    def cells2edges(v3, vol):
        nx, ny, nz = vol.shape
        outs = [np.zeros(s, order='F') for s in ((nx, ny + 1, nz + 1), (nx + 1, ny, nz + 1), (nx + 1, ny + 1, nz))]
        maps.cellaverages2edges(*(np.asfortranarray(v) for v in v3), np.asfortranarray(vol), *outs)
        return outs
    for shape in SHAPES[:2]:
        case = rows_case(shape, real, 3)
        v = np.random.default_rng(3).standard_normal(shape)
        gap = row_identity_gaps(case, v, cells2edges)
        print(f"transpose identity {shape} {'f64' if real else 'c128'}: {gap:.2e}")
        assert gap < 1e-13


# ---- 2. the rows on the model grid ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('freq', [1.5, -1.5], ids=['c128', 'f64'])
def test_planes_on_the_model_grid_bitwise(freq):
    """12 x 10 x 8 -> 7 x 5 x 4 ('unaligned' of tests/test_model_grid_host.py), three systems with a hole in each mask, random
    factors per direction: every plane that comes back on the model grid is, bit for bit, Q_dir * maps.volume_average_adjoint(F_dir *
    plane) of the computational-grid row of the same handle (the launch of grad_acc(3)_get_model, which maps.volume_average_adjoint
    runs too).  The summed form needs shared factors: -2 on this handle, and the same identity with the factors of direction x on a
    handle that shares them.  <Q (.) A^T (F (.) row), v> == <row, F (.) A (Q (.) v)> with maps.grid2grid(..., 'volume').  -7 before
    the factors are there; device_bytes grows by exactly the second buffer."""
    import emg3d_amd as em
    from emg3d_amd import models
    from emg3d_amd.solver import DeviceMG
    from test_model_grid_host import grid_pairs, volumes
    g = load_golden("survey_jacobian.npz")
    model_grid, grid = grid_pairs(em, ['unaligned'])['unaligned']
    vol = volumes(grid)
    nC, nM, nsys = int(grid.nC), int(model_grid.nC), 3
    model = em.Model(grid, g['tri_sig_x'], g['tri_sig_y'], g['tri_sig_z'], mapping='Conductivity')
    spec = em.fields.FrequencySpec(freq)
    real = freq < 0
    npart = 1 if real else 2
    rng = np.random.default_rng(57)
    fields = [[rng.standard_normal(grid.nE) if real else rng.standard_normal(grid.nE) + 1j * rng.standard_normal(grid.nE)
               for _ in range(nsys)] for _ in range(2)]
    use_fwd, use_adj = np.array([1, 0, 1], dtype=np.int32), np.array([0, 1, 1], dtype=np.int32)
    F = tuple(np.asfortranarray(rng.standard_normal(grid.vnC)) for _ in range(3))
    Q = tuple(np.asfortranarray(rng.standard_normal(model_grid.vnC)) for _ in range(3))
    v = np.asfortranarray(rng.standard_normal(model_grid.vnC))

    def on_model(plane, c):
        return Q[c] * em.maps.volume_average_adjoint(model_grid.nodes_x, model_grid.nodes_y, model_grid.nodes_z, grid.nodes_x,
                                                     grid.nodes_y, grid.nodes_z, np.asfortranarray(F[c] * plane), vol)

    def parts(row):
        return (row,) if real else (row.real, row.imag)
    for shared in (False, True):
        with DeviceMG.from_model(grid, models.model_parts(grid, model, raw=True), spec) as dev:
            dev.set_batch(nsys)
            dev.bvec_alloc(1)
            for b in range(nsys):
                dev.select(b)
                dev.set_efield(em.Field(grid, fields[1][b].copy(), freq=freq))
                dev.bvec_set(0, b, fields[0][b])
            split = not shared
            ndir = 3 if split else 1
            out = np.full(4 * ndir * npart * nM, np.nan)
            assert _raw(dev, spec.smu0, use_fwd, use_adj, split, 1, out) == -7
            dev.set_model_grid(model_grid)
            assert _raw(dev, spec.smu0, use_fwd, use_adj, split, 1, out) == -7          # linked, but no factors yet
            with pytest.raises(RuntimeError, match="model grid"):
                dev.sens_rows(0, spec.smu0, use_fwd, use_adj, components=split, model_grid=True)
            dev.set_regrid_factors((F[0],) * 3 if shared else F, (Q[0],) * 3 if shared else Q)
            rows = dev.sens_rows(0, spec.smu0, use_fwd, use_adj, components=split)
            before = dev.device_bytes
            if not shared:
                assert _raw(dev, spec.smu0, use_fwd, use_adj, 0, 1, out) == -2         # the summed form with factors per direction
                with pytest.raises(ValueError):
                    dev.sens_rows(0, spec.smu0, use_fwd, use_adj, model_grid=True)
                assert dev.device_bytes == before and np.isnan(out).all()
            got = dev.sens_rows(0, spec.smu0, use_fwd, use_adj, components=split, model_grid=True)
            assert dev.device_bytes - before == _align(4 * ndir * npart * nM * 8)
            assert got.shape == (4, ndir) + tuple(model_grid.vnC) and got.dtype == rows.dtype and np.abs(got).max() > 0
            for p in range(4):
                for c in range(ndir):
                    for a, b in zip(parts(got[p, c]), parts(rows[p, c])):
                        assert np.array_equal(a, on_model(b, c)), (shared, p, c)
            # the computational-grid rows are still what the handle returns, and a second read-back repeats
            assert np.array_equal(dev.sens_rows(0, spec.smu0, use_fwd, use_adj, components=split), rows)
            assert np.array_equal(dev.sens_rows(0, spec.smu0, use_fwd, use_adj, components=split, model_grid=True), got)
            # the adjoint identity of the regridding, A v by the device's volume averaging
            for c in range(ndir):
                Av = F[c] * em.maps.grid2grid(model_grid, np.asfortranarray(Q[c] * v), grid, method='volume')
                for a, b in zip(parts(got[0, c]), parts(rows[0, c])):
                    lhs, rhs = np.sum(a * v), np.sum(b * Av)
                    assert abs(lhs - rhs) <= 1e-13 * np.sum(np.abs(b * Av)) and abs(rhs) > 0


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------
def _jtvec_rows(sj, j, recs, srcs, components=False, mapped=False):
    """jtvec(e_d) + 1j * jtvec(1j * e_d) on the open SurveyJacobian for d = (s, j, r), s in srcs, r in recs -> ({(s, k): row or
    the three rows}, jtvec calls)."""
    shape = (sj.n_src, sj.n_freq, sj.n_rec)
    out, calls = {}, 0
    for s in srcs:
        for k, r in enumerate(recs):
            w = np.zeros(shape, dtype=np.complex128)
            w[s, j, r] = 1.0
            re = sj.jtvec(w, components=components, mapped=mapped)
            calls += 1
            if sj.freqs[j] < 0:
                out[s, k] = re
                continue
            w[s, j, r] = 1j
            im = sj.jtvec(w, components=components, mapped=mapped)
            calls += 1
            out[s, k] = tuple(a + 1j * b for a, b in zip(re, im)) if components else re + 1j * im
    return out, calls


def _worst(got, want, components=False, what=""):
    """Largest deviation of a row of ``want`` (``_jtvec_rows``) from ``got`` (``sensitivity_rows``), relative to the row's largest
    magnitude; the shares of the real and of the imaginary parts are printed beside it."""
    worst = re = im = 0.0
    for (s, k), row in want.items():
        for g, w in zip(got if components else (got,), row if components else (row,)):
            assert g[s, k].shape == w.shape and np.abs(w).max() > 0
            worst = max(worst, float(np.abs(g[s, k] - w).max() / np.abs(w).max()))
            re = max(re, float(np.abs(g[s, k].real - w.real).max() / np.abs(w).max()))
            im = max(im, float(np.abs(g[s, k].imag - w.imag).max() / np.abs(w).max()))
    print(f"{what}: rows vs jtvec rows {worst:.2e} (real parts {re:.2e}, imaginary parts {im:.2e}; tolerance {TOL_ROWS_SURVEY:.1e})")
    return worst


# Why sensitivity_rows solves twice per receiver at a frequency.  The real part of one solve's product equals jtvec(e_d) BIT FOR
# BIT -- the same solve, the same products.  jtvec(1j * e_d) is ANOTHER solve: its right-hand side is -1j times the receiver's
# adjoint source, and the multigrid solve of a rotated right-hand side is not the rotated solution bit for bit (a complex product
# rounds otherwise when its operand's parts are swapped); the unit roundoff differences come out of the solve amplified to 1e-14 ..
# 3e-13 of a row's largest magnitude (8 x 8 x 8, tol = 1e-8: 1.02e-13 for source 2 / receiver 1; -jtvec(-1j * e_d) equals
# jtvec(1j * e_d) bit for bit, so it is the rotation, not the repetition), far above TOL_ROWS_SURVEY = 4.5e-15.  So the rows take
# their imaginary part from that second solve too, 2 n_rec solves per frequency instead of 2 n_src n_rec, and both parts are the
# products of jtvec.


@pytest.mark.parametrize("j", [0, 1], ids=["1Hz", "s=2"])
def test_rows_equal_the_rows_of_jtvec(j):
    """8 x 8 x 8 stretched, 3 sources x (1 Hz, s = 2) x 4 receivers, batch = 2 (receiver chunks of 2 + 2, source chunks of 2 + 1):
    all 12 rows of a frequency against jtvec(e_d) + 1j * jtvec(1j * e_d) on the same open object (24 jtvec calls at 1 Hz, 12 at s =
    2).  The receiver-field solves are the solves jtvec(e_d) and jtvec(1j * e_d) run, so both sides start from the same fields:
    TOL_ROWS_SURVEY.  rows_info_imag holds the infos of the second solves (None in the Laplace domain)."""
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = em.Model(grid, sig, mapping='Conductivity')
    vnC = tuple(int(n) for n in grid.vnC)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, tol=1e-8, **OPTS) as sj:
        assert sj.rows_info is None
        got = sj.sensitivity_rows(j)
        info = sj.rows_info
        assert got.shape == (3, 4) + vnC and got.dtype == (np.complex128 if FREQS[j] > 0 else np.float64)
        assert got[1, 2].flags.f_contiguous and np.isfinite(got.real).all() and np.isfinite(got.imag).all()
        assert len(info) == 4 and all(x is not None and x['exit'] == 0 for x in info)
        if FREQS[j] > 0:
            assert len(sj.rows_info_imag) == 4 and all(x is not None and x['exit'] == 0 for x in sj.rows_info_imag)
        else:
            assert sj.rows_info_imag is None
        # deterministic, and a subset in another order is the same rows
        again = sj.sensitivity_rows(j, receivers=[3, 1])
        assert again.shape == (3, 2) + vnC and np.array_equal(again[:, 0], got[:, 3]) and np.array_equal(again[:, 1], got[:, 1])
        assert len(sj.rows_info) == 2
        want, calls = _jtvec_rows(sj, j, range(4), range(3))
    assert calls == (24 if FREQS[j] > 0 else 12)
    assert _worst(got, want, what=f"freq {FREQS[j]}") <= TOL_ROWS_SURVEY


TRI_CASES = {"1Hz-components": (0, dict(components=True)), "1Hz-components-mapped": (0, dict(components=True, mapped=True)),
             "1Hz-mapped": (0, dict(mapped=True)), "s=2-components-mapped": (1, dict(components=True, mapped=True)),
             "s=2": (1, dict()), "s=2-mapped": (1, dict(mapped=True))}


@pytest.mark.parametrize("name", list(TRI_CASES))
def test_components_and_mapped_on_a_triaxial_model(name):
    """Tri-axial 'LgConductivity' model, receivers [3, 1] (not ascending), sources 0 and 2: per direction, per direction mapped, and
    the mapped sum, against the same jtvec products."""
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = em.Model(grid, np.log10(sig), np.log10(1.5 * sig), np.log10(0.6 * sig), mapping='LgConductivity')
    recs, srcs = [3, 1], [0, 2]
    j, kw = TRI_CASES[name]
    comp = kw.get('components', False)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, tol=1e-8, **OPTS) as sj:
        got = sj.sensitivity_rows(j, receivers=recs, **kw)
        want, _ = _jtvec_rows(sj, j, recs, srcs, **kw)
        with pytest.raises(TypeError):
            sj.sensitivity_rows(0, mapped=1)
    assert (len(got) == 3 and all(g.shape == (3, 2) + tuple(grid.vnC) for g in got)) if comp else got.shape == (3, 2) + tuple(grid.vnC)
    assert _worst(got, want, comp, what=f"tri-axial {name}") <= TOL_ROWS_SURVEY


@pytest.mark.parametrize("j", [0, 1], ids=["1Hz", "s=2"])
@pytest.mark.parametrize("kind", ["magnetic", "reference-cubic", "linear"])
def test_other_receivers_and_adjoint_rules(kind, j):
    """Magnetic receivers, the reference's adjoint rule with cubic receivers, linear receivers; receivers [2, 0, 3], source 1."""
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = em.Model(grid, sig, mapping='Conductivity')
    kw = dict(magnetic=dict(electric=False), linear=dict(receiver_interpolation='linear'),
              **{'reference-cubic': dict(adjoint='reference', receiver_interpolation='cubic')})[kind]
    recs, srcs = [2, 0, 3], [1]
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, tol=1e-8, **kw, **OPTS) as sj:
        got = sj.sensitivity_rows(j, receivers=recs)
        want, _ = _jtvec_rows(sj, j, recs, srcs)
    assert _worst(got, want, what=f"{kind} freq {FREQS[j]}") <= TOL_ROWS_SURVEY


def test_set_model_bitwise_and_refusals():
    """After set_model the rows are those of a new object bit for bit, and the device buffers do not grow again; bad arguments and a
    closed object refuse."""
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = em.Model(grid, sig, mapping='Conductivity')
    model2 = em.Model(grid, sig * 10 ** rng.uniform(-0.2, 0.2, grid.nC), mapping='Conductivity')
    kw = dict(tol=1e-8, **OPTS)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, **kw) as sj:
        first = [sj.sensitivity_rows(j, components=True) for j in range(2)]
        before = sj.device_bytes
        sj.set_model(model2)
        assert sj.rows_info is None
        after = [sj.sensitivity_rows(j, components=True) for j in range(2)]
        assert sj.device_bytes == before
        assert not np.array_equal(after[0][0], first[0][0])
        for bad in (2, -1):
            with pytest.raises(ValueError, match="i_freq"):
                sj.sensitivity_rows(bad)
        with pytest.raises(ValueError, match="receivers"):
            sj.sensitivity_rows(0, receivers=[4])
    with pytest.raises(RuntimeError, match="closed"):
        sj.sensitivity_rows(0)
    with em.optimize.SurveyJacobian(grid, model2, SOURCES, FREQS, rec, batch=2, **kw) as sj:
        for j in range(2):
            assert all(np.array_equal(a, b) for a, b in zip(sj.sensitivity_rows(j, components=True), after[j]))


@pytest.mark.parametrize("method", ["cubic", "linear"])
def test_jvec_is_rows_times_v(method):
    """The 12 x 10 x 8 grid, sources, frequencies and receivers of tests/golden/survey_jacobian.npz, isotropic model, tol = 1e-8:
    jvec(v)[s, j, r] against sum_j rows[s, r][j] v[j], as the gap |sum conj(w) (J v) - sum conj(w) (rows . v)| / |lhs| below 10 x the
    fixture's reference-side adjoint gap for these receivers -- the margin tests/test_gpu_survey_jacobian.py uses for the adjoint
    identity at this tolerance: the rows come from adjoint solves, J v from forward ones."""
    import emg3d_amd as em
    from test_gpu_jacobian import OPTS as JOPTS
    g = load_golden("survey_jacobian.npz")
    grid = em.TensorMesh([g['hx'], g['hy'], g['hz']], origin=g['origin'])
    model = em.Model(grid, g['iso_sig_x'], g['iso_sig_y'], g['iso_sig_z'], mapping='Conductivity')
    rec = tuple(g['rec'])
    vnC = tuple(int(n) for n in grid.vnC)
    v, w = g['iso_v'].reshape(vnC, order='F'), g['iso_w']
    ref_gap = float(g['adj_gap_cubic' if method == 'cubic' else 'adj_gap_linear'])
    kw = dict(JOPTS, tol=1e-8, receiver_interpolation=method, adjoint='exact')
    with em.optimize.SurveyJacobian(grid, model, g['sources'], g['freqs'], rec, batch=2, **kw) as sj:
        jv = sj.jvec(v)
        rv = np.empty_like(jv)
        for j in range(sj.n_freq):
            rows = sj.sensitivity_rows(j)
            assert all(x['exit'] == 0 for x in sj.rows_info)
            rv[:, j] = np.einsum('skxyz,xyz->sk', rows, v)
    lhs, rhs = np.sum(np.conj(w) * jv), np.sum(np.conj(w) * rv)
    gap = abs(lhs - rhs) / abs(lhs)
    worst = np.abs(jv - rv).max() / np.abs(jv).max()
    print(f"{method}: J v vs rows . v, gap {gap:.2e} (reference gap {ref_gap:.2e}), largest datum deviation {worst:.2e}")
    assert np.abs(jv).max() > 0 and gap < 10 * ref_gap


MODEL_GRID_CASES = {"1.5Hz": (0, False), "s=1.2": (1, False), "1.5Hz-components": (0, True), "s=1.2-components": (1, True)}


@pytest.mark.parametrize("name", list(MODEL_GRID_CASES))
@pytest.mark.parametrize('kind', ['Resistivity', 'Conductivity-tri'])
def test_rows_on_a_model_grid_equal_the_rows_of_jtvec(kind, name):
    """The small case of tests/test_gpu_model_grid.py (12 x 10 x 8 from 7 x 5 x 4, 3 sources x (1.5 Hz, s = 1.2), batch = 2, tol =
    1e-6): sensitivity_rows(mapped=True) against the jtvec(mapped=True) pairs of unit data, receivers [2, 0], sources 0 and 2, within
    TOL_ROWS_SURVEY; the rows have the model grid's shape; mapped=False is refused."""
    import emg3d_amd as em
    from test_gpu_jacobian import OPTS as JOPTS
    from test_gpu_model_grid import SOURCES as MSOURCES, _models
    from test_model_grid_host import grid_pairs
    g = load_golden("survey_jacobian.npz")
    model_grid, grid = grid_pairs(em, ['unaligned'])['unaligned']
    model = _models(em, model_grid, kind)
    rec = tuple(g['rec'])
    vnM = tuple(int(n) for n in model_grid.vnC)
    recs, srcs = [2, 0], [0, 2]
    j, comp = MODEL_GRID_CASES[name]
    kw = dict(JOPTS, tol=1e-6, batch=2, model_grid=model_grid)
    with em.optimize.SurveyJacobian(grid, model, MSOURCES, [1.5, -1.2], rec, **kw) as sj:
        with pytest.raises(ValueError, match="model grid"):
            sj.sensitivity_rows(0)
        got = sj.sensitivity_rows(j, receivers=recs, components=comp, mapped=True)
        want, _ = _jtvec_rows(sj, j, recs, srcs, components=comp, mapped=True)
    assert all(x.shape == (3, 2) + vnM for x in (got if comp else (got,)))
    assert _worst(got, want, comp, what=f"model grid {kind} {name}") <= TOL_ROWS_SURVEY


