"""GPU: the one-solve form of the rows of J -- emg3d_mg_sens_rows_fill (k_sens_rows_fill) through the C ABI and
DeviceMG.sens_rows_fill, on the model grid, and SurveyJacobian.sensitivity_rows / park_rows with solves=1 end to end.

The contract: 1. the real parts are those of solves=2 bit for bit; 2. the imaginary parts are the imaginary planes of
the same sens_rows call and differ from those of solves=2 by no more than the truncation error of the solves; 3. park_rows(solves=1)
and sensitivity_rows(solves=1) agree bit for bit in both parts, on the computational grid (fused kernel) and on a model grid; 4. the
same bits at every call and for every batch; 5. the default is untouched (the existing tests).  Everything bitwise is asserted with
np.array_equal; the one closeness check is a condition between two measured figures, both printed."""
import numpy as np
import pytest

from conftest import load_golden
from test_gpu_row_store import _model
from test_gpu_sensitivity_diagonal import FREQS, OPTS, SOURCES, _handle, _survey, _upload
from test_sensitivity_rows_host import rows_case

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
FILL_SHAPES = [(5, 6, 7), (2, 3, 4), (9, 4, 2), (7, 6, 7)]            # the last: 294 cells, a second, ragged workgroup
FORMS = [(False, False), (True, False), (True, True)]               # (split, sum3): summed, split, split with sum3


def _align(nbytes):
    return (max(nbytes, 8) + 255) // 256 * 256


def _raw_fill(dev, smu0, use_fwd, use_adj, split, on_model, store, dest_re, dest_im, chain, sum3, fwd_bvec=0):
    a = complex(smu0)
    uf, ua = (np.ascontiguousarray(u, dtype=np.int32) for u in (use_fwd, use_adj))
    dre = np.ascontiguousarray(dest_re, dtype=np.int32)
    dim = None if dest_im is None else np.ascontiguousarray(dest_im, dtype=np.int32)
    return dev._lib.emg3d_mg_sens_rows_fill(dev._h, fwd_bvec, a.real, a.imag, uf.ctypes.data, ua.ctypes.data, int(split), int(on_model),
                                            store._h, dre.ctypes.data, None if dim is None else dim.ctypes.data, int(chain), int(sum3))


def _host_row(planes, chain, sum3):
    """The columns [dir][cell] of one real part: ``planes`` the real arrays of its directions, the chain factors and the sum applied
    in the order of SurveyJacobian.sensitivity_rows."""
    parts = list(planes)
    if chain is not None:
        parts = [d * g for d, g in zip(chain, parts)]
    if sum3:
        parts = [(parts[0] + parts[1]) + parts[2]]
    return np.concatenate([g.ravel(order='F') for g in parts])


def _nan_store(em, n_rows, n_cols):
    store = em.solver.DeviceRows(n_rows, n_cols)
    for i in range(n_rows):
        store.set_row(i, np.full(n_cols, np.nan))
    return store


def _destinations(rng, pairs, n_rows, imag):
    """A permutation of the store's rows dealt to the two tables, with holes: pair 1 keeps its imaginary part only, pair 2 its real
    part only, pair 3 neither (as far as there are that many pairs)."""
    perm = rng.permutation(n_rows).astype(np.int32)
    dre, dim = perm[:pairs].copy(), (perm[pairs:2 * pairs].copy() if imag else None)
    if imag and pairs > 1:
        dre[1] = -1
    if pairs > 2 and imag:
        dim[2] = -1
    if pairs > 3:
        dre[3] = -1
        if imag:
            dim[3] = -1
    return dre, dim


# ---- 1. the kernel through the C ABI --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsys", [1, 3, 64])
@pytest.mark.parametrize("real", [False, True], ids=["c128", "f64"])
@pytest.mark.parametrize("shape", FILL_SHAPES, ids=str)
def test_fill_equals_sens_rows_bitwise(shape, real, nsys):
    """Summed, split and split-with-sum3, each with and without chain factors, into a NaN store with permuted destinations and holes:
    every named row is the matching part of DeviceMG.sens_rows through the host's chain and sum, bit for bit; every other row is still
    all NaN; the masked-out systems hold NaN fields and leave no trace; part 0 is what sens_rows_park parks; dest_im=None keeps the
    real parts alone."""
    import emg3d_amd as em
    case = rows_case(shape, real, nsys)
    grid, smu0 = case['grid'], case['smu0']
    use = (case['use_fwd'], case['use_adj'])
    pairs, nC = len(case['pairs']), int(grid.nC)
    rng = np.random.default_rng(900 + nsys + sum(shape) + int(real))
    factors = [rng.uniform(0.5, 2.0, shape) for _ in range(3)]
    n_rows = 2 * pairs + 3
    with _handle(em, grid, smu0, nsys) as dev:
        _upload(dev, case)
        got = {True: dev.sens_rows(0, smu0, *use, components=True), False: dev.sens_rows(0, smu0, *use)}
        assert all(np.isfinite(g.real).all() and np.isfinite(g.imag).all() for g in got.values())
        for split, sum3 in FORMS:
            ncols = (3 if split and not sum3 else 1) * nC
            for chain in (False, True):
                for imag in ((False,) if real else (True, False)):
                    dre, dim = _destinations(rng, pairs, n_rows, imag)
                    with _nan_store(em, n_rows, ncols) as store, _nan_store(em, n_rows, ncols) as parked:
                        if chain:
                            store.set_chain(factors)
                            parked.set_chain(factors)
                        dev.sens_rows_fill(0, smu0, *use, store, dre, dim, components=split, chain=chain, sum3=sum3)
                        if (dre >= 0).any():
                            dev.sens_rows_park(0, smu0, *use, parked, dre, components=split, chain=chain, sum3=sum3)
                        named = {}
                        for p in range(pairs):
                            if dre[p] >= 0:
                                named[int(dre[p])] = (p, 'real')
                            if imag and dim[p] >= 0:
                                named[int(dim[p])] = (p, 'imag')
                        assert len(named) == int((dre >= 0).sum()) + (int((dim >= 0).sum()) if imag else 0) >= 1
                        for i in range(n_rows):
                            row = store.get_row(i)
                            if i not in named:
                                assert np.isnan(row).all(), (split, sum3, chain, imag, i)
                                continue
                            p, plane = named[i]
                            want = _host_row([getattr(g, plane) if not real else g for g in got[split][p]],
                                             factors if chain else None, sum3)
                            assert np.array_equal(row, want), (split, sum3, chain, imag, i, p, plane)
                            if plane == 'real':
                                assert np.array_equal(parked.get_row(i), row), (split, sum3, chain, i)


@pytest.mark.parametrize("real", [False, True], ids=["c128", "f64"])
def test_fill_refusals_write_nothing_and_no_row_buffer(real):
    """On a fresh handle: every refusal answers -2 or -7 and leaves the NaN store as it was; a fill leaves the handle's device_bytes
    unchanged (no row buffer), whereas sens_rows_park then grows it by the buffer of its planes."""
    import emg3d_amd as em
    shape, nsys = (7, 6, 7), 3
    case = rows_case(shape, real, nsys)
    grid, smu0 = case['grid'], case['smu0']
    use = (case['use_fwd'], case['use_adj'])
    pairs, nC, npart = len(case['pairs']), int(grid.nC), 1 if real else 2
    n_rows = 2 * pairs + 1
    good_re = np.arange(pairs, dtype=np.int32)
    good_im = None if real else np.arange(pairs, 2 * pairs, dtype=np.int32)
    none = np.zeros(nsys, dtype=np.int32)
    neg = np.full(pairs, -1, dtype=np.int32)
    with _handle(em, grid, smu0, nsys) as dev:
        _upload(dev, case)
        before = dev.device_bytes
        with _nan_store(em, n_rows, 3 * nC) as store, _nan_store(em, n_rows, nC) as narrow:
            def fill(*, uf=use[0], ua=use[1], split=1, on_model=0, st=store, dre=good_re, dim=good_im, chain=0, sum3=0, fwd_bvec=0):
                return _raw_fill(dev, smu0, uf, ua, split, on_model, st, dre, dim, chain, sum3, fwd_bvec=fwd_bvec)
            for bad in (-2, -1, 1, 9):
                assert fill(fwd_bvec=bad) == -2
            assert fill(uf=none) == -2 and fill(ua=none) == -2
            assert fill(on_model=1) == -7
            assert fill(split=0) == -2                  # a store of 3 nC columns for one direction
            assert fill(st=narrow) == -2                # ... and one of nC columns for three
            assert fill(split=0, st=narrow, sum3=1) == -2           # sum3 without the three directions
            assert fill(chain=1) == -2 and fill(st=narrow, sum3=1, chain=1) == -2          # no chain factors
            over = good_re.copy()
            over[-1] = n_rows
            assert fill(dre=over) == -2
            twice = good_re.copy()
            twice[0] = twice[-1]
            assert fill(dre=twice) == -2                # a row named twice in one table
            if real:
                assert fill(dim=np.arange(pairs, 2 * pairs, dtype=np.int32)) == -2         # no imaginary part on a float64 handle
                assert fill(dre=neg) == -2
                with pytest.raises(ValueError, match="sens_rows_fill"):
                    dev.sens_rows_fill(0, smu0, *use, store, good_re, good_re + pairs, components=True)
            else:
                across = good_im.copy()
                across[1] = good_re[2]
                assert fill(dim=across) == -2           # ... and across the two
                over_im = good_im.copy()
                over_im[0] = n_rows + 5
                assert fill(dim=over_im) == -2
                assert fill(dre=neg, dim=neg) == -2 and fill(dre=neg, dim=None) == -2
            with pytest.raises(ValueError, match="pairs"):
                dev.sens_rows_fill(0, smu0, *use, store, good_re[:-1], good_im, components=True)
            with pytest.raises(ValueError, match="sens_rows_fill"):
                dev.sens_rows_fill(0, smu0, *use, store, twice, good_im, components=True)
            with pytest.raises(RuntimeError, match="model grid"):
                dev.sens_rows_fill(0, smu0, *use, store, good_re, good_im, components=True, model_grid=True)
            for st in (store, narrow):
                assert all(np.isnan(st.get_row(i)).all() for i in range(n_rows))
            assert dev.device_bytes == before
            # the fill itself: nothing is allocated on the handle
            dev.sens_rows_fill(0, smu0, *use, store, good_re, good_im, components=True)
            dev.sens_rows_fill(0, smu0, *use, narrow, good_re, good_im, components=True, sum3=True)
            dev.sens_rows_fill(0, smu0, *use, narrow, good_re, good_im)
            assert dev.device_bytes == before
            assert np.isfinite(store.get_row(0)).all() and np.isnan(store.get_row(n_rows - 1)).all()
            filled = [store.get_row(i) for i in range(pairs)]
            dev.sens_rows_park(0, smu0, *use, store, good_re, components=True)
            assert dev.device_bytes - before == _align(pairs * 3 * npart * nC * 8)
            assert all(np.array_equal(store.get_row(i), filled[i]) for i in range(pairs))


# ---- 2. the model grid ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('freq', [1.5, -1.5], ids=['c128', 'f64'])
def test_fill_on_the_model_grid_bitwise(freq):
    """12 x 10 x 8 over 7 x 5 x 4 ('unaligned' of tests/test_model_grid_host.py, the handle of test_planes_on_the_model_grid_bitwise),
    factors per direction (split, and split with sum3 and chain factors) and shared (summed): both parts in the store are the planes of
    sens_rows(model_grid=True) of the same handle, bit for bit; rows not named stay NaN."""
    import emg3d_amd as em
    from emg3d_amd import models
    from emg3d_amd.solver import DeviceMG
    from test_model_grid_host import grid_pairs
    g = load_golden("survey_jacobian.npz")
    model_grid, grid = grid_pairs(em, ['unaligned'])['unaligned']
    nM, nsys = int(model_grid.nC), 3
    vnM = tuple(int(n) for n in model_grid.vnC)
    model = em.Model(grid, g['tri_sig_x'], g['tri_sig_y'], g['tri_sig_z'], mapping='Conductivity')
    spec = em.fields.FrequencySpec(freq)
    real = freq < 0
    rng = np.random.default_rng(58)
    fields = [[rng.standard_normal(grid.nE) if real else rng.standard_normal(grid.nE) + 1j * rng.standard_normal(grid.nE)
               for _ in range(nsys)] for _ in range(2)]
    use_fwd, use_adj = np.array([1, 0, 1], dtype=np.int32), np.array([0, 1, 1], dtype=np.int32)
    F = tuple(np.asfortranarray(rng.standard_normal(grid.vnC)) for _ in range(3))
    Q = tuple(np.asfortranarray(rng.standard_normal(model_grid.vnC)) for _ in range(3))
    factors = [rng.uniform(0.5, 2.0, vnM) for _ in range(3)]
    dre = np.array([5, -1, 0, 7], dtype=np.int32)
    dim = None if real else np.array([2, 8, -1, 1], dtype=np.int32)
    for shared in (False, True):
        with DeviceMG.from_model(grid, models.model_parts(grid, model, raw=True), spec) as dev:
            dev.set_batch(nsys)
            dev.bvec_alloc(1)
            for b in range(nsys):
                dev.select(b)
                dev.set_efield(em.Field(grid, fields[1][b].copy(), freq=freq))
                dev.bvec_set(0, b, fields[0][b])
            dev.set_model_grid(model_grid)
            dev.set_regrid_factors((F[0],) * 3 if shared else F, (Q[0],) * 3 if shared else Q)
            split = not shared
            planes = dev.sens_rows(0, spec.smu0, use_fwd, use_adj, components=split, model_grid=True)
            assert planes.shape == (4, 3 if split else 1) + vnM
            for sum3, chain in ((False, False), (True, True)) if split else ((False, False), (False, True)):
                ncols = (3 if split and not sum3 else 1) * nM
                with _nan_store(em, 9, ncols) as store:
                    if chain:
                        store.set_chain(factors)
                    dev.sens_rows_fill(0, spec.smu0, use_fwd, use_adj, store, dre, dim, components=split, model_grid=True, chain=chain,
                                       sum3=sum3)
                    named = {int(d): (p, 'real') for p, d in enumerate(dre) if d >= 0}
                    if not real:
                        named.update({int(d): (p, 'imag') for p, d in enumerate(dim) if d >= 0})
                    for i in range(9):
                        row = store.get_row(i)
                        if i not in named:
                            assert np.isnan(row).all()
                            continue
                        p, plane = named[i]
                        want = _host_row([q if real else getattr(q, plane) for q in planes[p]], factors if chain else None, sum3)
                        assert np.array_equal(row, want), (shared, sum3, chain, i, p, plane)
            if not shared:
                with _nan_store(em, 9, nM) as store:        # the summed form needs shared factors, as sens_rows
                    assert _raw_fill(dev, spec.smu0, use_fwd, use_adj, 0, 1, store, dre, dim, 0, 0) == -2
                    assert all(np.isnan(store.get_row(i)).all() for i in range(9))


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------
def _count_solves(sj):
    """Wrap ``sj._solve``; -> the list that grows by one per call."""
    calls, orig = [], sj._solve

    def counted(*args, **kwargs):
        calls.append(1)
        return orig(*args, **kwargs)
    sj._solve = counted
    return calls


def _tuple(x):
    return x if isinstance(x, tuple) else (x,)


def _check_contracts(sj, kw, receivers=None, data=None, count=None):
    """Contracts 1, 3 and 4 on an open SurveyJacobian for the keywords ``kw`` of both methods; -> the rows of both forms per entry of
    ``freqs``.  ``count``: the list of _count_solves."""
    rows1, rows2 = [], []
    for j in range(sj.n_freq):
        n0 = 0 if count is None else len(count)
        two = _tuple(sj.sensitivity_rows(j, receivers=receivers, solves=2, **kw))
        n2 = 0 if count is None else len(count) - n0
        assert sj.rows_info_imag is None or sj.freqs[j] > 0
        one = _tuple(sj.sensitivity_rows(j, receivers=receivers, solves=1, **kw))
        n1 = 0 if count is None else len(count) - n0 - n2
        assert sj.rows_info_imag is None and all(x['exit'] == 0 for x in sj.rows_info)
        again = _tuple(sj.sensitivity_rows(j, receivers=receivers, solves=1, **kw))
        assert len(one) == len(two) == (3 if kw.get('components') else 1)
        for a, b, c in zip(one, two, again):
            assert a.shape == b.shape and a.dtype == b.dtype and np.abs(a).max() > 0
            assert np.array_equal(a, c)                                         # 4: the same bits at every call
            if sj.freqs[j] > 0:
                assert np.array_equal(a.real, b.real)                           # 1: the real parts of the default
                assert np.isfinite(a.imag).all() and np.abs(a.imag).max() > 0
            else:
                assert np.array_equal(a, b)                                     # Laplace domain: the default wholly
        if count is not None:
            assert n2 > 0 and n1 == (n2 // 2 if sj.freqs[j] > 0 else n2), (j, n1, n2)
        rows1.append(one)
        rows2.append(two)
    if receivers is not None:
        return rows1, rows2
    # 3: parked against returned, both parts
    n0 = 0 if count is None else len(count)
    store = sj.park_rows(data=data, solves=1, **kw)
    assert store.solves == 1 and store.n_rows > 0
    if count is not None and data is None:
        assert len(count) - n0 == sum(-(-sj.n_rec // sj._nb) for _ in sj.freqs)       # one solve per chunk of receivers, every entry
    for i, (j, s, r, part) in enumerate(store.index):
        got = _tuple(store.row(i))
        assert part == 0 or sj.freqs[j] > 0
        for g, w in zip(got, rows1[j]):
            w = w[s, r]
            w = (w.real, w.imag)[part] if np.iscomplexobj(w) else w
            assert g.shape == w.shape and np.array_equal(g, w), (i, j, s, r, part, float(np.abs(g - w).max()))
    for j in range(sj.n_freq):
        for p in store.info[j]:
            assert p is None or (p[0]['exit'] == 0 and p[1] is None)
    store.close()
    return rows1, rows2


@pytest.mark.parametrize("mapped", [False, True], ids=["sigma", "mapped"])
@pytest.mark.parametrize("components", [False, True], ids=["sum", "components"])
@pytest.mark.parametrize("kind", ["iso", "tri-log"])
def test_one_solve_contracts(kind, components, mapped):
    """8 x 8 x 8, 3 sources x (1 Hz, s = 2) x 4 receivers, batch = 2, tol = 1e-8, isotropic and tri-axial LgConductivity: contracts 1, 3
    and 4; solves=1 makes half the _solve calls of the default at 1 Hz and as many at s = 2; the handles hold no more after
    park_rows(solves=1) than before (computational grid: no row buffer is touched)."""
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = _model(em, grid, sig, kind)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, tol=1e-8, **OPTS) as sj:
        count = _count_solves(sj)
        _check_contracts(sj, dict(components=components, mapped=mapped), count=count)
        n0 = len(count)
        with sj.park_rows(components=components, mapped=mapped) as two, sj.park_rows(components=components, mapped=mapped, solves=1) as one:
            assert two.solves == 2 and one.solves == 1 and np.array_equal(one.index, two.index)
            assert len(count) - n0 == (4 + 2) + (2 + 2)
            for i, (j, s, r, part) in enumerate(one.index):
                if part == 0:
                    assert all(np.array_equal(a, b) for a, b in zip(_tuple(one.row(i)), _tuple(two.row(i))))


def test_one_solve_keeps_the_row_buffer_off_the_handle():
    """At a frequency on the computational grid park_rows(solves=1) leaves device_bytes of the handle as it was (the Laplace-domain
    entries park as the default does, through their handle's row buffer, and are left out here); park_rows(solves=2) grows it."""
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = _model(em, grid, sig, "iso")
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS[:1], rec, batch=2, tol=1e-8, **OPTS) as sj:
        sj.park_rows(solves=1).close()              # (whatever the first adjoint solves set up is there now)
        before = sj.device_bytes
        with sj.park_rows(solves=1):
            assert sj.device_bytes == before
        with sj.park_rows(solves=2):
            assert sj.device_bytes > before


@pytest.mark.parametrize("kind", ["magnetic", "reference-cubic", "linear"])
def test_one_solve_other_receivers_and_adjoint_rules(kind):
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = em.Model(grid, sig, mapping='Conductivity')
    kw = dict(magnetic=dict(electric=False), linear=dict(receiver_interpolation='linear'),
              **{'reference-cubic': dict(adjoint='reference', receiver_interpolation='cubic')})[kind]
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, tol=1e-8, **kw, **OPTS) as sj:
        _check_contracts(sj, {})


def test_one_solve_subset_mask_set_model_and_batch():
    """A ``receivers`` subset out of order is the same rows; a ``data`` mask removes rows and solves; after set_model the rows are
    those of a new object; another batch gives the same bits."""
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = em.Model(grid, sig, mapping='Conductivity')
    other = em.Model(grid, sig * 10 ** rng.uniform(-0.2, 0.2, grid.nC), mapping='Conductivity')
    sel = np.ones((3, 2, 4), dtype=bool)
    sel[:, 0, 2] = False
    sel[1, 1, 0] = False                            # one datum of a receiver that is still solved for
    kw = dict(tol=1e-8, **OPTS)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, **kw) as sj:
        count = _count_solves(sj)
        full, _ = _check_contracts(sj, {}, data=sel)
        sub, _ = _check_contracts(sj, {}, receivers=[3, 1], count=count)
        for j in range(2):
            assert sub[j][0].shape[:2] == (3, 2)
            assert np.array_equal(sub[j][0][:, 0], full[j][0][:, 3]) and np.array_equal(sub[j][0][:, 1], full[j][0][:, 1])
        n0 = len(count)
        with sj.park_rows(data=sel, solves=1) as store:
            assert store.n_rows == 36 - 6 - 1 and store.info[0][2] is None and store.info[0][1][1] is None
            assert len(count) - n0 == 2 + 2         # receivers 0, 1, 3 at 1 Hz: chunks of 2 + 1, one solve each; 2 + 2 at s = 2
        sj.set_model(other)
        after, _ = _check_contracts(sj, {}, data=sel)
        assert not np.array_equal(after[0][0], full[0][0])
    for batch in (3, 1):
        with em.optimize.SurveyJacobian(grid, other, SOURCES, FREQS, rec, batch=batch, **kw) as sj:
            for j in range(2):
                assert np.array_equal(sj.sensitivity_rows(j, solves=1), after[j][0]), (batch, j)
            if batch == 3:
                with sj.park_rows(solves=1) as store:
                    for i, (j, s, r, part) in enumerate(store.index):
                        w = after[j][0][s, r]
                        assert np.array_equal(store.row(i), (w.real, w.imag)[part] if np.iscomplexobj(w) else w)


@pytest.mark.parametrize("components", [False, True], ids=["sum", "components"])
@pytest.mark.parametrize('kind', ['Resistivity', 'Conductivity-tri'])
def test_one_solve_on_a_model_grid(kind, components):
    """12 x 10 x 8 from 7 x 5 x 4 (tests/test_gpu_row_store.py: test_parked_rows_on_a_model_grid), 3 sources x (1.5 Hz, s = 1.2), batch
    = 2: the contracts with the rows on the model grid, a data mask, mapped=False refused."""
    import emg3d_amd as em
    from test_gpu_jacobian import OPTS as JOPTS
    from test_gpu_model_grid import SOURCES as MSOURCES, _models
    from test_model_grid_host import grid_pairs
    g = load_golden("survey_jacobian.npz")
    model_grid, grid = grid_pairs(em, ['unaligned'])['unaligned']
    model = _models(em, model_grid, kind)
    rec = tuple(g['rec'])
    n_rec = len(rec[0])
    kw = dict(JOPTS, tol=1e-6, batch=2, model_grid=model_grid)
    with em.optimize.SurveyJacobian(grid, model, MSOURCES, [1.5, -1.2], rec, **kw) as sj:
        with pytest.raises(ValueError, match="model grid"):
            sj.park_rows(solves=1)
        with pytest.raises(ValueError, match="model grid"):
            sj.sensitivity_rows(0, solves=1)
        sel = np.zeros((3, 2, n_rec), dtype=bool)
        sel[[0, 2]] = True
        sel[:, :, 1] = False                        # sources 0 and 2, every receiver but 1
        rows1, _ = _check_contracts(sj, dict(components=components, mapped=True), data=sel)
        assert rows1[0][0].shape[2:] == tuple(model_grid.vnC)


# ---- 4. contract 2: how far the imaginary parts are from those of the default ---------------------------------------------------
def _imag_gap(a, b):
    """Largest |Im a - Im b| of a row relative to the largest magnitude of that row of ``b``."""
    size = np.abs(b).reshape(b.shape[:2] + (-1,)).max(axis=2)
    return float((np.abs(a.imag - b.imag).reshape(b.shape[:2] + (-1,)).max(axis=2) / size).max())


def test_imaginary_parts_within_the_truncation_of_the_solves():
    """1 Hz on the 8 x 8 x 8 survey.  gap: the imaginary parts of solves=1 against those of solves=2 (tol = 1e-8); trunc: the
    imaginary parts of solves=2 at tol = 1e-8 against solves=2 at tol = 1e-11 -- what the default's own second solve leaves
    undetermined.  The condition is gap <= trunc (and trunc > 0): the one-solve form differs from the default by no more than the
    default's truncation error.  No number is fixed in advance; both figures are printed."""
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = em.Model(grid, sig, mapping='Conductivity')

    def exits(sj):
        return [x['exit'] for x in sj.rows_info] + [x['exit'] for x in (sj.rows_info_imag or [])]
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, tol=1e-8, **OPTS) as sj:
        two = sj.sensitivity_rows(0, solves=2)
        assert len(exits(sj)) == 8 and not any(exits(sj))
        one = sj.sensitivity_rows(0, solves=1)
        assert len(exits(sj)) == 4 and not any(exits(sj))
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, tol=1e-11, **OPTS) as sj:
        tight = sj.sensitivity_rows(0, solves=2)
        assert len(exits(sj)) == 8 and not any(exits(sj))
    gap, trunc = _imag_gap(one, two), _imag_gap(two, tight)
    print(f"imaginary parts, relative to the row's largest magnitude: solves=1 vs solves=2 {gap:.2e}; solves=2 at tol 1e-8 vs 1e-11 "
          f"{trunc:.2e}")
    assert np.array_equal(one.real, two.real)
    assert trunc > 0 and gap <= trunc


# ---- 5. the derivative and the products of a one-solve store ---------------------------------------------------------------------
@pytest.mark.parametrize("method", ["cubic", "linear"])
def test_jvec_is_one_solve_rows_times_v(method):
    """test_jvec_is_rows_times_v of tests/test_gpu_sensitivity_rows.py with solves=1, and its bound: 10 x the fixture's reference-side
    adjoint gap for these receivers."""
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
            rows = sj.sensitivity_rows(j, solves=1)
            assert all(x['exit'] == 0 for x in sj.rows_info) and sj.rows_info_imag is None
            rv[:, j] = np.einsum('skxyz,xyz->sk', rows, v)
    lhs, rhs = np.sum(np.conj(w) * jv), np.sum(np.conj(w) * rv)
    gap = abs(lhs - rhs) / abs(lhs)
    worst = np.abs(jv - rv).max() / np.abs(jv).max()
    print(f"{method}, solves=1: J v vs rows . v, gap {gap:.2e} (reference gap {ref_gap:.2e}), largest datum deviation {worst:.2e}")
    assert np.abs(jv).max() > 0 and gap < 10 * ref_gap


def test_products_of_a_one_solve_store():
    """gram() of a solves=1 store is exactly symmetric and repeats; matvec(v) is rows . v within the dot-product bound of
    tests/test_gpu_row_store.py; with_covariance and project carry ``solves`` over; posterior_variance runs."""
    import emg3d_amd as em
    grid, rec, rng, sig = _survey(em)
    model = _model(em, grid, sig, "iso")
    vnC = tuple(int(n) for n in grid.vnC)
    cov = em.maps.SmoothingCovariance(grid, (150.0, 100.0, 60.0), passes=2)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, batch=2, tol=1e-8, **OPTS) as sj:
        store = sj.park_rows(solves=1)
        n = store.n_rows
        assert n == 36 and store.solves == 1
        R = np.array([store.row(i).ravel(order='F') for i in range(n)])
        G = store.gram()
        assert np.array_equal(G, G.T) and np.array_equal(store.gram(), G) and np.all(np.diag(G) > 0)
        v = rng.standard_normal(vnC)
        vf = v.ravel(order='F')
        jv = store.matvec(v)
        nn = R.shape[1] + 2
        assert np.all(np.abs(jv - R.astype(np.longdouble) @ vf.astype(np.longdouble)) <= nn * U / (1 - nn * U) * (np.abs(R) @ np.abs(vf)))
        full = sj.jvec(v)
        assert np.abs(store.data(jv) - full).max() <= 1e-5 * np.abs(full).max()
        w = rng.uniform(0.5, 2.0, n)
        damping = 1e-3 * np.trace(G) / n
        post = store.posterior_variance(w, damping=damping)
        assert post.shape == vnC and np.isfinite(post).all()
        with store.project(np.eye(2, n)) as T:
            assert T.solves == 1 and np.array_equal(T.get_row(1), R[1])
        with store.with_covariance(cov) as new:
            assert new.solves == 1 and new.cov is cov
            Gc = new.gram()
            assert np.array_equal(Gc, Gc.T)
            pc = new.posterior_variance(w, damping=1e-3 * np.trace(Gc) / n)
            assert pc.shape == vnC and np.isfinite(pc).all()
