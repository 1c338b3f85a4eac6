"""CPU: maps.sensitivity_rows, the host restatement of the explicit rows of J (DeviceMG.sens_rows, k_sens_rows) -- no GPU needed.

* the transpose identity of every row and direction: sum_j v_j (c_c)_j == sum over the c-edges of C(v) s mu_0 lambda E, with the
  numpy restatement of the transposed statements of edges2cellaverages (tests/test_sensitivity_diagonal_host.py; the device's
  maps.cellaverages2edges takes its place in tests/test_gpu_sensitivity_rows.py);
* sum_d W_d |row_d|^2 is maps.sensitivity_diagonal on the inputs of the diagonal's kernel tests;
* the model-grid identity <Q (.) A^T (F (.) row), v> == <row, F (.) A (Q (.) v)> on dense per-axis matrices;
* the ROUNDING YARDSTICK of the kernel tests: the restatement in float64 against itself in np.longdouble on the inputs of
  tests/test_gpu_sensitivity_rows.py (``rows_case`` below, shared with that module).  ``ROWS_F64_VS_LONGDOUBLE`` records the largest
  deviation of a row relative to that row's largest magnitude; the kernel-level tolerance is 4 x that (FMA contraction and another
  association of the twelve-term sums, the margin of the diagonal's tests), the end-to-end tolerance twice the kernel-level one;
* the argument checks of SurveyJacobian.sensitivity_rows that need no device;
* the compiler's resource report of the four instantiations of k_sens_rows."""
import numpy as np
import pytest

from test_sensitivity_diagonal_host import (F64_VS_LONGDOUBLE, NSYS, SHAPES, _edge_shapes, cells2edges_numpy, kernel_case)

# Largest float64-versus-longdouble deviation of a row of maps.sensitivity_rows, relative to the row's largest magnitude, over all
# kernel cases (3 grids x 2 types x 3 widths x both forms), measured by test_rounding_yardstick below (x86-64, 80-bit long double:
# 5.549e-16, the summed form of (9, 4, 2) c128 with 3 systems) and rounded up to two digits.
ROWS_F64_VS_LONGDOUBLE = 5.6e-16
TOL_ROWS_KERNEL = 4 * ROWS_F64_VS_LONGDOUBLE
TOL_ROWS_SURVEY = 2 * TOL_ROWS_KERNEL


def rows_case(shape, real, nsys):
    """``kernel_case`` for the rows: every pair of the two masks is a row, so the active systems that the diagonal's weights leave
    unread (NaN there) get random fields; the systems that are masked out keep their NaN.  Adds ``ia``, ``jf`` (the active adjoint
    and forward systems, ascending) and ``pairs``, the (b_adj, b_fwd) of every row in the kernel's order."""
    case = dict(kernel_case(shape, real, nsys))
    rng = np.random.default_rng(7000 + 1000 * nsys + 10 * sum(shape) + int(real))
    nE = case['fwd'].shape[1]
    fwd, adj = case['fwd'].copy(), case['adj'].copy()
    for arr, use in ((fwd, case['use_fwd']), (adj, case['use_adj'])):
        for b in np.flatnonzero(use):
            if np.isnan(arr[b]).any():
                arr[b] = rng.standard_normal(nE) if real else rng.standard_normal(nE) + 1j * rng.standard_normal(nE)
    ia, jf = np.flatnonzero(case['use_adj']), np.flatnonzero(case['use_fwd'])
    case.update(fwd=fwd, adj=adj, ia=ia, jf=jf, pairs=[(int(a), int(f)) for a in ia for f in jf])
    return case


def host_rows(case, components=False, dtype=np.float64):
    from emg3d_amd import maps
    return maps.sensitivity_rows(case['grid'], case['fwd'][case['jf']], case['adj'][case['ia']], case['smu0'], components=components,
                                 dtype=dtype)


def row_deviation(got, want):
    """Largest |got - want| of a row relative to the largest magnitude of that row of ``want``; rows: the leading two axes."""
    want = np.asarray(want)
    diff = np.abs(np.asarray(got).astype(want.dtype) - want).reshape(want.shape[:2] + (-1,)).max(axis=2)
    return float((diff / np.abs(want).reshape(want.shape[:2] + (-1,)).max(axis=2)).max())


def row_identity_gaps(case, v, cells2edges):
    """Per pair and direction: |sum_j v_j (c_c)_j - sum over the c-edges of C(v) s mu_0 lambda E| relative to the sum of the absolute
    terms of the right-hand side, and the same for the summed row against all edges; the largest."""
    grid = case['grid']
    vnC = tuple(int(n) for n in grid.vnC)
    shapes = _edge_shapes(vnC)
    off = np.cumsum([0] + [int(np.prod(s)) for s in shapes])
    vol = np.asarray(grid.cell_volumes).reshape(vnC, order='F')
    cv = np.concatenate([a.ravel(order='F') for a in cells2edges((v, v, v), vol)])
    rows3, rows1 = host_rows(case, components=True), host_rows(case)
    worst = 0.0
    for p, (ba, bf) in enumerate(case['pairs']):
        prod = (case['adj'][ba] * case['fwd'][bf]) * case['smu0']
        for c in range(3):
            sl = slice(off[c], off[c + 1])
            lhs, rhs = np.sum(v * rows3[p, c]), np.sum(cv[sl] * prod[sl])
            worst = max(worst, abs(lhs - rhs) / np.sum(np.abs(cv[sl] * prod[sl])))
        worst = max(worst, abs(np.sum(v * rows1[p, 0]) - np.sum(cv * prod)) / np.sum(np.abs(cv * prod)))
    return worst


@pytest.mark.parametrize("real", [False, True], ids=["c128", "f64"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=str)
def test_row_is_the_transpose_of_the_jvec_source(shape, real):
    """Both sides are sums of ~4 nE products in float64: 1e-13 of the sum of their absolute values (the diagonal's bound)."""
    case = rows_case(shape, real, 3)
    v = np.random.default_rng(3).standard_normal(shape)
    gap = row_identity_gaps(case, v, cells2edges_numpy)
    print(f"transpose identity {shape} {'f64' if real else 'c128'}: {gap:.2e}")
    assert gap < 1e-13


@pytest.mark.parametrize("nsys", NSYS)
@pytest.mark.parametrize("real", [False, True], ids=["c128", "f64"])
def test_weighted_squares_are_the_diagonal(real, nsys):
    """On kernel_case's own inputs (NaN in every system its weights leave unread): the rows of the weighted pairs, squared and
    added in the kernel's order, are maps.sensitivity_diagonal, to the recorded yardstick of that module."""
    from emg3d_amd import maps
    for shape in SHAPES:
        case = kernel_case(shape, real, nsys)
        W = case['W_eff']
        ia, jf = np.flatnonzero(W.any(axis=1)), np.flatnonzero(W.any(axis=0))
        for split in (False, True):
            rows = maps.sensitivity_rows(case['grid'], case['fwd'][jf], case['adj'][ia], case['smu0'], components=split)
            assert rows.shape == (ia.size * jf.size, 3 if split else 1) + shape
            assert rows.dtype == (np.float64 if real else np.complex128)
            acc = [np.zeros(shape) for _ in range(rows.shape[1])]
            for p, (ba, bf) in enumerate((a, f) for a in ia for f in jf):
                if W[ba, bf] != 0:
                    acc = [a + W[ba, bf] * (r.real * r.real + r.imag * r.imag) for a, r in zip(acc, rows[p])]
            want = maps.sensitivity_diagonal(case['grid'], case['fwd'], case['adj'], case['smu0'], W, components=split)
            for a, w in zip(acc, want if split else (want,)):
                assert np.isfinite(a).all() and np.abs(a - w).max() <= F64_VS_LONGDOUBLE * np.abs(w).max()


@pytest.mark.parametrize("name", ['unaligned', 'beyond'])
def test_model_grid_identity(name):
    """<Q (.) A^T (F (.) row), v> == <row, F (.) A (Q (.) v)> for the real and the imaginary part of a row, A and A^T as dense
    per-axis matrices (tests/test_model_grid_host.py; the device's maps.volume_average_adjoint and maps.grid2grid(..., 'volume') take
    their place in tests/test_gpu_sensitivity_rows.py): sums of nC resp. nM products, 1e-13 of the sum of their absolute values."""
    import emg3d_amd as em
    from emg3d_amd import maps
    from test_model_grid_host import axis_matrices, dense_adjoint, dense_forward, grid_pairs, volumes
    model_grid, grid = grid_pairs(em, [name])[name]
    mats, vol = axis_matrices(em, model_grid, grid), volumes(grid)
    rng = np.random.default_rng(8)
    nE = int(grid.nE)
    fwd, adj = (rng.standard_normal((1, nE)) + 1j * rng.standard_normal((1, nE)) for _ in range(2))
    row = maps.sensitivity_rows(grid, fwd, adj, em.fields.FrequencySpec(1.0).smu0)[0, 0]
    F, Q = rng.standard_normal(grid.vnC), rng.standard_normal(model_grid.vnC)
    v = rng.standard_normal(model_grid.vnC)
    Av = F * dense_forward(mats, Q * v, vol)
    for part in (row.real, row.imag):
        on_model, _ = dense_adjoint(mats, part, vol, F, Q)
        lhs, rhs = np.sum(on_model * v), np.sum(part * Av)
        assert abs(lhs - rhs) <= 1e-13 * np.sum(np.abs(part * Av)) and abs(rhs) > 0


def yardsticks():
    """Per kernel case and form: (shape, real, nsys, split, float64 rows, longdouble rows)."""
    for shape in SHAPES:
        for real in (False, True):
            for nsys in NSYS:
                case = rows_case(shape, real, nsys)
                for split in (False, True):
                    yield shape, real, nsys, split, host_rows(case, split), host_rows(case, split, dtype=np.longdouble)


def test_rounding_yardstick():
    """The recorded deviation bounds every case, and is no looser than twice what is measured (where long double is wider)."""
    worst = 0.0
    for shape, real, nsys, split, f64, ld in yardsticks():
        pairs = {1: 1, 3: 4, 64: 30}[nsys]
        assert f64.shape == ld.shape == (pairs, 3 if split else 1) + shape
        assert f64.dtype == (np.float64 if real else np.complex128) and ld.dtype == (np.longdouble if real else np.clongdouble)
        assert np.isfinite(ld.real).all() and np.isfinite(ld.imag).all()
        dev = row_deviation(f64, ld)
        print(f"{shape} {'f64' if real else 'c128'} nsys {nsys} split {split}: float64 vs longdouble {dev:.2e}")
        worst = max(worst, dev)
    print(f"largest deviation {worst:.3e} (recorded: {ROWS_F64_VS_LONGDOUBLE:.1e})")
    assert worst <= ROWS_F64_VS_LONGDOUBLE
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        assert worst >= ROWS_F64_VS_LONGDOUBLE / 2


def test_order_and_shapes():
    """Pair p = b_adj * n_fwd + b_fwd, the split form's directions add up to the summed form bit for bit, rows are F-ordered."""
    from emg3d_amd import maps
    case = rows_case((2, 3, 4), False, 3)
    one, three = host_rows(case), host_rows(case, components=True)
    assert one.shape == (4, 1, 2, 3, 4) and three.shape == (4, 3, 2, 3, 4) and one[0, 0].flags.f_contiguous
    assert np.array_equal(one[:, 0], (three[:, 0] + three[:, 1]) + three[:, 2])
    for p, (ba, bf) in enumerate(case['pairs']):
        alone = maps.sensitivity_rows(case['grid'], case['fwd'][bf], case['adj'][ba], case['smu0'])
        assert alone.shape == (1, 1, 2, 3, 4) and np.array_equal(alone[0, 0], one[p, 0])
    assert case['pairs'] == [(0, 0), (0, 2), (1, 0), (1, 2)]
    with pytest.raises(ValueError):
        maps.sensitivity_rows(case['grid'], case['fwd'][:, :-1], case['adj'], case['smu0'])


def test_argument_checks_need_no_device():
    """A bad ``i_freq``, bad ``receivers``, a ``mapped`` that is no bool, ``mapped=False`` with a model grid and a closed object raise
    before any device call (the objects are never opened)."""
    import emg3d_amd as em
    h = [np.array([95., 70., 52., 40., 44., 57., 76., 104.])] * 3
    grid = em.TensorMesh(h, origin=(-269., -269., -269.))
    rec = (np.array([-55., 30., 5.]), np.array([12., -44., 50.]), np.array([-20., 35., -8.]), np.zeros(3), np.zeros(3))
    model = em.Model(grid, np.ones(grid.nC), mapping='Conductivity')
    sj = em.optimize.SurveyJacobian(grid, model, [[0., 0., 0., 0., 0.]], [1.0, -2.0], rec, batch=2)
    assert sj.rows_info is None
    for bad in (2, -1, 0.0, None, True, [0]):
        with pytest.raises(ValueError, match="i_freq"):
            sj.sensitivity_rows(bad)
    for bad in ([], [3], [-1], [0.5], [[0, 1]], 1):
        with pytest.raises(ValueError, match="receivers"):
            sj.sensitivity_rows(0, receivers=bad)
    with pytest.raises(TypeError, match="mapped"):
        sj.sensitivity_rows(0, mapped=1)
    with pytest.raises(RuntimeError, match="closed"):
        sj.sensitivity_rows(1, receivers=[2, 0])
    coarse = em.TensorMesh([np.array([x[0:4].sum(), x[4:8].sum()]) for x in h], origin=grid.origin)
    cmodel = em.Model(coarse, np.ones(coarse.nC), mapping='Conductivity')
    sjm = em.optimize.SurveyJacobian(grid, cmodel, [[0., 0., 0., 0., 0.]], [1.0], rec, batch=1, model_grid=coarse)
    with pytest.raises(ValueError, match="model grid"):
        sjm.sensitivity_rows(0)
    with pytest.raises(RuntimeError, match="closed"):
        sjm.sensitivity_rows(0, mapped=True)


def test_kernel_uses_no_scratch(tmp_path):
    """The compiler's resource remarks for the four instantiations of k_sens_rows on gfx950: no scratch (the edge values of a cell are
    indexed with compile-time constants only); the VGPR counts are printed, DESIGN 8.9 states them (needs hipcc, not a GPU)."""
    import os
    import shutil
    import subprocess
    import __graft_entry__ as g
    from conftest import ROOT
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = subprocess.run([hipcc] + g.FLAGS + ["-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "emg3d_hip.o"),
                          os.path.join(ROOT, "emg3d_amd", "csrc", "emg3d_hip.hip")], capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    name, seen = None, {}
    for line in out.stderr.splitlines():
        if "Function Name:" in line:
            name = line.split("Function Name:")[1].split()[0]
        elif name and "k_sens_rows" in name:
            for key in ("ScratchSize [bytes/lane]:", " VGPRs:"):
                if key in line:
                    seen.setdefault(name, {})[key.strip()] = int(line.split(key)[1].split()[0])
    print(seen)
    assert len(seen) == 4, seen
    assert all(v["ScratchSize [bytes/lane]:"] == 0 for v in seen.values()), seen
