"""Problems and references of the cycle-level accuracy tests (tests/test_oracle_cycle_truth.py on the CPU,
tests/test_gpu_cycle_accuracy.py on the GPU): whole multigrid solves on a layered marine model, measured against the same solve in
x87 extended precision.

`layered(shape, dtype)`: widths stretched by 1.25 per cell about the centre (axes of fewer than 8 cells: random widths, as in
tests/_hard_cases.py); conductivity 1 S/m, with sea water (3 S/m) over the upper middle, air (1e-8 S/m) above it and a resistive
block (1e-2 S/m) in the sediments; anisotropy factors (1, 2, 0.5); eta = -s mu_0 sigma V with the constants of _hard_cases.py
(0.1 Hz, float64: s = 0.6); zeta = V / mu_r, mu_r drawn from U(0.9, 1.3) -- the only random part where every axis has 8 cells;
the source: two x-edges at the sea floor in the centre set to 1.

The truth is `oracle.solve` on np.longdouble / np.clongdouble arrays: smoothing, residual and restriction then run in
libemg3d_oracle_ld.so, prolongation and the sums of the coarse models in NumPy's extended arithmetic.  The restriction weights, the
prolongation weights and the coarse widths REMAIN float64 in the truth: they are coefficients of the operator, which the product
forms on the host in float64 too -- the truth solves the same discrete problem on every level, in more digits.  The trace's
residual norms are accumulated in extended precision and rounded once to float64.

Every case runs six cycles with tol = 1e-30, so that the number of cycles never depends on rounding.  The float64 oracle is
3e-9 ... 3e-7 from the truth in the field's max-norm on these models (1e-14 on the two thin grids, which converge to rounding): parity at 1e-11 is not a
usable yardstick here, the float64 oracle's own error (`hc.bound`) is."""
import numpy as np

import _hard_cases as hc

MAXIT, TOL = 6, 1e-30
SIGMA_SEDIMENT, SIGMA_SEA, SIGMA_AIR, SIGMA_BODY = 1.0, 3.0, 1e-8, 1e-2
STRETCH = 1.25
SCLR = dict(semicoarsening=True, linerelaxation=True)
POINT = dict(semicoarsening=0, linerelaxation=0)
MEASURES = ("field", "anorm", "visit", "cycle")


def widths(shape):
    rng = np.random.default_rng(0)
    return [hc.BASE_WIDTH * (STRETCH ** np.abs(np.arange(n) - (n - 1) / 2) if n >= 8 else rng.uniform(1., 4., n)) for n in shape]


def conductivity(shape):
    """sigma per cell (before the anisotropy factors), F-ordered (nx, ny, nz); z grows upwards."""
    nx, ny, nz = shape
    sig = np.full(shape, SIGMA_SEDIMENT, order='F')
    top = nz // 2 + max(1, nz // 4)
    sig[:, :, nz // 2:top] = SIGMA_SEA
    sig[:, :, top:] = SIGMA_AIR
    sig[nx // 4:nx // 2, ny // 4:ny // 2, max(0, nz // 2 - 2):nz // 2 - 1] = SIGMA_BODY
    return sig


def source_cells(shape):
    """(i0, i1, j, k) of the source's x-edges [i0:i1, j, k]: the sea floor in the centre."""
    nx, ny, nz = shape
    return nx // 2 - 1, nx // 2 + 1, ny // 2, nz // 2


def source(shape, dtype, cells=None):
    i0, i1, j, k = cells or source_cells(shape)
    s = np.zeros(hc.n_edges(shape), dtype=dtype)
    hc.field_views(s, shape)[0][i0:i1, j, k] = 1.0
    return s


def smu0_of(dtype, freq=hc.FREQ):
    return (2j * np.pi * freq if np.dtype(dtype) == np.complex128 else hc.S_LAPLACE) * hc.MU_0


def layered(shape, dtype, freq=hc.FREQ):
    """The layered problem: dict(h, sigma, mu_r, eta, zeta, s); `freq` only for complex128."""
    shape = tuple(shape)
    key = ("layered", shape, np.dtype(dtype).char, freq)
    if key not in hc._cache:
        h = widths(shape)
        vol = np.einsum('i,j,k->ijk', *h)
        sigma = conductivity(shape)
        mu_r = np.asfortranarray(np.random.default_rng([7, *shape]).uniform(0.9, 1.3, shape))
        smu0 = smu0_of(dtype, freq)
        p = dict(h=h, sigma=sigma, mu_r=mu_r, eta=[np.asfortranarray(-smu0 * (f * sigma) * vol) for f in hc.ANISOTROPY],
                 zeta=np.asfortranarray(vol / mu_r), s=source(shape, dtype))
        for a in (*p['h'], p['sigma'], p['mu_r'], *p['eta'], p['zeta'], p['s']):
            a.setflags(write=False)
        hc._cache[key] = p
    return hc._cache[key]


def _case(shape, cycle, dtype, ordering="colour", **kw):
    return dict(shape=shape, cycle=cycle, dtype=dtype, ordering=ordering, kw=dict(kw or SCLR))


# The fifth shape was planned as 48 x 32 x 16 F.  It is not in the list, for two reasons found when the list was measured:
# * no level of it reaches a long-line kernel family: at 256 compute units the scan kernel serves lines of up to 256 blocks while a
#   colour has at most 1024 lines (csrc/sweep_plan.hpp: qpl_few_lines), so on a grid this narrow a long-line family needs a line
#   of MORE than 256 blocks;
# * its residual does not decrease in every cycle (float64 and extended alike, whatever the draw of mu_r): cycles 3 and 6 -- the
#   (sc_dir, lr_dir) = (3, 6) pair of the rotation -- raise it, 4.2e-3 -> 5.8e-3 ||s|| and 1.6e-4 -> 3.4e-4 ||s||.
# Lengthening its first axis to the smallest length with a long-line family, 257 x 32 x 16, gives widths stretched by 1.25^128: the
# solve diverges (1.4 ||s|| after three cycles, then DIVERGED) and the truth alone takes 22 s.  The family comes from a thin grid
# instead, with the long lines ALONG z, where they cross sediment, resistive body, sea water and air: 4 x 4 x 260 (260 = 4 x 65:
# the z-lines of level 0 run k_line_sweep_thm, those of the 130- and 65-block levels the scan kernel in several waves).  It
# converges in every cycle to 1e-13 ||s||, and the truth takes 1.6 s.
LONG = (4, 4, 260)
SHAPES = [((16, 16, 16), 'F'), ((32, 16, 8), 'F'), ((128, 4, 4), 'W'), ((24, 12, 20), 'V'), (LONG, 'F')]
LEX_TOO = [((16, 16, 16), 'F'), ((24, 12, 20), 'V')]
# grids on which six cycles converge to rounding: the float64 oracle's field is then 1e-14 from the truth, not 1e-8
CONVERGED = [(128, 4, 4), LONG]
CASES = [_case(shape, cycle, dtype) for shape, cycle in SHAPES for dtype in hc.DTYPES] + \
        [_case(shape, cycle, dtype, "lex") for shape, cycle in LEX_TOO for dtype in hc.DTYPES]
# The point smoother through the levels of 32 x 16 x 8, W-cycle, no semicoarsening, no line relaxation: kept, because the float64
# oracle's residual decreases in each of the six cycles (asserted in test_oracle_cycle_truth.py::test_truth_converges, which covers
# every case of this list); it decreases slowly -- the point smoother is no solver for stretched grids -- which is all the
# better for a test of accuracy: the errors of six cycles are not contracted away.
POINT_CASES = [_case((32, 16, 8), 'W', dtype, **POINT) for dtype in hc.DTYPES]
ALL_CASES = CASES + POINT_CASES

# The float64 oracle's own errors over ALL_CASES as measured (x86-64, g++ -O2 strict build), and the windows
# test_oracle_cycle_truth.py holds them to: a decade either side of the measured range of each measure.
#   field, grids not in CONVERGED   2.4e-9 (24 x 12 x 20 V lex) ... 2.2e-7 (32 x 16 x 8 W point, float64)
#   field, CONVERGED                3.9e-14 ... 7.6e-14
#   anorm                           3.9e-14 (128 x 4 x 4 W float64) ... 7.5e-14 (32 x 16 x 8 W point, complex)
#   visit                           5.5e-16 (32 x 16 x 8 W point, complex) ... 3.5e-14 (128 x 4 x 4 W complex)
#   cycle                           3.4e-17 ... 3.5e-14 (no lower end: a norm of 1e-5 ||s|| may well round as the truth's does)
WINDOWS = {"field": (2.4e-10, 2.2e-6), "field_converged": (3.9e-15, 7.6e-13), "anorm": (3.9e-15, 7.5e-13),
           "visit": (5.5e-17, 3.5e-13), "cycle": (0.0, 3.5e-13)}


def window(c, measure):
    return WINDOWS["field_converged" if measure == "field" and c["shape"] in CONVERGED else measure]


def case_id(c):
    nx, ny, nz = c["shape"]
    return f"{nx}x{ny}x{nz}-{c['cycle']}-{hc.tname(c['dtype'])}-{c['ordering']}" + ("" if c["kw"] == SCLR else "-point")


def solve_kw(c):
    return dict(cycle=c["cycle"], **c["kw"])


def mesh_of(oracle, p):
    return oracle.Mesh(p['h'], (0., 0., 0.))


def model_of(oracle, p, ext=False):
    up = hc.extended if ext else np.asarray
    return oracle.VModel(*(up(a) for a in p['eta']), up(p['zeta']))


def oracle_run(oracle, p, c, ext=False, fast=False, model=None):
    """A run = dict(records, norms, errs, field) of `oracle.solve` with a trace: float64 (strict or `fast`) or extended."""
    import _depth
    up = hc.extended if ext else np.array
    rec = []
    e, info = oracle.solve(mesh_of(oracle, p), model or model_of(oracle, p, ext), up(p['s']), maxit=MAXIT, tol=TOL,
                           order=1 if c["ordering"] == "colour" else 0, fast=fast, trace=rec, **solve_kw(c))
    records, norms = _depth.split_records(rec)
    return dict(records=records, norms=hc._frozen(norms), errs=hc._frozen(np.array(info['error_at_cycle'], dtype=float)),
                field=hc._frozen(e))


def references(oracle, c, p=None, tag=None):
    """(problem, float64 run, extended run) of a case: computed once.  `p` with a `tag`: another problem on the case's shape."""
    key = ("cycle", case_id(c), tag)
    if key not in hc._cache:
        p = layered(c["shape"], c["dtype"]) if p is None else p
        hc._cache[key] = (p, oracle_run(oracle, p, c), oracle_run(oracle, p, c, ext=True))
    return hc._cache[key]


def fast_run(oracle, c):
    key = ("cycle_fast", case_id(c))
    if key not in hc._cache:
        hc._cache[key] = oracle_run(oracle, layered(c["shape"], c["dtype"]), c, fast=True)
    return hc._cache[key]


def visit_errors(x_run, truth_run):
    """|norm - truth's| / ||s|| per record."""
    return np.abs(np.asarray(x_run["norms"], dtype=float) - truth_run["norms"]) / truth_run["errs"][0]


def cycle_errors(x_run, truth_run):
    """|error_at_cycle - truth's| / ||s|| of cycles 1 ... 6."""
    return np.abs(np.asarray(x_run["errs"], dtype=float)[1:] - truth_run["errs"][1:]) / truth_run["errs"][0]


def errors(oracle, x_run, truth_run, p):
    """The measures of a run against the truth, in units of the source norm where they are norms:

    field   max|e - e_truth| / max|e_truth|                         (`hc.err`)
    anorm   ||A (e - e_truth)|| / ||s||, A applied in extended precision (the extended `oracle.amat_x`)
    visit   max over the smoothing calls of |norm - truth's| / ||s||
    cycle   max over cycles 1 ... 6 of |error_at_cycle - truth's| / ||s||"""
    truth = truth_run["field"]
    d = np.asarray(x_run["field"]).astype(truth.dtype) - truth
    r = np.zeros_like(d)
    up = hc.extended
    oracle.amat_x(p['zeta'].shape, r, d, *(up(a) for a in p['eta']), up(p['zeta']), *(up(a) for a in p['h']))
    snorm = truth_run["errs"][0]
    return dict(field=hc.err(x_run["field"], truth), anorm=float(np.linalg.norm(r)) / snorm,
                visit=float(visit_errors(x_run, truth_run).max()), cycle=float(cycle_errors(x_run, truth_run).max()))


def reference_errors(oracle, c):
    """The float64 oracle's own errors on a case: the unit of the bound."""
    key = ("cycle_err", case_id(c))
    if key not in hc._cache:
        p, ref, truth = references(oracle, c)
        hc._cache[key] = errors(oracle, ref, truth, p)
    return hc._cache[key]


# ---- one smoothing call on the layered model (tests/test_gpu_accuracy.py::test_layered_sweep_residual) -------------------------------
# What the cycle tests found, isolated: two sweeps along one direction on level 0 of 16 x 16 x 16, started from the float64 oracle's
# field after ONE F-cycle -- a field that is non-zero in the air layer, as every field of a solve after its first cycle is.  The
# lines in and through the air cells are close to singular (eta is 1e-8 of its value in the water), so a line solve is far from the
# truth in the FIELD whatever the elimination order (1e-8 in float64, the oracle included): what tells the orders apart is the
# residual the solve leaves, ||A (e - e_truth)|| / ||s||.  An elimination that is backward stable leaves 1e-13 (its field error lies
# in the near-null space of A); one that is not leaves 1e-7.
SWEEP_SHAPE = (16, 16, 16)


def sweep_problem(oracle, dtype, shape=SWEEP_SHAPE):
    key = ("layered_sweep", shape, np.dtype(dtype).char)
    if key not in hc._cache:
        p = dict(layered(shape, dtype))
        e1, _ = oracle.solve(mesh_of(oracle, p), model_of(oracle, p), np.array(p['s']), maxit=1, tol=TOL, order=1, cycle='F', **SCLR)
        p['e0'] = hc._frozen(e1)
        hc._cache[key] = p
    return hc._cache[key]


def sweep_errors(oracle, p, e, truth):
    """(field, anorm) of a sweep's result against the extended sweep: hc.err, and ||A (e - truth)|| / ||s|| in extended precision."""
    d = np.asarray(e).astype(truth.dtype) - truth
    r = np.zeros_like(d)
    up = hc.extended
    oracle.amat_x(p['zeta'].shape, r, d, *(up(a) for a in p['eta']), up(p['zeta']), *(up(a) for a in p['h']))
    return dict(field=hc.err(e, truth), anorm=float(np.linalg.norm(r)) / float(np.linalg.norm(p['s'])))


def sweep_references(oracle, dtype, direction, shape=SWEEP_SHAPE):
    """(problem, extended truth, the float64 oracle's (field, anorm)) of two colour-ordered sweeps along `direction`."""
    key = ("layered_sweep_ref", shape, np.dtype(dtype).char, direction)
    if key not in hc._cache:
        p = sweep_problem(oracle, dtype, shape)
        truth = hc._frozen(hc.sweep(oracle, p, direction, 2, 1, ext=True))
        hc._cache[key] = (p, truth, sweep_errors(oracle, p, hc.sweep(oracle, p, direction, 2, 1), truth))
    return hc._cache[key]
