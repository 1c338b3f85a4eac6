"""Cycle parity at depth: the problems of tests/golden/depth.npz, the device's full-precision trace and the tolerance rule --
written once for the CPU test of the oracle (test_oracle_depth.py) and the GPU tests (test_gpu_depth.py).

A *record* is one smoothing call of a solve: ``(cycle, level, it, cycmax, kind, (nx, ny, nz))`` -- the cycle it belongs to,
the level, that level's loop counter (level 0: the cycle), the level's cycmax, kind 0 = coarsest level / 1 = pre- /
2 = post-smoothing, the level's grid -- followed by the residual norm of that level after the call.

Why per-visit norms: on thin deep grids the end-of-cycle quantities barely see the recursion (parity chain).  The
oracle's W- and F-cycles of the 128 x 4 x 4 case end with fields 1.1e-11 apart (FIELD_TOL of test_gpu_solver.py is 1e-11), but
make 319 smoothing calls against 99, and every one of them is compared here."""
import numpy as np

from conftest import assert_norms_close, load_golden

# tag -> (vnC, freq, solver keywords).  T*: thin grids, levels 0...6 along one axis (T4: 96 = 3 * 2^5, odd 3-cell coarsest
# axes); P*: the point smoother through five levels; M1: a medium grid; *L: the Laplace domain (float64 kernels).
SCLR = dict(semicoarsening=True, linerelaxation=True)
CASES = {
    'T1': ((128, 4, 4), 2.0, dict(cycle='W', **SCLR)),
    'T1L': ((128, 4, 4), -2.0, dict(cycle='W', **SCLR)),
    'T2': ((4, 4, 128), 2.0, dict(cycle='W', **SCLR)),
    'T3': ((4, 128, 4), 2.0, dict(cycle='F', **SCLR)),
    'T4': ((96, 6, 4), 2.0, dict(cycle='W', **SCLR)),
    'P1': ((32, 16, 8), 2.0, dict(cycle='W', semicoarsening=0, linerelaxation=0)),
    'P1L': ((32, 16, 8), -2.0, dict(cycle='W', semicoarsening=0, linerelaxation=0)),
    'M1': ((64, 16, 8), 2.0, dict(cycle='W', **SCLR)),
}
WITH_FIELD = ('T1', 'T1L', 'T2', 'T3', 'T4')
SRC = [10., -5., 7., 25., 15.]
MAXIT, TOL = 3, 1e-30


def problem_arrays(vnC):
    """Widths, origin, rho and mu_r of a case: the draws of test_gpu_solver.py::test_ragged_grids_and_parameter_combinations."""
    rng = np.random.default_rng(sum(vnC))
    h = [rng.uniform(30, 90, n) for n in vnC]
    origin = [-hh.sum() / 2 for hh in h]
    rho = 10 ** rng.uniform(-0.3, 1.0, int(np.prod(vnC)))
    mu_r = rng.uniform(0.9, 1.2, int(np.prod(vnC)))
    return h, origin, rho, mu_r


def checksum(h, rho, mu_r):
    """Stored with every case of depth.npz: a test that rebuilds the problem from the seed knows it got the same numbers."""
    return np.array([h[0].sum(), h[1].sum(), h[2].sum(), rho.sum(), mu_r.sum()])


def problem(pkg, vnC, freq):
    """(grid, model, sfield) of a case with the classes of ``pkg`` (the product package, or the reference in the generator)."""
    h, origin, rho, mu_r = problem_arrays(vnC)
    grid = pkg.meshes.TensorMesh(h, origin=origin)
    model = pkg.models.Model(grid, rho, 1.5 * rho, 2.5 * rho, mu_r=mu_r)
    sfield = pkg.fields.get_source_field(grid, SRC, freq)
    return grid, model, sfield


def oracle_problem(oracle, vnC, vm):
    """The oracle's mesh and model of a case; ``vm`` = the VolumeModel (eta_x, eta_y, eta_z, zeta) of `problem`."""
    h, origin, _, _ = problem_arrays(vnC)
    return oracle.Mesh(h, origin), oracle.VModel(np.asarray(vm.eta_x), np.asarray(vm.eta_y), np.asarray(vm.eta_z), np.asarray(vm.zeta))


def oracle_run(oracle, omesh, omodel, sfield, order=0, maxit=MAXIT, trace=True, **kw):
    """(records, norms, error_at_cycle, field) of an oracle solve."""
    rec = [] if trace else None
    e, info = oracle.solve(omesh, omodel, np.array(sfield), maxit=maxit, tol=TOL, order=order, trace=rec, **kw)
    records, norms = split_records(rec or [])
    return records, norms, info['error_at_cycle'], e


def split_records(raw):
    """[(it, level, cycmax, kind, vnC, norm)] in call order -> ([(cycle, level, it, cycmax, kind, vnC)], norms): a record of
    level 0 carries its cycle as `it`; the records of the coarse levels belong to the cycle of the level-0 record before them
    (nu_pre > 0 in every case here, so each cycle starts with one)."""
    records, norms, cycle = [], [], 0
    for it, level, cycmax, kind, vnC, norm in raw:
        if level == 0:
            cycle = int(it)
        records.append((cycle, int(level), int(it), int(cycmax), int(kind), tuple(int(n) for n in vnC)))
        norms.append(float(norm))
    return records, np.array(norms)


def stored(g, tag):
    """(records, norms, error_at_cycle, oracle_dev, oracle_dev of error_at_cycle) of a case of depth.npz."""
    rec = g[f'{tag}_records']
    records = [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4]), (int(r[5]), int(r[6]), int(r[7]))) for r in rec]
    return records, g[f'{tag}_norms'], g[f'{tag}_error_at_cycle'], g[f'{tag}_oracle_dev'], g[f'{tag}_oracle_dev_cycle']


def golden():
    return load_golden("depth.npz")


def assert_same_records(got, ref, what=""):
    """Structure: exactly the same sequence of smoothing calls."""
    if got == ref:
        return
    k = next((i for i, (a, b) in enumerate(zip(got, ref)) if a != b), min(len(got), len(ref)))
    raise AssertionError(f"{what}: {len(got)} smoothing calls against {len(ref)}; first difference at call {k}: "
                         f"(cycle, level, it, cycmax, kind, vnC) = {got[k] if k < len(got) else None} against "
                         f"{ref[k] if k < len(ref) else None}")


def _bar(ref, strict_above):
    """conftest.assert_norms_close's tolerance per entry, restated ONLY to name the records that exceed it (the verdict below
    is assert_norms_close's own)."""
    ref = np.abs(np.asarray(ref, dtype=float))
    tol = 2e-9 * ref + 1e-14 * ref[0]
    strict = ref > strict_above * ref[0]
    tol[strict] = 1e-10 * ref[strict] + 1e-16 * ref[0]
    return tol


def check_norms(got, ref, snorm, oracle_dev=None, strict_above=1e-5):
    """The tolerance rule.  ``conftest.assert_norms_close`` as it stands on ``[||s||, n_1, n_2, ...]``: every norm -- of
    whatever level -- is measured against the level-0 source norm ``snorm``; 1e-10 relative + 1e-16 ||s|| while a norm is
    above ``strict_above`` (1e-5) of ||s||, 2e-9 relative + 1e-14 ||s|| below.

    The only widening, and only against the reference (``oracle_dev`` = |oracle(lex) - reference| per record, stored in
    depth.npz by the generator): a record that exceeds the bar may deviate by 10 x oracle_dev of that record -- the spread
    between two independent implementations of the reference's arithmetic, with a margin for re-associated line solves.
    Returns [(index, deviation / (10 x oracle_dev))] of the records that needed it.

    ``strict_above=1e-4`` is the one other setting, for float64 (Laplace) cases where the oracle is the yard-stick -- the
    precedent of test_gpu_solver.py::test_solves_16_colour_laplace_vs_reference_arithmetic (its lines 155-158)."""
    assert strict_above in (1e-5, 1e-4)
    got = np.r_[snorm, np.asarray(got, dtype=float)]
    ref = np.r_[snorm, np.asarray(ref, dtype=float)]
    assert got.shape == ref.shape, (got.shape, ref.shape)
    widened = []
    if oracle_dev is not None:
        dev = np.abs(got - ref)
        wide = np.r_[0., 10 * np.asarray(oracle_dev, dtype=float)]
        over = dev > _bar(ref, strict_above)
        use = over & (dev <= wide)
        widened = [(int(k) - 1, float(dev[k] / wide[k])) for k in np.flatnonzero(use)]
        got = np.where(use, ref, got)       # (records within the widened tolerance; all others face the bar)
    assert_norms_close(got, ref, strict_above=strict_above)
    return widened


def device_run(em, grid, model, sfield, ordering, maxit=MAXIT, trace=True, drain_at_end=False, vmodel=None, **kw):
    """The level-0 loop of emg3d_amd.solver.multigrid on a handle of its own, with the device's full-precision trace:
    (records, norms, error_at_cycle, field).  Level 0 reports it = -1 (the host counts the cycles): mapped to the cycle.
    ``drain_at_end``: the records of all cycles are fetched with one get_trace() after the last cycle (the handle has to hold
    them all); the cycle of a level-0 record is then counted from the pre-smoothing calls of level 0.
    ``vmodel``: the handle's model arrays (an object with eta_x, eta_y, eta_z, zeta) given directly -- ``model`` is then not
    looked at and ``sfield`` may be the plain source buffer [fx | fy | fz] of the handle's dtype."""
    from emg3d_amd.solver import DeviceMG, MGParameters
    var = MGParameters(verb=0, sslsolver=False, vnC=grid.vnC, ordering=ordering, maxit=maxit, tol=TOL, cycle=kw['cycle'],
                       semicoarsening=kw['semicoarsening'], linerelaxation=kw['linerelaxation'])
    vm = em.VolumeModel(grid, model, sfield) if vmodel is None else vmodel
    raw = []
    with DeviceMG(grid, vm, sfield.dtype) as dev:
        dev.set_params(var)
        dev.set_sfield(sfield)
        dev.set_efield(None)
        errs = [dev.sfield_norm()]
        dev.begin(var.sc_dir)
        if trace:
            dev.set_trace(True)
        for cyc in range(maxit):
            nxt = (next(var.sc_cycle) if var.sc_cycle else var.sc_dir, next(var.lr_cycle) if var.lr_cycle else var.lr_dir)
            errs.append(dev.cycle(var.sc_dir, var.lr_dir))
            if trace and not drain_at_end:
                raw += [(cyc if level == 0 else it, level, cm, kind, vnC, norm) for it, level, cm, kind, vnC, norm in dev.get_trace()]
            var.sc_dir, var.lr_dir = nxt
        if trace and drain_at_end:
            cyc = -1
            for it, level, cm, kind, vnC, norm in dev.get_trace():
                cyc += level == 0 and kind < 2
                raw.append((cyc if level == 0 else it, level, cm, kind, vnC, norm))
        e = dev.get_efield()
    records, norms = split_records(raw)
    return records, norms, np.array(errs), e


def sweep_kernels(em, records, dtype, ordering, **kw):
    """For a failure message: the line-sweep kernel a handle selects per direction on a uniform grid of every level shape of
    ``records`` (a coarse level of a cycle plans its sweeps from the same shape)."""
    from emg3d_amd.solver import DeviceMG, MGParameters
    out = []
    for vnC in sorted({r[5] for r in records}, reverse=True):
        try:
            grid = em.TensorMesh([np.full(n, 50.) for n in vnC], origin=(0., 0., 0.))
            sfield = em.get_source_field(grid, [20., 20., 20., 25., 15.], 2.0 if dtype == np.complex128 else -2.0)
            vm = em.VolumeModel(grid, em.Model(grid, 1.5), sfield)
            var = MGParameters(verb=0, sslsolver=False, vnC=vnC, ordering=ordering, cycle=kw['cycle'],
                               semicoarsening=kw['semicoarsening'], linerelaxation=kw['linerelaxation'])
            names = []
            with DeviceMG(grid, vm, sfield.dtype) as dev:
                dev.set_params(var)
                dev.set_sfield(sfield)
                for d in (1, 2, 3):
                    if vnC[d - 1] > 2:
                        dev.smooth(1, d)
                        names.append(f"{'xyz'[d - 1]}: {dev.last_sweep_kernel()}")
            out.append(f"{vnC}: " + ", ".join(names))
        except Exception as exc:      # (a message helper must not hide the failure it describes)
            out.append(f"{vnC}: {exc!r}")
    return "\n".join(out)
