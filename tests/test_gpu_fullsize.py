"""GPU, BASELINE.json sizes (128^3 F-cycle, 256^3 V-cycle): the oracle cannot
run whole cycles at these sizes in seconds, so parity is checked through
size-independent properties: (a) the converged GPU field satisfies the discrete
equation as evaluated by the ORACLE's residual (independent CPU restatement of
core.amat_x), with the norm the device reported; (b) linearity of the solve;
(c) complex symmetry of the operator A (<Ax,y> = <x,Ay>, no conjugation) through
the device mat-vec; (d) lexicographic and coloured orderings reach the same
field to the solver tolerance (128^3, one cycle count each)."""
import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu


def _problem(em, name, freq=1.0):
    import bench
    return bench.build_problem(em, name, freq)


def test_128_fcycle_solution_satisfies_equation(oracle):
    import emg3d_amd as em
    grid, model, sfield, cycle = _problem(em, "128F")
    e, info = em.solve(grid, model, sfield, cycle=cycle, semicoarsening=True, linerelaxation=True,
                       return_info=True, tol=1e-6, verb=0)
    assert info['exit'] == 0 and info['it_mg'] <= 12
    vm = em.VolumeModel(grid, model, sfield)
    om = oracle.Mesh(grid.h, grid.origin)
    ov = oracle.VModel(vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta)
    l2 = oracle.residual(om, ov, np.array(sfield), np.array(e), True, fast=True)
    # the oracle's residual norm of the GPU field == the norm the device reported
    assert abs(l2 / info['abs_error'] - 1) < 1e-6
    assert l2 < 1e-6 * info['ref_error']
    # linearity: solve(2 s) == 2 solve(s) (same number of cycles, same relative history)
    s2 = em.SourceField(grid, 2 * np.array(sfield), freq=1.0)
    e2, info2 = em.solve(grid, model, s2, cycle=cycle, semicoarsening=True, linerelaxation=True,
                         return_info=True, tol=1e-6, verb=0)
    assert info2['it_mg'] == info['it_mg']
    assert relerr(np.array(e2), 2 * np.array(e)) < 1e-12


def test_128_operator_symmetry_and_orderings():
    import emg3d_amd as em
    from emg3d_amd.solver import DeviceMG
    grid, model, sfield, cycle = _problem(em, "128F")
    vm = em.VolumeModel(grid, model, sfield)
    rng = np.random.default_rng(0)
    x = em.Field(grid, rng.standard_normal(grid.nE) + 1j * rng.standard_normal(grid.nE), freq=1.0)
    y = em.Field(grid, rng.standard_normal(grid.nE) + 1j * rng.standard_normal(grid.nE), freq=1.0)
    x.ensure_pec
    y.ensure_pec
    with DeviceMG(grid, vm, np.complex128) as dev:
        Ax, Ay = dev.amatvec(x), dev.amatvec(y)
    a, b = np.sum(Ax * np.asarray(y)), np.sum(np.asarray(x) * Ay)     # bilinear form, no conjugation
    assert abs(a - b) / abs(a) < 1e-11
    # both orderings converge to the same field (solver tolerance 1e-7 -> agreement ~1e-6)
    ec = em.solve(grid, model, sfield, cycle='F', semicoarsening=True, linerelaxation=True, tol=1e-7, verb=0)
    el, info = em.solve(grid, model, sfield, cycle='F', semicoarsening=True, linerelaxation=True, tol=1e-7,
                        verb=0, ordering='lex', return_info=True)
    assert info['exit'] == 0
    assert relerr(np.array(ec), np.array(el)) < 5e-6


def test_256_vcycle_solution_satisfies_equation(oracle):
    import emg3d_amd as em
    grid, model, sfield, cycle = _problem(em, "256V")
    e, info = em.solve(grid, model, sfield, cycle=cycle, semicoarsening=True, linerelaxation=True,
                       return_info=True, maxit=6, verb=0)
    assert np.all(np.isfinite(info['error_at_cycle']))
    assert np.all(np.diff(info['error_at_cycle']) < 0)          # monotone decrease
    vm = em.VolumeModel(grid, model, sfield)
    om = oracle.Mesh(grid.h, grid.origin)
    ov = oracle.VModel(vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta)
    l2 = oracle.residual(om, ov, np.array(sfield), np.array(e), True, fast=True)
    assert abs(l2 / info['abs_error'] - 1) < 1e-6


# --------------------------------------------------------------------------------------------------
# ONE sweep of the line smoother at the sizes the roofline is quoted on, element by element against the
# oracle (strict build, colour order): the kernels the bench line names, on the layouts they run on
# (parity-split working copies, x-lines transposed + split, XCD-aware line map, 24-/32-bit strides).
# --------------------------------------------------------------------------------------------------
SWEEP_RTOL = 2e-10      # complex128; same bar as the small-size kernel tests


def _smooth_field(grid, seed):
    """A smooth non-zero field with noise on top (PEC enforced): exercises every neighbour term."""
    import emg3d_amd as em
    rng = np.random.default_rng(seed)
    e = em.Field(grid, freq=1.0)
    for comp, f in enumerate((e.fx, e.fy, e.fz)):
        ax = [np.linspace(0, 1, n) for n in f.shape]
        X, Y, Z = np.meshgrid(*ax, indexing='ij')
        f[...] = (np.sin(3 * X + comp) * np.cos(2 * Y) * (1 + Z) + 1j * np.cos(2 * X - Z + comp) * np.sin(3 * Y)
                  + 0.05 * (rng.standard_normal(f.shape) + 1j * rng.standard_normal(f.shape)))
    e.ensure_pec
    return e


# (workload, environment, expected kernel, tolerance).  The one-sided kernels (k_line_sweep_qc, _rp) eliminate in the
# reference's order, the two-sided k_line_sweep_thm (default below 8192 lines per colour) in that order and its mirror image:
# they agree with the reference to rounding at every size.  (Round 1's plain two-sided k_line_sweep_th grouped the right
# half's unknowns differently and was off by up to 1.2e-8 on the ill-conditioned lines of this model -- lines inside the
# 100 Ohm-m body, condition ~ 1/(omega mu sigma h^2) ~ 1e5; tests/tools/conditioning.py; removed in round 4.)
@pytest.mark.parametrize("workload,env,expect,tol", [
    ("128F", {}, "k_line_sweep_thm", SWEEP_RTOL),
    ("128F", {"EMG3D_THM_LIFO": "1"}, "k_line_sweep_thm", SWEEP_RTOL),
    ("128F", {"EMG3D_THA_BIG_LINES": "8192"}, "k_line_sweep_tha", SWEEP_RTOL),      # affine kernel on split copies, zeta from the widths
    ("128F", {"EMG3D_Q": "2"}, "k_line_sweep_qc<", SWEEP_RTOL),
    ("256V", {}, "k_line_sweep_qc<", SWEEP_RTOL),
    ("256V", {"EMG3D_ZSEP": "0"}, "k_line_sweep_qc<", SWEEP_RTOL),
    ("128F", {"EMG3D_ZSEP": "0"}, "k_line_sweep_thm", SWEEP_RTOL),
    ("256V", {"EMG3D_Q": "0"}, "k_line_sweep_rp", SWEEP_RTOL)])
def test_one_sweep_vs_oracle_fullsize(oracle, monkeypatch, request, workload, env, expect, tol):
    import emg3d_amd as em
    from emg3d_amd.solver import DeviceMG, MGParameters
    if env:                 # kernel variants exist in the lab build only; the defaults are tested on the product library
        request.getfixturevalue("lab")
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    grid, model, sfield, cycle = _problem(em, workload)
    vm = em.VolumeModel(grid, model, sfield)
    var = MGParameters(verb=0, cycle=cycle, sslsolver=False, linerelaxation=True, semicoarsening=True,
                       vnC=grid.vnC, ordering='colour')
    e0 = _smooth_field(grid, 7)
    # a source of the field's own magnitude, so that s and A e both matter in the right-hand sides
    s = em.SourceField(grid, np.array(_smooth_field(grid, 8)) * 1e-3, freq=1.0)
    eta = [np.asfortranarray(a) for a in (vm.eta_x, vm.eta_y, vm.eta_z)]
    zeta = np.asfortranarray(vm.zeta)
    names = {}
    with DeviceMG(grid, vm, np.complex128) as dev:
        dev.set_params(var)
        dev.set_sfield(s)
        for direction in (1, 2, 3):
            dev.set_efield(e0)
            dev.smooth(1, direction)                       # lr_dir 1/2/3 = x/y/z lines, nu = 1
            got = dev.get_efield()
            names[direction] = dev.last_sweep_kernel()
            key = (workload, direction)
            if key not in _ORACLE_SWEEPS:                  # one oracle sweep per (size, direction): 1 s / 10 s
                ref = np.array(e0)
                oracle.gauss_seidel(grid.vnC, ref, np.array(s), *eta, zeta, *grid.h, 1, direction=direction, order=1)
                _ORACLE_SWEEPS[key] = ref
            ref = _ORACLE_SWEEPS[key]
            assert relerr(got, ref) < tol, (workload, direction, names[direction], relerr(got, ref))
            # the sweep changed the field by far more than the tolerance (the comparison is not vacuous)
            assert relerr(got, np.array(e0)) > 1e-3
    print("kernels:", names)
    assert all(v.startswith(expect) for v in names.values()), names


_ORACLE_SWEEPS = {}


def test_128_two_cycles_vs_oracle(oracle):
    """The north star's criterion at BASELINE size: the 128^3 F-cycle (sc + lr), two cycles, against the oracle
    in the SAME ordering -- lexicographic (= the reference) and coloured: per-cycle residual norms within 1e-10
    relative, fields within 1e-10 (measured: lex 2e-13 / 2e-14, colour 3e-12 / 4e-12 with the two-sided
    level-0 kernel, 4e-14 / 2e-14 with the quad-per-line kernel forced).  ~45 s of oracle time."""
    import emg3d_amd as em
    grid, model, sfield, cycle = _problem(em, "128F")
    vm = em.VolumeModel(grid, model, sfield)
    om = oracle.Mesh(grid.h, grid.origin)
    ov = oracle.VModel(vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta)
    for ordering, order in (("lex", 0), ("colour", 1)):
        oe, oinfo = oracle.solve(om, ov, np.array(sfield), cycle=cycle, semicoarsening=True, linerelaxation=True,
                                 maxit=2, tol=1e-30, order=order)
        e, info = em.solve(grid, model, sfield, cycle=cycle, semicoarsening=True, linerelaxation=True, maxit=2,
                           tol=1e-30, return_info=True, verb=0, ordering=ordering)
        dev = np.abs(info['error_at_cycle'] / oinfo['error_at_cycle'] - 1)
        assert dev.max() < 1e-10, (ordering, dev)
        assert relerr(np.array(e), oe) < 1e-10, ordering


def test_128_two_cycles_laplace_vs_oracle(oracle):
    """The same at BASELINE size in the LAPLACE domain (s = 2, float64 fields: the `double` instantiations of every kernel of the
    cycle -- two-sided level-0 kernel, affine kernel, scan kernel and its chain form, residual, transfers -- at full size): two 128^3
    F-cycles (sc + lr) in the timed colour ordering against the oracle's, norms and field within 1e-10."""
    import emg3d_amd as em
    grid, model, sfield, cycle = _problem(em, "128F", -2.0)
    assert np.asarray(sfield).dtype == np.float64
    vm = em.VolumeModel(grid, model, sfield)
    om = oracle.Mesh(grid.h, grid.origin)
    ov = oracle.VModel(vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta)
    oe, oinfo = oracle.solve(om, ov, np.array(sfield), cycle=cycle, semicoarsening=True, linerelaxation=True,
                             maxit=2, tol=1e-30, order=1)
    e, info = em.solve(grid, model, sfield, cycle=cycle, semicoarsening=True, linerelaxation=True, maxit=2,
                       tol=1e-30, return_info=True, verb=0, ordering='colour')
    assert np.asarray(e).dtype == np.float64
    dev = np.abs(info['error_at_cycle'] / oinfo['error_at_cycle'] - 1)
    assert dev.max() < 1e-10, dev
    assert relerr(np.array(e), oe) < 1e-10
    assert info['error_at_cycle'][-1] < 0.1 * info['error_at_cycle'][0]


def test_256_one_vcycle_vs_oracle(oracle):
    """BASELINE configs[2], the configuration the roofline target is quoted on, at CYCLE level: ONE 256^3 V-cycle
    (semicoarsening + line relaxation: 8 levels, the compact-factor quad kernel on level 0, the z-marching residual
    kernel, 36 GB of device memory with 32-bit in-kernel offsets, the captured launch graph) against the strict oracle
    in the same ordering -- lexicographic (= the reference, emg3d/solver.py:434-607) and coloured.  Residual norm and
    field within 1e-10 (the north star's number).  ~2 min of oracle time per ordering."""
    import emg3d_amd as em
    grid, model, sfield, cycle = _problem(em, "256V")
    assert cycle == 'V'
    vm = em.VolumeModel(grid, model, sfield)
    om = oracle.Mesh(grid.h, grid.origin)
    ov = oracle.VModel(vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta)
    s = np.array(sfield)
    for ordering, order in (("colour", 1), ("lex", 0)):
        e, info = em.solve(grid, model, sfield, cycle=cycle, semicoarsening=True, linerelaxation=True, maxit=1,
                           tol=1e-30, return_info=True, verb=0, ordering=ordering)
        oe, oinfo = oracle.solve(om, ov, s, cycle=cycle, semicoarsening=True, linerelaxation=True,
                                 maxit=1, tol=1e-30, order=order)
        assert info['it_mg'] == oinfo['it_mg'] == 1
        dev = np.abs(info['error_at_cycle'] / oinfo['error_at_cycle'] - 1)
        assert dev.max() < 1e-10, (ordering, dev)
        assert relerr(np.array(e), oe) < 1e-10, ordering
        # not vacuous: the cycle reduced the residual by more than an order of magnitude
        assert info['error_at_cycle'][1] < 0.1 * info['error_at_cycle'][0]
        del e, oe


def test_256_one_vcycle_laplace_vs_oracle(oracle):
    """... and in the Laplace domain (float64: `k_line_sweep_qc<f64,...>` on levels 0 and 1, 403 MB working copies -- the placement
    search runs --, the float64 residual / transfer kernels at full size): ONE 256^3 V-cycle in the timed colour ordering against the
    strict oracle, norm and field within 1e-10."""
    import emg3d_amd as em
    grid, model, sfield, cycle = _problem(em, "256V", -2.0)
    assert cycle == 'V' and np.asarray(sfield).dtype == np.float64
    vm = em.VolumeModel(grid, model, sfield)
    om = oracle.Mesh(grid.h, grid.origin)
    ov = oracle.VModel(vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta)
    e, info = em.solve(grid, model, sfield, cycle=cycle, semicoarsening=True, linerelaxation=True, maxit=1,
                       tol=1e-30, return_info=True, verb=0, ordering='colour')
    oe, oinfo = oracle.solve(om, ov, np.array(sfield), cycle=cycle, semicoarsening=True, linerelaxation=True,
                             maxit=1, tol=1e-30, order=1)
    assert info['it_mg'] == oinfo['it_mg'] == 1
    dev = np.abs(info['error_at_cycle'] / oinfo['error_at_cycle'] - 1)
    assert dev.max() < 1e-10, dev
    assert relerr(np.array(e), oe) < 1e-10
    assert info['error_at_cycle'][1] < 0.1 * info['error_at_cycle'][0]


def test_128_bicgstab_one_iteration_vs_oracle(oracle):
    """BASELINE config 4 against the oracle at full size: 128^3, sslsolver='bicgstab' with the F-cycle (sc + lr)
    as preconditioner, ONE BiCGSTAB iteration = two preconditioner applications of three multigrid cycles each
    (emg3d/solver.py:610-734, 1359-1364), lexicographic order (the reference's).  The oracle drives SciPy's bicgstab
    on the host, the product its device-resident restatement: iteration counts, the callback's residual norm and
    the iterate must agree.  ~2 min of oracle time."""
    import emg3d_amd as em
    grid, model, sfield, cycle = _problem(em, "128F")
    vm = em.VolumeModel(grid, model, sfield)
    om = oracle.Mesh(grid.h, grid.origin)
    ov = oracle.VModel(vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta)
    e, info = em.solve(grid, model, sfield, cycle=cycle, sslsolver='bicgstab', semicoarsening=True,
                       linerelaxation=True, maxit=1, tol=1e-30, return_info=True, verb=0, ordering='lex')
    oe, oinfo = oracle.solve(om, ov, np.array(sfield), cycle=cycle, sslsolver='bicgstab', semicoarsening=True,
                             linerelaxation=True, maxit=1, tol=1e-30, order=0)
    assert info['it_ssl'] == oinfo['it_ssl'] == 1
    assert info['it_mg'] == oinfo['it_mg'] == 6
    assert info['exit_message'] == oinfo['exit_message']
    dev = np.abs(np.asarray(info['error_at_cycle']) / oinfo['error_at_cycle'] - 1)
    assert dev.max() < 1e-9, dev
    assert relerr(np.array(e), oe) < 1e-9
    assert info['error_at_cycle'][-1] < 1e-3 * info['error_at_cycle'][0]      # one iteration = six cycles' worth


def test_128_bicgstab_preconditioned(oracle):
    """BASELINE config 4: 128^3 with sslsolver='bicgstab' (device-resident iteration, F-cycle preconditioner):
    converges, and the field satisfies the discrete equation as the ORACLE evaluates it."""
    import emg3d_amd as em
    grid, model, sfield, cycle = _problem(em, "128F")
    e, info = em.solve(grid, model, sfield, cycle=cycle, sslsolver='bicgstab', semicoarsening=True,
                       linerelaxation=True, return_info=True, tol=1e-6, verb=0)
    assert info['exit'] == 0 and 1 <= info['it_ssl'] <= 6 and info['it_mg'] <= 30
    vm = em.VolumeModel(grid, model, sfield)
    l2 = oracle.residual(oracle.Mesh(grid.h, grid.origin), oracle.VModel(vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta),
                         np.array(sfield), np.array(e), True, fast=True)
    assert l2 < 1e-6 * info['ref_error']
    # info['abs_error'] is the residual norm of the last callback (the reference's semantics, solver.py:690-693):
    # BiCGSTAB can leave through its half-step exit after that, so it brackets the true residual only loosely
    assert 0.5 < l2 / info['abs_error'] < 2.0
    # same field as the plain multigrid solve to the solver tolerance
    e2 = em.solve(grid, model, sfield, cycle=cycle, semicoarsening=True, linerelaxation=True, tol=1e-7, verb=0)
    assert relerr(np.array(e), np.array(e2)) < 2e-5


def test_128_eight_frequency_shard(oracle):
    """BASELINE config 5's workload on ONE GPU: 8 frequencies x 1 source on the 128^3 grid through
    shard.solve_frequencies (shared sigma*V, eta and source formed on the device per frequency, three solves
    in flight).  Every field satisfies its own frequency's equation (oracle residual); sequential == concurrent."""
    import emg3d_amd as em
    from emg3d_amd import shard
    import bench
    grid, model, sfield, cycle = _problem(em, "128F")
    freqs = bench.FREQS
    res = shard.solve_frequencies(grid, model, [0., 0., 0., 30., 10.], freqs, concurrent=3, cycle=cycle,
                                  semicoarsening=True, linerelaxation=True, tol=1e-6, verb=0)
    assert len(res) == len(freqs)
    om = oracle.Mesh(grid.h, grid.origin)
    for f, (e, info) in zip(freqs, res):
        assert info['exit'] == 0, (f, info['exit_message'])
        sf = em.get_source_field(grid, [0., 0., 0., 30., 10.], f)
        vm = em.VolumeModel(grid, model, sf)
        l2 = oracle.residual(om, oracle.VModel(vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta), np.array(sf), np.array(e),
                             True, fast=True)
        assert l2 < 1e-6 * info['ref_error'], f
    # the same list again, one solve at a time: bit-identical (every solve is deterministic on its own stream)
    res1 = shard.solve_frequencies(grid, model, [0., 0., 0., 30., 10.], freqs, concurrent=1, cycle=cycle,
                                   semicoarsening=True, linerelaxation=True, tol=1e-6, verb=0)
    for (e3, _), (e1, _) in zip(res, res1):
        assert np.array_equal(np.array(e1), np.array(e3))


def test_384_one_sweep_vs_oracle(oracle):
    """The largest size the repository quotes a number for (profiles/r0*_bench_384V.json; not a BASELINE config): one
    colour-ordered sweep per line direction at 384^3 against the strict oracle, element-wise.  This is the first size at
    which the 24- / 32-bit in-kernel offsets of the level-0 kernels come within a factor 1.5 of their limits."""
    import emg3d_amd as em
    from emg3d_amd.solver import DeviceMG, MGParameters
    grid, model, sfield, cycle = _problem(em, "384V")
    vm = em.VolumeModel(grid, model, sfield)
    var = MGParameters(verb=0, cycle=cycle, sslsolver=False, linerelaxation=True, semicoarsening=True,
                       vnC=grid.vnC, ordering='colour')
    e0 = _smooth_field(grid, 7)
    s = em.SourceField(grid, np.array(_smooth_field(grid, 8)) * 1e-3, freq=1.0)
    eta = [np.asfortranarray(a) for a in (vm.eta_x, vm.eta_y, vm.eta_z)]
    zeta = np.asfortranarray(vm.zeta)
    names = {}
    with DeviceMG(grid, vm, np.complex128) as dev:
        dev.set_params(var)
        dev.set_sfield(s)
        for direction in (1, 2, 3):
            dev.set_efield(e0)
            dev.smooth(1, direction)
            got = dev.get_efield()
            names[direction] = dev.last_sweep_kernel()
            ref = np.array(e0)
            oracle.gauss_seidel(grid.vnC, ref, np.array(s), *eta, zeta, *grid.h, 1, direction=direction, order=1)
            assert relerr(got, ref) < SWEEP_RTOL, (direction, names[direction], relerr(got, ref))
            assert relerr(got, np.array(e0)) > 1e-3
            del got, ref
    print("kernels:", names)
    assert all(v.startswith("k_line_sweep_qc") for v in names.values()), names


@pytest.mark.parametrize("shape", [(256, 128, 64), (96, 160, 48), (320, 32, 40), (64, 72, 264), (136, 136, 136)])
def test_sweep_plan_matches_the_launches_and_the_oracle(oracle, shape):
    """Non-cubic grids, where every line direction lands in another kernel family: (a) the instantiation a handle launches on level 0 is
    the one `emg3d_sweep_plan` predicts from the shape and THIS device's CU count (plan and launch come from the same value,
    csrc/sweep_plan.hpp); (b) one colour-ordered sweep per direction against the strict oracle, element-wise."""
    import emg3d_amd as em
    from types import SimpleNamespace
    from emg3d_amd import _lib
    from emg3d_amd.solver import DeviceMG, MGParameters
    rng = np.random.default_rng(sum(shape))
    h = [rng.uniform(20., 40., n) * 1.01 ** np.abs(np.arange(n) - n / 2) for n in shape]
    grid = em.TensorMesh(h, origin=(0., 0., 0.))
    vol = grid.cell_volumes.reshape(grid.vnC, order='F')
    smu0 = em.SourceField(grid, freq=1.0).smu0
    eta = [np.asfortranarray(smu0 * vol * 10 ** rng.uniform(-1, 1, shape)) for _ in range(3)]
    zeta = np.asfortranarray(vol)
    e0 = em.Field(grid, rng.standard_normal(grid.nE) + 1j * rng.standard_normal(grid.nE), freq=1.0)
    e0.ensure_pec
    s = em.SourceField(grid, (rng.standard_normal(grid.nE) + 1j * rng.standard_normal(grid.nE)) * 1e-6, freq=1.0)
    var = MGParameters(verb=0, cycle='V', sslsolver=False, linerelaxation=True, semicoarsening=True, vnC=grid.vnC, ordering='colour')
    names = {}
    with DeviceMG(grid, SimpleNamespace(eta_x=eta[0], eta_y=eta[1], eta_z=eta[2], zeta=zeta), np.complex128) as dev:
        dev.set_params(var)
        dev.set_sfield(s)
        for direction in (1, 2, 3):
            dev.set_efield(e0)
            dev.smooth(1, direction)
            got = dev.get_efield()
            names[direction] = dev.last_sweep_kernel()
            plan = _lib.sweep_plan(shape, direction)            # cu_count = 0: the current device
            assert names[direction] == plan["kernel"], (direction, names[direction], plan)
            ref = np.array(e0)
            oracle.gauss_seidel(grid.vnC, ref, np.array(s), *eta, zeta, *grid.h, 1, direction=direction, order=1)
            assert relerr(got, ref) < SWEEP_RTOL, (direction, names[direction], relerr(got, ref))
    print(shape, names)
    assert len(set(n.split("<")[0] for n in names.values())) >= 2 or shape[0] == shape[1] == shape[2], names


@pytest.mark.parametrize("ordering,order", [("colour", 1), ("lex", 0)])
def test_point_smoother_one_sweep_vs_oracle_128(oracle, ordering, order):
    """`linerelaxation=False` at BASELINE size: one sweep of the node-block smoother (`k_point_sweep`: eight colours / the reference's
    hyperplanes) on the 128^3 workload against the strict oracle, element-wise, in both orderings."""
    import emg3d_amd as em
    from emg3d_amd.solver import DeviceMG, MGParameters
    grid, model, sfield, cycle = _problem(em, "128F")
    vm = em.VolumeModel(grid, model, sfield)
    var = MGParameters(verb=0, cycle=cycle, sslsolver=False, linerelaxation=False, semicoarsening=True,
                       vnC=grid.vnC, ordering=ordering)
    e0 = _smooth_field(grid, 7)
    s = em.SourceField(grid, np.array(_smooth_field(grid, 8)) * 1e-3, freq=1.0)
    eta = [np.asfortranarray(a) for a in (vm.eta_x, vm.eta_y, vm.eta_z)]
    zeta = np.asfortranarray(vm.zeta)
    with DeviceMG(grid, vm, np.complex128) as dev:
        dev.set_params(var)
        dev.set_sfield(s)
        dev.set_efield(e0)
        dev.smooth(1, 0)
        got = dev.get_efield()
    ref = np.array(e0)
    oracle.gauss_seidel(grid.vnC, ref, np.array(s), *eta, zeta, *grid.h, 1, direction=0, order=order)
    assert relerr(got, ref) < SWEEP_RTOL, relerr(got, ref)
    assert relerr(got, np.array(e0)) > 1e-3


@pytest.mark.parametrize("workload,expect", [("128F", "k_line_sweep_thm<c128,3,8>"), ("256V", "k_line_sweep_qc<c128,2,16>")])
def test_magnetic_permeability_one_sweep_vs_oracle_fullsize(oracle, workload, expect):
    """Models with mu_r at BASELINE sizes: zeta = V / mu_r is no longer the cell volume, so the level-0 kernels of the PRODUCT library
    read it (the instantiations without the zeta-from-the-widths shortcut, which the bench workloads never reach).  One colour-ordered
    sweep per line direction against the strict oracle, element-wise."""
    import emg3d_amd as em
    from emg3d_amd.solver import DeviceMG, MGParameters
    grid, model0, sfield, cycle = _problem(em, workload)
    rng = np.random.default_rng(11)
    mu_r = rng.uniform(0.7, 2.5, grid.nC)
    model = em.Model(grid, model0.property_x, model0.property_y, model0.property_z, mu_r=mu_r)
    vm = em.VolumeModel(grid, model, sfield)
    assert not np.array_equal(np.asarray(vm.zeta).ravel(order='F'), grid.cell_volumes)
    var = MGParameters(verb=0, cycle=cycle, sslsolver=False, linerelaxation=True, semicoarsening=True,
                       vnC=grid.vnC, ordering='colour')
    e0 = _smooth_field(grid, 7)
    s = em.SourceField(grid, np.array(_smooth_field(grid, 8)) * 1e-3, freq=1.0)
    eta = [np.asfortranarray(a) for a in (vm.eta_x, vm.eta_y, vm.eta_z)]
    zeta = np.asfortranarray(vm.zeta)
    with DeviceMG(grid, vm, np.complex128) as dev:
        dev.set_params(var)
        dev.set_sfield(s)
        for direction in (1, 2, 3):
            dev.set_efield(e0)
            dev.smooth(1, direction)
            got = dev.get_efield()
            assert dev.last_sweep_kernel() == expect, dev.last_sweep_kernel()
            ref = np.array(e0)
            oracle.gauss_seidel(grid.vnC, ref, np.array(s), *eta, zeta, *grid.h, 1, direction=direction, order=1)
            assert relerr(got, ref) < SWEEP_RTOL, (direction, relerr(got, ref))
            assert relerr(got, np.array(e0)) > 1e-3


@pytest.mark.parametrize("workload,expect", [("144V", "k_line_sweep_thm<c128,3,12>"), ("200V", "k_line_sweep_qc<c128,3,16>")])
def test_between_powers_of_two_one_sweep_and_cycle_vs_oracle(oracle, workload, expect):
    """Sizes between the powers of two get their launch shapes from ROUNDS of waves (HISTORY R5.19): 144^3 -- 5184 lines per colour --
    the two-sided kernel at 12 lines per pair of waves (one round instead of two at 8), 200^3 -- 10 000 lines -- the quad kernel's 16-line
    instantiation at 10 lines per wave (one round instead of two at 8).  The lane mapping does not touch a line's arithmetic: one
    colour-ordered sweep per direction against the strict oracle element-wise, and one V-cycle (coarse levels with 9- ... 13-line
    waves inside) against the oracle's cycle, norms and field to 1e-10."""
    import emg3d_amd as em
    from emg3d_amd.solver import DeviceMG, MGParameters
    grid, model, sfield, cycle = _problem(em, workload)
    vm = em.VolumeModel(grid, model, sfield)
    var = MGParameters(verb=0, cycle=cycle, sslsolver=False, linerelaxation=True, semicoarsening=True,
                       vnC=grid.vnC, ordering='colour')
    e0 = _smooth_field(grid, 7)
    s = em.SourceField(grid, np.array(_smooth_field(grid, 8)) * 1e-3, freq=1.0)
    eta = [np.asfortranarray(a) for a in (vm.eta_x, vm.eta_y, vm.eta_z)]
    zeta = np.asfortranarray(vm.zeta)
    with DeviceMG(grid, vm, np.complex128) as dev:
        dev.set_params(var)
        dev.set_sfield(s)
        for direction in (1, 2, 3):
            dev.set_efield(e0)
            dev.smooth(1, direction)
            got = dev.get_efield()
            assert dev.last_sweep_kernel() == expect, dev.last_sweep_kernel()
            ref = np.array(e0)
            oracle.gauss_seidel(grid.vnC, ref, np.array(s), *eta, zeta, *grid.h, 1, direction=direction, order=1)
            assert relerr(got, ref) < SWEEP_RTOL, (direction, relerr(got, ref))
            assert relerr(got, np.array(e0)) > 1e-3
    e, info = em.solve(grid, model, sfield, cycle=cycle, semicoarsening=True, linerelaxation=True, maxit=1, tol=1e-30,
                       return_info=True, verb=0)
    om = oracle.Mesh(grid.h, grid.origin)
    ov = oracle.VModel(vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta)
    oe, oinfo = oracle.solve(om, ov, np.array(sfield), cycle=cycle, semicoarsening=True, linerelaxation=True, maxit=1, tol=1e-30,
                             order=1)
    assert np.abs(info['error_at_cycle'] / oinfo['error_at_cycle'] - 1).max() < 1e-10
    assert relerr(np.array(e), oe) < 1e-10


def test_448_beyond_4GiB_sweeps_and_cycle_vs_oracle(oracle):
    """448^3 complex: 4.33 GB per field array -- the first cubic size whose level 0 is beyond the 32-bit byte offsets of the
    lane-group kernels.  The product library must serve it with k_line_sweep_qc_big (64-bit per-lane field offsets, split
    working copies), not with the thread-per-line fallback: (a) one colour-ordered sweep per line direction against the
    strict oracle, element-wise, at the small-size tolerance; (b) three V-cycles: monotone residuals, and the norm the
    device reports is the norm the oracle's residual computes from the downloaded field (residual on the split copy,
    restriction, prolongation and the conversions of a > 4 GiB level inside)."""
    import emg3d_amd as em
    from emg3d_amd.solver import DeviceMG, MGParameters
    grid, model, sfield, cycle = _problem(em, "448V")
    assert grid.nE * 16 >= 2 ** 32
    vm = em.VolumeModel(grid, model, sfield)
    var = MGParameters(verb=0, cycle=cycle, sslsolver=False, linerelaxation=True, semicoarsening=True,
                       vnC=grid.vnC, ordering='colour')
    e0 = _smooth_field(grid, 7)
    s = em.SourceField(grid, np.array(_smooth_field(grid, 8)) * 1e-3, freq=1.0)
    eta = [np.asfortranarray(a) for a in (vm.eta_x, vm.eta_y, vm.eta_z)]
    zeta = np.asfortranarray(vm.zeta)
    names = {}
    with DeviceMG(grid, vm, np.complex128) as dev:
        dev.set_params(var)
        dev.set_sfield(s)
        for direction in (1, 2, 3):
            dev.set_efield(e0)
            dev.smooth(1, direction)
            got = dev.get_efield()
            names[direction] = dev.last_sweep_kernel()
            ref = np.array(e0)
            oracle.gauss_seidel(grid.vnC, ref, np.array(s), *eta, zeta, *grid.h, 1, direction=direction, order=1)
            assert relerr(got, ref) < SWEEP_RTOL, (direction, names[direction], relerr(got, ref))
            assert relerr(got, np.array(e0)) > 1e-3
            del got, ref
    print("kernels:", names)
    assert all(v.startswith("k_line_sweep_qc_big") for v in names.values()), names
    del e0, s
    e, info = em.solve(grid, model, sfield, cycle=cycle, semicoarsening=True, linerelaxation=True,
                       return_info=True, maxit=3, verb=0)
    assert np.all(np.isfinite(info['error_at_cycle'])) and np.all(np.diff(info['error_at_cycle']) < 0)
    assert info['error_at_cycle'][-1] < 0.5 * info['ref_error']
    om = oracle.Mesh(grid.h, grid.origin)
    ov = oracle.VModel(vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta)
    l2 = oracle.residual(om, ov, np.array(sfield), np.array(e), True, fast=True)
    assert abs(l2 / info['abs_error'] - 1) < 1e-6


def test_placement_of_working_copies_changes_no_bit(monkeypatch):
    """256^3 (BASELINE configs[2]): the handle times candidate blocks for the working copies its level-0 sweeps write and keeps
    the fastest (MG::place_level0, HISTORY R6.1).  Which block a sweep runs on must not change a bit: three V-cycles with the search
    (default) and without (EMG3D_PLACE_TRIES=0) give identical norms and fields; the record says what was tried; a second
    handle of the process takes the blocks the first one found (DevicePool role tags) without searching."""
    import emg3d_amd as em
    from emg3d_amd import _lib
    from emg3d_amd.solver import DeviceMG, MGParameters
    import bench
    grid, model, sfield, cycle = _problem(em, "256V")
    vm = em.VolumeModel(grid, model, sfield)
    var = MGParameters(verb=0, cycle=cycle, sslsolver=False, linerelaxation=True, semicoarsening=True, vnC=grid.vnC, ordering='colour')

    def run(tries):
        if tries is None:
            monkeypatch.delenv("EMG3D_PLACE_TRIES", raising=False)
        else:
            monkeypatch.setenv("EMG3D_PLACE_TRIES", str(tries))
        with DeviceMG(grid, vm, np.complex128) as dev:
            dev.set_params(var); dev.set_sfield(sfield); dev.set_efield(None)
            norms = dev.cycles(3, bench.SC_CYCLE, bench.LR_CYCLE)
            return np.array(norms), dev.get_efield(), dev.placement()

    _lib.load().emg3d_hip_release_cached()
    n0, e0, p0 = run(0)
    assert p0 == {}
    _lib.load().emg3d_hip_release_cached()          # (no parked blocks: the next handle must search)
    n1, e1, p1 = run(None)
    assert set(p1) == {"x", "yz"}, p1
    for v in p1.values():
        assert 1 <= v["tries"] <= 12 and 0 <= v["kept"] < v["tries"] and v["kept_ms"] == min(v["ms_per_sweep"]) and v["kept_ms"] > 0, p1
    assert np.array_equal(n0, n1) and np.array_equal(np.asarray(e0), np.asarray(e1))
    n2, e2, p2 = run(None)                          # the pool now holds the placed blocks under their roles
    assert p2 == {"x": {"tries": 0, "kept": -1, "reused": True}, "yz": {"tries": 0, "kept": -1, "reused": True}}, p2
    assert np.array_equal(n0, n2) and np.array_equal(np.asarray(e0), np.asarray(e2))


@pytest.mark.parametrize("case", ["laplace_f64", "eager_launches", "two_systems"])
def test_placement_in_the_other_modes_changes_no_bit(monkeypatch, case):
    """The placement search on the paths the test above does not take: a float64 (Laplace-domain) handle -- working copies of 403 MB --,
    eager launches instead of captured graphs (EMG3D_GRAPH=0: the search runs from prepare()), and a handle that carries two
    systems (working copies of 1.5 GB, the sweeps of both systems timed together).  Two 256^3 V-cycles with and without the search:
    identical norms and fields."""
    import emg3d_amd as em
    from emg3d_amd import _lib
    from emg3d_amd.solver import DeviceMG, MGParameters
    import bench
    freq = -2.0 if case == "laplace_f64" else 1.0
    grid, model, sfield, cycle = _problem(em, "256V", freq)
    vm = em.VolumeModel(grid, model, sfield)
    dtype = np.float64 if case == "laplace_f64" else np.complex128
    assert np.asarray(sfield).dtype == dtype
    var = MGParameters(verb=0, cycle=cycle, sslsolver=False, linerelaxation=True, semicoarsening=True, vnC=grid.vnC, ordering='colour')
    if case == "eager_launches":
        monkeypatch.setenv("EMG3D_GRAPH", "0")

    def run(tries):
        if tries is None:
            monkeypatch.delenv("EMG3D_PLACE_TRIES", raising=False)
        else:
            monkeypatch.setenv("EMG3D_PLACE_TRIES", str(tries))
        _lib.load().emg3d_hip_release_cached()
        with DeviceMG(grid, vm, dtype) as dev:
            dev.set_params(var)
            if case == "two_systems":
                dev.set_batch(2)
                for b, src in enumerate(([0., 0., 0., 30., 10.], [200., -100., 50., 120., -20.])):
                    dev.select(b)
                    dev.set_source(src, sfield.smu0)
            else:
                dev.set_sfield(sfield); dev.set_efield(None)
            norms = dev.cycles(2, bench.SC_CYCLE, bench.LR_CYCLE)
            fields = []
            for b in range(2 if case == "two_systems" else 1):
                if case == "two_systems":
                    dev.select(b)
                fields.append(np.asarray(dev.get_efield()).copy())
            return np.array(norms), fields, dev.placement()

    n0, e0, p0 = run(0)
    n1, e1, p1 = run(None)
    assert p0 == {} and set(p1) == {"x", "yz"} and all(v["tries"] >= 1 for v in p1.values()), (p0, p1)
    assert np.all(np.isfinite(n1)) and np.array_equal(n0, n1)
    for a, b in zip(e0, e1):
        assert np.array_equal(a, b)


def test_512_one_sweep_vs_oracle(oracle):
    """512^3 complex (134 M cells, 6.4 GB per field array): the size README / DESIGN quote a V-cycle for (the 288 GB of one
    device).  One colour-ordered sweep per line direction through k_line_sweep_qc_big (64-bit field offsets, four whole rounds of
    waves) against the strict oracle, element-wise, at the small-size tolerance -- the check of test_448_..., at the size quoted."""
    import emg3d_amd as em
    from emg3d_amd.solver import DeviceMG, MGParameters
    grid, model, sfield, cycle = _problem(em, "512V")
    assert grid.nE * 16 >= 2 ** 32
    vm = em.VolumeModel(grid, model, sfield)
    var = MGParameters(verb=0, cycle=cycle, sslsolver=False, linerelaxation=True, semicoarsening=True,
                       vnC=grid.vnC, ordering='colour')
    e0 = _smooth_field(grid, 7)
    s = em.SourceField(grid, np.array(_smooth_field(grid, 8)) * 1e-3, freq=1.0)
    eta = [np.asfortranarray(a) for a in (vm.eta_x, vm.eta_y, vm.eta_z)]
    zeta = np.asfortranarray(vm.zeta)
    del model
    names = {}
    with DeviceMG(grid, vm, np.complex128) as dev:
        dev.set_params(var)
        dev.set_sfield(s)
        for direction in (1, 2, 3):
            dev.set_efield(e0)
            dev.smooth(1, direction)
            got = dev.get_efield()
            names[direction] = dev.last_sweep_kernel()
            ref = np.array(e0)
            oracle.gauss_seidel(grid.vnC, ref, np.array(s), *eta, zeta, *grid.h, 1, direction=direction, order=1)
            assert relerr(got, ref) < SWEEP_RTOL, (direction, names[direction], relerr(got, ref))
            assert relerr(got, np.array(e0)) > 1e-3
            del got, ref
    print("kernels:", names)
    assert all(v.startswith("k_line_sweep_qc_big") for v in names.values()), names


@pytest.mark.parametrize("nz,expect", [(704, "k_line_sweep_thm"), (768, "k_line_sweep_rp")])
def test_factor_offset_boundary_selects_the_right_kernel(oracle, nz, expect):
    """The two-sided kernel forms its factor offsets in 32 bits: the whole factor of a direction must stay below 4 GiB
    (sweep_twist_ok, csrc/sweep_plan.hpp).  160 x 160 x 704 (z-lines: 25 281 lines x 704 blocks x 240 B = 4.27e9 B) is just inside, 160 x 160 x 768
    (4.66e9 B) beyond -- there the one-sided k_line_sweep_rp (64-bit block pointer, 32-bit offsets within a block record)
    must serve.  Selected kernel by name, and the z-line sweep against the strict oracle on both sides."""
    import emg3d_amd as em
    from types import SimpleNamespace
    from emg3d_amd.solver import DeviceMG, MGParameters
    shape = (160, 160, nz)
    rng = np.random.default_rng(nz)
    h = [rng.uniform(20., 40., n) * 1.01 ** np.abs(np.arange(n) - n / 2) for n in shape]
    grid = em.TensorMesh(h, origin=(0., 0., 0.))
    vol = grid.cell_volumes.reshape(grid.vnC, order='F')
    sig = [10 ** rng.uniform(-1, 1, shape) for _ in range(3)]
    smu0 = em.SourceField(grid, freq=1.0).smu0
    eta = [np.asfortranarray(smu0 * vol * s_) for s_ in sig]
    zeta = np.asfortranarray(vol)
    e0 = em.Field(grid, rng.standard_normal(grid.nE) + 1j * rng.standard_normal(grid.nE), freq=1.0)
    e0.ensure_pec
    s = em.SourceField(grid, (rng.standard_normal(grid.nE) + 1j * rng.standard_normal(grid.nE)) * 1e-6, freq=1.0)
    var = MGParameters(verb=0, cycle='V', sslsolver=False, linerelaxation=True, semicoarsening=True, vnC=grid.vnC,
                       ordering='colour')
    with DeviceMG(grid, SimpleNamespace(eta_x=eta[0], eta_y=eta[1], eta_z=eta[2], zeta=zeta), np.complex128) as dev:
        dev.set_params(var)
        dev.set_sfield(s)
        dev.set_efield(e0)
        dev.smooth(1, 3)
        got = dev.get_efield()
        name = dev.last_sweep_kernel()
    ref = np.array(e0)
    oracle.gauss_seidel(grid.vnC, ref, np.array(s), *eta, zeta, *grid.h, 1, direction=3, order=1)
    assert name.startswith(expect), name
    assert relerr(got, ref) < SWEEP_RTOL, (name, relerr(got, ref))


_SNAPSHOT_WORKER = """
import sys
sys.path.insert(0, {root!r})
import torch        # first: its HIP runtime is the one the process uses
import numpy as np
import bench
import emg3d_amd as em
from emg3d_amd import shard
from emg3d_amd.solver import DeviceMG, MGParameters
grid, model, sfield, cycle = bench.build_problem(em, "128F", 1.0)
vm = em.VolumeModel(grid, model, sfield)
var = MGParameters(verb=0, cycle=cycle, sslsolver=False, linerelaxation=True, semicoarsening=True, vnC=grid.vnC,
                   ordering='colour')
with DeviceMG(grid, vm, np.complex128) as dev:
    dev.set_params(var); dev.set_sfield(sfield); dev.set_efield(None)
    dev.cycles(2, [1, 2, 3], [4, 5, 6])
    t1 = shard.efield_tensor(dev)          # (no host synchronisation: torch's current stream waits for the handle's stream)
    kept = t1.clone()
    assert np.array_equal(kept.cpu().numpy().view(np.complex128), np.asarray(dev.get_efield()))
    dev.cycles(1, [3], [6])
    t2 = shard.efield_tensor(dev)          # fetched again: the current field
    got2 = t2.cpu().numpy().view(np.complex128).copy()
    now = np.asarray(dev.get_efield())
    assert np.array_equal(got2, now)
    assert not np.array_equal(kept.cpu().numpy().view(np.complex128), now)
    assert t2.data_ptr() == dev.efield_devptr
print("snapshot ok")
"""


def test_efield_device_pointer_is_a_snapshot(tmp_path):
    """emg3d_mg_efield_devptr / shard.efield_tensor on a level that keeps its field in the x-split working copy between
    cycles (128^3, colour order: MG::home_on): every fetch converts the field back into the reference-layout buffer, so a
    tensor fetched AFTER further cycles equals get_efield, while one kept from before is the earlier state (documented:
    valid until the next cycle).  In a process of its own: torch must initialise the HIP runtime before the library does."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "snapshot_worker.py"
    script.write_text(_SNAPSHOT_WORKER.format(root=root))
    p = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "snapshot ok" in p.stdout
