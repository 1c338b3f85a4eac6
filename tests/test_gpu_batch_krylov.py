"""GPU: batched Krylov solves -- the batched vector workspace (emg3d_mg_bvec_*) and solver.solve_sources(sslsolver=...).
The reference solves one (source, frequency) pair per solver.solve call, with BiCGSTAB around the multigrid cycle as
the survey default (simulations.py:198-200); here the sources of one frequency go through the Krylov iteration in
lockstep on one handle.  The contract is that of tests/test_gpu_batch.py: batching is invisible -- every primitive gives
each system bit for bit what the single-system primitive gives on that system's vectors, and every system of
solve_sources gets bit for bit the field and the info_dict of a solve() of its own."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _grid_model(em, shape, seed=0, stretch=1.04):
    rng = np.random.default_rng(seed)
    h = [40.0 * stretch ** np.abs(np.arange(n) - n / 2 + 0.5) for n in shape]
    grid = em.TensorMesh(h, origin=tuple(-hh.sum() / 2 for hh in h))
    rho = 10 ** rng.uniform(-0.5, 2.0, grid.nC)
    model = em.Model(grid, rho, 1.5 * rho, 2 * rho)
    return grid, model


# four dipoles at clearly different distances from the grid centre (fractions of the half extents) ...
_PLACES = [(0.0, 0.0, 0.0, 0.0, 0.0), (0.2, -0.15, 0.1, 40.0, 15.0), (-0.5, 0.4, -0.3, 130.0, -35.0),
           (0.8, -0.7, 0.6, 250.0, 70.0)]
# ... and of different strengths
_STRENGTHS = [1.0, 50.0, 0.01, 1000.0]


def _sources(grid):
    half = [np.sum(h) / 2 for h in grid.h]
    return [[fx * half[0], fy * half[1], fz * half[2], azm, dip] for fx, fy, fz, azm, dip in _PLACES]


def _handle(em, grid, model, freq, nsys=1):
    from emg3d_amd import models
    from emg3d_amd.solver import DeviceMG
    proto = em.SourceField(grid, freq=freq)
    dev = DeviceMG(grid, models.VolumeModel(grid, model, proto), proto.dtype)
    if nsys > 1:
        dev.set_batch(nsys)
    return dev


# --------------------------------------------------------------------------- primitives
def _random(rng, n, dtype):
    v = rng.standard_normal(n)
    return (v + 1j * rng.standard_normal(n)).astype(dtype) if np.dtype(dtype).kind == 'c' else v


@pytest.mark.parametrize("freq", [1.0, -2.0])                       # complex128 / float64 kernels
@pytest.mark.parametrize("shape", [(12, 10, 8),                     # nE below one grid's worth of threads
                                   (80, 72, 64)])                   # nE = 1 137 112 > 4096 * 256: both grid-stride loops go round twice
def test_primitives_bitwise(shape, freq):
    import emg3d_amd as em
    grid, model = _grid_model(em, shape)
    nsys = 3
    rng = np.random.default_rng(11)
    with _handle(em, grid, model, freq) as one, _handle(em, grid, model, freq, nsys) as dev:
        dt, nE = dev.dtype, dev.nE
        if shape == (80, 72, 64):
            assert nE == 1137112
        cplx = dt.kind == 'c'
        a = [_random(rng, nE, dt) for _ in range(nsys)]
        c = [_random(rng, nE, dt) for _ in range(nsys)]
        alpha = [complex(*rng.standard_normal(2)) if cplx else float(rng.standard_normal()) for _ in range(nsys)]
        beta = [complex(*rng.standard_normal(2)) if cplx else float(rng.standard_normal()) for _ in range(nsys)]

        def reference(b):
            """axpy, scale, dot, norm, copy, amatvec of the single-system workspace on system b's vectors."""
            one.vec_alloc(4)
            one.vec_set(0, a[b])
            one.vec_set(1, c[b])
            one.vec_axpy(0, alpha[b], 1)
            r = {'axpy': one.vec_get(0)}
            one.vec_scale(0, beta[b])
            r['scale'] = one.vec_get(0)
            r['dot'] = one.vec_dot(0, 1)
            r['dot_aa'] = one.vec_dot(0, 0)
            r['norm'] = one.vec_norm(0)
            one.vec_copy(2, 0)
            r['copy'] = one.vec_get(2)
            one.vec_amatvec(3, 0)
            r['amatvec'] = one.vec_get(3)
            return r

        ref = [reference(b) for b in range(nsys)]
        before = dev.device_bytes
        dev.bvec_alloc(4)
        assert dev.device_bytes - before >= 4 * nsys * nE * dt.itemsize        # device_bytes counts the workspace
        with pytest.raises(RuntimeError):
            dev.set_batch(2)                                                    # refused once batched vectors exist

        def run(systems, sentinel=None):
            got = {}
            for b in range(nsys):
                dev.bvec_set(0, b, a[b])
                dev.bvec_set(1, b, c[b])
            dev.bvec_axpy(0, alpha, 1)
            got['axpy'] = [dev.bvec_get(0, b) for b in range(nsys)]
            dev.bvec_scale(0, beta)
            got['scale'] = [dev.bvec_get(0, b) for b in range(nsys)]
            out = None if sentinel is None else np.full(nsys, sentinel, dtype=dt)
            got['dot'] = dev.bvec_dot(0, 1, out=out)
            out = None if sentinel is None else np.full(nsys, sentinel, dtype=dt)
            got['dot_aa'] = dev.bvec_dot(0, 0, out=out)
            dev.bvec_copy(2, 0)
            got['copy'] = [dev.bvec_get(2, b) for b in range(nsys)]
            dev.bvec_amatvec(3, 0)
            got['amatvec'] = [dev.bvec_get(3, b) for b in range(nsys)]
            for b in systems:
                for key in ('axpy', 'scale', 'copy', 'amatvec'):
                    np.testing.assert_array_equal(got[key][b], ref[b][key], err_msg=f"{key}, system {b}")
                for key in ('dot', 'dot_aa'):
                    assert (complex(got[key][b]) if cplx else float(got[key][b])) == ref[b][key], (key, b)
                assert float(np.sqrt(abs(complex(got['dot_aa'][b]) if cplx else float(got['dot_aa'][b])))) == ref[b]['norm']
            return got

        run(range(nsys))
        # the whole level-0 arrays as batched vectors: -1 the sources, -2 the fields
        dev.bvec_copy(dev.SFIELD, 0)
        dev.bvec_copy(dev.EFIELD, 2)
        for b in range(nsys):
            dev.select(b)
            np.testing.assert_array_equal(dev.vec_get(dev.SFIELD), ref[b]['scale'])
            np.testing.assert_array_equal(dev.get_efield(), ref[b]['copy'])
            np.testing.assert_array_equal(dev.bvec_get(dev.EFIELD, b), ref[b]['copy'])
        # the middle system frozen: its vectors and its dot slot stay what they are
        for v in range(2, 4):
            dev.bvec_set(v, 1, np.full(nE, 3.0, dtype=dt))
        dev.set_mask([1, 0, 1])
        got = run([0, 2], sentinel=-7.5)
        for key in ('axpy', 'scale'):
            np.testing.assert_array_equal(got[key][1], a[1])            # as uploaded: neither updated nor scaled
        for key in ('copy', 'amatvec'):
            assert np.all(got[key][1] == 3.0)
        assert got['dot'][1] == -7.5 and got['dot_aa'][1] == -7.5
        dev.bvec_zero(2)
        assert np.all(dev.bvec_get(2, 1) == 3.0) and not np.any(dev.bvec_get(2, 0)) and not np.any(dev.bvec_get(2, 2))
        dev.set_mask([1, 1, 1])
        # the single-system workspace keeps its meaning on the batched handle: nE-sized, the selected system
        dev.select(2)
        dev.vec_alloc(1)
        dev.vec_copy(0, dev.SFIELD)
        np.testing.assert_array_equal(dev.vec_get(0), ref[2]['scale'])


# --------------------------------------------------------------------------- solve_sources(sslsolver=...)
# Tolerances: with the default 1e-6 every source of these small grids is done after one Krylov iteration.  The tighter ones make
# the sources stop at different iterations (CPU oracle, it_ssl / it_mg per source -- F-sclr-bicgstab, 1e-10: 2, 2, 2, 3 / 12, 14,
# 15, 14, the first source leaving through a breakdown test; V-sclr-cgs, 1e-8: 5, 3, 3, 3 / 34, 18, 18, 18, the first source's
# preconditioner DIVERGES: the per-system failure path; Laplace, 1e-10: 2, 2, 2, 3 / 12, 14, 15, 14), and in each the cycle
# counts are no common multiple of the iterations: inner calls ended early, the rotation drifted.
# test_cases_exercise_freezing_and_rotation_drift checks both conditions on the single solves of the GPU.
CASES = {
    'F-sclr-bicgstab': dict(shape=(32, 24, 16), freq=1.0, kw=dict(cycle='F', semicoarsening=True, linerelaxation=True,
                                                                  sslsolver='bicgstab', tol=1e-10)),
    'F-plain-lex-bicgstab': dict(shape=(32, 24, 16), freq=1.0, kw=dict(cycle='F', sslsolver='bicgstab', ordering='lex')),
    'V-sclr-cgs': dict(shape=(24, 40, 12), freq=1.0, kw=dict(cycle='V', semicoarsening=True, linerelaxation=True,
                                                             sslsolver='cgs', tol=1e-8)),
    'nocycle-bicgstab': dict(shape=(16, 16, 32), freq=1.0, kw=dict(cycle=None, maxit=300, sslsolver='bicgstab')),
    'F-sclr-bicgstab-laplace': dict(shape=(32, 24, 16), freq=-2.0, kw=dict(cycle='F', semicoarsening=True,
                                                                           linerelaxation=True, sslsolver='bicgstab',
                                                                           tol=1e-10)),
    'maxit1': dict(shape=(32, 24, 16), freq=1.0, kw=dict(cycle='F', semicoarsening=True, linerelaxation=True,
                                                         sslsolver=True, maxit=1)),
}
_REF = {}


def _problem(em, name):
    case = CASES[name]
    grid, model = _grid_model(em, case['shape'])
    sfields = [em.get_source_field(grid, src, case['freq'], strength=st) for src, st in zip(_sources(grid), _STRENGTHS)]
    return grid, model, sfields


def _reference(em, name):
    """One solve() per source on a fresh handle each: computed once per case, shared, never modified."""
    if name not in _REF:
        grid, model, sfields = _problem(em, name)
        _REF[name] = [em.solve(grid, model, sf, return_info=True, verb=0, **CASES[name]['kw']) for sf in sfields]
    return _REF[name]


def _same_info(got, want):
    for key in ('exit', 'exit_message', 'it_mg', 'it_ssl'):
        assert got[key] == want[key], (key, got[key], want[key])
    for key in ('abs_error', 'rel_error', 'ref_error'):                             # (NaN for a zero source)
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    np.testing.assert_array_equal(got['error_at_cycle'], want['error_at_cycle'])
    assert len(got['runtime_at_cycle']) == len(want['runtime_at_cycle'])


@pytest.mark.parametrize("name", list(CASES))
def test_solve_sources_krylov_equals_separate_solves(name):
    import emg3d_amd as em
    from emg3d_amd.solver import solve_sources
    grid, model, sfields = _problem(em, name)
    ref = _reference(em, name)
    efs, infos = solve_sources(grid, model, sfields, CASES[name]['freq'], verb=0, **CASES[name]['kw'])
    print(name, "it_ssl", [i['it_ssl'] for _, i in ref], "it_mg", [i['it_mg'] for _, i in ref],
          [i['exit_message'] for _, i in ref])
    for b, (e, info) in enumerate(ref):
        np.testing.assert_array_equal(np.array(efs[b]), np.array(e), err_msg=f"system {b}")
        _same_info(infos[b], info)
    if name == 'maxit1':
        assert all(i['exit_message'] == "MAX. ITERATION REACHED, NOT CONVERGED" and i['it_ssl'] == 1 for i in infos)
    else:
        assert all(i['it_ssl'] > 0 for i in infos)


def test_cases_exercise_freezing_and_rotation_drift():
    """The reference side decides whether the cases above test what they are meant to: the sources of a case with
    semicoarsening and line relaxation must stop at different Krylov iterations (systems are frozen while others
    iterate), and their multigrid cycle counts must not all be the same multiple of their Krylov iterations (a
    preconditioner call ended early for some system, so the systems entered the next one at different points of the
    direction rotation)."""
    import emg3d_amd as em
    froze, drifted = [], []
    for name in ('F-sclr-bicgstab', 'V-sclr-cgs', 'F-sclr-bicgstab-laplace'):
        infos = [i for _, i in _reference(em, name)]
        it_ssl = [i['it_ssl'] for i in infos]
        ratio = [i['it_mg'] / i['it_ssl'] for i in infos]
        if len(set(it_ssl)) > 1:
            froze.append(name)
        if len(set(ratio)) > 1:
            drifted.append(name)
    print("freezing in", froze, "; rotation drift in", drifted)
    assert froze and drifted


def test_solve_sources_krylov_zero_source():
    import emg3d_amd as em
    from emg3d_amd.solver import solve_sources
    grid, model, sfields = _problem(em, 'F-sclr-bicgstab')
    ref = _reference(em, 'F-sclr-bicgstab')
    kw = CASES['F-sclr-bicgstab']['kw']
    zero = em.SourceField(grid, freq=1.0)
    efs, infos = solve_sources(grid, model, [sfields[1], zero, sfields[3]], 1.0, verb=0, **kw)
    for b, k in ((0, 1), (2, 3)):
        np.testing.assert_array_equal(np.array(efs[b]), np.array(ref[k][0]))
        _same_info(infos[b], ref[k][1])
    e, info = em.solve(grid, model, zero, return_info=True, verb=0, **kw)
    assert not np.any(np.array(efs[1])) and not np.any(np.array(e))
    _same_info(infos[1], info)
    assert infos[1]['exit'] == 0 and infos[1]['it_ssl'] == 0 and infos[1]['it_mg'] == 0


# --------------------------------------------------------------------------- receivers, reuse, surveys
_REC = (np.array([100., -150., 60.]), np.array([50., 20., -80.]), np.array([-40., 10., 30.]), 30., 10.)


def test_receivers_on_device_and_handle_reuse():
    """rec= with download=False: the responses come from the solutions in the handle; two calls on one handle= equal
    two fresh calls (the workspace persists, every call starts from zero)."""
    import emg3d_amd as em
    from emg3d_amd.solver import solve_sources
    grid, model = _grid_model(em, (32, 24, 16))
    srcs = _sources(grid)
    kw = dict(cycle='F', semicoarsening=True, linerelaxation=True, sslsolver='bicgstab', verb=0)
    first, second = srcs[:3], [srcs[3], srcs[0], srcs[2]]
    fresh = [solve_sources(grid, model, s, 1.0, strength=2.0, rec=_REC, **kw) for s in (first, second)]
    for efs, infos, resp in fresh:
        for b in range(3):
            np.testing.assert_array_equal(resp[b], em.get_receiver_response(grid, efs[b], _REC))
    from emg3d_amd import fields, solver
    spec = fields.FrequencySpec(1.0)
    with solver.DeviceMG.from_model(grid, solver._exact_parts(grid, model, spec.smu0), spec) as dev:
        for s, (efs, infos, resp) in zip((first, second), fresh):
            none, infos2, resp2 = solve_sources(grid, None, s, 1.0, strength=2.0, rec=_REC, download=False, handle=dev, **kw)
            assert none is None
            np.testing.assert_array_equal(resp2, resp)
            for b in range(3):
                _same_info(infos2[b], infos[b])
                dev.select(b)
                np.testing.assert_array_equal(dev.get_efield(), np.array(efs[b]))      # the solutions stay in the handle


def test_solve_survey_with_krylov_solver():
    """3 sources x 2 frequencies, two sources per launch (a ragged last chunk), handles reused from frequency to frequency."""
    import emg3d_amd as em
    from emg3d_amd import shard
    grid, model = _grid_model(em, (16, 24, 16), seed=4)
    srcs = _sources(grid)[:3]
    freqs = [0.5, 2.0]
    kw = dict(cycle='F', semicoarsening=True, linerelaxation=True, sslsolver='bicgstab', verb=0)
    resp, infos = shard.solve_survey(grid, model, srcs, freqs, _REC, batch=2, **kw)
    assert resp.shape == (3, 2, 3)
    for i, src in enumerate(srcs):
        for j, f in enumerate(freqs):
            e, info = em.solve(grid, model, em.SourceField(grid, freq=f), source=(src, 0), return_info=True, **kw)
            np.testing.assert_array_equal(resp[i, j], em.get_receiver_response(grid, e, _REC))
            _same_info(infos[i][j], info)


def test_what_is_not_batched_raises():
    import emg3d_amd as em
    from emg3d_amd.solver import solve_sources
    grid, model = _grid_model(em, (16, 16, 16))
    srcs = _sources(grid)[:2]
    with pytest.raises(ValueError, match="'bicgstab' and 'cgs'"):
        solve_sources(grid, model, srcs, 1.0, sslsolver='gcrotmk', verb=0)
    with _handle(em, grid, model, 1.0, nsys=2) as dev:
        with pytest.raises(ValueError, match="resident"):
            solve_sources(grid, None, None, 1.0, sslsolver='bicgstab', handle=dev, resident=2, verb=0)
