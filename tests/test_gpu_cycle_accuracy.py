"""GPU: the accuracy of whole multigrid solves on a high-contrast model, against an extended-precision truth.

Every other test that runs more than one kernel in a row draws a benign model (rho = 10**U(-0.3, 1) or milder) and asks for parity with
the float64 oracle at 1e-11.  Here the model is the layered marine one of tests/_hard_models.py -- air at 1e-8 S/m over sea water at
3 S/m, a resistive block in the sediments, widths stretched by 1.25 per cell -- so that the restriction of the residual, the sums of
the coarse models, the factorisation of their lines, the prolongation and the recursion that chains them see seven orders of
magnitude of contrast between neighbouring cells on every level.  On such a model the float64 oracle itself is 3e-9 ... 3e-7 from the
same solve in x87 extended precision (tests/test_oracle_cycle_truth.py), so the yardstick is that of tests/test_gpu_accuracy.py:

    err(hip) <= 10 * max(err(float64 oracle), 16 * 2^-53)            (hc.bound; the comparison value is never a HIP result)

for four measures of a run of six cycles: the residual norm after every smoothing call of every level and error_at_cycle (both as
|norm - truth's| / ||s||), the A-norm of the field error ||A (e - e_truth)|| / ||s||, and the field's max-norm error.  The sequence
of smoothing calls must be exactly the truth's.  Every case prints one line per measure,
`[cycle-accuracy] shape cycle dtype ordering measure err(ref) err(hip) ratio`, ratio = err(hip) / max(err(ref), floor): what is held
below 10.  A failure names the first smoothing call whose norm leaves the bound and the sweep kernels of that level's shape.

The bit-for-bit contracts of the product -- device-formed eta against host arrays, batched sources against single solves, a
re-targeted handle against a fresh one, graph replay against eager launches -- were only ever checked on benign models: one case of
each runs on the layered model."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import _depth
import _hard_cases as hc
import _hard_models as hm

pytestmark = pytest.mark.gpu

KW = dict(cycle='F', **hm.SCLR)
SOLVE = dict(sslsolver=False, maxit=hm.MAXIT, tol=hm.TOL, verb=0, ordering='colour', return_info=True)


@pytest.fixture(scope="module")
def em():
    import emg3d_amd
    return emg3d_amd


@pytest.fixture(scope="module")
def orc(oracle):
    if not oracle.has_extended():
        pytest.skip("np.longdouble is not the x87 extended format (64-bit significand in 16 bytes)")
    return oracle


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in [k for k in os.environ if k.startswith("EMG3D_") and k != "EMG3D_HIP_LIB"]:
        monkeypatch.delenv(k)


class OffTheBound(AssertionError):
    """A measure above hc.bound: the only failure the expected-failure marks below stand for."""


def _grid(em, p):
    return em.TensorMesh([np.array(h) for h in p['h']], origin=(0., 0., 0.))


def _device(em, p, case):
    """The case's six cycles on a handle fed with the problem's arrays: a run as _hard_models.oracle_run returns it."""
    vm = SimpleNamespace(eta_x=p['eta'][0], eta_y=p['eta'][1], eta_z=p['eta'][2], zeta=p['zeta'])
    records, norms, errs, e = _depth.device_run(em, _grid(em, p), None, p['s'], case["ordering"], maxit=hm.MAXIT, vmodel=vm,
                                                **hm.solve_kw(case))
    return dict(records=records, norms=norms, errs=errs, field=e)


def _held_to_the_truth(em, orc, case, p, ref, truth, run, e_ref):
    """Records exactly the truth's; the four measures within hc.bound of the float64 oracle's; one printed line per measure."""
    what = hm.case_id(case)
    _depth.assert_same_records(run["records"], truth["records"], what)
    assert np.isfinite(run["field"]).all() and np.isfinite(run["norms"]).all()
    assert abs(run["errs"][0] - truth["errs"][0]) <= 1e-14 * truth["errs"][0]
    e_hip = hm.errors(orc, run, truth, p)
    nx, ny, nz = case["shape"]
    bad = []
    for m in hm.MEASURES:
        ratio = e_hip[m] / max(e_ref[m], hc.FLOOR)
        print(f"[cycle-accuracy] {nx}x{ny}x{nz} {case['cycle']} {hc.tname(case['dtype'])} {case['ordering']}"
              f"{'' if case['kw'] == hm.SCLR else ' point'} {m} err(ref) {e_ref[m]:.2e} err(hip) {e_hip[m]:.2e} ratio {ratio:.2f}")
        if not e_hip[m] <= hc.bound(e_ref[m]):
            bad.append((m, e_ref[m], e_hip[m], round(ratio, 2)))
    if bad:
        over = np.flatnonzero(hm.visit_errors(run, truth) > hc.bound(e_ref["visit"]))
        first = "no smoothing call leaves the bound of the per-visit norms"
        kernels = ""
        if over.size:
            k = int(over[0])
            rec = truth["records"][k]
            first = (f"first smoothing call off the bound: call {k}, (cycle, level, it, cycmax, kind, vnC) = {rec}, norm "
                     f"{run['norms'][k]:.17e} against {truth['norms'][k]:.17e}")
            kernels = "\nsweep kernels of that level's shape:\n" + _depth.sweep_kernels(em, [rec], case["dtype"], case["ordering"],
                                                                                      **hm.solve_kw(case))
        raise OffTheBound(f"{what}: (measure, err(ref), err(hip), ratio) = {bad}; {first}{kernels}")


# What the cases found on an MI355X (profiles/HISTORY.md, part T): wherever the smoothing is line relaxation on a grid
# with an air LAYER -- more than one cell of air above the water, at least 8 cells across --, the field measure sits at 1.0 x the
# float64 oracle's error and the three residual measures 1e5 ... 1e8 x above it: the line solves of the scan kernel
# (k_line_sweep_qpl, every level of these grids) are not backward stable on the nearly singular lines of the air layer and leave a
# residual of 1e-7 ... 1e-6 ||s|| there, which every later visit inherits.  Isolated per kernel family and direction in
# tests/test_gpu_accuracy.py::test_layered_sweep_residual: the one-sided eliminations leave the oracle's 1e-13.  The thin grids
# (one cell of air, converged to rounding) and the point smoother meet the bound at ratios <= 6.6.
# id -> ratio err(hip) / max(err(float64 oracle), floor) of (anorm, visit, cycle) as measured; the bound is 10.
KNOWN = {
    "16x16x16-F-c128-colour": (1.7e6, 5.5e5, 6.5e6), "16x16x16-F-f64-colour": (1.5e6, 1.1e6, 4.9e6),
    "32x16x8-F-c128-colour": (5.1e6, 3.0e7, 1.9e8), "32x16x8-F-f64-colour": (1.6e7, 4.0e7, 2.3e8),
    "24x12x20-V-c128-colour": (6.3e5, 1.8e5, 2.1e5), "24x12x20-V-f64-colour": (6.3e5, 2.9e5, 5.9e5),
    "16x16x16-F-c128-lex": (1.1e6, 1.4e6, 8.6e6), "16x16x16-F-f64-lex": (1.3e6, 3.8e6, 2.4e7),
    "24x12x20-V-c128-lex": (3.8e5, 3.7e4, 5.7e4), "24x12x20-V-f64-lex": (3.7e5, 1.4e5, 2.6e5),
}
KNOWN_SOLVE = {"c128": (1.9e6, 1.8e6, 5.4e6), "f64": (2.0e6, 1.2e6, 1.3e7)}


def _known(ratios):
    """The strict expected-failure mark of a case with the defect: for a measure above the bound only (a wrong sequence of smoothing
    calls or a broken bit-for-bit contract still fails), and it turns into a failure the day the case meets the bound."""
    if ratios is None:
        return []
    return [pytest.mark.xfail(strict=True, raises=OffTheBound, reason=(
        "scan-kernel line solves leave 1e-7 ... 1e-6 ||s|| of residual in the air layer (test_gpu_accuracy.py::"
        "test_layered_sweep_residual, profiles/HISTORY.md part T); field ratio 1.0, measured ratios anorm / visit / cycle = "
        + " / ".join(f"{r:.1e}" for r in ratios) + ", bound 10"))]


@pytest.mark.parametrize("case", [pytest.param(c, marks=_known(KNOWN.get(hm.case_id(c))), id=hm.case_id(c)) for c in hm.ALL_CASES])
def test_cycles_against_the_truth(em, orc, case):
    p, ref, truth = hm.references(orc, case)
    _held_to_the_truth(em, orc, case, p, ref, truth, _device(em, p, case), hm.reference_errors(orc, case))


# ---- the bit-for-bit contracts, on the layered model ------------------------------------------------------------------------------
def _em_problem(em, shape, dtype, freq=None):
    """The layered model as an em.Model (conductivities, anisotropy, mu_r) on its grid, and the frequency of `dtype`."""
    p = hm.layered(shape, dtype)
    grid = _grid(em, p)
    f = hc.ANISOTROPY
    model = em.Model(grid, f[0] * p['sigma'], f[1] * p['sigma'], f[2] * p['sigma'], mu_r=p['mu_r'], mapping='Conductivity')
    return p, grid, model, (freq or hc.FREQ) if np.dtype(dtype) == np.complex128 else -hc.S_LAPLACE


def _dipole(grid, shape, ix=None, iy=None):
    """An x-directed point dipole on the sea floor, centred on a node: its 1 m lie on two x-edges."""
    nx, ny, nz = shape
    return [float(grid.nodes_x[nx // 2 if ix is None else ix]), float(grid.nodes_y[ny // 2 if iy is None else iy]),
            float(grid.nodes_z[nz // 2]), 0., 0.]


def _sfield(em, grid, shape, freq):
    return em.get_source_field(grid, _dipole(grid, shape), freq)


@pytest.mark.parametrize("dtype", [pytest.param(d, marks=_known(KNOWN_SOLVE[hc.tname(d)]), id=hc.tname(d)) for d in hc.DTYPES])
def test_solve_forms_eta_on_the_device(em, orc, dtype):
    """em.solve on an em.Model of the layered model: eta formed on the device from sigma, V and s mu_0 gives bit for bit the field
    and the norms of a handle fed with the host's VolumeModel arrays, and that run meets the bounds against a truth computed from
    those arrays."""
    shape = (16, 16, 16)
    case = hm._case(shape, 'F', dtype)
    _, grid, model, freq = _em_problem(em, shape, dtype)
    sfield = _sfield(em, grid, shape, freq)
    assert np.count_nonzero(np.array(sfield)) == 2
    e, info = em.solve(grid, model, sfield, **KW, **SOLVE)
    assert info['it_mg'] == hm.MAXIT
    vm = em.VolumeModel(grid, model, sfield)
    records, norms, errs, e_dev = _depth.device_run(em, grid, model, sfield, 'colour', maxit=hm.MAXIT, **KW)
    assert np.array_equal(np.array(e), e_dev)
    assert np.array_equal(np.asarray(info['error_at_cycle'], dtype=float), errs)
    p = dict(h=grid.h, eta=[np.asarray(vm.eta_x), np.asarray(vm.eta_y), np.asarray(vm.eta_z)], zeta=np.asarray(vm.zeta),
             s=np.array(sfield))
    assert np.abs(p['eta'][2]).max() / np.abs(p['eta'][2]).min() > 1e8
    _, ref, truth = hm.references(orc, case, p=p, tag="em.solve")
    assert np.all(np.diff(truth["errs"]) < 0)
    _held_to_the_truth(em, orc, case, p, ref, truth, dict(records=records, norms=norms, errs=errs, field=e_dev),
                       hm.errors(orc, ref, truth, p))


def test_batched_sources_equal_single_solves(em):
    """Three sources at different places of the sea floor in one handle: each system is bit for bit its own solve."""
    shape = (32, 16, 8)
    _, grid, model, freq = _em_problem(em, shape, np.complex128)
    srcs = [_dipole(grid, shape, ix, iy) for ix, iy in ((8, 5), (16, 8), (25, 12))]
    efs, infos = em.solve_sources(grid, model, srcs, freq, **KW, **{k: v for k, v in SOLVE.items() if k != 'return_info'})
    fields = []
    for b, src in enumerate(srcs):
        e, info = em.solve(grid, model, em.SourceField(grid, freq=freq), source=(src, 0), **KW, **SOLVE)
        assert infos[b]['it_mg'] == info['it_mg'] == hm.MAXIT
        np.testing.assert_array_equal(infos[b]['error_at_cycle'], info['error_at_cycle'])
        np.testing.assert_array_equal(np.array(efs[b]), np.array(e))
        assert info['error_at_cycle'][-1] < 1e-3 * info['error_at_cycle'][0]
        fields.append(np.array(e))
    assert not np.array_equal(fields[0], fields[1]) and not np.array_equal(fields[1], fields[2])


def test_retargeted_handle_equals_a_fresh_one(em):
    """A handle created at 1 Hz and re-targeted to 0.1 Hz (set_smu0: eta, coarse models and every line factorisation recomputed
    on the device) against a handle created at 0.1 Hz."""
    from emg3d_amd import models
    from emg3d_amd.solver import DeviceMG
    shape = (32, 16, 8)
    _, grid, model, freq = _em_problem(em, shape, np.complex128)
    sfield = _sfield(em, grid, shape, freq)
    e, info = em.solve(grid, model, sfield, **KW, **SOLVE)
    parts = models.model_parts(grid, model, raw=True)
    with DeviceMG.from_model(grid, parts, em.fields.FrequencySpec(1.0)) as dev:
        e1, info1 = em.solve(grid, None, _sfield(em, grid, shape, 1.0), handle=dev, **KW, **SOLVE)       # (it has worked at 1 Hz)
        dev.set_smu0(sfield.smu0)
        e2, info2 = em.solve(grid, None, sfield, handle=dev, **KW, **SOLVE)
    assert info['it_mg'] == info2['it_mg'] == hm.MAXIT
    assert not np.array_equal(np.array(e1), np.array(e))
    assert np.array_equal(np.asarray(info['error_at_cycle']), np.asarray(info2['error_at_cycle']))
    assert np.array_equal(np.array(e), np.array(e2))


def test_graph_replay_equals_eager_launches(em, monkeypatch):
    """16 x 16 x 16 F, six cycles: cycles 4 to 6 replay the graphs captured for the three (sc_dir, lr_dir) pairs."""
    shape = (16, 16, 16)
    _, grid, model, freq = _em_problem(em, shape, np.complex128)
    sfield = _sfield(em, grid, shape, freq)
    e_graph, i_graph = em.solve(grid, model, sfield, **KW, **SOLVE)
    monkeypatch.setenv("EMG3D_GRAPH", "0")
    e_eager, i_eager = em.solve(grid, model, sfield, **KW, **SOLVE)
    assert i_graph['it_mg'] == i_eager['it_mg'] == hm.MAXIT
    assert np.array_equal(np.asarray(i_graph['error_at_cycle']), np.asarray(i_eager['error_at_cycle']))
    assert np.array_equal(np.array(e_graph), np.array(e_eager))
