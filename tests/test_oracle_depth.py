"""Pin the ORACLE's recursion (oracle/oracle.py::multigrid) to the reference at depth: every smoothing call of three W- / F-cycles
on hierarchies of up to seven levels (tests/golden/depth.npz, written by make_depth_golden.py from the reference's own
solver.solve) -- the same sequence of calls and, after each, the same residual norm.  The oracle's colour twin (order=1) runs
the same Python recursion, so this pins the yard-stick of test_gpu_depth.py's colour tests too.  CPU only."""
import numpy as np
import pytest

import _depth
from conftest import relerr


@pytest.fixture(scope="module")
def em():
    import emg3d_amd
    return emg3d_amd


def _case(em, oracle, g, tag):
    vnC, freq, kw = _depth.CASES[tag]
    assert tuple(g[f'{tag}_vnC']) == vnC and float(g[f'{tag}_freq']) == freq and str(g[f'{tag}_kw']) == repr(kw)
    h, _, rho, mu_r = _depth.problem_arrays(vnC)
    np.testing.assert_allclose(_depth.checksum(h, rho, mu_r), g[f'{tag}_check'], rtol=1e-15)
    grid, model, sfield = _depth.problem(em, vnC, freq)
    omesh, omodel = _depth.oracle_problem(oracle, vnC, em.VolumeModel(grid, model, sfield))
    return omesh, omodel, np.array(sfield), kw


def test_fixture_holds_every_case():
    g = _depth.golden()
    assert list(g['cases']) == list(_depth.CASES)
    for tag, (vnC, _, kw) in _depth.CASES.items():
        records = _depth.stored(g, tag)[0]
        if kw['cycle'] == 'W':      # W is distinguishable from F by the number of smoothing calls alone
            assert int(g[f'{tag}_nrec_F']) != len(records)
    # levels 0...6 under W with line relaxation, and five levels of the point smoother
    assert {r[1] for r in _depth.stored(g, 'T1')[0]} == set(range(7))
    assert {r[1] for r in _depth.stored(g, 'P1')[0]} == set(range(5))


@pytest.mark.parametrize("tag", list(_depth.CASES))
def test_oracle_lex_trace_vs_reference(em, oracle, tag):
    """Structure exact; per-visit norms and error_at_cycle by the project's bar (conftest.assert_norms_close on
    [||s||, n_1, n_2, ...]), without any widening; the T cases' fields."""
    g = _depth.golden()
    omesh, omodel, sfield, kw = _case(em, oracle, g, tag)
    records, norms, errs, _, _ = _depth.stored(g, tag)
    orec, onorms, oerrs, oe = _depth.oracle_run(oracle, omesh, omodel, sfield, **kw)
    _depth.assert_same_records(orec, records, tag)
    dev = np.abs(onorms - norms)
    print(f"{tag}: {len(records)} records, max |oracle - reference| = {dev.max() / errs[0]:.1e} ||s||, "
          f"relative {np.max(dev / norms):.1e}")
    _depth.check_norms(onorms, norms, errs[0])
    _depth.check_norms(oerrs[1:], errs[1:], errs[0])
    assert abs(oerrs[0] - errs[0]) <= 1e-14 * errs[0]
    if tag in _depth.WITH_FIELD:
        assert relerr(oe, g[f'{tag}_efield']) < 1e-11


@pytest.mark.parametrize("tag,order", [('T1', 0), ('T3', 1), ('P1L', 1), ('T4', 0)])
def test_trace_leaves_the_arithmetic_alone(em, oracle, tag, order):
    """A solve with a trace is bit for bit the solve without."""
    omesh, omodel, sfield, kw = _case(em, oracle, _depth.golden(), tag)
    _, _, errs0, e0 = _depth.oracle_run(oracle, omesh, omodel, sfield, order=order, trace=False, **kw)
    rec, _, errs1, e1 = _depth.oracle_run(oracle, omesh, omodel, sfield, order=order, **kw)
    assert len(rec) > 0
    assert np.array_equal(e0, e1) and np.array_equal(errs0, errs1)


def test_trace_through_multigrid_and_krylov(em, oracle):
    """`multigrid(..., trace=)` itself, and a solve preconditioned by it, record the same kind of calls."""
    omesh, omodel, sfield, kw = _case(em, oracle, _depth.golden(), 'P1')
    var = oracle.Var(omesh.vnC, maxit=1, tol=_depth.TOL, **kw)
    rec = []
    oracle.multigrid(omesh, omodel, sfield, np.zeros_like(sfield), var, trace=rec)
    records = _depth.stored(_depth.golden(), 'P1')[0]
    assert _depth.split_records(rec)[0] == [r for r in records if r[0] == 0]
    rec2 = []
    oracle.solve(omesh, omodel, sfield, sslsolver=True, maxit=1, trace=rec2, **kw)
    assert len(rec2) >= len(rec) and {r[3] for r in rec2} == {0, 1, 2}
