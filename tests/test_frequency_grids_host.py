"""CPU-only: the host side of a computational grid per frequency (optimize.SurveyJacobian / shard.solve_survey with a sequence for
``grid``) -- ``meshes.same_grid`` and the grouping, the argument checks that need no device, the pure byte count of the parked
forward fields, and ``solver.GridHandles`` against a stand-in of the handle.

Also home of what tests/test_gpu_frequency_grids.py shares: the three grids."""
import numpy as np
import pytest

from conftest import load_golden
from test_model_grid_host import grid_pairs

SOURCES = [[-100., 30., 20., 25., 5.], [140., -60., -25., -50., 20.], [20., 100., -40., 80., -30.]]


def survey_grids(em):
    """``(M, A, B)``: the 7 x 5 x 4 model grid and the 12 x 10 x 8 computational grid of the 'unaligned' pair, and a 16 x 12 x 8
    computational grid that shares no node with either and extends beyond ``M`` on all six sides."""
    M, A = grid_pairs(em, ['unaligned'])['unaligned']
    hx = em.meshes.stretched_widths(8, 4, 100., 1.3)
    hy = em.meshes.stretched_widths(6, 3, 100., 1.3)
    hz = em.meshes.stretched_widths(4, 2, 100., 1.4)
    B = em.TensorMesh([hx, hy, hz], origin=(-hx.sum() / 2 + 7, -hy.sum() / 2 - 11, -hz.sum() / 2 + 5))
    return M, A, B


def copy_of(em, grid):
    """Another object with the same widths and origin."""
    return em.TensorMesh([w.copy() for w in grid.h], origin=grid.origin.copy())


def test_the_grids_are_what_the_gpu_tests_need():
    import emg3d_amd as em
    M, A, B = survey_grids(em)
    rec = tuple(load_golden("survey_jacobian.npz")['rec'])
    assert tuple(M.vnC) == (7, 5, 4) and tuple(A.vnC) == (12, 10, 8) and tuple(B.vnC) == (16, 12, 8)
    for c, pts in zip('xyz', ([s[0] for s in SOURCES] + list(rec[0]), [s[1] for s in SOURCES] + list(rec[1]),
                              [s[2] for s in SOURCES] + list(rec[2]))):
        nb, na, nm = (getattr(g, 'nodes_' + c) for g in (B, A, M))
        assert not np.isin(nb, na).any() and not np.isin(nb, nm).any()          # no node in common
        assert nb[0] < nm[0] and nb[-1] > nm[-1]                                 # beyond the model grid on both sides
        assert all(nb[1] < p < nb[-2] and na[1] < p < na[-2] for p in pts)       # sources and receivers well inside both


# ---- 1. the same-grid function and the grouping ---------------------------------------------------------------------------------
def test_same_grid():
    import emg3d_amd as em
    same_grid = em.meshes.same_grid
    _, A, B = survey_grids(em)
    assert same_grid(A, A) and same_grid(A, copy_of(em, A)) and same_grid(copy_of(em, A), A)
    assert not same_grid(A, B) and not same_grid(B, A)
    for axis in range(3):
        h = [w.copy() for w in A.h]
        h[axis][-1] = np.nextafter(h[axis][-1], np.inf)         # one width differs in its last bit
        assert not same_grid(A, em.TensorMesh(h, origin=A.origin))
        origin = A.origin.copy()
        origin[axis] = np.nextafter(origin[axis], -np.inf)
        assert not same_grid(A, em.TensorMesh(A.h, origin=origin))
    assert not same_grid(A, em.TensorMesh([A.h[0][:-1], A.h[1], A.h[2]], origin=A.origin))
    assert em.TensorMesh.__eq__ is object.__eq__ and A != copy_of(em, A)         # meshes themselves compare by identity


def test_grouping_and_public_attributes():
    import emg3d_amd as em
    M, A, B = survey_grids(em)
    A2 = copy_of(em, A)
    distinct, index = em.meshes.distinct_grids([A, B, A2])
    assert index == [0, 1, 0] and len(distinct) == 2 and distinct[0] is A and distinct[1] is B
    assert em.meshes.distinct_grids([B, A, B, A2, B])[1] == [0, 1, 0, 1, 0]
    assert em.meshes.distinct_grids([]) == ([], [])
    rec = tuple(load_golden("survey_jacobian.npz")['rec'])
    model = em.Model(M, np.ones(M.nC))
    seq = [A, B, A2]
    sj = em.optimize.SurveyJacobian(seq, model, SOURCES, [1.5, 0.7, -1.2], rec, model_grid=M)
    assert sj.grid is seq and sj.grid_index == [0, 1, 0] and len(sj.grids) == 3
    assert sj.grids[0] is A and sj.grids[1] is B and sj.grids[2] is A2
    assert sj._vnM == (7, 5, 4) and sj.synthetic is None
    sj = em.optimize.SurveyJacobian((B, B), model, SOURCES, [1.5, 0.7], rec, model_grid=M)        # a tuple, repeats
    assert sj.grid_index == [0, 0] and sj.grids == [B, B]
    # a single mesh: as before, with or without a model grid
    for kw in (dict(model_grid=M), {}):
        m = model if kw else em.Model(A, np.ones(A.nC))
        sj = em.optimize.SurveyJacobian(A, m, SOURCES, [1.5, 0.7, -1.2], rec, **kw)
        assert sj.grid is A and sj.grids == [A, A, A] and sj.grid_index == [0, 0, 0] and sj._nb == 3


# ---- 2. every ValueError, with no device ----------------------------------------------------------------------------------------
def test_argument_checks_need_no_device(monkeypatch):
    import emg3d_amd as em
    from emg3d_amd import _lib, solver

    def no_device(*args, **kwargs):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_lib, 'load', no_device)
    monkeypatch.setattr(solver, 'GridHandles', no_device)
    M, A, B = survey_grids(em)
    rec = tuple(load_golden("survey_jacobian.npz")['rec'])
    model = em.Model(M, np.ones(M.nC))
    freqs = [1.5, 0.7, -1.2]
    calls = (lambda grid, **kw: em.optimize.SurveyJacobian(grid, model, SOURCES, freqs, rec, **kw),
             lambda grid, **kw: em.shard.solve_survey(grid, model, SOURCES, freqs, rec, **kw))
    for call in calls:
        with pytest.raises(ValueError, match="model_grid"):         # the products of different frequencies share no cells
            call([A, B, A])
        with pytest.raises(ValueError, match="model_grid"):
            call([A, A, A])
        for seq in ([A, B], [A, B, A, B], [], (A,)):
            with pytest.raises(ValueError, match="per entry of `freqs`"):
                call(seq, model_grid=M)
        for seq in ([A, None, A], [A, B, A.h], [A, 'B', A]):
            with pytest.raises(ValueError, match="TensorMesh"):
                call(seq, model_grid=M)
    # the model must live on the model grid, sequence or not
    with pytest.raises(ValueError, match="model_grid"):
        em.optimize.SurveyJacobian([A, B, A], em.Model(A, np.ones(A.nC)), SOURCES, freqs, rec, model_grid=M)


# ---- 3. the bytes of the parked forward fields -----------------------------------------------------------------------------------
def test_parked_slots_and_bytes():
    import emg3d_amd as em
    from emg3d_amd.optimize import _parked_bytes, _parked_slots
    _, A, B = survey_grids(em)
    assert A.nE != B.nE
    c128, f64 = np.dtype(np.complex128), np.dtype(np.float64)
    # [A, B, A] at (1.5 Hz, 0.7 Hz, s = 1.2), two chunks per frequency: three handles
    slot, nslots, first = _parked_slots([0, 1, 0], [c128, c128, f64], 2)
    assert slot == {0: 0, 1: 0, 2: 0}
    assert nslots == {(0, c128.str): 2, (1, c128.str): 2, (0, f64.str): 2}
    assert list(first.items()) == [((0, c128.str), 0), ((1, c128.str), 1), ((0, f64.str), 2)]     # in order of first appearance
    assert _parked_bytes(nslots, 2, [A.nE, B.nE]) == 2 * 2 * A.nE * 16 + 2 * 2 * B.nE * 16 + 2 * 2 * A.nE * 8
    # [A, B, A] at three frequencies: entry 2 shares A's complex handle and parks behind entry 0
    slot, nslots, first = _parked_slots([0, 1, 0], [c128, c128, c128], 2)
    assert slot == {0: 0, 1: 0, 2: 2} and nslots == {(0, c128.str): 4, (1, c128.str): 2}
    assert first == {(0, c128.str): 0, (1, c128.str): 1}
    assert _parked_bytes(nslots, 3, [A.nE, B.nE]) == (4 * A.nE + 2 * B.nE) * 3 * 16
    # one grid: the count of a single mesh, per dtype
    slot, nslots, _ = _parked_slots([0, 0, 0], [c128, f64, c128], 1)
    assert slot == {0: 0, 1: 0, 2: 1} and _parked_bytes(nslots, 2, [A.nE]) == 2 * 2 * A.nE * 16 + 1 * 2 * A.nE * 8


# ---- 4. GridHandles against a stand-in of the handle -------------------------------------------------------------------------------
class _StandIn:
    """What GridHandles and its FrequencyHandles ask of a DeviceMG, recorded."""

    def __init__(self, log, grid, parts, spec):
        self.log, self.grid, self.key = log, grid, np.dtype(spec.dtype).str
        log.append((self, 'create', parts))

    def retarget(self, spec):
        self.log.append((self, 'retarget', spec))

    def set_batch(self, n):
        self.log.append((self, 'set_batch', n))

    def set_model_grid(self, model_grid):
        self.log.append((self, 'set_model_grid', model_grid))

    def set_regrid_factors(self, F, Q):
        self.log.append((self, 'set_regrid_factors', F, Q))

    def _model_arrays(self, grid, parts):
        assert grid is self.grid
        self.log.append((self, 'check', parts))
        if getattr(self, 'refuse', False):
            raise ValueError("set_model: refused")

    def _set_parts(self, grid, parts):
        assert grid is self.grid
        self.log.append((self, 'upload', parts))

    def close(self):
        self.log.append((self, 'close'))


class _ModelOnM:
    """A model on the model grid that counts its regriddings."""

    def __init__(self, em, value, calls):
        self.em, self.value, self.calls = em, value, calls

    def interpolate2grid(self, grid, new_grid):
        self.calls.append((grid, new_grid))
        return self.em.Model(new_grid, np.full(new_grid.nC, self.value))


def test_grid_handles_against_a_stand_in(monkeypatch):
    import emg3d_amd as em
    from emg3d_amd import solver
    log, regrids = [], []
    monkeypatch.setattr(solver.DeviceMG, 'from_model',
                        classmethod(lambda cls, grid, parts, spec, device=0: _StandIn(log, grid, parts, spec)))
    M, A, B = survey_grids(em)
    A2 = copy_of(em, A)
    c128, f64 = em.fields.FrequencySpec(1.5), em.fields.FrequencySpec(-1.2)
    other = em.fields.FrequencySpec(0.7)
    with solver.GridHandles([A, B, A2, B], _ModelOnM(em, 2.0, regrids), 0, nsys=2, model_grid=M) as handles:
        assert handles.index == [0, 1, 0, 1] and handles.distinct == [A, B] and len(handles.members) == 2
        assert regrids == [(M, A), (M, B)] and not log            # regridded once per distinct grid, no handle yet
        assert all(isinstance(m, solver.FrequencyHandles) and m.nsys == 2 for m in handles.members)
        assert [m.grid for m in handles.members] == [A, B]
        assert all(np.array_equal(m.parts[0], np.full(m.grid.vnC, 2.0)) for m in handles.members)
        # one creation per (grid, dtype); an entry that shares both is re-targeted
        a_c = handles.target(0, c128)
        b_c = handles.target(1, other)
        assert handles.target(2, other) is a_c and log[-1] == (a_c, 'retarget', other)
        a_f = handles.target(2, f64)
        assert handles.target(3, c128) is b_c
        created = [e[0] for e in log if e[1] == 'create']
        assert created == [a_c, b_c, a_f] and [(d.grid, d.key) for d in created] == [(A, '<c16'), (B, '<c16'), (A, '<f8')]
        made_from = {e[0]: e[2] for e in log if e[1] == 'create'}
        assert all(made_from[d] is handles.members[0 if d.grid is A else 1].parts for d in created)
        assert list(handles) == [a_c, a_f, b_c]                    # iteration: every handle, grid by grid
        assert [e[1] for e in log if e[0] is a_f] == ['create', 'set_batch']
        # an extra key (solve_survey's systems per launch) makes a handle of its own on that grid
        assert handles.target(0, c128, key=(1,)) is not a_c and handles.target(0, c128, key=(1,)).grid is A
        n_handles = 4
        assert len(list(handles)) == n_handles
        # the link and the factors: every open handle; F is per grid
        handles.set_model_grid(M)
        FA, FB, Q = (np.ones(A.vnC),) * 3, (np.ones(B.vnC),) * 3, (np.ones(M.vnC),) * 3
        handles.set_regrid_factors(0, FA, Q)
        handles.set_regrid_factors(1, FB, Q)
        assert sum(e[1] == 'set_model_grid' and e[2] is M for e in log) == n_handles
        got = {e[0]: e[2] for e in log if e[1] == 'set_regrid_factors'}
        assert len(got) == n_handles and all(F is (FA if d.grid is A else FB) for d, F in got.items())
        # a handle created later gets the model grid and the factors of ITS grid
        n0 = len(log)
        b_f = handles.target(3, f64)
        assert [e[1:] for e in log[n0:]] == [('create', handles.members[1].parts), ('set_batch', 2), ('set_model_grid', M),
                                             ('set_regrid_factors', FB, Q)]
        assert all(e[0] is b_f for e in log[n0:])
        n_handles += 1
        # set_model: one regridding per distinct grid, every handle of every grid checked before the first upload
        n0 = len(log)
        del regrids[:]
        handles.set_model(_ModelOnM(em, 3.0, regrids))
        assert regrids == [(M, A), (M, B)]
        kinds = [e[1] for e in log[n0:]]
        assert kinds == ['check'] * n_handles + ['upload'] * n_handles
        assert all(np.array_equal(e[2][0], np.full(e[0].grid.vnC, 3.0)) for e in log[n0:])
        assert all(e[2] is handles.members[0 if e[0].grid is A else 1].parts for e in log[n0 + n_handles:])
        # a refusal on the LAST grid's handle leaves every handle and `parts` as they were
        b_f.refuse = True
        n0 = len(log)
        with pytest.raises(ValueError, match="refused"):
            handles.set_model(_ModelOnM(em, 4.0, regrids))
        assert 'upload' not in [e[1] for e in log[n0:]]
        assert all(np.array_equal(m.parts[0], np.full(m.grid.vnC, 3.0)) for m in handles.members)
        n0 = len(log)
    assert [e[1] for e in log[n0:]] == ['close'] * n_handles and {e[0] for e in log[n0:]} == set(handles_all(log))
    # without a model grid the model is taken as it is (one grid)
    log.clear()
    model = em.Model(A, np.ones(A.nC))
    with solver.GridHandles([A, A], model, 0) as handles:
        assert handles.index == [0, 0] and handles.on_grids(model) == [model]
        assert handles.target(1, c128) is handles.target(0, c128)
    assert [e[1] for e in log] == ['create', 'retarget', 'close']


def handles_all(log):
    return [e[0] for e in log if e[1] == 'create']
