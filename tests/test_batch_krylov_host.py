"""CPU-only: the host side of the batched Krylov solves (solver.solve_sources(sslsolver=...)) -- the partition of the
systems by rotation state, the lockstep drivers ``_bicgstab_device_batched`` / ``_cgs_device_batched`` against a NumPy
stand-in for the device handle, and the workspace estimate.  The contract of the drivers: every system of a batch
gets exactly what the single-system driver (``_bicgstab_device`` / ``_cgs_device``) gives when it runs alone."""
import numpy as np
import pytest
import scipy.sparse.linalg as ssl

from emg3d_amd import solver
from emg3d_amd.solver import MGParameters


# --------------------------------------------------------------------------- rotation partitions
def _var(sc=True, lr=True):
    return MGParameters(cycle='F', sslsolver='bicgstab', semicoarsening=sc, linerelaxation=lr, vnC=(16, 16, 16), verb=0)


def _run_cycles(var, k):
    """What the level-0 loop does to a system's parameters per cycle."""
    for _ in range(k):
        var.it += 1
        var.sc_dir = next(var.sc_cycle) if var.sc_cycle else var.sc_dir
        var.lr_dir = next(var.lr_cycle) if var.lr_cycle else var.lr_dir


def test_partitions_equal_states_one_group():
    vars_ = [_var() for _ in range(4)]
    for v in vars_:
        _run_cycles(v, 3)
    states = [solver._rotation_state(v) for v in vars_]
    assert solver._rotation_partitions(states, [1, 1, 1, 1]) == [[0, 1, 2, 3]]
    # without rotation every cycle count is the same state
    fixed = [_var(sc=False, lr=False) for _ in range(3)]
    _run_cycles(fixed[1], 2)
    assert solver._rotation_partitions([solver._rotation_state(v) for v in fixed], [1, 1, 1]) == [[0, 1, 2]]


def test_partitions_drifted_states():
    vars_ = [_var() for _ in range(5)]
    for v, k in zip(vars_, (3, 2, 3, 5, 6)):        # period 3: 3 = 6 (mod 3), 2 = 5 (mod 3)
        _run_cycles(v, k)
    states = [solver._rotation_state(v) for v in vars_]
    assert states[0] == states[2] == states[4] and states[1] == states[3] and states[0] != states[1]
    assert states[0][:2] == (1, 4) and states[1][:2] == (3, 6)      # sc 1,2,3 / lr 4,5,6 after 3 resp. 2 cycles
    assert solver._rotation_partitions(states, [1] * 5) == [[0, 2, 4], [1, 3]]
    # semicoarsening 1213 (period 4) beside line relaxation True (period 3): equal directions at different positions
    a = MGParameters(cycle='V', sslsolver='cgs', semicoarsening=1213, linerelaxation=True, vnC=(16, 16, 16), verb=0)
    b = MGParameters(cycle='V', sslsolver='cgs', semicoarsening=1213, linerelaxation=True, vnC=(16, 16, 16), verb=0)
    _run_cycles(a, 0)
    _run_cycles(b, 6)       # sc position 2 -> direction 1 again, lr position 0
    assert (a.sc_dir, a.lr_dir) == (b.sc_dir, b.lr_dir) == (1, 4)
    assert solver._rotation_partitions([solver._rotation_state(a), solver._rotation_state(b)], [1, 1]) == [[0], [1]]


def test_partitions_exclude_frozen_systems():
    states = [(1, 4, 0, 0), (2, 5, 1, 1), (1, 4, 0, 0), (2, 5, 1, 1)]
    assert solver._rotation_partitions(states, [1, 0, 1, 1]) == [[0, 2], [3]]
    assert solver._rotation_partitions(states, [0, 0, 1, 0]) == [[2]]
    assert solver._rotation_partitions(states, [0, 0, 0, 0]) == []
    assert solver._rotation_partitions(states, np.array([0, 1, 0, 1], dtype=np.int32)) == [[1, 3]]


# --------------------------------------------------------------------------- NumPy stand-in for the handle
class DenseHandle:
    """``vec_*`` (the selected system) and ``bvec_*`` (all systems that are not frozen) of ``DeviceMG`` on dense arrays."""
    SFIELD, EFIELD = -1, -2

    def __init__(self, A, rhs):
        self.A = np.asarray(A)
        self.dtype = np.dtype(self.A.dtype)
        self.s = np.array(rhs, dtype=self.dtype).reshape(-1, self.A.shape[0])
        self.e = np.zeros_like(self.s)
        self.nsys, self.nE = self.s.shape
        self.mask = np.ones(self.nsys, dtype=np.int32)
        self.cur = 0
        self.vecs, self.bvecs = [], []
        self.mask_calls = 0

    def set_mask(self, active):
        a = np.asarray(active, dtype=np.int32)
        assert a.size == self.nsys
        self.mask = a.copy()
        self.mask_calls += 1

    def _on(self):
        return [b for b in range(self.nsys) if self.mask[b]]

    # ---- single-system workspace
    def _v(self, i):
        return self.s[self.cur] if i == -1 else self.e[self.cur] if i == -2 else self.vecs[i]

    def vec_alloc(self, n):
        while len(self.vecs) < n:
            self.vecs.append(np.zeros(self.nE, dtype=self.dtype))

    def vec_set(self, i, x):
        self._v(i)[:] = x

    def vec_get(self, i):
        return self._v(i).copy()

    def vec_copy(self, dst, src):
        self._v(dst)[:] = self._v(src)

    def vec_axpy(self, y, alpha, x):
        self._v(y)[:] = self._v(y) + complex(alpha) * self._v(x)

    def vec_scale(self, y, alpha):
        self._v(y)[:] = complex(alpha) * self._v(y)

    def vec_dot(self, a, b):
        return complex(np.vdot(self._v(a), self._v(b)))

    def vec_norm(self, a):
        return float(np.sqrt(abs(self.vec_dot(a, a))))

    def vec_amatvec(self, dst, src):
        self._v(dst)[:] = self.A @ self._v(src)

    # ---- batched workspace
    def _bv(self, i):
        return self.s if i == -1 else self.e if i == -2 else self.bvecs[i]

    def bvec_alloc(self, n):
        while len(self.bvecs) < n:
            self.bvecs.append(np.zeros((self.nsys, self.nE), dtype=self.dtype))

    def _coef(self, alpha):
        return np.broadcast_to(np.asarray(alpha, dtype=np.complex128), (self.nsys,))

    def bvec_copy(self, dst, src):
        for b in self._on():
            self._bv(dst)[b] = self._bv(src)[b]

    def bvec_zero(self, i):
        for b in self._on():
            self._bv(i)[b] = 0

    def bvec_axpy(self, y, alpha, x):
        c = self._coef(alpha)
        for b in self._on():
            self._bv(y)[b] = self._bv(y)[b] + complex(c[b]) * self._bv(x)[b]

    def bvec_scale(self, y, alpha):
        c = self._coef(alpha)
        for b in self._on():
            self._bv(y)[b] = complex(c[b]) * self._bv(y)[b]

    def bvec_dot(self, a, b, out=None):
        out = np.zeros(self.nsys, dtype=self.dtype) if out is None else out
        for k in self._on():
            out[k] = np.vdot(self._bv(a)[k], self._bv(b)[k])
        return out

    def bvec_amatvec(self, dst, src):
        for b in self._on():
            self._bv(dst)[b] = self.A @ self._bv(src)[b]

    def bvec_get(self, i, b):
        return self._bv(i)[b].copy()


class RecordingHandle(DenseHandle):
    """``DenseHandle`` that logs every primitive call as (method name, integer arguments...): the vector ids, and for
    ``set_mask`` the flags.  (``vec_norm`` is followed by the ``vec_dot`` it is made of.)"""

    def __init__(self, A, rhs):
        super().__init__(A, rhs)
        self.trace = []


def _recorded(name):
    inner = getattr(DenseHandle, name)

    def call(self, *args):
        ints = args[0] if name == 'set_mask' else [a for a in args if isinstance(a, (int, np.integer))]
        self.trace.append((name,) + tuple(int(a) for a in ints))
        return inner(self, *args)
    return call


for _name in dir(DenseHandle):
    if _name.startswith(('vec_', 'bvec_')) or _name == 'set_mask':
        setattr(RecordingHandle, _name, _recorded(_name))

N = 40


def _x_start(warm):
    return np.linspace(1.0, 2.0, N) * (1 - 0.5j) if warm else np.zeros(N, dtype=complex)


@pytest.fixture(scope="module")
def problem():
    """A complex-symmetric, strictly diagonally dominant matrix and four right-hand sides: a random one, two that are
    combinations of a few eigenvectors (the Krylov iterations end after about as many steps) with norms 1e-6 and 1e4
    of the first, and a zero one."""
    rng = np.random.default_rng(42)
    off = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    off = 0.05 * (off + off.T)
    np.fill_diagonal(off, 0)
    A = off + np.diag(6.0 + 4.0 * rng.uniform(size=N) + 1j * (2.0 + rng.uniform(size=N)))
    assert np.array_equal(A, A.T) and not np.array_equal(A, A.conj().T)
    assert all(abs(A[i, i]) > np.abs(A[i]).sum() - abs(A[i, i]) for i in range(N))
    _, vec = np.linalg.eig(A)
    rhs = np.zeros((4, N), dtype=np.complex128)
    rhs[0] = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    rhs[1] = 1e-6 * vec[:, [3, 17, 29]].sum(axis=1)
    rhs[2] = 1e4 * vec[:, [0, 5, 9, 14, 21, 33, 38]].sum(axis=1)
    return A, rhs


DRIVERS = {'bicgstab': (solver._bicgstab_device, solver._bicgstab_device_batched, ssl.bicgstab),
           'cgs': (solver._cgs_device, solver._cgs_device_batched, ssl.cgs)}
RTOL = 1e-13


def _alone(single, A, b):
    dev = DenseHandle(A, b[None, :])
    its = []
    x, code = single(dev, b, np.zeros_like(b), rtol=RTOL, maxiter=100, atol=1e-30, psolve=None, callback=its.append)
    return x, code, its


@pytest.mark.parametrize("name", ['bicgstab', 'cgs'])
def test_batched_driver_equals_single_driver(problem, name):
    A, rhs = problem
    single, batched, scipy_solver = DRIVERS[name]
    dev = DenseHandle(A, rhs)
    res = [[] for _ in range(4)]
    codes = batched(dev, 4, rtol=RTOL, maxiter=100, atol=1e-30, psolve=None, callbacks=[r.append for r in res])
    counts = []
    for b in range(4):
        x, code, its = _alone(single, A, rhs[b])
        assert codes[b] == code == 0
        assert res[b] == its                                    # same number of iterations, same residual norms
        np.testing.assert_array_equal(dev.bvec_get(0, b), x)
        counts.append(len(its))
        if np.any(rhs[b]):
            xs, info = scipy_solver(A, rhs[b], rtol=RTOL, atol=0.0, maxiter=100)
            assert info == 0                                    # SciPy itself converges on this matrix
            np.testing.assert_allclose(x, xs, rtol=1e-10, atol=1e-10 * np.abs(xs).max())
            np.testing.assert_allclose(A @ x, rhs[b], rtol=0, atol=1e-10 * np.linalg.norm(rhs[b]))
        else:
            assert not np.any(x) and its == []
    print(name, "iterations per system:", counts)
    assert len(set(counts[:3])) == 3 and counts[3] == 0         # the systems finish at different iterations


@pytest.mark.parametrize("name", ['bicgstab', 'cgs'])
def test_batched_driver_max_iterations_and_subset(problem, name):
    """maxiter per system; systems beyond ``n`` and systems left out from the start are never touched."""
    A, rhs = problem
    single, batched, _ = DRIVERS[name]
    dev = DenseHandle(A, rhs)
    dev.bvec_alloc(12)
    dev.bvecs[0][:] = 7.0                   # a workspace that an earlier call left behind
    res = [[] for _ in range(3)]
    codes = batched(dev, 3, rtol=RTOL, maxiter=4, atol=1e-30, psolve=None, callbacks=[r.append for r in res],
                    active=[1, 0, 1])
    for b in (0, 2):
        dev1 = DenseHandle(A, rhs[b][None, :])
        its = []
        x, code = single(dev1, rhs[b], np.zeros(N, dtype=complex), rtol=RTOL, maxiter=4, atol=1e-30, psolve=None,
                         callback=its.append)
        assert codes[b] == code == 4 and res[b] == its and len(its) == 4
        np.testing.assert_array_equal(dev.bvec_get(0, b), x)
    assert res[1] == [] and codes[1] == 0
    assert not np.any(dev.bvec_get(0, 1))                       # zeroed with the others at the start, then left alone
    assert np.all(dev.bvec_get(0, 3) == 7.0)                    # beyond n: untouched


@pytest.mark.parametrize("name", ['bicgstab', 'cgs'])
def test_failing_preconditioner_is_per_system(problem, name):
    """A preconditioner that reports a failure for one system: that system ends with code -1 and a zero iterate, the
    others go on to what they reach with this (identity) preconditioner alone."""
    A, rhs = problem
    single, batched, _ = DRIVERS[name]
    dev = DenseHandle(A, rhs[:3])
    calls = []

    def psolve(src, dst, mask):
        np.testing.assert_array_equal(dev.mask, mask)           # the driver hands over the mask the device holds
        calls.append(mask.copy())
        dev.bvec_copy(dst, src)
        return [0] if len(calls) == 3 and mask[0] else []

    failed = []
    codes = batched(dev, 3, rtol=RTOL, maxiter=100, atol=1e-30, psolve=psolve, callbacks=None, failed=failed)
    assert codes[0] == -1 and failed == [0] and not np.any(dev.bvec_get(0, 0))
    for b in (1, 2):
        dev1 = DenseHandle(A, rhs[b][None, :])
        x, code = single(dev1, rhs[b], np.zeros(N, dtype=complex), rtol=RTOL, maxiter=100, atol=1e-30,
                         psolve=lambda s, d: dev1.vec_copy(d, s), callback=None)
        assert codes[b] == code == 0
        np.testing.assert_array_equal(dev.bvec_get(0, b), x)
    assert all(m[0] == 0 for m in calls[3:]) and len(calls) > 3


@pytest.mark.parametrize("name", ['bicgstab', 'cgs'])
def test_negative_maxiter_is_not_a_failed_preconditioner(problem, name):
    """maxiter = -1 (the reference's test of the error message): no iteration, every system returns -1 as the single
    driver does, and no preconditioner is reported as failed."""
    A, rhs = problem
    single, batched, _ = DRIVERS[name]
    dev = DenseHandle(A, rhs[:2])
    failed = []
    codes = batched(dev, 2, rtol=RTOL, maxiter=-1, atol=1e-30, psolve=None, callbacks=None, failed=failed)
    dev1 = DenseHandle(A, rhs[0][None, :])
    _, code = single(dev1, rhs[0], np.zeros(N, dtype=complex), rtol=RTOL, maxiter=-1, atol=1e-30, psolve=None, callback=None)
    assert codes == [code, code] == [-1, -1] and failed == []
    var = MGParameters(cycle=None, sslsolver=name, semicoarsening=False, linerelaxation=False, vnC=(8, 8, 8), verb=0)
    solver._krylov_exit_message(var, -1, False)
    assert var.exit_message == f"Error in {name} (-1)"
    var.exit_message = "DIVERGED"
    solver._krylov_exit_message(var, -1, True)
    assert var.exit_message == "DIVERGED (returned field is zero)"


# --------------------------------------------------------------------------- the primitive calls of either path
# Recorded from the drivers as they stood before the iteration was written once (``_bicgstab_device`` / ``_cgs_device`` on
# ``vec_*``, their batched restatements on ``bvec_*``), on ``RecordingHandle`` with the arguments of the tests below:
# the shared bodies must issue exactly these calls through either backend.  x0 = 0 / x0 != 0 differ in how r is formed.
def _calls(prefix, text):
    """'copy 1 9; set_mask 1 0 1' -> [(prefix + 'copy', 1, 9), ('set_mask', 1, 0, 1)]"""
    return [(w[0] if w[0] == 'set_mask' else prefix + w[0],) + tuple(int(i) for i in w[1:])
            for w in (c.split() for c in text.split(';'))]


BICGSTAB_ITERATIONS = (     # (norm: followed by the dot it is made of)
    "norm 1; dot 1 1; dot 2 1; copy 3 1; copy 7 3; amatvec 4 7; dot 2 4; axpy 1 4; copy 5 1; norm 5; dot 5 5; copy 8 5;"
    "amatvec 6 8; dot 6 5; dot 6 6; axpy 0 7; axpy 0 8; axpy 1 6; amatvec 10 0; copy 11 9; axpy 11 10; norm 11; dot 11 11;"
    "norm 1; dot 1 1; dot 2 1; axpy 3 4; scale 3; axpy 3 1; copy 7 3; amatvec 4 7; dot 2 4; axpy 1 4; copy 5 1; norm 5; dot 5 5;"
    "copy 8 5; amatvec 6 8; dot 6 5; dot 6 6; axpy 0 7; axpy 0 8; axpy 1 6; amatvec 10 0; copy 11 9; axpy 11 10; norm 11;"
    "dot 11 11; get 0")
CGS_ITERATIONS = (
    "norm 1; dot 1 1; dot 2 1; copy 3 1; copy 4 1; copy 6 3; amatvec 7 6; dot 2 7; copy 5 4; axpy 5 7; copy 8 4; axpy 8 5;"
    "copy 9 8; axpy 0 9; amatvec 11 0; copy 1 10; axpy 1 11; norm 1; dot 1 1;"
    "norm 1; dot 1 1; dot 2 1; copy 4 1; axpy 4 5; scale 3; axpy 3 5; scale 3; axpy 3 4; copy 6 3; amatvec 7 6; dot 2 7;"
    "copy 5 4; axpy 5 7; copy 8 4; axpy 8 5; copy 9 8; axpy 0 9; amatvec 11 0; copy 1 10; axpy 1 11; norm 1; dot 1 1; get 0")
SINGLE_TRACES = {           # (method, x0 != 0)
    ('bicgstab', False): "alloc 12; set 9; set 0; norm 9; dot 9 9; copy 1 9; copy 2 1;" + BICGSTAB_ITERATIONS,
    ('bicgstab', True): "alloc 12; set 9; set 0; norm 9; dot 9 9; amatvec 10 0; copy 1 9; axpy 1 10; copy 2 1;"
                        + BICGSTAB_ITERATIONS,
    ('cgs', False): "alloc 12; set 10; set 0; norm 10; dot 10 10; copy 1 10; copy 2 1;" + CGS_ITERATIONS,
    ('cgs', True): "alloc 12; set 10; set 0; norm 10; dot 10 10; amatvec 11 0; copy 1 10; axpy 1 11; copy 2 1;" + CGS_ITERATIONS}
BATCHED_TRACES = {
    'bicgstab':
        "alloc 12; set_mask 1 1 1; zero 0; set_mask 1 0 1; copy 9 -1; dot 9 9; copy 1 9; copy 2 1;"
        "dot 1 1; dot 2 1; copy 3 1; copy 7 3; amatvec 4 7; dot 2 4; axpy 1 4; copy 5 1; dot 5 5; axpy 0 7; copy 8 5;"
        "amatvec 6 8; dot 6 5; dot 6 6; axpy 0 8; axpy 1 6; amatvec 10 0; copy 11 9; axpy 11 10; dot 11 11;"
        "dot 1 1; dot 2 1; axpy 3 4; scale 3; axpy 3 1; copy 7 3; amatvec 4 7; dot 2 4; axpy 1 4; copy 5 1; dot 5 5; axpy 0 7;"
        "copy 8 5; amatvec 6 8; dot 6 5; dot 6 6; axpy 0 8; axpy 1 6; amatvec 10 0; copy 11 9; axpy 11 10; dot 11 11",
    'cgs':
        "alloc 12; set_mask 1 1 1; zero 0; set_mask 1 0 1; copy 10 -1; dot 10 10; copy 1 10; copy 2 1;"
        "dot 1 1; dot 2 1; copy 3 1; copy 4 1; copy 6 3; amatvec 7 6; dot 2 7; copy 5 4; axpy 5 7; copy 8 4; axpy 8 5; copy 9 8;"
        "axpy 0 9; amatvec 11 0; copy 1 10; axpy 1 11; dot 1 1;"
        "dot 1 1; dot 2 1; copy 4 1; axpy 4 5; scale 3; axpy 3 5; scale 3; axpy 3 4; copy 6 3; amatvec 7 6; dot 2 7; copy 5 4;"
        "axpy 5 7; copy 8 4; axpy 8 5; copy 9 8; axpy 0 9; amatvec 11 0; copy 1 10; axpy 1 11; dot 1 1"}
BATCHED_MASK_CALLS = 2


@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("identity", [False, True])
@pytest.mark.parametrize("name", ['bicgstab', 'cgs'])
def test_single_path_call_trace(problem, name, identity, warm):
    """A single solve issues the ``vec_*`` calls it always has, in their order, and nothing of the batched machinery."""
    A, rhs = problem
    dev = RecordingHandle(A, rhs[0][None, :])
    its = []
    _, code = DRIVERS[name][0](dev, rhs[0], _x_start(warm), rtol=RTOL, maxiter=2, atol=1e-30,
                               psolve=(lambda s, d: dev.vec_copy(d, s)) if identity else None, callback=its.append)
    assert code == 2 and len(its) == 2
    assert dev.trace == _calls('vec_', SINGLE_TRACES[name, warm])
    assert not [c for c in dev.trace if c[0].startswith('bvec_') or c[0] == 'set_mask'] and dev.mask_calls == 0


@pytest.mark.parametrize("identity", [False, True])
@pytest.mark.parametrize("name", ['bicgstab', 'cgs'])
def test_batched_path_call_trace(problem, name, identity):
    """A batched solve issues the ``bvec_*`` calls and writes the masks it always has, and no ``vec_*``."""
    A, rhs = problem
    dev = RecordingHandle(A, rhs[:3])

    def psolve(src, dst, mask):
        dev.bvec_copy(dst, src)
        return []
    res = [[] for _ in range(3)]
    codes = DRIVERS[name][1](dev, 3, rtol=RTOL, maxiter=2, atol=1e-30, psolve=psolve if identity else None,
                             callbacks=[r.append for r in res], active=[1, 0, 1])
    assert codes == [2, 0, 2] and [len(r) for r in res] == [2, 0, 2]
    assert dev.trace == _calls('bvec_', BATCHED_TRACES[name])
    assert not [c for c in dev.trace if c[0].startswith('vec_')]
    assert dev.mask_calls <= BATCHED_MASK_CALLS


@pytest.mark.parametrize("name", ['bicgstab', 'cgs'])
def test_single_driver_warm_start(problem, name):
    """x0 != 0 (r = b - A x0): started from the iterate of a 3-iteration run, the driver reaches the solution of the cold
    run in fewer iterations."""
    A, rhs = problem
    single = DRIVERS[name][0]
    cold, code, its_cold = _alone(single, A, rhs[0])
    assert code == 0
    dev = DenseHandle(A, rhs[0][None, :])
    x3, code = single(dev, rhs[0], np.zeros(N, dtype=complex), rtol=RTOL, maxiter=3, atol=1e-30, psolve=None, callback=None)
    assert code == 3 and np.any(x3)
    its = []
    x, code = single(DenseHandle(A, rhs[0][None, :]), rhs[0], x3, rtol=RTOL, maxiter=100, atol=1e-30, psolve=None,
                     callback=its.append)
    assert code == 0 and len(its) < len(its_cold)
    np.testing.assert_allclose(x, cold, rtol=0, atol=1e-10 * np.abs(cold).max())


# --------------------------------------------------------------------------- workspace estimate
class _Sized:
    nE = 1_000_000
    dtype = np.dtype(np.complex128)
    device = 0


def test_fits_estimate_scales_with_nsys(monkeypatch):
    from emg3d_amd import _lib
    one = solver._krylov_workspace_bytes(_Sized, 'bicgstab')
    assert one == 9 * _Sized.nE * 16
    for nsys in (2, 8, 64):
        assert solver._krylov_workspace_bytes(_Sized, 'bicgstab', nsys=nsys) == nsys * one
        assert solver._krylov_workspace_bytes(_Sized, 'cgs', nsys=nsys) == nsys * solver._krylov_workspace_bytes(_Sized, 'cgs')
    monkeypatch.setattr(_lib, "mem_info", lambda device=0: {"free": 4 * one, "total": 8 * one, "pooled": 0,
                                                             "pooled_on_device": one})
    assert solver._krylov_fits_device(_Sized, 'bicgstab')
    assert solver._krylov_fits_device(_Sized, 'bicgstab', nsys=4)           # 4 < 0.92 * 5
    assert not solver._krylov_fits_device(_Sized, 'bicgstab', nsys=5)
    assert not solver._krylov_fits_device(_Sized, 'bicgstab', nsys=8)


def test_solve_sources_refuses_what_is_not_batched():
    import emg3d_amd as em
    grid = em.TensorMesh([np.ones(4) * 10.0] * 3, origin=(-20., -20., -20.))
    model = em.Model(grid, 1.0)
    with pytest.raises(ValueError, match="'bicgstab' and 'cgs'"):
        solver.solve_sources(grid, model, [[0., 0., 0., 0., 0.]], 1.0, sslsolver='gcrotmk', verb=0)
    with pytest.raises(ValueError, match="resident"):
        solver.solve_sources(grid, model, None, 1.0, sslsolver='bicgstab', resident=1, handle=object(), verb=0)
