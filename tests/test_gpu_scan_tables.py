"""GPU: the scan tables of the scan kernel's colour launches (k_line_sweep_qpl SM, csrc/smooth_qpl.hpp; MG::ensure_scantab; the rule:
csrc/sweep_plan.hpp sweep_scantab).

The matrix part of a lane's row after every full Kogge-Stone step depends on the cached factor and the level's coefficients, not on
the field or the source.  The kernel's own scans write it once per factor build; every sweep launch thereafter loads it and scans
the offsets alone.  The table holds what the instructions of the computing path produce and the offset's four multiply-adds keep
their order, so the claim of every test here is BIT identity with the path that has no table (EMG3D_QPL_SCANTAB=0, lab build), on
top of the usual parity with the reference.  EMG3D_QPL_SCANTAB=1 admits every launch the kernel form allows whatever its size.

Two blocks per quad (EMG3D_QPL_M2) have no table: the planner never admits M = 2 (the in-quad composition would need rows of its
own, and the one M = 2 class of the flagship cycle is far beyond the size at which a table pays), so there is no such case."""
import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu

KNOBS = ("EMG3D_QPL_SCANTAB", "EMG3D_QPL_SCANTAB_BYTES", "EMG3D_QPL_SCANTAB_MAX", "EMG3D_QPL_CHAIN", "EMG3D_GRAPH")
ON = {"EMG3D_QPL_SCANTAB": "1", "EMG3D_QPL_CHAIN": "0"}
OFF = {"EMG3D_QPL_SCANTAB": "0", "EMG3D_QPL_CHAIN": "0"}
# seg 8 along each axis; seg 16; ragged: lines of 12 and 6 blocks in segments of 16 and 8 quads (blocks beyond the line: the zero map)
SHAPES = [(40, 8, 8), (8, 40, 8), (8, 8, 40), (24, 16, 6), (6, 24, 16), (24, 12, 6), (6, 24, 6)]
DTYPES = [np.complex128, np.float64]


@pytest.fixture(autouse=True)
def _lab_build(lab):
    yield


def _env(monkeypatch, env):
    """The knobs are read when a handle is created."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _problem(shape, dtype, seed=5):
    import emg3d_amd as em
    rng = np.random.default_rng(seed)
    cplx = dtype == np.complex128
    grid = em.TensorMesh([rng.uniform(0.5, 2, n) for n in shape], origin=(0, 0, 0))

    def rnd(n):
        a = rng.standard_normal(n)
        return (a + 1j * rng.standard_normal(n)) if cplx else a

    class VM:
        case = 3
    for name in ("eta_x", "eta_y", "eta_z"):
        setattr(VM, name, np.asfortranarray(rng.uniform(0.5, 2, shape) * (0.3j if cplx else -1.0)))
    VM.zeta = np.asfortranarray(rng.uniform(0.5, 2, shape))
    return grid, VM, rnd(grid.nE).astype(dtype), rnd(grid.nE).astype(dtype)


def _handle(grid, VM, dtype):
    from emg3d_amd.solver import DeviceMG, MGParameters
    dev = DeviceMG(grid, VM, dtype)
    dev.set_params(MGParameters(verb=0, cycle='F', sslsolver=False, linerelaxation=True, semicoarsening=True, vnC=grid.vnC,
                                ordering='colour'))
    return dev


def _table_dirs(lab, shape, dtype):
    """The directions whose colour launches load a table under the knobs that are set."""
    return [d for d in (1, 2, 3) if lab.sweep_plan(shape, d, dtype=dtype)["scan_table"]]


_sweeps = {}


def _sweep_results(monkeypatch, shape, dtype):
    """{(tag, direction, nu): field} of one smoothing call, table forced on / off: computed once per (shape, dtype)."""
    key = (shape, np.dtype(dtype).name)
    if key not in _sweeps:
        grid, VM, e0, s = _problem(shape, dtype)
        out = {}
        for tag, env in (("on", ON), ("off", OFF)):
            _env(monkeypatch, env)
            with _handle(grid, VM, dtype) as dev:
                dev.set_sfield(s)
                for direction in (1, 2, 3):
                    for nu in (1, 2, 3):
                        dev.set_efield(e0)
                        dev.smooth(nu, direction)
                        out[tag, direction, nu] = dev.get_efield()
                        out["kernel", tag, direction] = dev.last_sweep_kernel()
        _sweeps[key] = (grid, VM, e0, s, out)
    return _sweeps[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=["c128", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_table_is_bit_identical_to_the_computing_path(lab, monkeypatch, shape, dtype):
    """One smoothing call of nu = 1, 2, 3 sweeps per line direction, table forced on against off: the same field, bit for bit; and the
    plan says that the table was on where the lines are scanned inside one wave."""
    _, _, e0, _, out = _sweep_results(monkeypatch, shape, dtype)
    _env(monkeypatch, ON)
    on_dirs = _table_dirs(lab, shape, dtype)
    want = [d for d in (1, 2, 3) if shape[d - 1] <= 16]
    assert on_dirs == want, (shape, on_dirs)
    _env(monkeypatch, OFF)
    assert _table_dirs(lab, shape, dtype) == []
    for direction in (1, 2, 3):
        assert out["kernel", "on", direction] == out["kernel", "off", direction]
        for nu in (1, 2, 3):
            got, ref = out["on", direction, nu], out["off", direction, nu]
            assert np.isfinite(got).all() and not np.array_equal(got, e0)
            assert np.array_equal(got, ref), (shape, direction, nu, np.abs(got - ref).max())


@pytest.mark.parametrize("dtype", DTYPES, ids=["c128", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_table_against_the_reference(oracle, lab, monkeypatch, shape, dtype):
    """The same calls with the table against the oracle's colour-ordered line smoother (order = 1), at the tolerance
    test_chain_kernels_colour_vs_reference holds the kernel families to."""
    grid, VM, e0, s, out = _sweep_results(monkeypatch, shape, dtype)
    for direction in (1, 2, 3):
        for nu in (1, 2, 3):
            eo = np.array(e0)
            oracle.gauss_seidel(grid.vnC, eo, np.array(s), VM.eta_x, VM.eta_y, VM.eta_z, VM.zeta, *grid.h, nu, direction=direction,
                                order=1)
            assert relerr(out["on", direction, nu], eo) < 2e-10, (shape, direction, nu)


@pytest.mark.parametrize("dtype", DTYPES, ids=["c128", "f64"])
@pytest.mark.parametrize("shape", [(8, 40, 8), (6, 24, 16)], ids=str)
def test_batch_of_three_with_a_frozen_system(lab, monkeypatch, shape, dtype):
    """Three systems share the tables as they share the factor: each active system is bit for bit its own single handle, the frozen
    one keeps its field."""
    grid, VM, _, _ = _problem(shape, dtype)
    rng = np.random.default_rng(17)
    cplx = dtype == np.complex128
    fields = [tuple((rng.standard_normal(grid.nE) + (1j * rng.standard_normal(grid.nE) if cplx else 0)).astype(dtype) for _ in range(2))
              for _ in range(3)]
    _env(monkeypatch, ON)
    assert _table_dirs(lab, shape, dtype)
    for direction in _table_dirs(lab, shape, dtype):
        single = []
        with _handle(grid, VM, dtype) as dev:
            for e0, s in fields:
                dev.set_sfield(s)
                dev.set_efield(e0)
                dev.smooth(2, direction)
                single.append(dev.get_efield())
        with _handle(grid, VM, dtype) as dev:
            dev.set_batch(3)
            for b, (e0, s) in enumerate(fields):
                dev.select(b)
                dev.set_sfield(s)
                dev.set_efield(e0)
            dev.set_mask([1, 0, 1])
            dev.smooth(2, direction)
            got = []
            for b in range(3):
                dev.select(b)
                got.append(dev.get_efield())
        assert np.array_equal(got[0], single[0]) and np.array_equal(got[2], single[2]), (shape, direction)
        assert np.array_equal(got[1], fields[1][0]), (shape, direction)
        assert not np.array_equal(single[1], fields[1][0])


@pytest.mark.parametrize("freq", [1.5, -1.5], ids=["c128", "f64"])
def test_set_model_rewrites_the_tables(lab, monkeypatch, freq):
    """Another model on an open handle whose tables exist: the sweeps that follow are those of a fresh handle on that model, bit for
    bit (a table left over from the first model would not be)."""
    import emg3d_amd as em
    from emg3d_amd import models
    from emg3d_amd.solver import DeviceMG, MGParameters
    shape = (16, 12, 8)
    dtype = np.complex128 if freq > 0 else np.float64
    rng = np.random.default_rng(3)
    grid = em.TensorMesh([rng.uniform(40, 60, n) for n in shape], origin=(0, 0, 0))
    m1, m2 = (em.Model(grid, *(10 ** rng.uniform(-0.5, 1.5, grid.nC) for _ in range(3))) for _ in range(2))
    spec = em.fields.FrequencySpec(freq)
    e0, s = (rng.standard_normal(grid.nE).astype(dtype) for _ in range(2))
    _env(monkeypatch, ON)
    assert _table_dirs(lab, shape, dtype) == [1, 2, 3]

    def sweeps(dev):
        out = []
        for direction in (1, 2, 3):
            dev.set_efield(e0)
            dev.smooth(2, direction)
            out.append(dev.get_efield())
        return out

    def handle(model):
        dev = DeviceMG.from_model(grid, models.model_parts(grid, model, raw=True), spec)
        dev.set_params(MGParameters(verb=0, cycle='F', sslsolver=False, linerelaxation=True, semicoarsening=True, vnC=grid.vnC,
                                    ordering='colour'))
        dev.set_sfield(s)
        return dev

    with handle(m2) as fresh:
        ref = sweeps(fresh)
    with handle(m1) as dev:
        first = sweeps(dev)
        dev.set_model(grid, m2)
        got = sweeps(dev)
    for d in range(3):
        assert not np.array_equal(first[d], ref[d])
        assert np.array_equal(got[d], ref[d]), d + 1


@pytest.mark.parametrize("shape", [(16, 16, 16), (32, 16, 8)], ids=str)
def test_whole_f_cycle_solves(lab, monkeypatch, shape):
    """F-cycle solves (semicoarsening, line relaxation: every level of <= 16-block lines loads tables), table on against off: the
    same norms at every cycle and the same field."""
    import emg3d_amd as em
    rng = np.random.default_rng(11)
    h = [rng.uniform(40, 60, n) * 1.1 ** np.abs(np.arange(n) - n / 2) for n in shape]
    grid = em.TensorMesh(h, origin=(0, 0, 0))
    rho = 10 ** rng.uniform(-0.5, 1.5, grid.nC)
    model = em.Model(grid, rho, 2 * rho, 3 * rho, mu_r=rng.uniform(1., 2., grid.nC))
    out = {}
    for tag, env in (("on", {"EMG3D_QPL_SCANTAB": "1"}), ("off", {"EMG3D_QPL_SCANTAB": "0"})):
        _env(monkeypatch, env)
        sf = em.get_source_field(grid, [h[0].sum() / 2, h[1].sum() / 2, h[2].sum() / 2, 30., 10.], 1.0)
        e, info = em.solve(grid, model, sf, cycle='F', semicoarsening=True, linerelaxation=True, return_info=True, maxit=4, tol=1e-30,
                           verb=0)
        out[tag] = (np.array(e), np.array(info['error_at_cycle']))
    assert np.isfinite(out["on"][0]).all() and np.abs(out["on"][0]).max() > 0
    assert np.array_equal(out["on"][1], out["off"][1])
    assert np.array_equal(out["on"][0], out["off"][0])


def test_graph_replays_equal_eager_cycles(lab, monkeypatch):
    """Three replays of one captured cycle (the captured launches hold the tables' addresses) equal three eager cycles."""
    shape, dtype = (16, 16, 8), np.complex128
    grid, VM, _, s = _problem(shape, dtype)
    out = {}
    for tag, env in (("graph", dict(ON)), ("eager", dict(ON, EMG3D_GRAPH="0"))):
        _env(monkeypatch, env)
        with _handle(grid, VM, dtype) as dev:
            dev.set_sfield(s)
            dev.set_efield(None)
            dev.prepare(1, 4)
            norms = dev.cycles(3, [1], [4])
            out[tag] = (dev.get_efield(), np.array(norms))
    assert np.isfinite(out["graph"][0]).all() and np.abs(out["graph"][0]).max() > 0
    assert np.array_equal(out["graph"][1], out["eager"][1])
    assert np.array_equal(out["graph"][0], out["eager"][0])


@pytest.mark.parametrize("shape", [(8, 40, 8), (24, 16, 6)], ids=str)
def test_a_refused_table_keeps_the_computing_path(lab, monkeypatch, shape):
    """A byte budget of a few bytes: the plan reports the table off, the level sweeps as it does without, the same results."""
    dtype = np.complex128
    _, _, _, _, out = _sweep_results(monkeypatch, shape, dtype)
    grid, VM, e0, s = _problem(shape, dtype)
    _env(monkeypatch, dict(ON, EMG3D_QPL_SCANTAB_BYTES="64"))
    for d in (1, 2, 3):
        p = lab.sweep_plan(shape, d, dtype=dtype)
        assert not p["scan_table"] and (p["scan_table_bytes"] > 64 or p["scan_table_bytes"] == 0)
    with _handle(grid, VM, dtype) as dev:
        dev.set_sfield(s)
        for direction in (1, 2, 3):
            dev.set_efield(e0)
            dev.smooth(2, direction)
            assert np.array_equal(dev.get_efield(), out["off", direction, 2]), (shape, direction)
