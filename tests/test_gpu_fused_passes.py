"""GPU: the fused colour passes of the short-line levels (k_line_sweep_qpl FZ + k_scatter_slabs, csrc/sweep_plan.hpp plan_fuse) are
BIT-identical to the per-pass launches of the same library (lab build, EMG3D_QPL_FUSE=0): one smoothing call on small grids in every
direction the scan kernel serves with <= 8 blocks, nu = 1, 2, 3, both scalar types, with and without mu_r, own widths 2, 3 and the
default; a batched handle with a frozen system; whole F- and V-cycles on the captured-graph and the eager path; a scratch budget that
forces the fall-back; the product library with no knob set against the lab build with fusion off.  Both sides run the same per-line code, so every comparison is `array_equal`."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_KNOBS = ("EMG3D_QPL_FUSE", "EMG3D_QPL_FUSE_W", "EMG3D_QPL_FUSE_BYTES", "EMG3D_GRAPH", "EMG3D_LOG")
OFF = {"EMG3D_QPL_FUSE": "0"}
ON = {"EMG3D_QPL_FUSE": "8"}          # 4- and 8-block lines, whatever the product's default is


@pytest.fixture(autouse=True)
def _lab_build(lab):
    yield


def _env(monkeypatch, env):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)      # read when a handle is created


def _problem(shape, dtype, seed, mu_r):
    import emg3d_amd as em
    rng = np.random.default_rng(seed)
    cplx = dtype == np.complex128
    h = [rng.uniform(0.5, 2, n) * 1.15 ** np.abs(np.arange(n) - n / 2) for n in shape]      # stretched
    grid = em.TensorMesh(h, origin=(0, 0, 0))

    def rnd(n):
        a = rng.standard_normal(n)
        return a + 1j * rng.standard_normal(n) if cplx else a

    scale = 0.3j if cplx else -1.0
    eta = [np.asfortranarray(rng.uniform(0.5, 2, shape) * scale) for _ in range(3)]          # tri-axial
    vol = np.einsum('i,j,k->ijk', *h)
    zeta = np.asfortranarray(vol / rng.uniform(1., 2., shape) if mu_r else vol)
    kw = dict(freq=1. if cplx else -1.)
    return em, grid, eta, zeta, em.Field(grid, rnd(grid.nE), **kw), em.Field(grid, rnd(grid.nE), **kw)


@pytest.mark.parametrize("dtype", [np.complex128, np.float64])
@pytest.mark.parametrize("shape", [(40, 4, 4), (4, 40, 8), (8, 6, 40), (24, 8, 5), (12, 4, 4)])
def test_one_smoothing_call(monkeypatch, capfd, shape, dtype):
    fused_calls = 0
    for mu_r in (False, True):
        em, grid, eta, zeta, s, e0 = _problem(shape, dtype, 7 + mu_r, mu_r)
        for direction in (1, 2, 3):
            if shape[direction - 1] > 8:
                continue
            for nu in (1, 2, 3):
                res = {}
                for tag, env in (("off", OFF), ("w2", dict(ON, EMG3D_QPL_FUSE_W="2")), ("w3", dict(ON, EMG3D_QPL_FUSE_W="3")),
                                 ("default", ON)):
                    _env(monkeypatch, dict(env, EMG3D_LOG="1"))
                    e = e0.copy()
                    capfd.readouterr()
                    em.core._gs(direction, e.fx, e.fy, e.fz, s.fx, s.fy, s.fz, *eta, zeta, *grid.h, nu, order=1)
                    log = capfd.readouterr().err
                    # (the fused path was taken where it was asked for, and only there)
                    assert ("fused passes" in log) == (tag != "off"), (tag, direction, nu, log[-300:])
                    fused_calls += tag != "off"
                    res[tag] = np.array(e)
                assert not np.array_equal(res["off"], np.array(e0))
                for tag, got in res.items():
                    assert np.array_equal(got, res["off"]), (tag, direction, nu, mu_r,
                                                             int((got != res["off"]).sum()), float(np.abs(got - res["off"]).max()))
    assert fused_calls > 0


def _cycle_problem(shape, dtype, seed):
    import emg3d_amd as em
    rng = np.random.default_rng(seed)
    h = [rng.uniform(40, 60, n) * 1.1 ** np.abs(np.arange(n) - n / 2) for n in shape]
    grid = em.TensorMesh(h, origin=(0, 0, 0))
    rho = 10 ** rng.uniform(-0.5, 1.5, grid.nC)
    model = em.Model(grid, rho, 2 * rho, 3 * rho, mu_r=rng.uniform(1., 2., grid.nC))
    freq = 1.0 if dtype == np.complex128 else -1.0
    src = [h[0].sum() / 2, h[1].sum() / 2, h[2].sum() / 2, 30., 10.]
    return em, grid, model, freq, src


@pytest.mark.parametrize("shape,cycle,dtype", [((32, 16, 16), 'F', np.complex128), ((16, 16, 16), 'V', np.complex128),
                                               ((16, 16, 16), 'F', np.float64), ((32, 16, 16), 'V', np.float64)])
def test_whole_cycles(monkeypatch, capfd, shape, cycle, dtype):
    """sc + lr cycles: per-cycle residual norms and the final field, fused against off, captured graphs and eager launches; the
    lexicographic order does not fuse and does not change."""
    em, grid, model, freq, src = _cycle_problem(shape, dtype, 21)
    sf = em.get_source_field(grid, src, freq)
    out = {}
    for ordering in ("colour", "lex"):
        for graph in ("1", "0"):
            for tag, env in (("off", OFF), ("on", ON), ("w2", dict(ON, EMG3D_QPL_FUSE_W="2")), ("w3", dict(ON, EMG3D_QPL_FUSE_W="3"))):
                _env(monkeypatch, dict(env, EMG3D_GRAPH=graph, EMG3D_LOG="1"))
                capfd.readouterr()
                e, info = em.solve(grid, model, sf, cycle=cycle, semicoarsening=True, linerelaxation=True, return_info=True, maxit=3,
                                   tol=1e-30, verb=0, ordering=ordering)
                log = capfd.readouterr().err
                assert ("fused passes" in log) == (tag != "off" and ordering == "colour"), (ordering, graph, tag)
                out[ordering, graph, tag] = (np.array(e), np.array(info['error_at_cycle']))
    for (ordering, graph, tag), (e, norms) in out.items():
        ref = out[ordering, "1", "off"]
        assert np.array_equal(e, ref[0]) and np.array_equal(norms, ref[1]), (ordering, graph, tag)
    assert np.abs(out["colour", "1", "on"][0]).max() > 0


def test_batched_handle_with_a_frozen_system(monkeypatch):
    """Three systems through one handle, the middle one frozen: the live systems equal their unfused results bit for bit, the frozen
    one keeps its field."""
    from emg3d_amd.solver import DeviceMG, MGParameters
    em, grid, model, freq, _ = _cycle_problem((16, 16, 16), np.complex128, 33)
    srcs = [[400., 400., 400., 30., 10.], [300., 250., 400., -40., 5.], [500., 420., 300., 90., 45.]]
    sfield = em.get_source_field(grid, srcs[0], freq)
    vm = em.VolumeModel(grid, model, sfield)
    var = MGParameters(verb=0, cycle='F', sslsolver=False, linerelaxation=True, semicoarsening=True, vnC=grid.vnC)
    out = {}
    for tag, env in (("off", OFF), ("on", ON), ("w2", dict(ON, EMG3D_QPL_FUSE_W="2"))):
        _env(monkeypatch, env)

        def fields(dev):
            got = []
            for b in range(3):
                dev.select(b)
                got.append(np.array(dev.get_efield()))
            return got

        with DeviceMG(grid, vm, sfield.dtype) as dev:
            dev.set_params(var)
            dev.set_batch(3)
            for b, src in enumerate(srcs):
                dev.select(b)
                dev.set_sfield(em.get_source_field(grid, src, freq))
            res = [np.array(dev.cycles(2, [1, 2, 3], [4, 5, 6]))]
            mid = fields(dev)
            dev.set_mask(np.array([1, 0, 1], dtype=np.int32))
            res.append(np.array(dev.cycles(2, [3, 1], [6, 5]))[:, [0, 2]])       # (the norm of a frozen system is not defined)
            end = fields(dev)
            np.testing.assert_array_equal(end[1], mid[1])                        # frozen: untouched
            assert not np.array_equal(end[0], mid[0]) and not np.array_equal(end[2], mid[2])
        out[tag] = res + mid + end
    for tag in ("on", "w2"):
        for a, b in zip(out[tag], out["off"]):
            np.testing.assert_array_equal(a, b)


def test_scratch_over_budget_falls_back(monkeypatch, capfd):
    """A byte budget too small for the private copies: the handle keeps the per-pass launches, with identical results."""
    em, grid, model, freq, src = _cycle_problem((16, 16, 16), np.complex128, 5)
    sf = em.get_source_field(grid, src, freq)
    out = {}
    for tag, env in (("off", OFF), ("on", ON), ("tiny", dict(ON, EMG3D_QPL_FUSE_BYTES="1000"))):
        _env(monkeypatch, dict(env, EMG3D_LOG="1"))
        capfd.readouterr()
        e, info = em.solve(grid, model, sf, cycle='F', semicoarsening=True, linerelaxation=True, return_info=True, maxit=2, tol=1e-30,
                           verb=0)
        assert ("fused passes" in capfd.readouterr().err) == (tag == "on")
        out[tag] = (np.array(e), np.array(info['error_at_cycle']))
    for tag in ("on", "tiny"):
        assert np.array_equal(out[tag][0], out["off"][0]) and np.array_equal(out[tag][1], out["off"][1])


@pytest.mark.parametrize("shape,cycle,dtype", [((32, 16, 16), 'F', np.complex128), ((16, 16, 16), 'V', np.float64)])
def test_product_library_default_configuration(monkeypatch, capfd, lab, shape, cycle, dtype):
    """What ships -- the PRODUCT library, no variable set but the launch log: 4-block lines fused, the default own width -- against the
    lab build with fusion off: per-cycle norms and the final field bit for bit, and the product did fuse."""
    em, grid, model, freq, src = _cycle_problem(shape, dtype, 44)
    sf = em.get_source_field(grid, src, freq)
    out = {}
    for tag, path, env in (("off", lab.LAB_PATH, OFF), ("product", lab.LIB_PATH, {})):
        prev = lab.use(path)
        try:
            _env(monkeypatch, dict(env, EMG3D_LOG="1"))
            capfd.readouterr()
            e, info = em.solve(grid, model, sf, cycle=cycle, semicoarsening=True, linerelaxation=True, return_info=True, maxit=3, tol=1e-30,
                               verb=0)
            assert ("fused passes" in capfd.readouterr().err) == (tag == "product")
            out[tag] = (np.array(e), np.array(info['error_at_cycle']))
        finally:
            lab.use(prev)
    assert np.array_equal(out["product"][0], out["off"][0]) and np.array_equal(out["product"][1], out["off"][1])
    assert np.abs(out["product"][0]).max() > 0
