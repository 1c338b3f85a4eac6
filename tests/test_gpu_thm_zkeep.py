"""GPU: the z keep of the two-sided chain kernel (k_line_sweep_thm, csrc/smooth_thm.hpp) changes no bit.

The forward pass of a half leaves one z per row and step for the backward pass; the last steps of a half keep theirs in LDS
instead of parking them in the field (how many: csrc/sweep_plan.hpp sweep_thm_zkeep, tests/test_thm_zkeep_plan.py).  Parked and
kept steps run in loops of their own, split at a multiple of the prefetch depth.  Checked here, on the lab build with the scan
and affine kernels off (EMG3D_QPL=0 EMG3D_THA=0: k_line_sweep_thm serves every shape below): two sweeps against the oracle's
smoother, and -- the strong check -- bit for bit against the same call with the keep off (EMG3D_THM_ZKEEP=0), on line lengths
where the split can go wrong, with caps that put the parked / kept boundary at every residue of the prefetch depth, crossed with
the prefetch depth, the lines per pair of waves, split copies, both scalar types and both orderings.  Then the product library,
where the planner itself chooses the kernel: one-round launches of 66-block lines in all three directions against the oracle, and
a two-system handle with one system frozen against separate solves."""
import numpy as np
import pytest

from conftest import assert_norms_close, load_golden, relerr

pytestmark = pytest.mark.gpu

_THM = {"EMG3D_QPL": "0", "EMG3D_THA": "0"}
CAPS = ["-1", "1", "2", "3", "4", "5"]
# z-lines whose halves have 1 + 0, 1 + 1, 2 + 1, 7 + 7, 8 + 7 and 16 + 15 steps; the x- and y-line twins; 144 lines in several
# workgroups with a ragged last pair
SHAPES = [((9, 11, 3), 3), ((8, 6, 4), 3), ((6, 8, 5), 3), ((5, 7, 16), 3), ((7, 5, 17), 3), ((6, 5, 33), 3),
          ((16, 5, 6), 1), ((6, 16, 5), 2), ((24, 24, 7), 3)]

_problems = {}
_results = {}


def _problem(oracle, shape, direction, dtype):
    """Random widths, model, source and start fields of a shape, and the oracle's two sweeps in both orderings: computed once."""
    key = (shape, direction, np.dtype(dtype).char)
    if key not in _problems:
        rng = np.random.default_rng(sum(shape) + 7 * direction)
        cplx = np.dtype(dtype) == np.complex128
        h = [rng.uniform(0.5, 2, n) for n in shape]
        nE = shape[0] * (shape[1] + 1) * (shape[2] + 1) + (shape[0] + 1) * shape[1] * (shape[2] + 1) + \
            (shape[0] + 1) * (shape[1] + 1) * shape[2]

        def rnd(n):
            a = rng.standard_normal(n)
            return a + 1j * rng.standard_normal(n) if cplx else a

        if cplx:
            eta = [np.asfortranarray(rng.uniform(0.5, 2, shape) * 0.3j) for _ in range(3)]
        else:
            eta = [np.asfortranarray(-rng.uniform(0.5, 2, shape)) for _ in range(3)]
        zeta = np.asfortranarray(rng.uniform(0.5, 2, shape))
        s, e0 = rnd(nE), [rnd(nE), rnd(nE)]
        ref = []
        for order in (0, 1):
            eo = e0[order].copy()
            oracle.gauss_seidel(np.array(shape), eo, s.copy(), *eta, zeta, *h, 2, direction=direction, order=order)
            ref.append(eo)
        for a in e0 + ref:          # shared by every case of the shape: never written again
            a.setflags(write=False)
        _problems[key] = dict(h=h, eta=eta, zeta=zeta, s=s, e0=e0, ref=ref, freq=1. if cplx else -1.)
    return _problems[key]


def _sweeps(monkeypatch, oracle, shape, direction, dtype, env):
    """Two sweeps in both orderings under `env` (the handle reads it when it is created); cached per setting."""
    import emg3d_amd as em
    from emg3d_amd import _lib
    key = (shape, direction, np.dtype(dtype).char, tuple(sorted(env.items())))
    if key in _results:
        return _results[key]
    p = _problem(oracle, shape, direction, dtype)
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        for ordering in ('colour', 'lex'):
            name = _lib.sweep_plan(shape, direction, dtype=dtype, ordering=ordering)["kernel"]
            assert name.startswith("k_line_sweep_thm<"), (shape, direction, ordering, env, name)
        grid = em.TensorMesh([np.array(x) for x in p['h']], origin=(0, 0, 0))
        s = em.Field(grid, p['s'].copy(), freq=p['freq'])
        out = []
        for order in (0, 1):
            e = em.Field(grid, p['e0'][order].copy(), freq=p['freq'])
            em.core._gs(direction, e.fx, e.fy, e.fz, s.fx, s.fy, s.fz, *p['eta'], p['zeta'], *grid.h, 2, order=order)
            out.append(np.array(e))
    _results[key] = out
    return out


def _check(monkeypatch, oracle, shape, direction, dtype, env, cap):
    p = _problem(oracle, shape, direction, dtype)
    off = _sweeps(monkeypatch, oracle, shape, direction, dtype, dict(_THM, EMG3D_THM_ZKEEP="0", **env))
    got = _sweeps(monkeypatch, oracle, shape, direction, dtype, dict(_THM, EMG3D_THM_ZKEEP=cap, **env))
    for order in (0, 1):
        assert np.isfinite(got[order]).all()
        assert relerr(got[order], p['ref'][order]) < 1e-10, (order, relerr(got[order], p['ref'][order]))
        assert np.array_equal(got[order], off[order]), (order, relerr(got[order], off[order]))
        assert not np.array_equal(got[order], p['e0'][order])


@pytest.fixture(autouse=True)
def _lab_build(lab):
    yield


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("shape,direction", SHAPES)
def test_line_lengths(oracle, monkeypatch, shape, direction, cap):
    _check(monkeypatch, oracle, shape, direction, np.complex128, {}, cap)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("shape,direction", [((5, 7, 16), 3), ((16, 5, 6), 1)])
def test_float64(oracle, monkeypatch, shape, direction, cap):
    _check(monkeypatch, oracle, shape, direction, np.float64, {}, cap)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("stages", ["2", "3"])
@pytest.mark.parametrize("shape,direction", [((7, 5, 17), 3), ((6, 5, 33), 3), ((6, 8, 5), 3)])
def test_prefetch_depths(oracle, monkeypatch, shape, direction, stages, cap):
    _check(monkeypatch, oracle, shape, direction, np.complex128, {"EMG3D_TW_STAGES": stages}, cap)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("lpw", ["4", "8", "12"])
@pytest.mark.parametrize("shape,direction", [((24, 24, 7), 3), ((16, 5, 6), 1)])
def test_lines_per_pair(oracle, monkeypatch, shape, direction, lpw, cap):
    _check(monkeypatch, oracle, shape, direction, np.complex128, {"EMG3D_TH_LPW": lpw}, cap)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("shape,direction", [((5, 7, 16), 3), ((16, 5, 6), 1), ((6, 16, 5), 2)])
def test_split_copies(oracle, monkeypatch, shape, direction, split, cap):
    _check(monkeypatch, oracle, shape, direction, np.complex128, {"EMG3D_SPLIT": split}, cap)


def test_long_lines_parked_prefix(oracle, monkeypatch):
    """599 steps per half, 59 of them fit: the parked loops run for hundreds of steps before the kept ones."""
    _check(monkeypatch, oracle, (16, 16, 1200), 3, np.complex128, {}, "-1")


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("zsep", ["1", "0"])
@pytest.mark.parametrize("dtype", [np.complex128, np.float64])
def test_cycles_with_zeta_from_widths_and_read(monkeypatch, zsep, cap, dtype):
    """Whole cycles on a model without mu_r: level 0 forms zeta from the widths (the ZS instantiations) or reads it
    (EMG3D_ZSEP=0), dipole source (source-free and flagged waves): fields and per-cycle norms bit for bit against the keep off."""
    import emg3d_amd as em
    shape = (16, 12, 20)
    rng = np.random.default_rng(29)
    h = [rng.uniform(20., 60., n) * 1.07 ** np.abs(np.arange(n) - n / 2) for n in shape]
    grid = em.TensorMesh(h, origin=tuple(-hh.sum() / 2 for hh in h))
    model = em.Model(grid, *(10 ** rng.uniform(-0.5, 1.5, shape) for _ in range(3)))
    sfield = em.get_source_field(grid, [0., 0., 0., 30., 10.], 1.0 if dtype is np.complex128 else -3.0)
    key = ("cycles", zsep, np.dtype(dtype).char)
    out = {}
    for c in ("0", cap):
        if c == "0" and key in _results:
            out[c] = _results[key]
            continue
        for k, v in dict(_THM, EMG3D_ZSEP=zsep, EMG3D_THM_ZKEEP=c).items():
            monkeypatch.setenv(k, v)
        e, info = em.solve(grid, model, sfield, cycle='F', semicoarsening=True, linerelaxation=True, maxit=3, tol=1e-30, verb=0,
                           return_info=True)
        out[c] = (np.array(e), np.array(info['error_at_cycle']))
    _results[key] = out["0"]
    assert np.isfinite(out[cap][0]).all() and np.abs(out[cap][0]).max() > 0
    np.testing.assert_array_equal(out[cap][0], out["0"][0])
    np.testing.assert_array_equal(out[cap][1], out["0"][1])


@pytest.mark.parametrize("ordering", ["lex", "colour"])
def test_f_cycle_matches_reference_arithmetic(oracle, monkeypatch, ordering):
    """The 16^3 F-cycle solve with k_line_sweep_thm on every line level and the keep at its default depth, held as
    tests/test_gpu_variants.py::test_variant_matches_oracle holds the two-sided kernel: against the oracle in both orderings, and in
    the colour ordering against the reference's own arithmetic (tests/golden/solves_16_colour.npz) -- cycle count equal, per-cycle
    norms to 1e-10 while the residual is above 1e-4 of the source norm, field below 1e-11."""
    import emg3d_amd as em
    for k, v in _THM.items():
        monkeypatch.setenv(k, v)
    g = load_golden("solves_16.npz")
    grid = em.TensorMesh([g['hx'], g['hy'], g['hz']], origin=g['origin'])
    model = em.Model(grid, g['rho_b'], 2 * g['rho_b'], 3 * g['rho_b'])
    sfield = em.get_source_field(grid, g['src'], float(g['freq']))
    e, info = em.solve(grid, model, sfield, return_info=True, ordering=ordering, cycle='F', semicoarsening=True, linerelaxation=True)
    vm = em.VolumeModel(grid, model, sfield)
    oe, oinfo = oracle.solve(oracle.Mesh(grid.h, grid.origin), oracle.VModel(vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta),
                             np.array(sfield), cycle='F', semicoarsening=True, linerelaxation=True, order=0 if ordering == 'lex' else 1)
    assert info['it_mg'] == oinfo['it_mg']
    assert_norms_close(info['error_at_cycle'], oinfo['error_at_cycle'], strict_above=1e-4)
    assert relerr(e, oe) < 1e-11
    if ordering == 'colour':
        c = load_golden("solves_16_colour.npz")
        assert info['it_mg'] == c['F_sclr_it'][0] and info['exit'] == int(c['F_sclr_exit'])
        assert_norms_close(info['error_at_cycle'], c['F_sclr_error_at_cycle'], strict_above=1e-4)
        assert relerr(e, c['F_sclr_efield']) < 1e-11


# ---- the product library: the planner itself chooses k_line_sweep_thm ---------------------------------------------------------------
@pytest.fixture
def product():
    from emg3d_amd import _lib
    prev = _lib.use(None)
    yield _lib
    _lib.use(prev)


@pytest.mark.parametrize("dtype", [np.complex128, np.float64])
@pytest.mark.parametrize("shape,direction", [((92, 92, 66), 3), ((66, 92, 92), 1), ((92, 66, 92), 2)])
def test_product_library_one_round_launches(oracle, product, monkeypatch, shape, direction, dtype):
    """2116 lines per colour of 66 blocks: one round of waves, every half kept whole (32 steps); z-lines, x-lines on the
    transposed copy, y-lines."""
    from test_gpu_kernels import _sweeps_against_oracle
    for k in ("EMG3D_QPL", "EMG3D_THA", "EMG3D_THM_ZKEEP"):
        monkeypatch.delenv(k, raising=False)
    z = product.sweep_thm_zkeep(shape, direction, dtype=dtype)
    assert z["kept"] == z["half"] == 32
    _sweeps_against_oracle(oracle, dtype, shape, {direction: "k_line_sweep_thm<"}, elsewhere_not="k_line_sweep_thm<")


def test_product_library_two_systems_one_frozen(product):
    """Two sources in one handle on 92 x 92 x 66, z-lines, the second frozen after the first cycle: each system bit for bit its own
    solve (the check of tests/test_gpu_batch.py at a size where the planner chooses k_line_sweep_thm for the batched launch too)."""
    import emg3d_amd as em
    from emg3d_amd import models
    from emg3d_amd.solver import DeviceMG, MGParameters
    shape = (92, 92, 66)
    rng = np.random.default_rng(3)
    h = [40.0 * 1.04 ** np.abs(np.arange(n) - n / 2 + 0.5) for n in shape]
    grid = em.TensorMesh(h, origin=tuple(-hh.sum() / 2 for hh in h))
    rho = 10 ** rng.uniform(-0.5, 2.0, grid.nC)
    model = em.Model(grid, rho, 1.5 * rho, 2 * rho)
    srcs = [[0., 0., 0., 30., 10.], [220., -310., -150., 110., -20.]]
    var = MGParameters(cycle='V', sslsolver=False, semicoarsening=False, linerelaxation=True, vnC=grid.vnC, verb=0)
    proto = em.SourceField(grid, freq=1.0)
    vm = models.VolumeModel(grid, model, proto)
    assert product.sweep_plan(shape, 3, nsys=2)["kernel"].startswith("k_line_sweep_thm<")

    def handle(nsys):
        dev = DeviceMG(grid, vm, proto.dtype)
        dev.set_params(var, ordering='colour')
        if nsys > 1:
            dev.set_batch(nsys)
        return dev

    ref = []
    for b, ncyc in ((0, 2), (1, 1)):
        with handle(1) as dev:
            dev.set_source(srcs[b], proto.smu0)
            for _ in range(ncyc):
                n = dev.cycle(0, 7)
            ref.append((n, dev.get_efield()))
    with handle(2) as dev:
        for b in range(2):
            dev.select(b)
            dev.set_source(srcs[b], proto.smu0)
        n1 = dev.cycle(0, 7)
        dev.set_mask([1, 0])
        n2 = dev.cycle(0, 7)
        dev.time_sweep(3, 1)
        assert dev.last_sweep_kernel().startswith("k_line_sweep_thm<"), dev.last_sweep_kernel()
        assert n1[1] == ref[1][0] and n2[0] == ref[0][0]
    with handle(2) as dev:       # (time_sweep changed the fields: compare them in a fresh run)
        for b in range(2):
            dev.select(b)
            dev.set_source(srcs[b], proto.smu0)
        dev.cycle(0, 7)
        dev.set_mask([1, 0])
        dev.cycle(0, 7)
        for b in range(2):
            dev.select(b)
            np.testing.assert_array_equal(dev.get_efield(), ref[b][1])
