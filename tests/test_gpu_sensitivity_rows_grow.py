"""GPU: the row buffers of emg3d_mg_sens_rows when they GROW -- a small call, then a larger one, then the small one again on one
handle.  The buffers are blocks of the handle's own, given back whole when a larger call needs more; nothing else the handle holds
may move or go with them: the rows, the accumulators and the weight table of sens_acc_add, the model-grid tables and factors, and
device_bytes are checked after every step against a second handle whose largest calls come first (the order every other test of
tests/test_gpu_sensitivity_rows.py uses)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FREQ = 1.5
NSYS = 3
USE_FWD, USE_ADJ = np.array([1, 0, 1], dtype=np.int32), np.array([0, 1, 1], dtype=np.int32)       # 4 pairs; the last: (2, 2)
ONE = np.array([0, 0, 1], dtype=np.int32)                                                          # 1 pair: (2, 2)


def _align(nbytes):
    return (max(nbytes, 8) + 255) // 256 * 256


def _open(em, grid, model_grid, fields, F, Q):
    from emg3d_amd import models
    from emg3d_amd.solver import DeviceMG
    model = em.Model(grid, np.ones(grid.nC), mapping='Conductivity')
    spec = em.fields.FrequencySpec(FREQ)
    dev = DeviceMG.from_model(grid, models.model_parts(grid, model, raw=True), spec)
    dev.set_batch(NSYS)
    dev.bvec_alloc(1)
    for b in range(NSYS):
        dev.select(b)
        dev.set_efield(em.Field(grid, fields[1][b].copy(), freq=FREQ))
        dev.bvec_set(0, b, fields[0][b])
    dev.set_model_grid(model_grid)
    dev.set_regrid_factors(F, Q)
    return dev, spec.smu0


# 'unaligned': 12 x 10 x 8 from 7 x 5 x 4 -- every buffer a few hundred KB at most (what an arena chunk of the handle would take);
# '48': 48 x 40 x 32 from 20 x 16 x 12 -- one pair per direction 2.9 MB, four pairs 11.8 MB (beyond what an arena chunk takes)
@pytest.mark.parametrize('name', ['unaligned', '48'])
def test_small_then_large_then_small(name):
    import emg3d_amd as em
    from test_model_grid_host import grid_pairs
    model_grid, grid = grid_pairs(em, [name])[name]
    nC, nM = int(grid.nC), int(model_grid.nC)
    rng = np.random.default_rng(91)
    fields = [[rng.standard_normal(grid.nE) + 1j * rng.standard_normal(grid.nE) for _ in range(NSYS)] for _ in range(2)]
    F = tuple(np.asfortranarray(rng.standard_normal(grid.vnC)) for _ in range(3))
    Q = tuple(np.asfortranarray(rng.standard_normal(model_grid.vnC)) for _ in range(3))
    W = rng.uniform(0.5, 2.0, (NSYS, NSYS))

    # the reference handle: the largest calls first
    dev, smu0 = _open(em, grid, model_grid, fields, F, Q)
    with dev:
        big = dev.sens_rows(0, smu0, USE_FWD, USE_ADJ, components=True)
        big_m = dev.sens_rows(0, smu0, USE_FWD, USE_ADJ, components=True, model_grid=True)
        few = dev.sens_rows(0, smu0, ONE, ONE, components=True)
        few_m = dev.sens_rows(0, smu0, ONE, ONE, components=True, model_grid=True)
        dev.grad_acc_reset(True)
        dev.sens_acc_add(0, smu0, USE_FWD, USE_ADJ, W, components=True)
        acc_once = dev.grad_acc_get(True)
        acc_once_m = dev.grad_acc_get_model(True)
        dev.sens_acc_add(0, smu0, USE_FWD, USE_ADJ, W, components=True)
        acc_twice = dev.grad_acc_get(True)
    assert np.array_equal(few[0], big[-1]) and np.array_equal(few_m[0], big_m[-1]) and np.abs(big_m).max() > 0
    assert all(a.max() > 0 for a in acc_once)

    s0, sm = _align(1 * 3 * 2 * nC * 8), _align(1 * 3 * 2 * nM * 8)
    l0, lm = _align(4 * 3 * 2 * nC * 8), _align(4 * 3 * 2 * nM * 8)
    if name == '48':
        assert s0 <= (8 << 20) < l0         # from a size an arena chunk would take to one it would not
    dev, smu0 = _open(em, grid, model_grid, fields, F, Q)
    with dev:
        def same(got, want):
            return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
        # small: the two buffers come into being, and what sens_acc_add needs is allocated after them
        b = dev.device_bytes
        assert np.array_equal(dev.sens_rows(0, smu0, ONE, ONE, components=True), few)
        assert dev.device_bytes - b == s0
        b = dev.device_bytes
        assert np.array_equal(dev.sens_rows(0, smu0, ONE, ONE, components=True, model_grid=True), few_m)
        assert dev.device_bytes - b == sm
        dev.grad_acc_reset(True)
        dev.sens_acc_add(0, smu0, USE_FWD, USE_ADJ, W, components=True)
        assert same(dev.grad_acc_get(True), acc_once)
        # large: both buffers grow, the small blocks are given back and no longer counted
        b = dev.device_bytes
        assert np.array_equal(dev.sens_rows(0, smu0, USE_FWD, USE_ADJ, components=True), big)
        assert dev.device_bytes - b == l0 - s0
        b = dev.device_bytes
        assert np.array_equal(dev.sens_rows(0, smu0, USE_FWD, USE_ADJ, components=True, model_grid=True), big_m)
        assert dev.device_bytes - b == lm - sm
        # everything else the handle holds is where it was: accumulators, model-grid tables and factors, forward and adjoint fields
        assert same(dev.grad_acc_get(True), acc_once)
        assert same(dev.grad_acc_get_model(True), acc_once_m)
        # small again: no new memory, only its own rows; then the large ones once more
        b = dev.device_bytes
        assert np.array_equal(dev.sens_rows(0, smu0, ONE, ONE, components=True), few)
        assert np.array_equal(dev.sens_rows(0, smu0, ONE, ONE, components=True, model_grid=True), few_m)
        assert np.array_equal(dev.sens_rows(0, smu0, USE_FWD, USE_ADJ, components=True), big)
        assert np.array_equal(dev.sens_rows(0, smu0, USE_FWD, USE_ADJ, components=True, model_grid=True), big_m)
        assert dev.device_bytes == b
        # the weight table and the accumulators take another call
        dev.sens_acc_add(0, smu0, USE_FWD, USE_ADJ, W, components=True)
        assert same(dev.grad_acc_get(True), acc_twice)


def test_survey_rows_in_growing_calls():
    """SurveyJacobian: sensitivity_rows(j), then components=True (three times the buffer), then a receiver subset -- each equal, bit
    for bit, to the rows of an object that is asked for it first; jtvec on the object afterwards is what it was before."""
    import emg3d_amd as em
    from test_gpu_sensitivity_diagonal import FREQS, OPTS, SOURCES, _survey
    grid, rec, rng, sig = _survey(em)
    model = em.Model(grid, sig, mapping='Conductivity')
    kw = dict(batch=2, tol=1e-8, **OPTS)
    w = rng.standard_normal((3, 2, 4)) + 0j
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, **kw) as sj:
        want3 = sj.sensitivity_rows(0, components=True)
        want1 = sj.sensitivity_rows(0)
        want_g = sj.jtvec(w)
    with em.optimize.SurveyJacobian(grid, model, SOURCES, FREQS, rec, **kw) as sj:
        one = sj.sensitivity_rows(0, receivers=[2])
        got1 = sj.sensitivity_rows(0)
        got3 = sj.sensitivity_rows(0, components=True)
        assert np.array_equal(got1, want1) and all(np.array_equal(g, x) for g, x in zip(got3, want3))
        assert np.array_equal(sj.sensitivity_rows(0), want1) and np.array_equal(sj.sensitivity_rows(0, receivers=[2]), one)
        assert np.array_equal(one[:, 0], want1[:, 2])
        assert np.array_equal(sj.jtvec(w), want_g)
