"""CPU-only: the oracle in extended precision (oracle/libemg3d_oracle_ld.so: oracle/emg3d_oracle.cpp with every scalar a long double)
is fit to be the TRUTH that tests/test_gpu_accuracy.py measures float64 results against.

* It is the same program as the float64 oracle: on well-conditioned inputs the two agree to 1e-13, every smoother, both orders, both
  scalar types -- and the other kernels (amat_x, restrict, core_solve, blocks_to_amat) dispatch on the dtype in the same way.
* It really solves the lines: after one colour-ordered sweep, `s - A e` (extended amat_x) at the edges the last colour's lines wrote
  is zero to the extended format's rounding; a float64 sweep leaves hundreds of times more there.
* The hard cases (tests/_hard_cases.py) are hard enough to matter and no single pathological line: for every case the GPU tests use,
  the float64 reference is 1e-13 ... 1e-9 from the truth, and the sweep changes the field by more than 1e-3.
* Cases and bound see what they are for: the two-sided grouping the project rejected for accuracy misses the bound on the hard inputs
  (and is invisible on the benign ones), the mirrored grouping the kernels use holds it."""
import numpy as np
import pytest

import _hard_cases as hc


@pytest.fixture(scope="module")
def orc(oracle):
    if not oracle.has_extended():
        pytest.skip("np.longdouble is not the x87 extended format (64-bit significand in 16 bytes)")
    return oracle


SHAPES = [(48, 4, 4), (5, 64, 6), (6, 5, 130), (16, 16, 16)]


def test_has_extended_matches_the_format(oracle):
    fi = np.finfo(np.longdouble)
    assert oracle.has_extended() == (fi.nmant == 63 and np.dtype(np.longdouble).itemsize == 16)


def test_float64_dtypes_run_the_float64_library(oracle):
    """float64 / complex128 fields do not touch the extended library; other dtypes are refused."""
    p = hc.problem("benign", (6, 5, 4), 1, np.complex128)
    e = np.array(p['e0'])
    oracle.gauss_seidel((6, 5, 4), e, np.array(p['s']), *p['eta'], p['zeta'], *p['h'], 1, direction=1, order=1)
    assert e.dtype == np.complex128 and not np.array_equal(e, p['e0'])
    with pytest.raises(TypeError):
        oracle.gauss_seidel((6, 5, 4), e.astype(np.complex64), np.array(p['s']), *p['eta'], p['zeta'], *p['h'], 1, direction=1)


@pytest.mark.parametrize("dtype", hc.DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_extended_agrees_with_float64_on_benign_inputs(orc, shape, dtype):
    for direction in (0, 1, 2, 3):
        for order in (0, 1):
            p, ref, truth = hc.references(orc, "benign", shape, direction, dtype, order=order)
            assert truth.dtype == (np.clongdouble if np.dtype(dtype) == np.complex128 else np.longdouble)
            assert hc.err(p['e0'], truth) > 1e-3                    # (the sweep did something)
            assert hc.err(ref, truth) <= 1e-13, (direction, order, hc.err(ref, truth))
            assert hc.err(ref, truth) > 0                           # (and the truth is not the float64 result converted)


@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_other_kernels_dispatch_on_the_dtype(orc, dtype):
    """amat_x, restrict, core_solve, blocks_to_amat: extended against float64 on the same inputs."""
    shape = (8, 6, 10)
    p = hc.problem("benign", shape, 1, dtype)
    r64, rld = hc.amat_x(orc, p, p['e0']), hc.amat_x(orc, p, p['e0'], ext=True)
    assert rld.dtype == hc.extended(p['s']).dtype and 0 < hc.err(r64, rld) <= 1e-14
    # restriction: all three axes coarsened, the oracle's own weights
    m = orc.Mesh(p['h'], (0., 0., 0.))
    cm = orc.Mesh([np.diff(n[::2]) for n in m.nodes], (0., 0., 0.))
    w = orc.get_restriction_weights(m, cm, 0)
    c64 = np.zeros(cm.nE, dtype=dtype)
    cld = hc.extended(c64)
    orc.restrict(m.vnC, cm.vnC, c64, np.array(p['e0']), *w, 0)
    orc.restrict(m.vnC, cm.vnC, cld, hc.extended(p['e0']), *w, 0)
    assert np.abs(c64).max() > 0 and 0 < hc.err(c64, cld) <= 1e-14
    # a banded system through blocks_to_amat and core_solve
    rng = np.random.default_rng(4)
    n = 5
    a64 = np.zeros(6 * (5 * n - 4), dtype=dtype); b64 = np.zeros(5 * n - 4, dtype=dtype)
    ald, bld = hc.extended(a64), hc.extended(b64)
    for im in range(n):
        middle = (rng.standard_normal(25) + 10 * np.eye(5).ravel()).astype(dtype)
        left, rhs = rng.standard_normal(25), rng.standard_normal(5).astype(dtype)
        orc.blocks_to_amat(a64, b64, middle, left, rhs, im, n)
        orc.blocks_to_amat(ald, bld, hc.extended(middle), left, hc.extended(rhs), im, n)
    assert np.array_equal(a64, ald.astype(dtype)) and np.array_equal(b64, bld.astype(dtype))
    orc.core_solve(a64, b64)
    orc.core_solve(ald, bld)
    assert np.abs(b64).max() > 0 and 0 < hc.err(b64, bld) <= 1e-13


def _diag_max(orc, p):
    """max |A_ii| in extended precision: A applied to the indicator of the edges of one component and one parity of the two
    transverse indices -- edges of a component couple only to their transverse neighbours at distance one, so the result at a probed
    edge is its diagonal entry alone.  The largest entry of A is on the diagonal: an entry that couples two components is
    zeta / (2 h_a h_b), the two diagonals it belongs to hold zeta / (2 h_a^2) and zeta / (2 h_b^2)."""
    shape = p['zeta'].shape
    up = hc.extended
    model = [up(a) for a in (*p['eta'], p['zeta'], *p['h'])]
    amax = 0.
    for c in range(3):
        t1, t2 = [a for a in range(3) if a != c]
        for pa in (0, 1):
            for pb in (0, 1):
                e = up(np.zeros_like(p['s']))
                idx = [slice(None)] * 3
                idx[t1], idx[t2] = slice(pa, None, 2), slice(pb, None, 2)
                hc.field_views(e, shape)[c][tuple(idx)] = 1
                r = np.zeros_like(e)
                orc.amat_x(shape, r, e, *model)
                amax = max(amax, float(np.abs(hc.field_views(r, shape)[c][tuple(idx)]).max()))
    return amax


def _last_colour_edges(shape, direction):
    """Mask of the edges the lines of the last colour of ONE colour-ordered sweep write: the sweep runs backward, colours 0, 3, 2, 1
    (oracle/emg3d_oracle.cpp gs_line), colour 1 = lines at even P-nodes and odd Q-nodes."""
    L, P, Q = {1: (0, 1, 2), 2: (1, 0, 2), 3: (2, 0, 1)}[direction]
    mask = np.zeros(hc.n_edges(shape), dtype=bool)
    v = hc.field_views(mask, shape)

    def at(vL, vP, vQ):
        i = [0, 0, 0]
        i[L], i[P], i[Q] = vL, vP, vQ
        return tuple(i)
    for iQ in range(1, shape[Q], 2):
        for iP in range(2, shape[P], 2):
            v[L][at(slice(0, shape[L]), iP, iQ)] = True
            for k in (iP - 1, iP):
                v[P][at(slice(1, shape[L]), k, iQ)] = True
            for k in (iQ - 1, iQ):
                v[Q][at(slice(1, shape[L]), iP, k)] = True
    return mask


@pytest.mark.parametrize("dtype", hc.DTYPES)
@pytest.mark.parametrize("kind", ["benign", "hard"])
@pytest.mark.parametrize("shape,direction", [((48, 4, 4), 1), ((5, 64, 6), 2), ((6, 5, 130), 3), ((16, 16, 16), 1), ((16, 16, 16), 2),
                                             ((16, 16, 16), 3)])
def test_the_truth_solves_the_lines(orc, shape, direction, kind, dtype):
    """Scaled by max|s| + max|A| max|e| over the case.  Extended precision: <= 1e-16 -- and <= 16 x 2^-64, a few roundings of its own
    format, which is the level at which the check discriminates: a float64 sweep leaves 1e-17 ... 1e-16 (measured: 500 to 2000 times
    the extended sweep's 1e-20 ... 6e-20), above that and 100 times the extended sweep's."""
    p = hc.problem(kind, shape, direction, dtype)
    mask = _last_colour_edges(shape, direction)
    assert mask.sum() > 100
    amax = _diag_max(orc, p)
    out = {}
    for ext in (True, False):
        e = hc.sweep(orc, p, direction, nu=1, order=1, ext=ext)
        r = hc.amat_x(orc, p, e, ext=True)
        scale = np.abs(p['s']).max() + amax * np.abs(e).max()
        out[ext] = float(np.abs(r[mask]).max() / scale)
        assert float(np.abs(r[~mask]).max() / scale) > 1e-6         # (a sweep is no solve: elsewhere the residual is not small)
    assert out[True] <= 1e-16, out
    assert out[True] <= 16 * 2.0 ** -64, out
    assert out[False] > 16 * 2.0 ** -64 and out[False] > 100 * out[True], out


@pytest.mark.parametrize("dtype", hc.DTYPES)
@pytest.mark.parametrize("shape,direction,order", hc.sweep_runs())
def test_hard_cases_of_the_gpu_tests_are_in_the_window(orc, shape, direction, order, dtype):
    p, ref, truth = hc.references(orc, "hard", shape, direction, dtype, order=order)
    e = hc.err(ref, truth)
    assert 1e-13 <= e <= 1e-9, e
    assert hc.err(p['e0'], truth) > 1e-3


@pytest.mark.parametrize("dtype", hc.DTYPES)
@pytest.mark.parametrize("shape,direction,order", hc.sweep_runs())
def test_further_systems_of_the_hard_cases_are_in_the_window(orc, shape, direction, order, dtype):
    """Systems 1 and 2 of the batched runs (tests/test_gpu_batch_families.py, hc.system_fields): the band system 0 is held to."""
    for b in (1, 2):
        e0, s = hc.system_fields("hard", shape, direction, dtype, b)
        p = hc.problem("hard", shape, direction, dtype)
        assert not np.array_equal(e0, p['e0']) and not np.array_equal(s, p['s'])
        ref, truth = hc.references_b(orc, "hard", shape, direction, dtype, b, order)
        e, change = hc.err(ref, truth), hc.err(e0, truth)
        print(f"[system] {shape} dir {direction} order {order} {hc.tname(dtype)} system {b} err(ref) {e:.2e} change {change:.2e}")
        assert 1e-13 <= e <= 1e-9, (b, e)
        assert change > 1e-3, (b, change)


def test_system_fields_are_cached_frozen_and_leave_the_case_alone():
    shape, dtype = (6, 5, 12), np.complex128
    p = hc.problem("hard", shape, 3, dtype)
    assert hc.system_fields("hard", shape, 3, dtype, 0)[0] is p['e0']
    e1, s1 = hc.system_fields("hard", shape, 3, dtype, 1)
    e2, s2 = hc.system_fields("hard", shape, 3, dtype, 2)
    assert hc.system_fields("hard", shape, 3, dtype, 1)[0] is e1 and not e1.flags.writeable and not s1.flags.writeable
    assert not np.array_equal(e1, e2) and not np.array_equal(s1, s2)
    assert 0.1 < np.abs(s1).max() / np.abs(p['s']).max() < 10 and np.abs(s1).max() < 1e-4            # (the hard source scale)
    assert np.abs(hc.system_fields("benign", shape, 3, dtype, 1)[1]).max() > 1
    for f in (e1, s1):
        fx, fy, fz = hc.field_views(f, shape)
        assert not fx[:, [0, -1], :].any() and not fy[:, :, [0, -1]].any() and not fz[[0, -1], :, :].any()
    assert hc.first_difference(e1, e1, shape) is None
    other = np.array(e1)
    other[6 * 6 * 13 + 3] += 1          # the fourth edge of the y-component
    assert hc.first_difference(e1, other, shape) == (1, 3, 0, 0)


@pytest.mark.parametrize("dtype", hc.DTYPES)
@pytest.mark.parametrize("shape,direction,order", hc.sweep_runs())
def test_benign_cases_of_the_gpu_tests_are_near_the_floor(orc, shape, direction, order, dtype):
    """On the benign generator the reference is a few ulp from the truth: the bound of the GPU tests there is the floor's."""
    p, ref, truth = hc.references(orc, "benign", shape, direction, dtype, order=order)
    assert 0 < hc.err(ref, truth) <= 1e-13
    assert hc.err(p['e0'], truth) > 1e-3


@pytest.mark.parametrize("shape,direction", [((5, 7, 16), 3), ((16, 5, 6), 1), ((6, 33, 5), 2)])
def test_the_bound_rejects_the_order_the_project_rejected(orc, shape, direction):
    """What the accuracy tests are for, shown on the CPU: round 1's plain two-sided grouping (tests/tools/conditioning.py
    solve_two_sided, float64 NumPy) against long double, per line solve, next to the one-sided order of the reference and the mirrored
    two-sided order the kernels use.  On the benign inputs the three are alike at 1e-15 -- no parity test could tell them apart; on the
    hard inputs the rejected order is 30 to 500 times the reference order's error (measured: 4e-10 ... 3e-9 against 5e-12 ... 1e-11)
    and misses the bound, the mirrored order holds it."""
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import conditioning as cd
    from reduced_line import LineSys, axes
    dtype = np.complex128
    worst = {}
    for kind in ("benign", "hard"):
        p = hc.problem(kind, shape, direction, dtype)
        L, P, Q = axes(direction)
        ls = LineSys(shape, np.array(p['e0']), np.array(p['s']), list(p['eta']), p['zeta'], p['h'], direction)
        rows = []
        for jQ in range(1, shape[Q]):
            for jP in range(1, shape[P]):
                truth = cd.solve_mirrored(ls, jP, jQ, np.clongdouble, cd.inv_ld)
                orders = (cd.solve_two_sided(ls, jP, jQ, dtype, np.linalg.inv), cd.solve_mirrored(ls, jP, jQ, dtype, np.linalg.inv),
                          cd.solve_block5(ls, jP, jQ, dtype, np.linalg.inv, True))
                rows.append([hc.err(x, truth) for x in orders])
        worst[kind] = np.array(rows).max(axis=0)         # plain two-sided, mirrored, one-sided
    two, mirrored, one = worst["benign"]
    assert two <= hc.bound(one) and mirrored <= hc.bound(one), worst
    two, mirrored, one = worst["hard"]
    assert 1e-13 <= one <= 1e-9, worst
    assert mirrored <= hc.bound(one), worst
    assert two > hc.bound(one), worst


def test_bound_formula():
    assert hc.bound(0.) == 10 * 16 * 2.0 ** -53 and hc.bound(1e-12) == 1e-11
